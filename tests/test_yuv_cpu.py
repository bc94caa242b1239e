"""CPU tests of the 8-bit Y'CbCr 4:2:0 path: tests/yuv_ref.py - the numpy restatement of the arithmetic in include/film_hip.h that
tests/test_yuv_gpu.py compares the kernels with, bit for bit - against an independent float64 evaluation, known answers and its own
round trip; the refusals of the new pixel codes on a plan-only handle; the Y4M reader / writer; the parser of eval/video_cli.py; and,
as tests/test_tile_map_cpu.py does for the RGB cuts, which kernel instance and branch every GPU case reaches and that the comparison on
the designed data finds each planted fault.  No GPU."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import yuv_ref as R
from conftest import ROOT

FMT = R.FORMATS['i420']
LAYOUTS = FMT.layouts      # ('i420', 'nv12')
COLOURS = [(m, f) for m in ('bt709', 'bt601') for f in (False, True)]      # the four colour settings of the 4:2:0 tests
FAULTS = ('chroma_from_tile_coordinate', 'cb_cr_swapped', 'nv12_as_i420')      # what the cut of an 8-bit 4:2:0 frame can get wrong


@pytest.fixture(scope='module')
def geos():
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    out = {}
    for c in R.CASES:
        eng.set_block_overlap(c.overlap)
        out[c.name] = eng.tiling(c.H, c.W, c.align, c.block)
    eng.close()
    return out


# ---- the restatement against float64 ----------------------------------------------------------------------------------------------------
def _in_f64(Y, Cb, Cr, matrix, full):
    """BT.709 / BT.601 from the definition Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)), in float64;
    G is solved from the luma equation, not taken from the restatement's g_b / g_r."""
    Kr, Kb = R.KR_KB[matrix]
    Kg = 1 - Kr - Kb
    Y, Cb, Cr = (a.astype(np.float64) for a in (Y, Cb, Cr))
    y, cb, cr = (Y / 255, (Cb - 128) / 255, (Cr - 128) / 255) if full else ((Y - 16) / 219, (Cb - 128) / 224, (Cr - 128) / 224)
    r = y + 2 * (1 - Kr) * cr
    b = y + 2 * (1 - Kb) * cb
    g = (y - Kr * r - Kb * b) / Kg
    return np.clip(np.stack([r, g, b], -1), 0, 1)


def _out_f64(rgb, matrix, full):
    """The code values before rounding, float64: (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2])."""
    Kr, Kb = R.KR_KB[matrix]
    x = np.clip(rgb.astype(np.float64), 0, 1)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = Kr * r + (1 - Kr - Kb) * g + Kb * b
    box = lambda c: c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean((1, 3))       # noqa: E731
    cb, cr = box((b - y) / (2 * (1 - Kb))), box((r - y) / (2 * (1 - Kr)))
    return (y * 255, cb * 255 + 128, cr * 255 + 128) if full else (y * 219 + 16, cb * 224 + 128, cr * 224 + 128)


@pytest.mark.parametrize('matrix,full', COLOURS)
def test_in_against_float64(matrix, full):
    """Every (Y, Cb, Cr) triple of a 64-step grid plus the extremes: at most 1e-6 apart - five float32 roundings on magnitudes up to 2."""
    v = np.unique(np.concatenate([np.arange(0, 256, 4), [1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255]]))
    Y, Cb, Cr = np.meshgrid(v, v, v, indexing='ij')
    got = FMT.samples_to_rgb(Y, Cb, Cr, matrix, full)
    err = np.abs(got.astype(np.float64) - _in_f64(Y, Cb, Cr, matrix, full)).max()
    print(f'{matrix} full={full}: in, max |float32 - float64| = {err:.3g}')
    assert err <= 1e-6


@pytest.mark.parametrize('matrix,full', COLOURS)
def test_out_against_float64(matrix, full):
    """Uniform random RGB in [-0.1, 1.1]: equal bytes wherever the float64 value is farther than 1e-4 from a rounding tie, at most one
    code apart elsewhere, and at most 1 % of the values so excused."""
    rgb = np.random.default_rng(7).uniform(-0.1, 1.1, (120, 160, 3)).astype(np.float32)
    got = FMT.unpack(FMT.yuv_out(rgb, 'i420', matrix, full), 'i420')
    f32 = FMT.out_unquantised(rgb, matrix, full)
    near_all, n_all = 0, 0
    for name, g, v32, v64 in zip('Y Cb Cr'.split(), got, f32, _out_f64(rgb, matrix, full)):
        v64 = np.clip(v64, 0, 255)
        want = np.floor(v64 + 0.5)
        near = np.abs(v64 - (np.floor(v64) + 0.5)) <= 1e-4
        diff = np.abs(g.astype(np.int64) - want.astype(np.int64))
        print(f'{matrix} full={full} {name}: max |float32 - float64| before q = {np.abs(v32 - v64).max():.3g} codes, '
              f'{near.sum()} of {near.size} within 1e-4 of a tie, {int((diff > 0).sum())} bytes differ')
        assert not diff[~near].any() and diff.max() <= 1
        near_all += int(near.sum()); n_all += near.size
    assert near_all <= 0.01 * n_all


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def _solid(y, cb, cr, layout='i420'):
    return FMT.pack(np.full((2, 2), y), np.full((1, 1), cb), np.full((1, 1), cr), layout)


@pytest.mark.parametrize('matrix', ['bt709', 'bt601'])
def test_known_answers(matrix):
    """Limited-range black and white exactly; the 100 % primaries against the standards' 8-bit tables (Rec. ITU-R BT.709 / BT.601 colour
    bars): out gives the table's codes, in gives the primary back within 0.01 - half a code of Y (0.5 / 219) plus half a code of chroma
    times the largest coefficient (1.86 * 0.5 / 224) is 0.0064."""
    assert not FMT.yuv_in(_solid(16, 128, 128), 'i420', matrix, False).any()
    assert (FMT.yuv_in(_solid(235, 128, 128), 'i420', matrix, False) == 1).all()
    assert not FMT.yuv_in(_solid(0, 128, 128), 'i420', matrix, True).any() and (FMT.yuv_in(_solid(255, 128, 128), 'i420', matrix, True) == 1).all()
    table = {'bt709': {(1, 0, 0): (63, 102, 240), (0, 1, 0): (173, 42, 26), (0, 0, 1): (32, 240, 118), (1, 1, 0): (219, 16, 138),
                       (0, 1, 1): (188, 154, 16), (1, 0, 1): (78, 214, 230), (1, 1, 1): (235, 128, 128), (0, 0, 0): (16, 128, 128)},
             'bt601': {(1, 0, 0): (81, 90, 240), (0, 1, 0): (145, 54, 34), (0, 0, 1): (41, 240, 110), (1, 1, 0): (210, 16, 146),
                       (0, 1, 1): (170, 166, 16), (1, 0, 1): (106, 202, 222), (1, 1, 1): (235, 128, 128), (0, 0, 0): (16, 128, 128)}}[matrix]
    for rgb, codes in table.items():
        x = np.broadcast_to(np.array(rgb, np.float32), (2, 2, 3))
        for layout in LAYOUTS:
            fr = FMT.yuv_out(x, layout, matrix, False)
            assert np.array_equal(fr, _solid(*codes, layout)), (rgb, layout, fr.ravel())
            assert np.abs(FMT.yuv_in(fr, layout, matrix, False) - x).max() <= 0.01, rgb


# ---- round trip, layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('matrix,full', COLOURS)
def test_in_gamut_round_trip_is_the_identity(matrix, full, layout):
    """Replicate in and box mean out are inverse: a frame whose RGB stays inside the gamut returns byte for byte."""
    rng = np.random.default_rng(3)
    fr = FMT.pack(rng.integers(90, 166, (30, 50)), rng.integers(108, 149, (15, 25)), rng.integers(108, 149, (15, 25)), layout)
    rgb = FMT.yuv_in(fr, layout, matrix, full)
    assert rgb.min() > 0 and rgb.max() < 1
    assert np.array_equal(FMT.yuv_out(rgb, layout, matrix, full), fr)


def test_layouts():
    fr = FMT.designed_frames(2, 30, 50, 9)
    for f in fr:
        nv = R.convert_layout(f, 'i420', 'nv12')
        assert nv.shape == f.shape and np.array_equal(nv[:30], f[:30]) and not np.array_equal(nv, f)
        assert np.array_equal(nv.ravel()[1500::2], f.ravel()[1500:1875]) and np.array_equal(nv.ravel()[1501::2], f.ravel()[1875:])
        assert np.array_equal(R.convert_layout(nv, 'nv12', 'i420'), f)
        assert np.array_equal(FMT.yuv_in(nv, 'nv12'), FMT.yuv_in(f, 'i420'))
    rgb = np.random.default_rng(1).uniform(-0.1, 1.1, (16, 18, 3)).astype(np.float32)
    assert np.array_equal(FMT.yuv_out(rgb, 'nv12'), R.convert_layout(FMT.yuv_out(rgb, 'i420'), 'i420', 'nv12'))


def test_designed_data():
    """Every byte value in every plane that has 256 samples; in the smaller chroma planes of y5 over the frames of the batch."""
    for c in R.CASES:
        fr = FMT.designed_frames(c.B, c.H, c.W, 5)
        planes = [FMT.unpack(f, 'i420') for f in fr]
        for pi in range(3):
            if planes[0][pi].size >= 256:
                assert all(len(np.unique(p[pi])) == 256 for p in planes), (c.name, pi)
            elif c.B * planes[0][pi].size >= 400:
                assert len(np.unique(np.concatenate([p[pi].ravel() for p in planes]))) == 256, (c.name, pi)
        nv = FMT.designed_frames(c.B, c.H, c.W, 5, 'nv12')
        assert all(np.array_equal(R.convert_layout(a, 'i420', 'nv12'), b) for a, b in zip(fr, nv))


# ---- the cut: agreement, branches, planted faults -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_cut_equals_frame_conversion_then_float_cut(case, geos):
    geo = geos[case.name]
    total = case.B * len(geo['origins_y']) * len(geo['origins_x'])
    for layout in LAYOUTS:
        fr = FMT.designed_frames(case.B, case.H, case.W, 4, layout)
        for matrix, full in COLOURS:
            a = FMT.cut(fr, geo, 0, total, layout, matrix, full)
            b = FMT.cut_via_frames(fr, geo, 0, total, layout, matrix, full)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (layout, matrix, full)


ALL_BRANCHES = {
    'frame_yuv_to_tiles_kernel<false, FILM_PIX_I420>', 'frame_yuv_to_tiles_kernel<false, FILM_PIX_NV12>', 'frame_yuv_to_tiles_kernel<true, FILM_PIX_I420>',
    'frame_yuv_to_tiles_kernel<true, FILM_PIX_NV12>', 'odd row origin', 'odd column origin', 'word path, Y in one aligned word',
    'word path, Y across two words', 'word path, even column: two chroma samples', 'word path, odd column: three chroma samples',
    'word path, chroma in one word', 'word path, chroma across two words', 'byte path', 'padding group', 'vector stores', 'scalar stores'}
ALL_OUT_BRANCHES = {'rgb_to_yuv_kernel<FILM_PIX_I420>', 'rgb_to_yuv_kernel<FILM_PIX_NV12>', 'vector loads', 'scalar loads', 'Y word stores', 'Y byte stores',
                    'chroma word stores', 'chroma byte stores'}
OUT_SIZES = [(2, 2), (16, 18), (30, 50)]       # what tests/test_yuv_gpu.py runs film_to_yuv420 on


def test_the_cases_reach_every_instance_and_branch(geos):
    """Which instance of the cut kernel and which of its branches the calls of tests/test_yuv_gpu.py take, from the kernel's own
    conditions restated in yuv_ref.Format.branches; the same for rgb_to_yuv420_kernel on that test's sizes.  The table goes to the log."""
    seen = {}
    for c in R.CASES:
        s = seen[c.name] = set()
        for layout in LAYOUTS:
            for ranges in R.ranges_of(c, geos[c.name]).values():
                for tile0, nt in ranges:
                    s |= FMT.branches(c, geos[c.name], layout, tile0, nt)
        print(c.name, '|', ', '.join(sorted(s)))
    union = set().union(*seen.values())
    assert union == ALL_BRANCHES, (sorted(ALL_BRANCHES - union), sorted(union - ALL_BRANCHES))
    assert 'odd column origin' in seen['y1-30x50-b3x2'] and 'odd row origin' not in seen['y1-30x50-b3x2']
    assert {'odd column origin', 'odd row origin', 'frame_yuv_to_tiles_kernel<true, FILM_PIX_NV12>'} <= seen['y2-30x50-b3x2-ov3x5']
    assert not seen['y3-16x16'] & {'byte path', 'padding group', 'scalar stores', 'word path, Y across two words'}       # the pure fast path
    assert not any(b.startswith('word path') for b in seen['y4-2x2'])
    assert 'scalar stores' in seen['y6-12x22-b1x2-noalign']
    # chroma rows at every byte offset mod 4 (30 x 50: rows of 25 bytes)
    assert {(1500 + j * 25) % 4 for j in range(15)} == {0, 1, 2, 3}
    out = {}
    for h, w in OUT_SIZES:
        for layout in LAYOUTS:
            out[h, w, layout] = FMT.out_branches(h, w, layout, 0) | FMT.out_branches(h, w, layout, R.T.GUARD_U8)
            print(f'{h}x{w} {layout} |', ', '.join(sorted(out[h, w, layout])))
    assert set().union(*out.values()) == ALL_OUT_BRANCHES


def test_the_restatement_passes_its_own_comparison(geos):
    backend = FMT.NumpyBackend(lambda c: geos[c.name])
    for c in (R.CASES[1], R.CASES[3]):
        for layout in LAYOUTS:
            for ranges in R.ranges_of(c, geos[c.name]).values():
                assert not list(FMT.check_cut(backend, c, geos[c.name], layout, 'bt601', True, ranges, twice=False)), c.name


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_fails_the_comparison(fault, geos):
    """The restatement with one fault planted as the backend of the comparison the GPU test runs, on the same designed data: found in
    every case in which the fault changes what the backend does (the chroma pairing cannot go wrong from an even origin; a frame with
    one chroma sample per plane reads the same as I420 and as NV12)."""
    must = {'chroma_from_tile_coordinate': ['y1-30x50-b3x2', 'y2-30x50-b3x2-ov3x5', 'y6-12x22-b1x2-noalign'],
            'cb_cr_swapped': ['y1-30x50-b3x2', 'y2-30x50-b3x2-ov3x5', 'y3-16x16', 'y5-18x44-b1x2', 'y6-12x22-b1x2-noalign'],
            'nv12_as_i420': ['y1-30x50-b3x2', 'y2-30x50-b3x2-ov3x5', 'y3-16x16', 'y5-18x44-b1x2', 'y6-12x22-b1x2-noalign']}[fault]
    backend = FMT.NumpyBackend(lambda c: geos[c.name], fault)
    for c in R.CASES:
        if c.name in must:
            for layout in (['nv12'] if fault == 'nv12_as_i420' else LAYOUTS):
                ranges = R.ranges_of(c, geos[c.name])['one']
                first = next(FMT.check_cut(backend, c, geos[c.name], layout, 'bt709', False, ranges, seed=17, twice=False), None)
                print(fault, layout, '->', first)
                assert first is not None, (fault, c.name, layout)


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------
def test_pixel_codes_entry_points_and_refusals():
    from film_hip import engine
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID, FILM_ERR_NO_DEVICE
    from film_hip.options import TINY
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    for name, val in (('FILM_PIX_I420', '16'), ('FILM_PIX_NV12', '17'), ('FILM_YUV_BT601', '0x100'), ('FILM_YUV_FULL', '0x400')):
        assert re.search(rf'^#define {name}\s+{val}\b', header, re.M), name
    assert (engine.FILM_PIX_I420, engine.FILM_PIX_NV12, engine.FILM_YUV_BT601, engine.FILM_YUV_FULL) == (16, 17, 0x100, 0x400)
    assert re.search(r'^int film_to_yuv420\(const float\* src, void\* dst, int H, int W, int pix, void\* stream\);', header, re.M)
    assert re.search(r'^int film_debug_yuv_cut\(film_t\* h, int pix, void\* frames_dev, float\* tiles_dev, int B, int H, int W, int align, '
                     r'int block_h, int block_w,\s+int tile0, int ntiles, void\* stream\);', header, re.M)
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    lib = engine.load_library()
    for sym in ('film_to_yuv420', 'film_debug_yuv_cut'):
        assert re.search(rf'\b{sym};', mapfile) and sym in engine.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    assert engine.pix_code('i420') == 16 and engine.pix_code('nv12', 'bt601', True) == 17 | 0x100 | 0x400
    assert engine.PIX['i420'][1] is np.uint8 and engine.PIX['nv12'][1] is np.uint8

    eng = FilmEngine(TINY, device=-1)
    h = eng._h
    err = lambda: lib.film_last_error(h).decode()       # noqa: E731
    H, W = 32, 48
    valid = [lay | m | f for lay in (16, 17) for m in (0, 0x100) for f in (0, 0x400)]
    for pix in valid:
        assert lib.film_stream_open(h, H, W, 0, 1, 1, pix) == FILM_ERR_NO_DEVICE, pix
        assert lib.film_stream_open(h, H, W, 8, 2, 2, pix) == FILM_ERR_NO_DEVICE, pix
    bad = [2, -1, 15, 18, 16 | 0x200, 16 | 0x800, 17 | 0x1000, 16 | (1 << 30), 0 | 0x100, 1 | 0x400, 0 | 0x500, 1 | 0x100]
    for pix in bad:
        assert lib.film_stream_open(h, H, W, 0, 1, 1, pix) == FILM_ERR_INVALID and 'pix' in err(), (pix, err())
    for hh, ww in ((31, 48), (32, 47), (31, 47)):
        for pix in (16, 17 | 0x400):
            assert lib.film_stream_open(h, hh, ww, 0, 1, 1, pix) == FILM_ERR_INVALID
            assert 'pix' in err() and '4:2:0 needs even sizes' in err(), err()
        assert lib.film_stream_open(h, hh, ww, 0, 1, 1, 1) == FILM_ERR_NO_DEVICE       # (RGB layouts take odd sizes)

    P = ctypes.c_void_p(4096)        # (never dereferenced: every call below is refused before any device call)

    def cut(pix=16, frames=P, tiles=P, B=2, H=30, W=50, align=8, bh=3, bw=2, tile0=0, ntiles=12):
        rc = lib.film_debug_yuv_cut(h, pix, frames, tiles, B, H, W, align, bh, bw, tile0, ntiles, None)
        return rc, err()

    for pix in valid:
        assert cut(pix=pix)[0] == FILM_ERR_NO_DEVICE and 'plan-only' in cut(pix=pix)[1]
    assert cut(tile0=11, ntiles=1)[0] == FILM_ERR_NO_DEVICE
    for pix in bad + [0, 1]:
        rc, msg = cut(pix=pix)
        assert rc == FILM_ERR_INVALID and 'pix' in msg, (pix, msg)
    for kw in (dict(frames=None), dict(tiles=None), dict(frames=ctypes.c_void_p(4098)), dict(ntiles=0), dict(tile0=-1), dict(tile0=12, ntiles=1),
               dict(ntiles=13), dict(B=0), dict(H=0), dict(W=-2), dict(bh=4), dict(bw=4), dict(H=33, bh=3), dict(W=51, bw=1)):
        rc, msg = cut(**kw)
        assert rc == FILM_ERR_INVALID and msg, (kw, rc, msg)
    assert '4:2:0 needs even sizes' in cut(H=33, bh=3)[1]
    eng.set_block_overlap((6, 0))        # 2 o > p: refused like the compute entry points
    rc, msg = cut()
    assert rc == FILM_ERR_INVALID and msg.startswith('block_overlap_h')
    eng.set_block_overlap(0)
    # film_debug_tile_map stays as it is: the 4:2:0 codes are not its business
    assert lib.film_debug_tile_map(h, 0, 16, P, P, 2, 30, 50, 8, 3, 2, 0, 12, None) == FILM_ERR_INVALID
    # film_to_yuv420 has no handle: codes only
    S = ctypes.c_void_p(4096)
    assert lib.film_to_yuv420(None, S, 4, 4, 16, None) == FILM_ERR_INVALID and lib.film_to_yuv420(S, None, 4, 4, 16, None) == FILM_ERR_INVALID
    for hh, ww, pix in ((3, 4, 16), (4, 5, 17), (0, 4, 16), (4, -2, 16), (4, 4, 0), (4, 4, 1), (4, 4, 2), (4, 4, 16 | 0x200), (4, 4, -1)):
        assert lib.film_to_yuv420(S, S, hh, ww, pix, None) == FILM_ERR_INVALID, (hh, ww, pix)
    # the Python layer
    with pytest.raises(FilmError) as e:
        eng.open_stream(H, W, pix='i420', matrix='bt601', full_range=True)
    assert e.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(FilmError) as e:
        eng.open_stream(31, W, pix='nv12')
    assert e.value.code == FILM_ERR_INVALID and 'even' in str(e.value)
    with pytest.raises(FilmError) as e:
        eng.open_stream(H, W, pix='u8', matrix='bt601')
    assert e.value.code == FILM_ERR_INVALID and 'pix' in str(e.value)
    with pytest.raises(ValueError):
        eng.open_stream(H, W, pix='i420', matrix='bt2020')
    with pytest.raises(ValueError):
        eng.open_stream(H, W, pix='yv12')
    with pytest.raises(FilmError) as e:
        eng.debug_yuv_cut(4096, 4096, 2, 30, 50, 8, (3, 2), 0, 12, pix='nv12', matrix='bt601')
    assert e.value.code == FILM_ERR_NO_DEVICE
    eng.close()


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------------------
def _y4m_bytes(tokens, frames):
    from film_hip import y4m
    f = io.BytesIO()
    w = y4m.Y4MWriter(f, tokens)
    for fr in frames:
        w.write(fr)
    return f.getvalue()


def test_y4m_round_trip_and_header():
    from film_hip import y4m
    frames = FMT.designed_frames(3, 30, 50, 2)
    tokens = ['W50', 'H30', 'F30000:1001', 'Ip', 'A1:1', 'C420mpeg2', 'XYSCSS=420MPEG2', 'XCOLORRANGE=FULL']
    data = _y4m_bytes(tokens, frames)
    assert data.startswith(b'YUV4MPEG2 W50 H30 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\nFRAME\n')
    assert len(data) == len(b'YUV4MPEG2 ' + ' '.join(tokens).encode() + b'\n') + 3 * (6 + 2250)
    r = y4m.Y4MReader(io.BytesIO(data))
    assert (r.width, r.height, r.tokens, r.full_range, r.rate, r.frame_bytes) == (50, 30, tokens, True, (30000, 1001), 2250)
    got = list(r)
    assert len(got) == 3 and r.frames_read == 3 and all(g.dtype == np.uint8 and g.shape == (45, 50) for g in got)
    assert all(np.array_equal(g, f) for g, f in zip(got, frames))
    assert r.read_frame() is None
    # F doubled, everything else kept; frame parameters are skipped; a stream without C / I tokens is 4:2:0 progressive
    assert y4m.double_rate(tokens) == ['W50', 'H30', 'F60000:1001'] + tokens[3:]
    assert y4m.double_rate(['W2', 'H2']) == ['W2', 'H2']
    plain = b'YUV4MPEG2 W2 H2 F25:1\nFRAME Ip\n' + bytes(range(6)) + b'FRAME\n' + bytes(range(6, 12))
    r = y4m.Y4MReader(io.BytesIO(plain))
    assert not r.full_range and [f.ravel().tolist() for f in r] == [list(range(6)), list(range(6, 12))]
    for c in y4m.C420:
        for i in ('Ip', 'I?'):
            assert y4m.Y4MReader(io.BytesIO(f'YUV4MPEG2 W4 H2 F25:1 {i} C{c}\n'.encode())).read_frame() is None
    assert y4m.header_tokens(50, 30, (24, 1), True) == ['W50', 'H30', 'F24:1', 'Ip', 'A1:1', 'C420jpeg', 'XCOLORRANGE=FULL']
    with pytest.raises(ValueError):
        y4m.Y4MWriter(io.BytesIO(), ['W4', 'H2']).write(np.zeros((2, 4), np.uint8))


@pytest.mark.parametrize('token', ['C422', 'C444', 'C444alpha', 'Cmono', 'C420p10', 'C420p12', 'C422p10', 'C444p16', 'C411', 'It', 'Ib', 'Im'])
def test_y4m_refuses_with_the_token_in_the_message(token):
    from film_hip import y4m
    with pytest.raises(y4m.Y4MError) as e:
        y4m.Y4MReader(io.BytesIO(f'YUV4MPEG2 W4 H2 F25:1 {token} A1:1\n'.encode() + b'FRAME\n' + bytes(64)))
    assert repr(token) in str(e.value)


def test_y4m_reports_bad_and_truncated_streams():
    from film_hip import y4m
    data = _y4m_bytes(['W4', 'H2', 'F25:1'], [np.arange(12, dtype=np.uint8).reshape(3, 4)] * 2)
    for cut_at, what in ((len(data) - 1, 'frame 1 has 11 of 12 bytes'), (len(data) - 12, 'frame 1 has 0 of 12 bytes'), (len(data) - 15, 'ends inside the line')):
        r = y4m.Y4MReader(io.BytesIO(data[:cut_at]))
        assert r.read_frame() is not None
        with pytest.raises(y4m.Y4MError) as e:
            r.read_frame()
        assert 'truncated' in str(e.value) and what in str(e.value), str(e.value)
    for head, what in ((b'', 'empty'), (b'RIFF....AVI \n', 'not a YUV4MPEG2'), (b'YUV4MPEG2 H2 F25:1\n', 'no W / H'), (b'YUV4MPEG2 W5 H2\n', 'even sizes'),
                       (b'YUV4MPEG2 W4 H3\n', 'even sizes'), (b'YUV4MPEG2 Wx H2\n', "'Wx'"), (b'YUV4MPEG2 W4 H2' + b' X' * 3000, 'more than')):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.Y4MReader(io.BytesIO(head))
        assert what in str(e.value), str(e.value)
    r = y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H2\nFRAMES\n' + bytes(12)))
    with pytest.raises(y4m.Y4MError) as e:
        r.read_frame()
    assert 'expected a FRAME line' in str(e.value)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_video_cli_parser_and_frame_order():
    from eval import video_cli as cli
    from film_hip import y4m
    a = cli.build_parser().parse_args(['--input', '-', '--output', 'o.y4m'])
    assert (a.input, a.output, a.model_path, a.align, a.block_height, a.block_width) == ('-', 'o.y4m', None, 64, 1, 1)
    assert (a.block_overlap_height, a.block_overlap_width, a.matrix, a.full_range) == (0, 0, 'bt709', None)
    a = cli.build_parser().parse_args(['--input', 'i.y4m', '--output', '-', '--model_path', 'm', '--align', '32', '--block_height', '2',
                                       '--block_width', '3', '--block_overlap_height', '-1', '--block_overlap_width', '4', '--matrix', 'bt601',
                                       '--full_range'])
    assert (a.model_path, a.align, a.block_height, a.block_width, a.block_overlap_height, a.block_overlap_width) == ('m', 32, 2, 3, -1, 4)
    assert a.matrix == 'bt601' and a.full_range is True
    for bad in (['--input', 'i'], ['--output', 'o'], ['--input', 'i', '--output', 'o', '--matrix', 'bt2020']):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(bad)
    with pytest.raises(y4m.Y4MError):           # the header is refused before any model is loaded
        import tempfile
        with tempfile.NamedTemporaryFile(suffix='.y4m') as f:
            f.write(b'YUV4MPEG2 W4 H2 F25:1 C444\n'); f.flush()
            cli.main(['--input', f.name, '--output', os.devnull])

    # the frame order and the header, with a stand-in for the interpolator: n frames in, 2 n - 1 out, inputs verbatim
    class Stream:
        def __init__(self, log): self.prev, self.log = None, log
        def __enter__(self): return self
        def __exit__(self, *exc): self.log.append('closed')
        def push(self, frame):
            mid = None if self.prev is None else ((self.prev.astype(np.int32) + frame) // 2).astype(np.uint8)
            self.prev = frame
            return mid

    class It:
        def __init__(self): self.log = []
        def open_stream(self, h, w, pix, matrix, full_range):
            self.log.append((h, w, pix, matrix, full_range))
            return Stream(self.log)

    frames = FMT.designed_frames(5, 4, 6, 1)
    tokens = ['W6', 'H4', 'F25:1', 'Ip', 'A1:1', 'C420jpeg', 'XCOLORRANGE=FULL']
    for override, want_full in ((None, True), (False, False)):
        it, out = It(), io.BytesIO()
        n = cli.double_frame_rate(it, y4m.Y4MReader(io.BytesIO(_y4m_bytes(tokens, frames))), out, 'bt601', override)
        assert n == 9 and it.log == [(4, 6, 'i420', 'bt601', want_full), 'closed']
        r = y4m.Y4MReader(io.BytesIO(out.getvalue()))
        assert r.tokens == ['W6', 'H4', 'F50:1'] + tokens[3:]
        got = list(r)
        assert len(got) == 9 and all(np.array_equal(got[2 * i], frames[i]) for i in range(5))
        assert all(np.array_equal(got[2 * i + 1], ((frames[i].astype(np.int32) + frames[i + 1]) // 2).astype(np.uint8)) for i in range(4))
