"""CPU tests of the 10-bit Y'CbCr 4:2:0 path (FILM_PIX_I010 / FILM_PIX_P010): tests/yuv_ref.py - the numpy restatement of "The 10-bit
4:2:0 arithmetic" in include/film_hip.h that tests/test_yuv10_gpu.py compares the kernels with, bit for bit - against an independent float64
evaluation, known answers and its own round trip; I010 <-> P010; which kernel instance and branch every GPU case reaches and that the
comparison on the designed data finds each planted fault; the refusals of the new pixel codes on a plan-only handle; the Y4M reader /
writer on C420p10; eval/video_cli.py on a 10-bit stream with a stand-in interpolator.  No GPU."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import yuv_ref as R
from conftest import ROOT

FMT = R.FORMATS['i010']
LAYOUTS = FMT.layouts
COLOURS = [(m, f) for m in ('bt709', 'bt601') for f in (False, True)]      # the four colour settings of the 4:2:0 tests
FAULTS = ('p010_as_i010', 'i010_as_p010', 'ignored_bits_not_masked', 'eight_bit_scale_shifted', 'cb_cr_swapped', 'chroma_from_tile_coordinate')


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


# ---- the restatement against float64, known answers -------------------------------------------------------------------------------------
def _in_f64(Y, Cb, Cr, matrix, full):
    """From the definition Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)) in float64, with the 10-bit
    code ranges of Rec. ITU-R BT.709 / BT.2100 (64 .. 940, 64 .. 960, centre 512); G is solved from the luma equation."""
    Kr, Kb = R.KR_KB[matrix]
    Kg = 1 - Kr - Kb
    Y, Cb, Cr = (a.astype(np.float64) for a in (Y, Cb, Cr))
    y, cb, cr = (Y / 1023, (Cb - 512) / 1023, (Cr - 512) / 1023) if full else ((Y - 64) / 876, (Cb - 512) / 896, (Cr - 512) / 896)
    r = y + 2 * (1 - Kr) * cr
    b = y + 2 * (1 - Kb) * cb
    g = (y - Kr * r - Kb * b) / Kg
    return np.clip(np.stack([r, g, b], -1), 0, 1)


@pytest.mark.parametrize('matrix,full', COLOURS)
def test_in_against_float64(matrix, full):
    """Every (Y, Cb, Cr) triple of a 64-step grid plus the extremes: at most 1e-6 apart - five float32 roundings on magnitudes up to 2."""
    v = np.unique(np.concatenate([np.arange(0, 1024, 16), R.EXTREMES]))
    Y, Cb, Cr = np.meshgrid(v, v, v, indexing='ij')
    got = FMT.samples_to_rgb(Y, Cb, Cr, matrix, full)
    err = np.abs(got.astype(np.float64) - _in_f64(Y, Cb, Cr, matrix, full)).max()
    print(f'{matrix} full={full}: in, max |float32 - float64| = {err:.3g}')
    assert err <= 1e-6


def _solid(y, cb, cr, layout='i010'):
    return FMT.pack(FMT.store(np.full((2, 2), y), layout), FMT.store(np.full((1, 1), cb), layout), FMT.store(np.full((1, 1), cr), layout), layout)


@pytest.mark.parametrize('matrix', ['bt709', 'bt601'])
def test_known_answers(matrix):
    """Limited-range black (64) and white (940) exactly, full-range 0 and 1023 exactly; the 100 % primaries: the 10-bit codes are the 8-bit
    table's codes times four (the 10-bit ranges are the 8-bit ranges shifted by two bits, so a colour whose 8-bit value before rounding is
    within 1/8 of its code lands on four times that code) - within one code - and come back within 0.0025 (half a code of Y, 0.5 / 876,
    plus half a code of chroma times the largest coefficient, 1.86 * 0.5 / 896, is 0.0016)."""
    for layout in LAYOUTS:
        assert not FMT.yuv_in(_solid(64, 512, 512, layout), layout, matrix, False).any()
        assert (FMT.yuv_in(_solid(940, 512, 512, layout), layout, matrix, False) == 1).all()
        assert not FMT.yuv_in(_solid(0, 512, 512, layout), layout, matrix, True).any() and (FMT.yuv_in(_solid(1023, 512, 512, layout), layout, matrix, True) == 1).all()
    table = {'bt709': {(1, 0, 0): (63, 102, 240), (0, 1, 0): (173, 42, 26), (0, 0, 1): (32, 240, 118), (1, 1, 1): (235, 128, 128), (0, 0, 0): (16, 128, 128)},
             'bt601': {(1, 0, 0): (81, 90, 240), (0, 1, 0): (145, 54, 34), (0, 0, 1): (41, 240, 110), (1, 1, 1): (235, 128, 128), (0, 0, 0): (16, 128, 128)}}[matrix]
    for rgb, codes8 in table.items():
        x = np.broadcast_to(np.array(rgb, np.float32), (2, 2, 3))
        for layout in LAYOUTS:
            fr = FMT.yuv_out(x, layout, matrix, False)
            got = [int(FMT.code(p, layout).ravel()[0]) for p in FMT.unpack(fr, layout)]
            assert all(abs(g - 4 * c) <= 2 for g, c in zip(got, codes8)), (rgb, layout, got)
            if sum(rgb) in (0, 3):
                assert got == [4 * c for c in codes8]
            assert np.abs(FMT.yuv_in(fr, layout, matrix, False) - x).max() <= 0.0025, rgb


# ---- round trip, layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('matrix,full', COLOURS)
def test_in_gamut_round_trip_is_the_identity(matrix, full, layout):
    """Replicate in and box mean out are inverse: every 2 x 2 block of a random frame whose four decoded pixels stay strictly inside the
    gamut returns code for code - Y and chroma -, junk in the ignored bits or not.  The blocks inside the gamut are asserted to be a
    non-trivial share: more than a quarter of the frame and more than 200 000 samples."""
    rng = np.random.default_rng(3)
    h, w = 480, 960
    fr = FMT.pack(FMT.store(rng.integers(200, 824, (h, w)), layout), FMT.store(rng.integers(400, 625, (h // 2, w // 2)), layout),
                FMT.store(rng.integers(400, 625, (h // 2, w // 2)), layout), layout)
    fr = FMT.with_junk(fr, layout, 4)
    rgb = FMT.yuv_in(fr, layout, matrix, full)
    inside = ((rgb > 0) & (rgb < 1)).all(-1)
    block = inside[0::2, 0::2] & inside[0::2, 1::2] & inside[1::2, 0::2] & inside[1::2, 1::2]
    samples = 6 * int(block.sum())
    print(f'{layout} {matrix} full={full}: {block.mean():.3f} of the blocks inside the gamut, {samples} samples')
    assert block.mean() > 0.25 and samples > 200000
    back = FMT.yuv_out(rgb, layout, matrix, full)
    Y0, Cb0, Cr0 = (FMT.code(p, layout) for p in FMT.unpack(fr, layout))
    Y1, Cb1, Cr1 = FMT.unpack(back, layout)
    assert not ((Y1 if layout == 'i010' else Y1 & 63) >> (10 if layout == 'i010' else 0)).any()      # the ignored bits come back as zero
    Y1, Cb1, Cr1 = (FMT.code(p, layout) for p in (Y1, Cb1, Cr1))
    pix = block.repeat(2, 0).repeat(2, 1)
    assert np.array_equal(Y1[pix], Y0[pix]) and np.array_equal(Cb1[block], Cb0[block]) and np.array_equal(Cr1[block], Cr0[block])


def test_layouts_and_codes():
    w = np.array([0, 1, 63, 64, 1023, 1024, 0xffc0, 0xffff, 0x8001], np.uint16)
    assert FMT.code(w, 'i010').tolist() == [0, 1, 63, 64, 1023, 0, 960, 1023, 1] and FMT.code(w, 'p010').tolist() == [0, 0, 0, 1, 15, 16, 1023, 1023, 512]
    assert FMT.store([0, 1, 1023], 'p010').tolist() == [0, 64, 0xffc0] and FMT.store([0, 1, 1023], 'i010').tolist() == [0, 1, 1023]
    fr = FMT.designed_frames(2, 30, 50, 9)
    for f in fr:
        clean = R.convert_layout(f, 'i010', 'i010')
        assert not np.array_equal(clean, f) and clean.max() <= 1023                      # (the designed frames carry junk)
        p = R.convert_layout(f, 'i010', 'p010')
        assert p.shape == f.shape and p.dtype == np.uint16 and not (p & 63).any()
        assert np.array_equal(p[:30] >> 6, f[:30] & 1023)
        assert np.array_equal(p.ravel()[1500::2] >> 6, f.ravel()[1500:1875] & 1023) and np.array_equal(p.ravel()[1501::2] >> 6, f.ravel()[1875:] & 1023)
        assert np.array_equal(R.convert_layout(p, 'p010', 'i010'), clean)
        for matrix, full in COLOURS:
            assert np.array_equal(FMT.yuv_in(FMT.with_junk(p, 'p010', 1), 'p010', matrix, full), FMT.yuv_in(f, 'i010', matrix, full))
        assert np.array_equal(FMT.histogram(p, 'p010'), FMT.histogram(f, 'i010')) and FMT.histogram(f, 'i010').sum(1).tolist() == [1500, 375, 375]
    rgb = np.random.default_rng(1).uniform(-0.1, 1.1, (16, 18, 3)).astype(np.float32)
    for matrix, full in COLOURS:
        assert np.array_equal(FMT.yuv_out(rgb, 'p010', matrix, full), R.convert_layout(FMT.yuv_out(rgb, 'i010', matrix, full), 'i010', 'p010'))
    # the 10-bit out is the 8-bit out at four times the resolution: the codes agree after >> 2 up to the rounding of the two quantisers
    a, b = FMT.code(FMT.yuv_out(rgb, 'i010'), 'i010').astype(np.int64), R.FORMATS['i420'].yuv_out(rgb, 'i420').astype(np.int64)
    assert np.abs(a - 4 * b).max() <= 3


def test_designed_data():
    """Every code 0 .. 1023 in every Y plane of 1024 samples or more; the extreme codes in every plane that has room; random junk in the
    ignored bits of both layouts; the P010 frames hold the codes of the I010 frames."""
    for c in R.CASES:
        fr = FMT.designed_frames(c.B, c.H, c.W, 5)
        pf = FMT.designed_frames(c.B, c.H, c.W, 5, 'p010')
        assert fr.dtype == np.uint16 and fr.shape == (c.B, c.H * 3 // 2, c.W)
        for f, p in zip(fr, pf):
            Y = FMT.code(FMT.unpack(f, 'i010')[0], 'i010')
            if Y.size >= 1024:
                assert len(np.unique(Y)) == 1024, c.name
            if Y.size >= 40:
                assert {0, 1023, 64, 940} <= set(Y.ravel().tolist()), c.name
            assert np.array_equal(R.convert_layout(p, 'p010', 'i010'), R.convert_layout(f, 'i010', 'i010'))
            if f.size >= 24:
                assert (f >> 10).any() and (p & 63).any(), c.name
        allY = np.concatenate([FMT.code(FMT.unpack(f, 'i010')[0], 'i010').ravel() for f in fr])
        assert {0, 1023} <= set(allY.tolist()) or c.H * c.W < 8, c.name


# ---- the cut: agreement, branches, planted faults -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_cut_equals_frame_conversion_then_float_cut(case, geos):
    """The cut (the formulas on the gathered words) == table look-ups on the whole frame, then tile_map_ref's float cut."""
    geo = geos[case.name]
    total = case.B * len(geo['origins_y']) * len(geo['origins_x'])
    for layout in LAYOUTS:
        fr = FMT.designed_frames(case.B, case.H, case.W, 4, layout)
        for matrix, full in COLOURS:
            a = FMT.cut(fr, geo, 0, total, layout, matrix, full)
            b = FMT.cut_via_frames(fr, geo, 0, total, layout, matrix, full)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (layout, matrix, full)


ALL_BRANCHES = {
    'frame_yuv_to_tiles_kernel<false, FILM_PIX_I010>', 'frame_yuv_to_tiles_kernel<false, FILM_PIX_P010>', 'frame_yuv_to_tiles_kernel<true, FILM_PIX_I010>',
    'frame_yuv_to_tiles_kernel<true, FILM_PIX_P010>', 'odd row origin', 'odd column origin', 'word path, Y in two aligned words',
    'word path, Y across three words', 'word path, even column: two chroma samples', 'word path, odd column: three chroma samples',
    'word path, chroma in one word', 'word path, chroma across two words', 'word path, two CbCr pair words', 'word path, three CbCr pair words',
    'sample path', 'padding group', 'vector stores', 'scalar stores'}
ALL_OUT_BRANCHES = {'rgb_to_yuv_kernel<FILM_PIX_I010>', 'rgb_to_yuv_kernel<FILM_PIX_P010>', 'vector loads', 'scalar loads', 'Y word stores', 'Y sample stores',
                    'chroma word stores', 'chroma sample stores'}
OUT_SIZES = [(2, 2), (16, 18), (30, 50)]       # what tests/test_yuv10_gpu.py runs film_to_yuv420 on
OUT_OFFSETS = (0, 2)                           # ... with dst 4-byte aligned and 2 bytes behind that


def test_the_cases_reach_every_instance_and_branch(geos):
    """Which instance of the 10-bit cut kernel and which of its branches the calls of tests/test_yuv10_gpu.py take, from the kernel's own
    conditions restated in yuv_ref.Format.branches; the same for rgb_to_yuv10_kernel on that test's sizes.  The table goes to the log."""
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
    assert {'odd column origin', 'odd row origin', 'frame_yuv_to_tiles_kernel<true, FILM_PIX_P010>'} <= seen['y2-30x50-b3x2-ov3x5']
    assert not seen['y3-16x16'] & {'sample path', 'padding group', 'scalar stores', 'word path, Y across three words'}       # the pure fast path
    assert not any(b.startswith('word path') for b in seen['y4-2x2'])
    assert 'scalar stores' in seen['y6-12x22-b1x2-noalign']
    out = {}
    for h, w in OUT_SIZES:
        for layout in LAYOUTS:
            out[h, w, layout] = set().union(*[FMT.out_branches(h, w, layout, o) for o in OUT_OFFSETS])
            print(f'{h}x{w} {layout} |', ', '.join(sorted(out[h, w, layout])))
    assert set().union(*out.values()) == ALL_OUT_BRANCHES


def test_the_restatement_passes_its_own_comparison(geos):
    """On every case, both layouts, every partition (the colour settings take turns over the cases)."""
    backend = FMT.NumpyBackend(lambda c: geos[c.name])
    for i, c in enumerate(R.CASES):
        matrix, full = COLOURS[i % 4]
        for layout in LAYOUTS:
            for ranges in R.ranges_of(c, geos[c.name]).values():
                assert not list(FMT.check_cut(backend, c, geos[c.name], layout, matrix, full, ranges, twice=False)), c.name


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_fails_the_comparison(fault, geos):
    """The restatement with one fault planted as the backend of the comparison the GPU test runs, on the same designed data: found in
    every case in which the fault changes what the backend does (a code rule only with the layout it belongs to; the shifted 8-bit scale
    only in full range; the chroma pairing cannot go wrong from an even origin)."""
    every = [c.name for c in R.CASES]
    must = {'p010_as_i010': every, 'i010_as_p010': every, 'ignored_bits_not_masked': every, 'eight_bit_scale_shifted': every, 'cb_cr_swapped': every,
            'chroma_from_tile_coordinate': ['y1-30x50-b3x2', 'y2-30x50-b3x2-ov3x5', 'y6-12x22-b1x2-noalign']}[fault]
    layouts = {'p010_as_i010': ['p010'], 'i010_as_p010': ['i010']}.get(fault, LAYOUTS)
    full = fault == 'eight_bit_scale_shifted'
    backend = FMT.NumpyBackend(lambda c: geos[c.name], fault)
    for c in R.CASES:
        if c.name in must:
            for layout in layouts:
                ranges = R.ranges_of(c, geos[c.name])['one']
                first = next(FMT.check_cut(backend, c, geos[c.name], layout, 'bt709', full, ranges, seed=17, twice=False), None)
                print(fault, layout, '->', first)
                assert first is not None, (fault, c.name, layout)
    if fault == 'eight_bit_scale_shifted':      # limited range: 219 << 2, 224 << 2 ARE the 10-bit divisors
        c = R.CASES[0]
        assert not list(FMT.check_cut(backend, c, geos[c.name], 'i010', 'bt709', False, R.ranges_of(c, geos[c.name])['one'], twice=False))


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------
def test_pixel_codes_and_refusals():
    from film_hip import engine
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID, FILM_ERR_NO_DEVICE
    from film_hip.options import TINY
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    for name, val in (('FILM_PIX_I010', '32'), ('FILM_PIX_P010', '33')):
        assert re.search(rf'^#define {name}\s+{val}\b', header, re.M), name
    assert (engine.FILM_PIX_I010, engine.FILM_PIX_P010) == (32, 33)
    assert engine.pix_code('i010') == 32 and engine.pix_code('p010', 'bt601', True) == 33 | 0x100 | 0x400
    assert engine.PIX['i010'][1] is np.uint16 and engine.PIX['p010'][1] is np.uint16
    # no new exported symbol: the map file and the Python list name the same functions
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    assert set(re.findall(r'\b(film_\w+);', mapfile)) == set(engine.EXPORTED_SYMBOLS)
    lib = engine.load_library()

    eng = FilmEngine(TINY, device=-1)
    h = eng._h
    err = lambda: lib.film_last_error(h).decode()       # noqa: E731
    H, W = 32, 48
    valid = [lay | m | f for lay in (32, 33) for m in (0, 0x100) for f in (0, 0x400)]
    for pix in valid:
        assert lib.film_stream_open(h, H, W, 0, 1, 1, pix) == FILM_ERR_NO_DEVICE, pix
        assert lib.film_stream_open(h, H, W, 8, 2, 2, pix) == FILM_ERR_NO_DEVICE, pix
    bad = [32 | 0x200, 33 | 0x200, 32 | 0x800, 33 | 0x1000, 32 | (1 << 30), 34, 31, 48]
    for pix in bad:
        assert lib.film_stream_open(h, H, W, 0, 1, 1, pix) == FILM_ERR_INVALID and 'pix' in err(), (pix, err())
    for hh, ww in ((31, 48), (32, 47), (31, 47)):
        for pix in (32, 33 | 0x400):
            assert lib.film_stream_open(h, hh, ww, 0, 1, 1, pix) == FILM_ERR_INVALID
            assert 'pix' in err() and '4:2:0 needs even sizes' in err(), err()

    P = ctypes.c_void_p(4096)        # (never dereferenced: every call below is refused before any device call)

    def cut(pix=32, frames=P, tiles=P, B=2, H=30, W=50, align=8, bh=3, bw=2, tile0=0, ntiles=12):
        rc = lib.film_debug_yuv_cut(h, pix, frames, tiles, B, H, W, align, bh, bw, tile0, ntiles, None)
        return rc, err()

    for pix in valid:
        assert cut(pix=pix)[0] == FILM_ERR_NO_DEVICE and 'plan-only' in cut(pix=pix)[1]
    for pix in bad:
        rc, msg = cut(pix=pix)
        assert rc == FILM_ERR_INVALID and 'pix' in msg, (pix, msg)
    for kw in (dict(frames=ctypes.c_void_p(4098)), dict(frames=ctypes.c_void_p(4097)), dict(pix=33, frames=ctypes.c_void_p(4098)), dict(frames=None),
               dict(ntiles=13), dict(H=33, bh=3), dict(W=51, bw=1)):
        rc, msg = cut(**kw)
        assert rc == FILM_ERR_INVALID and msg, (kw, rc, msg)
    assert '4:2:0 needs even sizes' in cut(H=33, bh=3)[1] and '4-byte aligned' in cut(frames=ctypes.c_void_p(4098))[1]
    # film_debug_tile_map stays as it is: the 4:2:0 codes are not its business
    assert lib.film_debug_tile_map(h, 0, 32, P, P, 2, 30, 50, 8, 3, 2, 0, 12, None) == FILM_ERR_INVALID
    # film_to_yuv420 and film_frame_histogram have no handle: codes only.  A 10-bit dst holds 16-bit samples: an odd address is refused
    S = ctypes.c_void_p(4096)
    for pix in (32, 33, 33 | 0x100 | 0x400):
        assert lib.film_to_yuv420(S, ctypes.c_void_p(4097), 4, 4, pix, None) == FILM_ERR_INVALID, pix
        assert lib.film_to_yuv420(S, ctypes.c_void_p(4099), 4, 4, pix, None) == FILM_ERR_INVALID, pix
        assert lib.film_to_yuv420(None, S, 4, 4, pix, None) == FILM_ERR_INVALID and lib.film_to_yuv420(S, None, 4, 4, pix, None) == FILM_ERR_INVALID
    for hh, ww, pix in ((3, 4, 32), (4, 5, 33), (0, 4, 32), (4, -2, 33), (4, 4, 32 | 0x200), (4, 4, 33 | 0x800), (4, 4, 34)):
        assert lib.film_to_yuv420(S, S, hh, ww, pix, None) == FILM_ERR_INVALID, (hh, ww, pix)
        assert lib.film_frame_histogram(S, hh, ww, pix, S, None) == FILM_ERR_INVALID, (hh, ww, pix)
    for pix in (32, 33):
        for ptr in (4097, 4098, 4099):
            assert lib.film_frame_histogram(ctypes.c_void_p(ptr), 4, 4, pix, S, None) == FILM_ERR_INVALID, (pix, ptr)
        assert lib.film_frame_histogram(None, 4, 4, pix, S, None) == FILM_ERR_INVALID and lib.film_frame_histogram(S, 4, 4, pix, None, None) == FILM_ERR_INVALID
    # the Python layer
    with pytest.raises(FilmError) as e:
        eng.open_stream(H, W, pix='i010', matrix='bt601', full_range=True)
    assert e.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(FilmError) as e:
        eng.open_stream(31, W, pix='p010')
    assert e.value.code == FILM_ERR_INVALID and 'even' in str(e.value)
    with pytest.raises(ValueError):
        eng.open_stream(H, W, pix='p010', matrix='bt2020')
    with pytest.raises(ValueError):
        eng.open_stream(H, W, pix='p016')
    with pytest.raises(FilmError) as e:
        eng.debug_yuv_cut(4096, 4096, 2, 30, 50, 8, (3, 2), 0, 12, pix='p010', matrix='bt601')
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


def test_y4m_10bit_round_trip_and_byte_order():
    from film_hip import y4m
    frames = FMT.designed_frames(3, 30, 50, 2) & 1023
    tokens = y4m.header_tokens(50, 30, (30000, 1001), True, colour='420p10')
    assert tokens == ['W50', 'H30', 'F30000:1001', 'Ip', 'A1:1', 'C420p10', 'XCOLORRANGE=FULL']
    assert y4m.header_tokens(50, 30, (24, 1), True) == ['W50', 'H30', 'F24:1', 'Ip', 'A1:1', 'C420jpeg', 'XCOLORRANGE=FULL']       # (as before)
    data = _y4m_bytes(tokens, frames)
    assert data.startswith(b'YUV4MPEG2 W50 H30 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\nFRAME\n')
    assert len(data) == len(b'YUV4MPEG2 ' + ' '.join(tokens).encode() + b'\n') + 3 * (6 + 4500)
    r = y4m.Y4MReader(io.BytesIO(data), depths=(8, 10))
    assert (r.width, r.height, r.tokens, r.full_range, r.rate, r.frame_bytes, r.depth) == (50, 30, tokens, True, (30000, 1001), 4500, 10)
    got = list(r)
    assert len(got) == 3 and r.frames_read == 3 and all(g.dtype == np.uint16 and g.shape == (45, 50) for g in got)
    assert all(np.array_equal(g, f) for g, f in zip(got, frames))
    assert r.read_frame() is None
    # the byte order, against hand-written bytes: little-endian words, low byte first
    plain = b'YUV4MPEG2 W2 H2 F25:1 C420p10\nFRAME\n' + bytes([0x01, 0x00, 0xff, 0x03, 0x40, 0x00, 0xac, 0x03, 0x00, 0x02, 0x34, 0x02])
    r = y4m.Y4MReader(io.BytesIO(plain), depths=(8, 10))
    fr = r.read_frame()
    assert fr.dtype == np.uint16 and fr.tolist() == [[1, 1023], [64, 940], [512, 564]] and r.read_frame() is None
    assert _y4m_bytes(['W2', 'H2', 'F25:1', 'C420p10'], [fr]) == plain
    assert _y4m_bytes(['W2', 'H2', 'F25:1', 'C420p10'], [fr.astype('>u2').astype(np.uint16)]) == plain      # (whatever the array's own byte order)
    # an 8-bit stream through a reader that takes both: uint8 as always
    r = y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W2 H2 F25:1\nFRAME\n' + bytes(range(6))), depths=(8, 10))
    assert r.depth == 8 and r.frame_bytes == 6 and r.read_frame().dtype == np.uint8
    assert y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W2 H2 F25:1\nFRAME\n' + bytes(range(6)))).depth == 8
    assert y4m.double_rate(tokens) == ['W50', 'H30', 'F60000:1001'] + tokens[3:]
    # the writer refuses an array of the wrong dtype for its header, both ways
    with pytest.raises(ValueError) as e:
        y4m.Y4MWriter(io.BytesIO(), ['W2', 'H2', 'C420p10']).write(np.zeros((3, 2), np.uint8))
    assert 'uint16' in str(e.value)
    with pytest.raises(ValueError) as e:
        y4m.Y4MWriter(io.BytesIO(), ['W2', 'H2']).write(np.zeros((3, 2), np.uint16))
    assert 'uint8' in str(e.value)


def test_y4m_depths_and_refusals():
    from film_hip import y4m
    head = lambda t: io.BytesIO(f'YUV4MPEG2 W4 H2 F25:1 {t} A1:1\n'.encode() + b'FRAME\n' + bytes(64))       # noqa: E731
    for make in (lambda f: y4m.Y4MReader(f), lambda f: y4m.Y4MReader(f, depths=(8,))):      # the default reader still refuses C420p10
        with pytest.raises(y4m.Y4MError) as e:
            make(head('C420p10'))
        assert repr('C420p10') in str(e.value)
    for token in ('C420p12', 'C422p10', 'C444p10', 'C420p16', 'C422', 'C444', 'Cmono', 'It', 'Ib', 'Im'):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.Y4MReader(head(token), depths=(8, 10))
        assert repr(token) in str(e.value), token
    with pytest.raises(y4m.Y4MError) as e:
        y4m.Y4MReader(head('C420jpeg'), depths=(10,))
    assert repr('C420jpeg') in str(e.value)
    assert y4m.Y4MReader(head('C420p10'), depths=(10,)).depth == 10
    for bad in ((), (12,), (8, 16)):
        with pytest.raises(ValueError):
            y4m.Y4MReader(head('C420p10'), depths=bad)
    with pytest.raises(y4m.Y4MError) as e:
        y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W5 H2 C420p10\n'), depths=(8, 10))
    assert 'even sizes' in str(e.value)


def test_y4m_reports_truncated_10bit_frames_with_the_byte_counts():
    from film_hip import y4m
    data = _y4m_bytes(['W4', 'H2', 'F25:1', 'C420p10'], [np.arange(12, dtype=np.uint16).reshape(3, 4)] * 2)
    for cut_at, what in ((len(data) - 1, 'frame 1 has 23 of 24 bytes'), (len(data) - 13, 'frame 1 has 11 of 24 bytes'), (len(data) - 24, 'frame 1 has 0 of 24 bytes'),
                         (len(data) - 27, 'ends inside the line')):
        r = y4m.Y4MReader(io.BytesIO(data[:cut_at]), depths=(8, 10))
        assert r.read_frame() is not None
        with pytest.raises(y4m.Y4MError) as e:
            r.read_frame()
        assert 'truncated' in str(e.value) and what in str(e.value), str(e.value)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_video_cli_frame_order_and_header_on_a_10bit_stream(tmp_path, monkeypatch):
    """n frames in, 2 n - 1 out, the inputs verbatim (junk bits and all), the header back with F doubled and everything else as it was;
    the stream is opened as 'i010' for a C420p10 input and as 'i420' for an 8-bit one - through double_frame_rate and through main()."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m

    class Stream:
        def __init__(self, log): self.prev, self.log = None, log
        def __enter__(self): return self
        def __exit__(self, *exc): self.log.append('closed')
        def push(self, frame):
            mid = None if self.prev is None else ((self.prev.astype(np.int64) + frame) // 2).astype(frame.dtype)
            self.prev = frame
            return mid

    class It:
        def __init__(self, *a, **kw): self.log = []
        def open_stream(self, h, w, pix, matrix, full_range):
            self.log.append((h, w, pix, matrix, full_range))
            return Stream(self.log)

    frames = FMT.designed_frames(5, 4, 6, 1)
    tokens = ['W6', 'H4', 'F25:1', 'Ip', 'A1:1', 'C420p10', 'XCOLORRANGE=FULL', 'XYSCSS=420P10']
    data = _y4m_bytes(tokens, frames)

    def check(out_bytes):
        r = y4m.Y4MReader(io.BytesIO(out_bytes), depths=(8, 10))
        assert r.tokens == ['W6', 'H4', 'F50:1'] + tokens[3:] and r.depth == 10
        got = list(r)
        assert len(got) == 9 and all(g.dtype == np.uint16 for g in got)
        assert all(np.array_equal(got[2 * i], frames[i]) for i in range(5))
        assert all(np.array_equal(got[2 * i + 1], ((frames[i].astype(np.int64) + frames[i + 1]) // 2).astype(np.uint16)) for i in range(4))

    for override, want_full in ((None, True), (False, False)):
        it, out = It(), io.BytesIO()
        n = cli.double_frame_rate(it, y4m.Y4MReader(io.BytesIO(data), depths=(8, 10)), out, 'bt601', override)
        assert n == 9 and it.log == [(4, 6, 'i010', 'bt601', want_full), 'closed']
        check(out.getvalue())
    it, out = It(), io.BytesIO()      # an 8-bit stream goes on as before
    f8 = R.FORMATS['i420'].designed_frames(2, 4, 6, 1)
    assert cli.double_frame_rate(it, y4m.Y4MReader(io.BytesIO(_y4m_bytes(tokens[:5], f8)), depths=(8, 10)), out) == 3
    assert it.log == [(4, 6, 'i420', 'bt709', False), 'closed']
    # main() opens its reader for both depths and needs no flag
    made = []
    monkeypatch.setattr(interpolator_lib, 'Interpolator', lambda *a, **kw: made.append(It()) or made[-1])
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    assert cli.main(['--input', str(src), '--output', str(dst)]) == 9
    assert made[0].log == [(4, 6, 'i010', 'bt709', True), 'closed']
    check(dst.read_bytes())
