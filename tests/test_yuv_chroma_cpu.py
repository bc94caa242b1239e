"""CPU tests of the planar 4:2:2 / 4:4:4 layouts (FILM_PIX_I422 / I444 / I210 / I410) and of the BT.2020 matrix flag (FILM_YUV_BT2020,
'bt2020nc'): tests/yuv_ref.py - the numpy restatement tests/test_yuv_chroma_gpu.py compares the kernels with, bit for bit - against an
independent float64 evaluation, known answers and its own round trip; against the digests recorded from the modules it replaced; which
kernel instance and branch every GPU case reaches and that the comparisons on the designed data find each planted fault; the codes and
refusals on a plan-only handle; film_to_yuv; the Y4M reader / writer on the four new tokens; eval/video_cli.py with a stand-in interpolator.
No GPU."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import yuv_ref as R
from conftest import ROOT

NEW, OLD = R.NEW_LAYOUTS, R.OLD_LAYOUTS
COLOURS = [(m, f) for m in R.MATRICES for f in (False, True)]      # the six colour settings
FAULTS = ('chroma_row_halved', 'chroma_col_halved', 'chroma_from_tile_coordinate', 'cb_cr_swapped', 'bt709_under_bt2020', 'box_2x2_mean')


@pytest.fixture(scope='module')
def geos():
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    out = {}
    for c in list(R.CASES) + R.CASES_422 + R.CASES_444:
        eng.set_block_overlap(c.overlap)
        out[c.name] = eng.tiling(c.H, c.W, c.align, c.block)
    eng.close()
    return out


# ---- the restatement against float64 and against the 4:2:0 restatements ------------------------------------------------------------------
def _ranges(depth, full):
    s = 1 << (depth - 8)
    top = (1 << depth) - 1
    return (0, top, top, 128 * s) if full else (16 * s, 219 * s, 224 * s, 128 * s)       # y offset, y scale, c scale, c mid


def _in_f64(Y, Cb, Cr, depth, matrix, full):
    """From the definition Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)) in float64; G from the luma equation."""
    Kr, Kb = R.KR_KB[matrix]
    yo, ys, cs, mid = _ranges(depth, full)
    y, cb, cr = (Y.astype(np.float64) - yo) / ys, (Cb.astype(np.float64) - mid) / cs, (Cr.astype(np.float64) - mid) / cs
    r = y + 2 * (1 - Kr) * cr
    b = y + 2 * (1 - Kb) * cb
    g = (y - Kr * r - Kb * b) / (1 - Kr - Kb)
    return np.clip(np.stack([r, g, b], -1), 0, 1)


def _out_f64(rgb, depth, sx, sy, matrix, full):
    Kr, Kb = R.KR_KB[matrix]
    yo, ys, cs, mid = _ranges(depth, full)
    x = np.clip(rgb.astype(np.float64), 0, 1)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = Kr * r + (1 - Kr - Kb) * g + Kb * b
    box = lambda c: c.reshape(c.shape[0] >> sy, 1 << sy, c.shape[1] >> sx, 1 << sx).mean((1, 3))       # noqa: E731
    return y * ys + yo, box((b - y) / (2 * (1 - Kb))) * cs + mid, box((r - y) / (2 * (1 - Kr))) * cs + mid


@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('matrix,full', COLOURS)
def test_in_against_float64(matrix, full, depth):
    """Every (Y, Cb, Cr) triple of a 64-step grid plus the extremes: at most 1e-6 apart - five float32 roundings on magnitudes below 2
    (BT.2020's largest coefficient is 1.8814)."""
    s = 1 << (depth - 8)
    ext = np.array([1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255]) * s
    v = np.unique(np.concatenate([np.arange(0, 256 * s, 4 * s), ext, [256 * s - 1]]))
    Y, Cb, Cr = np.meshgrid(v, v, v, indexing='ij')
    got = R.FORMATS['i444' if depth == 8 else 'i410'].samples_to_rgb(Y, Cb, Cr, matrix, full)
    err = np.abs(got.astype(np.float64) - _in_f64(Y, Cb, Cr, depth, matrix, full)).max()
    print(f'{depth}-bit {matrix} full={full}: in, max |float32 - float64| = {err:.3g}')
    assert err <= 1e-6
    assert max(float(c) for c in R.constants('bt2020nc').values()) < 1.8815


@pytest.mark.parametrize('layout', NEW)
@pytest.mark.parametrize('matrix,full', COLOURS)
def test_out_against_float64(matrix, full, layout):
    """The bound of tests/test_yuv_cpu.py's test_out_against_float64: equal codes wherever the float64 value is farther than 1e-4 of an 8-bit
    code from a rounding tie, at most one code apart elsewhere, at most 1 % of the values so excused.  A 10-bit code is a quarter of an 8-bit
    one, and the float32 error before the quantiser is relative to the value (three roundings of a value below 1024): the same 1e-4 of an
    8-bit code is 4e-4 of a 10-bit one."""
    f = R.FORMATS[layout]
    rgb = np.random.default_rng(7).uniform(-0.1, 1.1, (120, 160, 3)).astype(np.float32)
    got = f.unpack(f.yuv_out(rgb, layout, matrix, full), layout)
    tie, top = 1e-4 * (1 << (f.depth - 8)), (1 << f.depth) - 1
    near_all = n_all = 0
    for name, g, v32, v64 in zip('Y Cb Cr'.split(), got, f.out_unquantised(rgb, matrix, full), _out_f64(rgb, f.depth, f.sx, f.sy, matrix, full)):
        v64 = np.clip(v64, 0, top)
        want = np.floor(v64 + 0.5)
        near = np.abs(v64 - (np.floor(v64) + 0.5)) <= tie
        diff = np.abs(f.code(g, layout).astype(np.int64) - want.astype(np.int64))
        print(f'{layout} {matrix} full={full} {name}: max |float32 - float64| before q = {np.abs(v32 - v64).max():.3g} codes, '
              f'{near.sum()} of {near.size} within {tie:g} of a tie, {int((diff > 0).sum())} codes differ')
        assert g.shape == v64.shape and not diff[~near].any() and diff.max() <= 1
        near_all += int(near.sum()); n_all += near.size
    assert near_all <= 0.01 * n_all


def test_the_restatement_computes_what_the_recorded_digests_say():
    """tests/golden/yuv_ref_digests.json was written from the three reference modules that tests/yuv_ref.py replaced: the designed frames, in,
    out, histogram, the cut with and without every planted fault and the branch names of all ten layouts - the 4:2:0 ones both with their own
    designed frames and colour settings and as the (SX, SY) = (1, 1) instance of the general statement - are still those, digest for digest."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('make_yuv_ref_golden', os.path.join(ROOT, 'tools', 'make_yuv_ref_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want, got = json.load(open(tool.PATH)), tool.digests()
    assert len(want) > 600 and sorted(got) == sorted(want)
    assert got == want, sorted(k for k in want if got[k] != want[k])[:12]


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------
def _solid(layout, y, cb, cr):
    f = R.FORMATS[layout]
    h, w = 2, 2
    ch, cw = f.chroma_shape(h, w)
    return f.pack(f.store(np.full((h, w), y), layout), f.store(np.full((ch, cw), cb), layout), f.store(np.full((ch, cw), cr), layout), layout)


@pytest.mark.parametrize('layout', NEW + ('i420', 'p010'))
def test_known_answers(layout):
    """Black and white exact in both ranges, all three matrices; the BT.2020 limited-range 100 % primaries, computed from the definition in
    float64, met within one code."""
    f = R.FORMATS[layout]
    s = 1 << (f.depth - 8)
    top = (1 << f.depth) - 1
    for matrix in R.MATRICES:
        assert not f.yuv_in(_solid(layout, 16 * s, 128 * s, 128 * s), layout, matrix, False).any()
        assert (f.yuv_in(_solid(layout, 235 * s, 128 * s, 128 * s), layout, matrix, False) == 1).all()
        assert not f.yuv_in(_solid(layout, 0, 128 * s, 128 * s), layout, matrix, True).any()
        assert (f.yuv_in(_solid(layout, top, 128 * s, 128 * s), layout, matrix, True) == 1).all()
        for rgb, codes, full in (((0, 0, 0), (16 * s, 128 * s, 128 * s), False), ((1, 1, 1), (235 * s, 128 * s, 128 * s), False),
                                 ((0, 0, 0), (0, 128 * s, 128 * s), True), ((1, 1, 1), (top, 128 * s, 128 * s), True)):
            fr = f.yuv_out(np.broadcast_to(np.array(rgb, np.float32), (2, 2, 3)), layout, matrix, full)
            assert [int(f.code(p, layout).ravel()[0]) for p in f.unpack(fr, layout)] == list(codes), (matrix, rgb, full)
    table = {8: {(1, 0, 0): (73.53, 96.72, 240), (0, 1, 0): (164.48, 47.28, 25.01), (0, 0, 1): (28.99, 240, 118.99)},
             10: {(1, 0, 0): (294.1, 386.9, 960), (0, 1, 0): (657.9, 189.1, 100.0), (0, 0, 1): (115.9, 960, 476.0)}}[f.depth]
    for rgb, want in table.items():
        fr = f.yuv_out(np.broadcast_to(np.array(rgb, np.float32), (2, 2, 3)), layout, 'bt2020nc', False)
        got = [int(f.code(p, layout).ravel()[0]) for p in f.unpack(fr, layout)]
        assert all(abs(g - w) <= 1 for g, w in zip(got, want)), (layout, rgb, got, want)


# ---- round trip -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', NEW + OLD)
def test_in_gamut_round_trip_is_the_identity(layout):
    """480 x 960 random frames, Y codes 50 .. 205 and chroma codes 100 .. 156 at 8 bits (times 4 at 10 bits): every block (2 x 2, 1 x 2 or
    one pixel) whose decoded pixels stay strictly inside the gamut returns code for code, and more than half of the blocks are inside.  The
    new layouts with all six colour settings, the older four with 'bt2020nc'."""
    f = R.FORMATS[layout]
    s = 1 << (f.depth - 8)
    h, w = 480, 960
    ch, cw = f.chroma_shape(h, w)
    rng = np.random.default_rng(3)
    fr = f.pack(f.store(rng.integers(50 * s, 206 * s, (h, w)), layout), f.store(rng.integers(100 * s, 157 * s, (ch, cw)), layout),
                f.store(rng.integers(100 * s, 157 * s, (ch, cw)), layout), layout)
    fr = f.with_junk(fr, layout, 4)
    for matrix, full in (COLOURS if layout in NEW else [('bt2020nc', False), ('bt2020nc', True)]):
        rgb = f.yuv_in(fr, layout, matrix, full)
        inside = ((rgb > 0) & (rgb < 1)).all(-1)
        block = inside.reshape(ch, 1 << f.sy, cw, 1 << f.sx).all((1, 3))
        print(f'{layout} {matrix} full={full}: {block.mean():.3f} of the blocks inside the gamut')
        assert block.mean() > 0.5
        back = f.yuv_out(rgb, layout, matrix, full)
        Y0, Cb0, Cr0 = (f.code(p, layout) for p in f.unpack(fr, layout))
        Y1, Cb1, Cr1 = (f.code(p, layout) for p in f.unpack(back, layout))
        assert np.array_equal(back, f.store(f.code(back, layout), layout))      # the ignored bits come back as zero
        pix = block.repeat(1 << f.sy, 0).repeat(1 << f.sx, 1)
        assert np.array_equal(Y1[pix], Y0[pix]) and np.array_equal(Cb1[block], Cb0[block]) and np.array_equal(Cr1[block], Cr0[block])


# ---- which kernel instances and branches the GPU cases reach -----------------------------------------------------------------------------------
def test_the_cases_reach_every_instance_and_branch(geos):
    """From the kernels' own conditions restated in yuv_ref.Format.branches / out_branches: the calls of tests/test_yuv_chroma_gpu.py reach both
    cut instances and the quantiser instance of every new layout and every branch of theirs - chroma from row fy, four chroma samples per
    group, an odd block row, an odd pixel count per row, a frame of a batch that starts off a word boundary among them.  The table goes to the log."""
    for layout in NEW:
        f = R.FORMATS[layout]
        seen = {}
        for c in R.cases_of(layout):
            s = seen[c.name] = set()
            for ranges in R.ranges_of(c, geos[c.name]).values():
                for tile0, nt in ranges:
                    s |= f.branches(c, geos[c.name], layout, tile0, nt)
            print(layout, c.name, '|', ', '.join(sorted(s)))
        union = set().union(*seen.values())
        L = f'FILM_PIX_{layout.upper()}'
        word = 'byte' if f.depth == 8 else 'sample'
        y_words = {8: ['one word', 'two words'], 10: ['two words', 'three words']}[f.depth]
        want = {f'frame_yuv_to_tiles_kernel<false, {L}>', f'frame_yuv_to_tiles_kernel<true, {L}>', 'odd row origin', 'odd column origin', 'padding group',
                f'{word} path', 'vector stores', 'scalar stores'} | {f'word path, Y in {n}' for n in y_words}
        if f.sx:
            want |= {'chroma from row fy (an odd row)', 'word path, odd column: three chroma samples', 'word path, even column: two chroma samples',
                     'word path, chroma in one word', 'word path, chroma in two words'}
        else:
            want |= {'word path, four chroma samples', 'frame starts off a word boundary'} | {f'word path, chroma in {n}' for n in y_words}
        assert union == want, (layout, sorted(want - union), sorted(union - want))
        if f.sx:
            assert 'chroma from row fy (an odd row)' in seen['s2-33x50-b3x2'] and 'odd row origin' in seen['s2-33x50-b3x2']
            assert not any(b.startswith('word path') for b in seen['s1-1x2'])
        else:
            assert 'frame starts off a word boundary' in seen['f2-33x51-b3x3'] and not any(b.startswith('word path') for b in seen['f1-1x1'])
        out = {}
        for h, w in R.out_sizes(layout):
            out[h, w] = set().union(*[f.out_branches(h, w, layout, o * f.dtype.itemsize) for o in R.OUT_OFFSETS])
            print(f'{layout} {h}x{w} |', ', '.join(sorted(out[h, w])))
        want = {f'rgb_to_yuv_kernel<{L}>', 'block of two rows', 'odd block row: one row', 'vector loads', 'scalar loads', 'Y word stores', f'Y {word} stores',
                'chroma word stores', f'chroma {word} stores'} | (set() if f.sx else {'odd pixel count per row'})
        union = set().union(*out.values())
        assert union == want, (layout, sorted(want - union), sorted(union - want))
        assert 'odd block row: one row' in out[31, 50] and (f.sx or 'odd pixel count per row' in out[31, 49])


def test_the_restatement_passes_its_own_comparison(geos):
    backend = {layout: R.FORMATS[layout].NumpyBackend(lambda c: geos[c.name]) for layout in NEW}
    for layout in NEW:
        f = R.FORMATS[layout]
        for i, c in enumerate(R.cases_of(layout)):
            matrix, full = COLOURS[i % 6]
            for ranges in R.ranges_of(c, geos[c.name]).values():
                assert not list(f.check_cut(backend[layout], c, geos[c.name], layout, matrix, full, ranges, twice=False)), (layout, c.name)
                fr = f.frames_view(f.new_frames_alloc(c, layout, 1), c)
                r0 = ranges[0]
                assert np.array_equal(f.cut(fr, geos[c.name], r0[0], r0[1], layout, matrix, full).view(np.uint32),
                                      f.cut_via_frames(fr, geos[c.name], r0[0], r0[1], layout, matrix, full).view(np.uint32))


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_fails_the_comparison(fault, geos):
    """The restatement with one fault planted, in the comparison the GPU test runs on the same designed data: found in every case in which
    the fault changes what is computed (a wrong chroma row needs more than one row; the pairing cannot go wrong from an even origin - and
    with (SX, SY) = (0, 0) not at all)."""
    if fault == 'box_2x2_mean':      # a fault of the way out: the comparison of the film_to_yuv test
        for layout in ('i422', 'i210'):
            f = R.FORMATS[layout]
            for h, w in [(2, 2), (16, 18), (30, 50)]:
                src = R.designed_rgb(h, w, seed=h + w)
                for matrix, full in COLOURS:
                    assert not np.array_equal(f.yuv_out(src, layout, matrix, full, fault), f.yuv_out(src, layout, matrix, full)), (layout, h, w)
        return
    layouts = {'chroma_row_halved': ('i422', 'i210'), 'chroma_col_halved': ('i444', 'i410')}.get(fault, NEW)
    for layout in layouts:
        f = R.FORMATS[layout]
        names = [c.name for c in R.cases_of(layout)]
        must = {'chroma_row_halved': [n for n in names if n != 's1-1x2'],
                'chroma_col_halved': [n for n in names if n != 'f1-1x1'],
                'cb_cr_swapped': names, 'bt709_under_bt2020': names,
                'chroma_from_tile_coordinate': ['y1-30x50-b3x2', 'y2-30x50-b3x2-ov3x5', 'y6-12x22-b1x2-noalign', 's2-33x50-b3x2', 's3-33x50-b3x2-ov3x5'] if f.sx else []}[fault]
        backend = f.NumpyBackend(lambda c: geos[c.name], fault)
        for c in R.cases_of(layout):
            if c.name in must:
                ranges = R.ranges_of(c, geos[c.name])['one']
                first = next(f.check_cut(backend, c, geos[c.name], layout, 'bt2020nc', False, ranges, seed=17, twice=False), None)
                print(fault, layout, c.name, '->', first)
                assert first is not None, (fault, c.name, layout)
    if fault == 'bt709_under_bt2020':      # ... and under the other flags nothing changes
        f, c = R.FORMATS['i444'], R.CASES[0]
        backend = f.NumpyBackend(lambda c: geos[c.name], fault)
        assert not list(f.check_cut(backend, c, geos[c.name], 'i444', 'bt601', False, R.ranges_of(c, geos[c.name])['one'], twice=False))


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------
def test_pixel_codes_and_refusals():
    from film_hip import engine
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID, FILM_ERR_NO_DEVICE
    from film_hip.options import TINY
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    codes = {'FILM_PIX_I422': 20, 'FILM_PIX_I444': 24, 'FILM_PIX_I210': 36, 'FILM_PIX_I410': 40}
    for name, val in codes.items():
        assert re.search(rf'^#define {name}\s+{val}\b', header, re.M), name
        assert getattr(engine, name) == val
    assert re.search(r'^#define FILM_YUV_BT2020\s+0x2000\b', header, re.M) and engine.FILM_YUV_BT2020 == 0x2000
    assert 'The 4:2:2 and 4:4:4 arithmetic' in header
    assert engine.pix_code('i210', 'bt2020nc', True) == 36 | 0x2000 | 0x400 and engine.pix_code('i420', 'bt2020nc') == 16 | 0x2000
    assert [engine.PIX[n][1] for n in NEW] == [np.uint8, np.uint8, np.uint16, np.uint16]
    assert [engine.frame_shape(n, 5, 6) for n in ('i422', 'i444', 'i210', 'i410', 'u8')] == [(10, 6), (15, 6), (10, 6), (15, 6), (5, 6, 3)]
    # film_to_yuv: declared, exported, listed
    assert re.search(r'^int film_to_yuv\(const float\* src, void\* dst, int H, int W, int pix, void\* stream\);', header, re.M)
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    assert re.search(r'\bfilm_to_yuv;', mapfile) and 'film_to_yuv' in engine.EXPORTED_SYMBOLS
    assert set(re.findall(r'\b(film_\w+);', mapfile)) == set(engine.EXPORTED_SYMBOLS)
    lib = engine.load_library()
    assert lib.film_to_yuv is not None

    eng = FilmEngine(TINY, device=-1)
    h = eng._h
    err = lambda: lib.film_last_error(h).decode()       # noqa: E731
    colours = [m | f for m in (0, 0x100, 0x2000) for f in (0, 0x400)]
    valid = [lay | c for lay in codes.values() for c in colours] + [lay | c for lay in (16, 17, 32, 33) for c in (0x2000, 0x2400)]
    for pix in valid:
        assert lib.film_stream_open(h, 32, 48, 0, 1, 1, pix) == FILM_ERR_NO_DEVICE, pix
        assert lib.film_stream_open(h, 32, 48, 8, 2, 2, pix) == FILM_ERR_NO_DEVICE, pix
    for pix in (20, 36 | 0x400):      # 4:2:2: an odd H is fine, an odd W is not
        assert lib.film_stream_open(h, 33, 48, 0, 1, 1, pix) == FILM_ERR_NO_DEVICE
        for hh, ww in ((32, 47), (33, 47)):
            assert lib.film_stream_open(h, hh, ww, 0, 1, 1, pix) == FILM_ERR_INVALID
            assert 'pix' in err() and '4:2:2 needs an even width' in err(), err()
    for pix in (24, 40 | 0x2000):     # 4:4:4: any size
        for hh, ww in ((33, 48), (32, 47), (33, 47), (1, 1)):
            assert lib.film_stream_open(h, hh, ww, 0, 1, 1, pix) == FILM_ERR_NO_DEVICE, (pix, hh, ww)
    for pix in (16 | 0x2000, 33 | 0x2000):      # 4:2:0 as before
        for hh, ww in ((31, 48), (32, 47)):
            assert lib.film_stream_open(h, hh, ww, 0, 1, 1, pix) == FILM_ERR_INVALID
            assert 'pix' in err() and '4:2:0 needs even sizes' in err(), err()
    bad = [lay | 0x100 | 0x2000 for lay in (16, 20, 24, 33, 36, 40)] + [20 | 0x200, 24 | 0x800, 36 | 0x1000, 40 | (1 << 30), 0x2000, 1 | 0x2000, 21, 25, 37, 41, 28, 44]
    for pix in bad:
        assert lib.film_stream_open(h, 32, 48, 0, 1, 1, pix) == FILM_ERR_INVALID and 'pix' in err(), (pix, err())

    P = ctypes.c_void_p(4096)        # (never dereferenced: every call below is refused before any device call)

    def cut(pix=20, frames=P, tiles=P, B=2, H=33, W=50, align=8, bh=3, bw=2, tile0=0, ntiles=12):
        rc = lib.film_debug_yuv_cut(h, pix, frames, tiles, B, H, W, align, bh, bw, tile0, ntiles, None)
        return rc, err()

    for pix in valid:
        rc, msg = cut(pix=pix, H=30)
        assert rc == FILM_ERR_NO_DEVICE and 'plan-only' in msg, (pix, msg)
    assert cut(pix=20)[0] == FILM_ERR_NO_DEVICE and cut(pix=40, W=51, bw=3, ntiles=18)[0] == FILM_ERR_NO_DEVICE
    for pix in bad:
        rc, msg = cut(pix=pix, H=30)
        assert rc == FILM_ERR_INVALID and 'pix' in msg, (pix, msg)
    assert '4:2:2 needs an even width' in cut(pix=36, W=51, bw=1)[1] and '4:2:0 needs even sizes' in cut(pix=16 | 0x2000)[1]
    assert '4-byte aligned' in cut(frames=ctypes.c_void_p(4098))[1] and cut(pix=24, frames=ctypes.c_void_p(4097))[0] == FILM_ERR_INVALID
    # film_to_yuv / film_to_yuv420 / film_frame_histogram have no handle: codes only
    S = ctypes.c_void_p(4096)
    for pix in valid:
        assert lib.film_to_yuv(None, S, 4, 4, pix, None) == FILM_ERR_INVALID and lib.film_to_yuv(S, None, 4, 4, pix, None) == FILM_ERR_INVALID
        for hh, ww in ((0, 4), (4, 0), (-1, 4)):
            assert lib.film_to_yuv(S, S, hh, ww, pix, None) == FILM_ERR_INVALID
            assert lib.film_frame_histogram(S, hh, ww, pix, S, None) == FILM_ERR_INVALID
    for pix in (36, 40, 40 | 0x2000, 32 | 0x2000):      # a 10-bit dst holds 16-bit samples
        assert lib.film_to_yuv(S, ctypes.c_void_p(4097), 4, 4, pix, None) == FILM_ERR_INVALID
    for pix in (0, 1, 2, 21, 48, 20 | 0x200, 24 | 0x100 | 0x2000):
        assert lib.film_to_yuv(S, S, 4, 4, pix, None) == FILM_ERR_INVALID, pix
    for hh, ww, pix in ((4, 5, 20), (3, 5, 36), (3, 4, 16 | 0x2000), (4, 5, 33)):
        assert lib.film_to_yuv(S, S, hh, ww, pix, None) == FILM_ERR_INVALID, (hh, ww, pix)
        assert lib.film_frame_histogram(S, hh, ww, pix, S, None) == FILM_ERR_INVALID, (hh, ww, pix)
    for pix in list(codes.values()) + [20 | 0x2000, 40 | 0x400]:      # film_to_yuv420 stays with the 4:2:0 layouts
        assert lib.film_to_yuv420(S, S, 4, 4, pix, None) == FILM_ERR_INVALID, pix
    for pix in codes.values():
        assert lib.film_frame_histogram(ctypes.c_void_p(4098), 4, 4, pix, S, None) == FILM_ERR_INVALID
        assert lib.film_frame_histogram(None, 4, 4, pix, S, None) == FILM_ERR_INVALID and lib.film_frame_histogram(S, 4, 4, pix, None, None) == FILM_ERR_INVALID
    # the Python layer
    for pix in NEW:
        with pytest.raises(FilmError) as e:
            eng.open_stream(32, 48, pix=pix, matrix='bt2020nc', full_range=True)
        assert e.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(FilmError) as e:
        eng.open_stream(32, 47, pix='i210')
    assert e.value.code == FILM_ERR_INVALID and '4:2:2 needs an even width' in str(e.value)
    for kw in (dict(pix='i444', matrix='bt2020'), dict(pix='yv12'), dict(pix='p016'), dict(pix='i412')):
        with pytest.raises(ValueError):
            eng.open_stream(32, 48, **kw)
    with pytest.raises(FilmError) as e:
        eng.debug_yuv_cut(4096, 4096, 2, 33, 51, 8, (3, 3), 0, 18, pix='i410', matrix='bt2020nc')
    assert e.value.code == FILM_ERR_NO_DEVICE
    assert hasattr(eng, 'to_yuv_device')
    eng.close()


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------------------------
ALL = dict(depths=(8, 10), chroma=('420', '422', '444'))
TOKENS = {'422': 'i422', '444': 'i444', '422p10': 'i210', '444p10': 'i410'}


def _y4m_bytes(tokens, frames):
    from film_hip import y4m
    f = io.BytesIO()
    w = y4m.Y4MWriter(f, tokens)
    for fr in frames:
        w.write(fr)
    return f.getvalue()


@pytest.mark.parametrize('colour', list(TOKENS))
def test_y4m_round_trip_and_byte_counts(colour):
    from film_hip import y4m
    layout = TOKENS[colour]
    f = R.FORMATS[layout]
    H, W = 31, 50 if f.sx else 49
    frames = [f.store(f.code(fr, layout), layout) for fr in f.designed_frames(3, H, W, 2, layout)]
    tokens = y4m.header_tokens(W, H, (30000, 1001), True, colour=colour)
    assert tokens == [f'W{W}', f'H{H}', 'F30000:1001', 'Ip', 'A1:1', f'C{colour}', 'XCOLORRANGE=FULL']
    data = _y4m_bytes(tokens, frames)
    per = (2 if f.sx else 3) * H * W * (2 if f.depth == 10 else 1)
    assert len(data) == len(b'YUV4MPEG2 ' + ' '.join(tokens).encode() + b'\n') + 3 * (6 + per)
    r = y4m.Y4MReader(io.BytesIO(data), **ALL)
    assert (r.width, r.height, r.tokens, r.full_range, r.frame_bytes, r.depth, r.chroma, r.pix) == (W, H, tokens, True, per, f.depth, colour[:3], layout)
    got = list(r)
    assert len(got) == 3 and all(g.dtype == f.dtype and g.shape == (f.rows(H), W) for g in got) and all(np.array_equal(g, x) for g, x in zip(got, frames))
    only = y4m.Y4MReader(io.BytesIO(data), depths=(f.depth,), chroma=(colour[:3],))
    assert only.pix == layout and np.array_equal(only.read_frame(), frames[0])
    # a reader that was not asked keeps refusing, with the token in the message
    for kw in ({}, dict(depths=(8, 10)), dict(depths=(8, 10), chroma=('420',)), dict(depths=(8, 10), chroma=tuple(c for c in ('420', '422', '444') if c != colour[:3]))):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.Y4MReader(io.BytesIO(data), **kw)
        assert repr('C' + colour) in str(e.value), kw
    if f.depth == 10:
        with pytest.raises(y4m.Y4MError) as e:
            y4m.Y4MReader(io.BytesIO(data), depths=(8,), chroma=('420', '422', '444'))
        assert repr('C' + colour) in str(e.value)
    # truncated frames report their byte counts
    for cut_at, what in ((len(data) - 1, f'frame 2 has {per - 1} of {per} bytes'), (len(data) - per, f'frame 2 has 0 of {per} bytes')):
        r = y4m.Y4MReader(io.BytesIO(data[:cut_at]), **ALL)
        assert r.read_frame() is not None and r.read_frame() is not None
        with pytest.raises(y4m.Y4MError) as e:
            r.read_frame()
        assert 'truncated' in str(e.value) and what in str(e.value), str(e.value)


def test_y4m_byte_order_and_refusals():
    from film_hip import y4m
    # little-endian words, low byte first: Y 1 1023, Cb 64, Cr 940 of a 1 x 2 4:2:2 frame
    plain = b'YUV4MPEG2 W2 H1 F25:1 C422p10\nFRAME\n' + bytes([0x01, 0x00, 0xff, 0x03, 0x40, 0x00, 0xac, 0x03])
    r = y4m.Y4MReader(io.BytesIO(plain), **ALL)
    fr = r.read_frame()
    assert fr.dtype == np.uint16 and fr.tolist() == [[1, 1023], [64, 940]] and r.read_frame() is None and r.pix == 'i210'
    assert _y4m_bytes(['W2', 'H1', 'F25:1', 'C422p10'], [fr]) == plain
    r = y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W1 H1 C444\nFRAME\n' + bytes([9, 8, 7])), **ALL)
    assert r.read_frame().tolist() == [[9], [8], [7]] and r.pix == 'i444'
    head = lambda t: io.BytesIO(f'YUV4MPEG2 W4 H2 F25:1 {t} A1:1\n'.encode() + b'FRAME\n' + bytes(64))       # noqa: E731
    for token in ('C444alpha', 'Cmono', 'C411', 'C420p12', 'C422p12', 'C444p16', 'C422p16', 'It', 'Ib', 'Im'):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.Y4MReader(head(token), **ALL)
        assert repr(token) in str(e.value), token
    r = y4m.Y4MReader(head('C420jpeg'), **ALL)
    assert (r.chroma, r.pix, r.depth) == ('420', 'i420', 8) and y4m.Y4MReader(head('C420p10'), **ALL).pix == 'i010'
    with pytest.raises(y4m.Y4MError) as e:
        y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W5 H2 C422\n'), **ALL)
    assert 'even width' in str(e.value)
    assert y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H3 C422\n'), **ALL).frame_bytes == 24      # an odd H is fine
    assert y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W5 H3 C444p10\n'), **ALL).frame_bytes == 90
    for bad in ((), ('411',), ('420', '440')):
        with pytest.raises(ValueError):
            y4m.Y4MReader(head('C422'), chroma=bad)
    with pytest.raises(ValueError) as e:
        y4m.Y4MWriter(io.BytesIO(), ['W2', 'H2', 'C444']).write(np.zeros((3, 2), np.uint8))
    assert '(6, 2)' in str(e.value)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------
def test_video_cli_frame_order_and_header_on_a_422p10_stream(tmp_path, monkeypatch):
    """n frames in, 2 n - 1 out, the inputs verbatim, the header back with F doubled; the stream is opened as 'i210' for a C422p10 input with
    --chroma any, and without it the file is refused before the model is loaded."""
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

    f = R.FORMATS['i210']
    frames = f.designed_frames(5, 3, 6, 1, 'i210')
    tokens = ['W6', 'H3', 'F25:1', 'Ip', 'A1:1', 'C422p10', 'XCOLORRANGE=FULL']
    data = _y4m_bytes(tokens, frames)
    made = []
    monkeypatch.setattr(interpolator_lib, 'Interpolator', lambda *a, **kw: made.append(It()) or made[-1])
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    with pytest.raises(y4m.Y4MError) as e:
        cli.main(['--input', str(src), '--output', str(dst)])
    assert repr('C422p10') in str(e.value) and not made and not dst.exists()
    with pytest.raises(SystemExit):
        cli.main(['--input', str(src), '--output', str(dst), '--chroma', 'any', '--matrix', 'bt2020'])
    assert not made
    assert cli.main(['--input', str(src), '--output', str(dst), '--chroma', 'any', '--matrix', 'bt2020nc']) == 9
    assert made[0].log == [(3, 6, 'i210', 'bt2020nc', True), 'closed']
    r = y4m.Y4MReader(io.BytesIO(dst.read_bytes()), **ALL)
    assert r.tokens == ['W6', 'H3', 'F50:1'] + tokens[3:] and (r.depth, r.chroma) == (10, '422')
    got = list(r)
    assert len(got) == 9 and all(g.dtype == np.uint16 and g.shape == (6, 6) for g in got)
    assert all(np.array_equal(got[2 * i], frames[i]) for i in range(5))
    assert all(np.array_equal(got[2 * i + 1], ((frames[i].astype(np.int64) + frames[i + 1]) // 2).astype(np.uint16)) for i in range(4))
    # a 4:2:0 file goes on as before, --chroma any or not
    f8 = R.FORMATS['i420'].designed_frames(2, 4, 6, 1)
    src.write_bytes(_y4m_bytes(['W6', 'H4', 'F25:1', 'Ip', 'A1:1'], f8))
    assert cli.main(['--input', str(src), '--output', str(dst), '--chroma', 'any']) == 3 and made[1].log == [(4, 6, 'i420', 'bt709', False), 'closed']
