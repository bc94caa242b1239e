"""CPU tests of tests/tile_map_ref.py - the numpy restatement of the frame <-> tile kernels and the comparison that
tests/test_tile_map_gpu.py runs film_debug_tile_map through - and of that entry point's declaration and refusals on a plan-only handle.
No GPU: the geometry comes from film_tiling_json on a plan-only handle, the "backend" of the comparison is the restatement itself, clean
(it must pass) or with one fault planted (the comparison on the designed data must find every one of them)."""
import ctypes
import os
import re

import numpy as np
import pytest

import tile_map_ref as R
from conftest import ROOT

U = 2.0 ** -24


@pytest.fixture(scope='module')
def geos():
    """{case name: film_tiling_json of the case}, from a plan-only handle."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    out = {}
    for c in R.CASES:
        eng.set_block_overlap(c.overlap)
        out[c.name] = eng.tiling(c.H, c.W, c.align, c.block)
    eng.close()
    return out


def _frames(case, seed, scale=1.0):
    n = case.B * case.H * case.W * 3
    return (R.designed_floats(n, seed) * np.float32(scale)).astype(np.float32).reshape(case.B, case.H, case.W, 3)


# ---- the geometry and the data -----------------------------------------------------------------------------------------------------
def test_geometry_of_the_cases(geos):
    for c in R.CASES:
        assert geos[c.name] == R.expected_geometry(c), c.name
        for k, v in R.PINNED.get(c.name, {}).items():
            assert geos[c.name][k] == v, (c.name, k, geos[c.name][k], v)
    # nine tiles cover some pixel of g2; a tile row of g3 is 123 floats; together the 8-bit rows start at every byte offset mod 4
    g2 = next(c for c in R.CASES if c.name.startswith('g2'))
    cover = sum(R.covered((1, g2.H, g2.W), geos[g2.name], n, 1).astype(int) for n in range(15))
    assert cover.max() == 9 and cover.min() >= 1
    assert geos['g3-ov5x10']['padded_w'] * 3 == 123
    starts = set()
    for c in R.CASES:
        g = geos[c.name]
        starts |= {((b * c.H + y0 + r) * c.W + x0) * 3 % 4 for b in range(c.B) for y0 in g['origins_y'] for x0 in g['origins_x']
                   for r in range(g['tile_h'])}
    assert starts == {0, 1, 2, 3}


def test_designed_data():
    v = R.designed_floats(5000, 3)
    assert v.dtype == np.float32 and np.unique(v.view(np.uint32)).size == v.size
    assert np.isfinite(v).all() and (v > 0).sum() > 1000 and (v < 0).sum() > 1000
    assert (np.abs(v) > 100).sum() > 1000 and (np.abs(v) < 10).sum() > 1000 and np.abs(v).min() >= 1e-3
    u = R.designed_u8(3, 20, 22, 1)
    assert all(len(np.unique(u[i, ..., c])) == 256 for i in range(3) for c in range(3))
    assert np.array_equal(R.cut(u, {'origins_y': [0], 'origins_x': [0], 'tile_h': 20, 'tile_w': 22, 'padded_h': 20, 'padded_w': 22,
                                    'pad_y': 0, 'pad_x': 0, 'overlap_h': 0, 'overlap_w': 0}, 0, 3), u.astype(np.float32) / np.float32(255))


# every kernel instance and branch that the cases together must reach (names: tile_map_ref.branches)
ALL_BRANCHES = {
    'frame_to_tiles_kernel<false>', 'frame_to_tiles_kernel<true>', 'frame_u8_to_tiles_kernel<false>', 'frame_u8_to_tiles_kernel<true>',
    'tiles_to_frame_kernel', 'blend_tiles_kernel',
    'u8 fast path, aligned words', 'u8 fast path, shifted words', 'u8 byte path', 'u8 padding group',
    'u8 vector stores', 'u8 scalar stores, partial group', 'u8 scalar stores, unaligned group',
    'blend continues from dst', 'blend skips later tiles', 'blend one-frame row window', 'blend row window smaller than the frame',
    'blend multi-frame launch'}


def test_the_cases_reach_every_instance_and_branch(geos):
    """Which kernel instance and which of its branches the calls of tests/test_tile_map_gpu.py take, from the kernels' own conditions
    restated in tile_map_ref.branches (the tile tensor 16-byte aligned, the frames 4-byte aligned, as that test asserts).  The table goes
    to the log."""
    seen = {}
    for c in R.CASES:
        geo = geos[c.name]
        bh, bw = R.blocks(c)
        s = seen[c.name] = set()
        for ranges in R.partitions(c.B * bh * bw, bh * bw).values():
            for tile0, nt in ranges:
                for mode, u8 in (('cut', False), ('cut', True), ('join', False)):
                    s |= R.branches(c, geo, mode, u8, tile0, nt)
        print(c.name, '|', ', '.join(sorted(s)))
    union = set().union(*seen.values())
    assert union == ALL_BRANCHES, (sorted(ALL_BRANCHES - union), sorted(union - ALL_BRANCHES))
    # the paths no forward of a net with >= 3 pyramid levels can reach: a tile row that is no multiple of 12 floats
    assert {'u8 scalar stores, partial group', 'u8 scalar stores, unaligned group'} <= seen['g3-ov5x10']
    assert 'frame_u8_to_tiles_kernel<true>' in seen['g3-ov5x10'] and 'frame_u8_to_tiles_kernel<false>' in seen['g3-ov0x0']
    assert 'blend multi-frame launch' in seen['g1-ov3x5'] and 'blend continues from dst' in seen['g2-ov6x3']
    assert {'blend row window smaller than the frame', 'blend skips later tiles'} <= seen['g2-ov6x3']


# ---- properties of the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_cut_then_join_with_overlap_zero_is_the_identity(case):
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)          # (overlap 0 for EVERY geometry listed, whatever overlaps its cases carry)
    geo = eng.tiling(case.H, case.W, case.align, case.block)
    eng.close()
    assert geo['overlap_h'] == geo['overlap_w'] == 0
    bh, bw = R.blocks(case)
    total = case.B * bh * bw
    x = _frames(case, 11)
    tiles = R.cut(x, geo, 0, total)
    pad = np.ones(tiles.shape, bool)
    pad[:, geo['pad_y']:geo['pad_y'] + geo['tile_h'], geo['pad_x']:geo['pad_x'] + geo['tile_w']] = False
    assert not R.bits(tiles)[pad].any()
    back = R.join(_frames(case, 12), tiles, geo, 0, total)
    assert np.array_equal(R.bits(back), R.bits(x))


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_blending_tiles_cut_from_one_frame_gives_it_back(case, geos):
    """Within 16 x 2^-24 |v| per float: at most 4 roundings per term (two divisions, wy * wx, w * v) and weights that sum to 1 give 4 u,
    the at most 8 additions 8 u."""
    geo = geos[case.name]
    bh, bw = R.blocks(case)
    total = case.B * bh * bw
    x = (np.random.default_rng(5).standard_normal((case.B, case.H, case.W, 3)) * 1e3).astype(np.float32)
    back = R.join(_frames(case, 12), R.cut(x, geo, 0, total), geo, 0, total)
    err = np.abs(back.astype(np.float64) - x) / (U * np.abs(x.astype(np.float64)))
    print(f'{case.name}: max error {err.max():.2f} units of 2^-24 |v|')
    assert err.max() <= 16


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_joining_range_by_range_gives_the_bits_of_one_call(case, geos):
    geo = geos[case.name]
    bh, bw = R.blocks(case)
    total = case.B * bh * bw
    tiles = R.designed_floats(total * geo['padded_h'] * geo['padded_w'] * 3, 21).reshape(total, geo['padded_h'], geo['padded_w'], 3)
    bg = _frames(case, 22)
    parts = R.partitions(total, bh * bw)
    want = R.join(bg, tiles, geo, 0, total)
    ever = R.covered(bg.shape, geo, 0, total)
    assert ever.all()
    for name, ranges in parts.items():
        fr = bg
        for tile0, nt in ranges:
            nxt = R.join(fr, tiles[tile0:tile0 + nt], geo, tile0, nt)
            own = R.covered(bg.shape, geo, tile0, nt)
            assert np.array_equal(R.bits(nxt)[~own], R.bits(fr)[~own]), (name, tile0)      # only what the range covers is written
            fr = nxt
        assert np.array_equal(R.bits(fr), R.bits(want)), name
    if case.name.startswith(('g1', 'g2')):      # the ranges end in the middle of a block row; for g1 they cross into the next frame
        assert any((t0 + nt) % bw for rs in parts.values() for t0, nt in rs)
    if case.name.startswith('g1'):
        assert any(t0 // (bh * bw) != (t0 + nt - 1) // (bh * bw) and t0 % bw for rs in parts.values() for t0, nt in rs)


# ---- the comparison: the clean restatement passes, every planted fault is found ----------------------------------------------------
def test_the_restatement_passes_its_own_comparison(geos):
    backend = R.NumpyBackend(lambda c: geos[c.name])
    for c in (R.CASES[1], R.CASES[4], R.CASES[6]):          # (an identity up to the harness's own bookkeeping, which is what this checks)
        assert not list(R.check_case(backend, c, geos[c.name], twice=False)), c.name


@pytest.mark.parametrize('fault', R.FAULTS)
def test_every_planted_fault_fails_the_comparison(fault, geos):
    """The restatement with one fault planted as the backend of the comparison the GPU test runs, on the same designed data: it must be
    found in every case listed for it: those in which the fault changes what the backend does (a fault of the batch index cannot show
    with one frame, exchanged pad offsets cannot where both are 0, and so on)."""
    must = {
        'origin_not_clamped': ['g1-ov3x5', 'g2-ov6x3', 'g3-ov5x10'], 'wy_wx_exchanged': ['g1-ov3x5', 'g2-ov6x3'],
        'normalised_over_both_axes': ['g2-ov6x3'], 'sum_restarts': ['g1-ov3x5', 'g2-ov6x3', 'g4-ov7x5'],
        'padding_kept': ['g1-ov0x0', 'g5-ov1x1', 'g6-ov0x0'], 'oy_ox_exchanged': ['g1-ov0x0', 'g2-ov6x3', 'g6-ov0x0'],
        'read_one_pixel_off': ['g1-ov0x0', 'g2-ov6x3', 'g3-ov0x0', 'g6-ov0x0'], 'frame_index_dropped': ['g1-ov0x0', 'g1-ov3x5', 'g4-ov7x5', 'g6-ov0x0'],
        'u8_row_one_byte_off': ['g1-ov0x0', 'g2-ov6x3', 'g3-ov5x10', 'g6-ov0x0'], 'fma': ['g1-ov3x5', 'g2-ov6x3', 'g4-ov7x5'],
    }[fault]
    backend = R.NumpyBackend(lambda c: geos[c.name], fault)
    for c in R.CASES:
        if c.name in must:
            first = next(R.check_case(backend, c, geos[c.name], twice=False), None)
            print(fault, '->', first)
            assert first is not None, (fault, c.name)


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def test_tile_map_entry_point_is_declared_exported_and_refuses():
    from film_hip import engine
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID, FILM_ERR_NO_DEVICE
    from film_hip.options import TINY
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    assert re.search(r'^int film_debug_tile_map\(film_t\* h, int mode, int pix, void\* frames_dev, float\* tiles_dev, int B, int H, int W, '
                     r'int align, int block_h,\s+int block_w, int tile0, int ntiles, void\* stream\);', header, re.M)
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    assert re.search(r'\bfilm_debug_tile_map;', mapfile) and 'film_debug_tile_map' in engine.EXPORTED_SYMBOLS
    assert engine.load_library().film_debug_tile_map is not None
    # ONE dispatch: the five cut launchers of old are gone from csrc/, and in frame_kernels.hip only film_launch_cut_tiles launches a cut kernel
    csrc = os.path.join(ROOT, 'frame-interpolation_amd', 'csrc')
    old = ('film_launch_frame_to_tiles', 'film_launch_frame_to_tiles_overlap', 'film_launch_frame_to_tiles_u8',
           'film_launch_frame_to_tiles_overlap_u8', 'film_launch_yuv420_to_tiles')
    for name in sorted(f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f))):
        text = open(os.path.join(csrc, name)).read()
        assert not [o for o in old if re.search(r'\b' + o + r'\b', text)], name
    src = open(os.path.join(csrc, 'frame_kernels.hip')).read()
    assert src.count('hipLaunchKernelGGL(') == 1 and '<<<' not in src          # launch_units, behind the kernels, is how this file launches
    cut_kernel = r'\bframe_(?:u8_|yuv_)?to_tiles_kernel\b'
    assert not re.search(r'\bframe_(?!to_|u8_to_|yuv_to_)\w*to_tiles_kernel\b', src)          # (the three cut kernels are all there are)
    host = re.split(r'^(?=hipError_t film_launch_\w+\()', src[src.index('hipLaunchKernelGGL('):], flags=re.M)
    named = {re.match(r'hipError_t (\w+)\(', f).group(1): len(re.findall(cut_kernel, f)) for f in host[1:]}
    # float32, u8 and 4:2:0 (every layout through one helper): each named with and without overlap
    assert named == {'film_launch_cut_tiles': 2 + 2 + 2, 'film_launch_join_tiles': 0, 'film_launch_to_uint8': 0, 'film_launch_rgb_to_yuv': 0}
    assert not re.search(cut_kernel, host[0])

    eng = FilmEngine(TINY, device=-1)
    lib, h = eng._lib, eng._h
    P = ctypes.c_void_p(4096)        # (never dereferenced: every call below is refused before any device call)

    def call(mode=0, pix=0, frames=P, tiles=P, B=2, H=30, W=42, align=8, bh=3, bw=2, tile0=0, ntiles=12):
        rc = lib.film_debug_tile_map(h, mode, pix, frames, tiles, B, H, W, align, bh, bw, tile0, ntiles, None)
        return rc, lib.film_last_error(h).decode()

    assert call()[0] == FILM_ERR_NO_DEVICE and 'plan-only' in call()[1]
    assert call(mode=1)[0] == FILM_ERR_NO_DEVICE and call(pix=1)[0] == FILM_ERR_NO_DEVICE
    assert call(tile0=11, ntiles=1)[0] == FILM_ERR_NO_DEVICE
    for kw in (dict(frames=None), dict(tiles=None), dict(mode=2), dict(mode=-1), dict(pix=2), dict(pix=-1), dict(mode=1, pix=1),
               dict(ntiles=0), dict(ntiles=-3), dict(tile0=-1), dict(tile0=12, ntiles=1), dict(tile0=11, ntiles=2), dict(ntiles=13),
               dict(tile0=2 ** 31 - 1, ntiles=2 ** 31 - 1), dict(B=0), dict(H=0), dict(W=-1), dict(bh=4), dict(bw=4)):
        rc, msg = call(**kw)
        assert rc == FILM_ERR_INVALID and msg, (kw, rc, msg)
    eng.set_block_overlap((6, 0))        # 2 o > p: refused like the compute entry points
    rc, msg = call()
    assert rc == FILM_ERR_INVALID and msg.startswith('block_overlap_h')
    eng.set_block_overlap(0)
    with pytest.raises(FilmError) as e:
        eng.debug_tile_map('cut', 4096, 4096, 2, 30, 42, 8, (3, 2), 0, 12)
    assert e.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(FilmError) as e:
        eng.debug_tile_map('join', 4096, 4096, 2, 30, 42, 8, (3, 2), 0, 12, u8=True)
    assert e.value.code == FILM_ERR_INVALID
    eng.close()
