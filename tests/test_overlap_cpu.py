"""CPU tests of the overlapped tiled path (options "block_overlap_h" / "block_overlap_w", film_tiling_json) WITHOUT a GPU: the geometry a
plan-only handle reports against a numpy restatement of the definition (include/film_hip.h), the option range, the refusals, the CLI
flags and TileShardedRecursion's refusal.  The restatement is this file's own, not a helper of the package."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT


def axis(n, nb, o, align):
    p = n // nb; assert n == p * nb
    pad0 = (align - p % align) % align if align else 0
    if nb == 1: o = 0
    elif o < 0: o = min(pad0 // 2, p // 2)
    assert 0 <= 2 * o <= p
    e = p + 2 * o
    E = e + ((align - e % align) % align if align else 0)
    starts = [min(max(i * p - o, 0), n - e) for i in range(nb)]
    a = np.zeros((nb, n), np.float32)
    for i, s in enumerate(starts):
        y = np.arange(s, s + e)
        d = np.full(e, 1 if nb == 1 else 1 << 30, np.int64)
        if s > 0: d = np.minimum(d, y - s + 1)
        if s + e < n: d = np.minimum(d, s + e - y)
        a[i, s:s + e] = d
    w = (a / a.sum(0, keepdims=True, dtype=np.float32)).astype(np.float32)
    return e, E, (E - e) // 2, o, starts, w          # content, padded, pad offset, resolved overlap, origins, weights


def _engine(overlap=None):
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    if overlap is not None:
        eng.set_block_overlap(overlap)
    return eng


def _want(h, w, block, overlap, align):
    eh, EH, py, oh, ys, _ = axis(h, block[0], overlap[0], align)
    ew, EW, px, ow, xs, _ = axis(w, block[1], overlap[1], align)
    return {'overlap_h': oh, 'overlap_w': ow, 'tile_h': eh, 'tile_w': ew, 'padded_h': EH, 'padded_w': EW, 'pad_y': py, 'pad_x': px,
            'origins_y': ys, 'origins_x': xs}


# (H, W, block, overlap, align, pinned values of the issue)
GEOMETRY = [
    (144, 240, (3, 3), (8, 8), 8, {}),
    (144, 240, (3, 3), (24, 40), 8, {}),
    (1080, 1920, (2, 2), (-1, -1), 64, {'overlap_h': 18, 'overlap_w': 0, 'padded_h': 576, 'padded_w': 960, 'origins_y': [0, 504], 'origins_x': [0, 960]}),
    (1080, 1920, (2, 2), (18, 32), 64, {'padded_h': 576, 'padded_w': 1024, 'origins_x': [0, 896]}),
    (2160, 3840, (4, 4), (64, 64), 64, {'tile_h': 668, 'tile_w': 1088, 'padded_h': 704, 'padded_w': 1088, 'origins_y': [0, 476, 1016, 1492]}),
    (256, 384, (1, 2), (5, 7), 64, {'overlap_h': 0, 'overlap_w': 7}),
    (270, 480, (2, 2), (-1, -1), 64, {'overlap_h': 28, 'overlap_w': 8}),
    (1080, 1920, (2, 2), (0, 0), 64, {'tile_h': 540, 'tile_w': 960, 'padded_h': 576, 'padded_w': 960, 'pad_y': 18, 'pad_x': 0}),
    (256, 384, (2, 2), (64, 96), None, {'origins_y': [0, 0], 'tile_h': 256}),     # 2 o = p: both tiles cover the axis
]


@pytest.mark.parametrize('h,w,block,overlap,align,pinned', GEOMETRY)
def test_tiling_json_equals_the_restatement(h, w, block, overlap, align, pinned):
    eng = _engine(overlap)
    got = eng.tiling(h, w, align, block)
    want = _want(h, w, block, overlap, align)
    assert got == want, (got, want)
    for k, v in pinned.items():
        assert got[k] == v, (k, got[k], v)
    assert eng.block_overlap == tuple(overlap)
    eng.close()


def test_weights_of_the_restatement_sum_to_one_and_at_most_three_tiles_cover_a_pixel():
    """Guards the restatement itself (and the kernel's candidate set k - 1, k, k + 1)."""
    for n, nb, o in ((144, 3, 8), (144, 3, 24), (240, 3, 40), (256, 2, 64), (2160, 4, 64), (2160, 4, 270)):
        e, _, _, _, starts, w = axis(n, nb, o, 8)
        assert np.abs(w.sum(0) - 1).max() < 1e-6
        cover = (w > 0).sum(0)
        assert cover.min() >= 1 and cover.max() <= 3
        p = n // nb
        for y in range(n):
            assert all(abs(i - y // p) <= 1 for i in np.nonzero(w[:, y])[0])


def test_option_range_and_refusals():
    from film_hip.engine import FilmError, FILM_ERR_INVALID
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    eng = _engine()
    for key in ('block_overlap_h', 'block_overlap_w'):
        assert f'"{key}"' in header
        for v in (-1, 65535, 0):
            eng.set_option(key, v)
        for v in (-2, 65536):
            with pytest.raises(FilmError) as e:
                eng.set_option(key, v)
            assert e.value.code == FILM_ERR_INVALID and e.value.msg.startswith(key), e.value.msg
    assert 'film_tiling_json' in header
    # 2 o > p: refused by film_tiling_json and by the compute entry that checks its arguments before the device
    eng.set_block_overlap((25, 0))
    with pytest.raises(FilmError) as e:
        eng.tiling(144, 240, 8, (3, 3))
    assert e.value.code == FILM_ERR_INVALID and e.value.msg.startswith('block_overlap_h') and '48' in e.value.msg, e.value.msg
    with pytest.raises(FilmError) as e:
        eng.interpolate_sequence(np.zeros((2, 144, 240, 3), np.float32), align=8, block_shape=(3, 3))
    assert e.value.code == FILM_ERR_INVALID and e.value.msg.startswith('block_overlap_h') and '48' in e.value.msg, e.value.msg
    assert eng.tiling(144, 240, 8, (1, 3))['overlap_h'] == 0        # one block: no overlap whatever was asked
    eng.set_block_overlap((0, 41))
    with pytest.raises(FilmError) as e:
        eng.tiling(144, 240, 8, (3, 3))
    assert e.value.msg.startswith('block_overlap_w') and '80' in e.value.msg
    # the reference's divisibility refusals stay
    with pytest.raises(FilmError) as e:
        eng.tiling(144, 240, 8, (5, 3))
    assert 'block_height=5 should evenly divide height=144.' in e.value.msg
    # buffer convention of film_plan_json
    need = ctypes.c_int64()
    eng.set_block_overlap(8)
    assert eng._lib.film_tiling_json(eng._h, 144, 240, 8, 3, 3, None, 0, ctypes.byref(need)) == 0 and need.value > 10
    small = ctypes.create_string_buffer(4)
    assert eng._lib.film_tiling_json(eng._h, 144, 240, 8, 3, 3, small, 4, ctypes.byref(need)) == FILM_ERR_INVALID
    eng.close()


def test_overlap_options_keep_the_plans():
    """No drop_plans: the plan key carries the tile size; a plan described before is the same object after."""
    eng = _engine()
    a = eng.plan(1, 64, 96)
    eng.set_block_overlap((8, 8))
    assert eng.plan(1, 64, 96) == a
    eng.close()


def test_cli_flags():
    from eval import eval_cli, interpolator_cli
    a = interpolator_cli.build_parser().parse_args(['--pattern', 'x'])
    assert a.block_overlap_height == 0 and a.block_overlap_width == 0
    a = interpolator_cli.build_parser().parse_args(['--pattern', 'x', '--block_overlap_height', '16', '--block_overlap_width', '-1'])
    assert a.block_overlap_height == 16 and a.block_overlap_width == -1
    b = eval_cli.build_parser().parse_args(['--model_path', 'm', '--triplet_dir', 't', '--output_dir', 'o', '--block_overlap_width', '32'])
    assert b.block_overlap_height == 0 and b.block_overlap_width == 32
    assert interpolator_cli.tile_mode(1, 8, 16) and not interpolator_cli.tile_mode(1, 8, 16, True)


def test_tile_sharded_recursion_refuses_overlapped_tiles():
    from film_hip.sharding import TileShardedRecursion

    class It:           # (what DeviceInterpolator(engine).batch looks like to the driver)
        def __init__(self, engine):
            self._engine = engine

        def batch(self, a, b):
            return a

    eng = _engine((16, 0))
    with pytest.raises(ValueError, match='block_overlap'):
        TileShardedRecursion(It(eng).batch, [2, 2], None)
    with pytest.raises(ValueError, match='block_overlap'):
        TileShardedRecursion(lambda a, b: a, [2, 2], None, engine=eng)
    TileShardedRecursion(It(eng).batch, [1, 2], None)       # no block rows to overlap
    eng.set_block_overlap(0)
    TileShardedRecursion(It(eng).batch, [2, 2], None)
    TileShardedRecursion(lambda a, b: a, [2, 2], None)
    eng.close()
