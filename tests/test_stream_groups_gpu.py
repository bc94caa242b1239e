"""GPU tests of tile groups in a frame stream (include/film_hip.h, "Tile groups"): a stream whose frame does not fit one invocation runs it
as G groups of n tiles through one plan of n tiles, with a carry buffer for what a pair run reads of an extracted frame.  Groups are forced
with "max_batch" on two small geometries of 64 x 64 tiles - 128 x 128 in 2 x 2 (max_batch 1, 2, 3: 4 x 1, 2 x 2, 2 x 2 tiles) and 320 x 64
in 5 x 1 (max_batch 2, 3: 2 + 2 + 1 and 3 + 2, the short last group) - and every frame of every push is compared, bit for bit, with
interpolate_frames on its float32 parents, with film_to_uint8 / film_to_yuv420 of those, and with the same stream at max_batch 0.

(No in-process "graph" = 1 cases: profiles/r06_hipgraph_crash_diagnosis.md.)
"""
import contextlib

import numpy as np
import pytest

from test_stream_recursion_gpu import F, _assert_pushes, _frames, _frames_u8, _push_all, _recursion, _yuv_scene

pytestmark = pytest.mark.gpu

ALIGN = 64
# (h, w, block_shape, max_batch) -> (tiles per group, groups)
GROUPINGS = {(128, 128, (2, 2), 1): (1, 4), (128, 128, (2, 2), 2): (2, 2), (128, 128, (2, 2), 3): (2, 2),
             (320, 64, (5, 1), 2): (2, 3), (320, 64, (5, 1), 3): (3, 2)}


@pytest.fixture(scope='module')
def published():
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    w = W.make_synthetic_weights(PUBLISHED, seed=0)
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(w)
    yield PUBLISHED, w, eng
    eng.close()


_ONE = {}


@contextlib.contextmanager
def _max_batch(eng, value):
    eng.set_option('max_batch', value)
    try:
        yield
    finally:
        eng.set_option('max_batch', 0)


def _check_layout(lay, h, w, block, mb, times):
    n, groups = GROUPINGS[(h, w, block, mb)] if mb else (block[0] * block[1], 1)
    assert (lay['tiles'], lay['groups'], lay['group_tiles'], lay['slots']) == (block[0] * block[1], groups, n, times + 1)
    assert lay['workspace_bytes'] > 0
    if groups == 1:
        assert lay['carry_bytes'] == 0 and lay['states'] == [] and lay['carry'] == []
        return
    assert len(lay['states']) == groups * (times + 1)
    floats, spans = 0, []
    for st in lay['states']:
        assert st['ntiles'] == min(n, lay['tiles'] - st['group'] * n) and st['tile0'] == st['group'] * n
        assert [s['buf'] for s in st['segments']] == lay['carry']
        for s in st['segments']:
            floats += s['floats']
            spans.append((s['carry_off'], s['carry_off'] + s['floats']))
    assert lay['carry_bytes'] == 4 * floats
    spans.sort()
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == floats    # the segments tile the carry


@pytest.mark.parametrize('graph', [2, 0])
@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('times', [1, 2, 3])
@pytest.mark.parametrize('h,w,block,mb', list(GROUPINGS))
def test_grouped_stream_is_bit_identical_to_pairs_and_to_one_group(published, h, w, block, mb, times, mem, graph):
    opt, weights, eng = published
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, ('groups', times, h, w), frames, times, ALIGN, block)
    if (times, h, w) not in _ONE:                               # the same stream at max_batch 0: once per key, shared, never written to
        _ONE[(times, h, w)] = _push_all(eng, frames, ALIGN, block, 'host', times)
    one = _ONE[(times, h, w)]
    eng.set_option('graph', graph)
    try:
        with _max_batch(eng, mb):
            got = _push_all(eng, frames, ALIGN, block, mem, times)
    finally:
        eng.set_option('graph', 2)
    got = [g if g is None or times > 1 else g[None] for g in got]
    _assert_pushes(got, want)
    for g, o in zip(got[1:], one[1:]):
        assert np.array_equal(g, o if times > 1 else o[None])
    assert len({m.tobytes() for m in want.reshape((-1,) + want.shape[2:])}) == (F - 1) * ((1 << times) - 1)   # (a stale frame would show)


@pytest.mark.parametrize('h,w,block,mb', list(GROUPINGS))
def test_layout(published, h, w, block, mb):
    from film_hip.torch_io import DeviceInterpolator
    opt, weights, eng = published
    for times in (1, 3):
        with _max_batch(eng, mb):
            with eng.open_stream(h, w, align=ALIGN, block_shape=block, times=times) as st:
                eng.set_option('max_batch', 0)                      # a later change does not touch the open stream
                _check_layout(st.layout(), h, w, block, mb, times)
        with eng.open_stream(h, w, align=ALIGN, block_shape=block, times=times) as st:
            _check_layout(st.layout(), h, w, block, 0, times)
    with _max_batch(eng, mb):
        with DeviceInterpolator(eng, align=ALIGN, block_shape=list(block)).stream(h, w) as ds:
            _check_layout(ds.layout(), h, w, block, mb, 1)


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('h,w,block,mb', [(128, 128, (2, 2), 1), (320, 64, (5, 1), 2)])
def test_grouped_u8_stream(published, h, w, block, mb, mem):
    """'u8', T = 2: film_to_uint8 (eval.util.to_uint8) of the float32 recursion on u8 / 255, and the bytes of the one-group stream."""
    from eval import util
    opt, weights, eng = published
    u8 = _frames_u8(3, h, w, seed=31)
    want = _recursion(eng, ('groups u8', h, w), u8.astype(np.float32) / 255, 2, ALIGN, block)
    one = _push_all(eng, u8, ALIGN, block, 'host', 2, pix='u8')
    with _max_batch(eng, mb):
        got = _push_all(eng, u8, ALIGN, block, mem, 2, pix='u8')
    assert got[0] is None
    for j in (1, 2):
        assert got[j].dtype == np.uint8 and got[j].shape == (3, h, w, 3)
        for k in range(3):
            assert np.array_equal(got[j][k], util.to_uint8(want[j - 1][k])), (j, k)
            assert np.array_equal(got[j][k], one[j][k]), (j, k)


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('layout,matrix,full', [('i420', 'bt709', False), ('i010', 'bt601', True)])
@pytest.mark.parametrize('h,w,block,mb', [(128, 128, (2, 2), 3), (320, 64, (5, 1), 3)])
def test_grouped_yuv_stream(published, h, w, block, mb, layout, matrix, full, mem):
    """'i420' / 'i010', T = 2: film_to_yuv420 of the float32 recursion on the frames dequantised by tests/yuv_ref.py, and the samples of the
    one-group stream."""
    import torch
    import yuv_ref
    R = yuv_ref.FORMATS[layout]
    opt, weights, eng = published
    frames = _yuv_scene(layout, 3, h, w, seed=h + w)
    x = np.stack([R.yuv_in(fr, layout, matrix, full) for fr in frames])
    ref = _recursion(eng, ('groups yuv', layout, h, w), x, 2, ALIGN, block)
    one = _push_all(eng, frames, ALIGN, block, 'host', 2, pix=layout, matrix=matrix, full_range=full)
    with _max_batch(eng, mb):
        got = _push_all(eng, frames, ALIGN, block, mem, 2, pix=layout, matrix=matrix, full_range=full)
    assert got[0] is None
    out = torch.empty((h * 3 // 2, w), dtype=torch.uint8 if layout == 'i420' else torch.int16, device='cuda')
    for j in (1, 2):
        g = got[j].view(frames.dtype) if got[j].dtype != frames.dtype else got[j]
        assert g.shape == (3, h * 3 // 2, w)
        for k in range(3):
            src = torch.from_numpy(np.array(ref[j - 1][k])).cuda()
            eng.to_yuv420_device(src.data_ptr(), out.data_ptr(), h, w, layout, matrix, full)
            torch.cuda.synchronize()
            want = out.cpu().numpy().view(frames.dtype)
            assert np.array_equal(g[k], want), (j, k)
            assert np.array_equal(g[k], one[j][k]), (j, k)


@pytest.mark.parametrize('overlap', [(16, 16), (-1, -1)])
@pytest.mark.parametrize('h,w,block,mb', [(128, 128, (2, 2), 2), (320, 64, (5, 1), 3)])
def test_grouped_stream_with_overlapped_tiles(published, h, w, block, mb, overlap):
    """align 128: a 64-pixel patch grows by its overlap (16, or the 32 its padding holds) into a 128-pixel tile; the joins of a frame add
    up in tile order over the groups, and the frames fed back are the blended ones."""
    opt, weights, eng = published
    frames = _frames(3, h, w, seed=77)
    eng.set_block_overlap(overlap)
    try:
        til = eng.tiling(h, w, align=128, block_shape=block)
        assert til['overlap_h'] == (16 if overlap[0] > 0 else 32) and til['padded_h'] == 128
        want = _recursion(eng, ('groups overlap', overlap, h, w), frames, 2, 128, block)
        with _max_batch(eng, mb):
            got = _push_all(eng, frames, 128, block, 'host', 2)
            got_dev = _push_all(eng, frames, 128, block, 'device', 2)
    finally:
        eng.set_block_overlap(0)
    plain = _recursion(eng, ('groups overlap', 0, h, w), frames, 2, 128, block)
    assert not np.array_equal(plain[0][0], want[0][0])      # (the overlap was in force, also one level down)
    _assert_pushes(got, want)
    _assert_pushes(got_dev, want)


@pytest.mark.parametrize('h,w,block,mb', [(128, 128, (2, 2), 1), (320, 64, (5, 1), 2)])
def test_grouped_selection_reset_cut_and_duplicate(published, h, w, block, mb):
    """T = 3: {6} leaves an extraction-only step (the depth-1 mid is extracted for its right child only), the empty selection only extracts;
    reset; a scene cut ('u8', a designed histogram distance); a dropped duplicate changes nothing."""
    opt, weights, eng = published
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, ('groups', 3, h, w), frames, 3, ALIGN, block)
    with _max_batch(eng, mb):
        with eng.open_stream(h, w, align=ALIGN, block_shape=block, times=3) as st:
            assert st.layout()['groups'] == GROUPINGS[(h, w, block, mb)][1]
            st.select([6])
            assert st.push(frames[0]) is None
            got = st.push(frames[1])
            assert got.shape == (1, h, w, 3) and np.array_equal(got[0], want[0][5])
            st.select([])
            assert st.push(frames[2]) is None                      # (extracted, carried)
            st.select([2, 6])
            got = st.push(frames[3])
            assert np.array_equal(got[0], want[2][1]) and np.array_equal(got[1], want[2][5])
            st.reset()
            st.select(None)
            assert st.push(frames[0]) is None
            assert np.array_equal(st.push(frames[1]), want[0])
    # a scene cut and a duplicate, against the one-group stream of the same pushes
    a, b = _frames_u8(2, h, w, seed=5), _frames_u8(2, h, w, seed=5) // 2
    seq = [a[0], a[1], a[1], b[0], b[1]]

    def run():
        try:
            with eng.open_stream(h, w, align=ALIGN, block_shape=block, pix='u8', times=2, scene_cut=250, dedup=0) as st:
                outs = []
                for fr in seq:
                    outs.append((st.push(fr), st.cut_info()[2], st.dup_info()[1]))
                return outs
        finally:
            eng.set_option('scene_cut', 0)
            eng.set_option('dup_hi', -1)

    one = run()
    with _max_batch(eng, mb):
        got = run()
    assert [(o is None, c, d) for o, c, d in got] == [(True, 0, 0), (False, 0, 0), (True, 0, 1), (True, 1, 0), (False, 0, 0)]
    for (g, _, _), (o, _, _) in zip(got, one):
        assert (g is None) == (o is None) and (g is None or np.array_equal(g, o))


def test_grouped_stream_survives_eviction_and_a_changed_overlap(published):
    """Other shapes run on the handle between pushes until the stream plan is evicted (three device plans are kept): the carry is the truth,
    nothing is extracted again.  set_block_overlap between pushes changes the tile geometry: every group is extracted again from the
    stream's copy of the frame, and the next frames are those of film_interpolate under the new overlap."""
    opt, weights, eng = published
    h, w, block, mb = 320, 64, (5, 1), 2
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, ('groups 128', 2, h, w), frames, 2, 128, block)
    other = [_frames(2, a, b, seed=a) for a, b in ((64, 64), (64, 128), (128, 64))]
    with _max_batch(eng, mb):
        with eng.open_stream(h, w, align=128, block_shape=block, times=2) as st:
            assert st.layout()['groups'] == 3
            assert st.push(frames[0]) is None
            assert np.array_equal(st.push(frames[1]), want[0])
            assert st.layout()['workspace_resident'] == 1
            for o in other:
                eng.interpolate_frames(o[:1], o[1:])
            assert st.layout()['workspace_resident'] == 0           # (evicted: three device plans are kept, the three other shapes' now)
            assert np.array_equal(st.push(frames[2]), want[1])
            assert st.layout()['workspace_resident'] == 1
            eng.set_block_overlap((16, 16))
            try:
                assert eng.tiling(h, w, align=128, block_shape=block)['overlap_h'] == 16
                faded = _recursion(eng, ('groups 128 faded', 2, h, w), frames, 2, 128, block)
                assert np.array_equal(st.push(frames[3]), faded[2])
                for o in other:
                    eng.interpolate_frames(o[:1], o[1:])
                assert st.layout()['workspace_resident'] == 0
                assert np.array_equal(st.push(frames[4]), faded[3])
            finally:
                eng.set_block_overlap(0)
            assert not np.array_equal(faded[3], want[3])
            assert np.array_equal(st.push(frames[3]), _recursion(eng, ('groups 128 back', 2, h, w), frames[[4, 3]], 2, 128, block)[0])
