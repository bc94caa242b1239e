"""GPU tests of recursive mid-frames in a frame stream (engine option "stream_times" = T): a primed push writes the 2^T - 1 frames of the
times_to_interpolate recursion, every one bit-identical to film_interpolate on its two float32 parents - from host and device memory,
on both executors, tiled, padded, with overlapped tiles, with 8-bit and 4:2:0 frames - and the stream's state: other calls between
pushes, reset, scene cuts, the option changing under an open stream, the error path, the profile, eval.video_cli.

(No in-process "graph" = 1 cases: profiles/r06_hipgraph_crash_diagnosis.md.)
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 5    # frames per case: both input slots receive a frame twice


def _frames(f, h, w, seed):
    """f frames of a scene moving by (2, -3) px per frame (+ noise), float32 [f, h, w, 3]."""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3), dtype=np.float32)
    out = [np.roll(base, (2 * i, -3 * i), axis=(0, 1)) + rng.normal(0, 0.01, base.shape).astype(np.float32) for i in range(f)]
    return np.stack(out).astype(np.float32)


def _frames_u8(f, h, w, seed):
    """f uint8 frames of a scene moving by (2, -3) px per frame: a permutation of the same bytes, frame after frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.stack([np.roll(base, (2 * i, -3 * i), axis=(0, 1)) for i in range(f)])


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


_WANT = {}


def _recursion(eng, key, frames, times, align, block):
    """[f - 1, 2^T - 1, h, w, 3]: the recursion built level by level with interpolate_frames on the parents (float32 all the way),
    under the engine's current options.  Computed once per key, shared, never written to."""
    if key not in _WANT:
        seq = [f for f in frames]
        for _ in range(times):
            mids = eng.interpolate_frames(np.stack(seq[:-1]), np.stack(seq[1:]), align=align, block_shape=block)
            nxt = []
            for a, m in zip(seq[:-1], mids):
                nxt += [a, m]
            seq = nxt + [seq[-1]]
        n = 1 << times
        want = np.stack([np.stack(seq[j * n + 1:(j + 1) * n]) for j in range(len(frames) - 1)])
        assert want.shape == (len(frames) - 1, n - 1) + frames.shape[1:] and np.isfinite(want).all()
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def _push_all(eng, frames, align, block, mem, times, pix='f32', **kw):
    """Pushes every frame through a fresh stream; returns the list of results (None for the first)."""
    h, w = (frames.shape[1] * 2 // 3, frames.shape[2]) if frames.ndim == 3 else frames.shape[1:3]
    if mem == 'host':
        with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, times=times, **kw) as st:
            return [st.push(f) for f in frames]
    import torch
    from film_hip.torch_io import DeviceInterpolator
    it = DeviceInterpolator(eng, align=align, block_shape=list(block) if block else None)
    with it.stream(h, w, pix, times=times, **kw) as st:
        up = lambda f: np.array(f).view(np.int16) if f.dtype == np.uint16 else np.array(f)   # noqa: E731  (16-bit words: int16 as a bit pattern)
        outs = [st.push(torch.from_numpy(up(f)).cuda()) for f in frames]
        torch.cuda.synchronize()
        return [None if o is None else o.cpu().numpy() for o in outs]


def _assert_pushes(got, want):
    assert got[0] is None
    for j in range(len(want)):
        assert got[j + 1].shape == want[j].shape and got[j + 1].dtype == want[j].dtype, j
        for k in range(want.shape[1]):
            assert np.array_equal(got[j + 1][k], want[j][k]), (j, k, float(np.abs(got[j + 1][k].astype(np.float64) - want[j][k]).max()))
    assert sum(len(g) for g in got[1:]) == len(want) * want.shape[1]


CASES = [(2, 256, 256, None, None), (2, 256, 256, 64, (2, 2)), (2, 192, 320, 64, (1, 2)),    # the last one pads: 192 x 160 patches -> 192 x 192
         (3, 256, 256, None, None)]


@pytest.mark.parametrize('graph', [2, 0])
@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('times,h,w,align,block', CASES)
def test_recursive_stream_is_bit_identical_to_pairs(published, times, h, w, align, block, mem, graph):
    opt, weights, eng = published
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, (times, h, w, align, block), frames, times, align, block)
    assert want.shape[:2] == (F - 1, (1 << times) - 1)
    eng.set_option('graph', graph)
    try:
        got = _push_all(eng, frames, align, block, mem, times)
    finally:
        eng.set_option('graph', 2)
    _assert_pushes(got, want)
    assert len({m.tobytes() for m in want.reshape((-1,) + want.shape[2:])}) == (F - 1) * ((1 << times) - 1)   # (a stale frame would show)


@pytest.mark.parametrize('overlap', [(8, 8), (-1, -1)])
def test_recursive_stream_with_overlapped_tiles(published, overlap):
    """256 x 256 in 2 x 2 tiles that overlap (align 96), T = 2: the frames fed back are the blended ones."""
    opt, weights, eng = published
    frames = _frames(3, 256, 256, seed=77)
    eng.set_block_overlap(overlap)
    try:
        til = eng.tiling(256, 256, align=96, block_shape=(2, 2))
        assert til['overlap_h'] == (8 if overlap[0] > 0 else 32) and til['padded_h'] == 192
        want = _recursion(eng, ('overlap', overlap), frames, 2, 96, (2, 2))
        got = _push_all(eng, frames, 96, (2, 2), 'host', 2)
        got_dev = _push_all(eng, frames, 96, (2, 2), 'device', 2)
    finally:
        eng.set_block_overlap(0)
    plain = _recursion(eng, ('overlap', 0), frames, 2, 96, (2, 2))
    assert not np.array_equal(plain[0][0], want[0][0])      # (the overlap was in force, also one level down)
    _assert_pushes(got, want)
    _assert_pushes(got_dev, want)


@pytest.mark.parametrize('mem', ['host', 'device'])
def test_u8_recursive_stream(published, mem):
    """'u8', T = 2: the bytes are film_to_uint8's (eval.util.to_uint8) of the float32 T = 2 stream on u8 / 255 - the fed-back frames
    were not quantised on the way."""
    from eval import util
    opt, weights, eng = published
    h, w, align, block = 256, 256, 64, (2, 2)
    u8 = _frames_u8(3, h, w, seed=31)
    x = u8.astype(np.float32) / 255
    key = ('u8', h, w)
    if key not in _WANT:
        _WANT[key] = _push_all(eng, x, align, block, 'host', 2)
    ref = _WANT[key]
    want = _recursion(eng, ('u8rec', h, w), x, 2, align, block)
    got = _push_all(eng, u8, align, block, mem, 2, pix='u8')
    assert got[0] is None
    for j in (1, 2):
        assert got[j].dtype == np.uint8 and got[j].shape == (3, h, w, 3)
        for k in range(3):
            assert np.array_equal(got[j][k], util.to_uint8(ref[j][k])), (j, k)
            assert np.array_equal(got[j][k], util.to_uint8(want[j - 1][k])), (j, k)
    # feeding the QUANTISED mid back would have given other quarter frames
    q = util.to_uint8(ref[1][1]).astype(np.float32) / 255
    other = eng.interpolate_frames(x[:1], q[None], align=align, block_shape=block)[0]
    assert not np.array_equal(util.to_uint8(other), got[1][0])


def _yuv_scene(layout, f, h, w, seed):
    """f 4:2:0 frames (clean samples) of a scene that moves by (2, -2) px per frame."""
    import yuv_ref
    R = yuv_ref.FORMATS[layout]
    base = R.designed_frames(1, h, w, seed)[0]
    Y, Cb, Cr = R.unpack(base, layout)
    if layout == 'i010':      # (the designed 10-bit words carry junk in the ignored bits: keep the codes)
        Y, Cb, Cr = (R.code(p, layout).astype(np.uint16) for p in (Y, Cb, Cr))
    return np.stack([R.pack(np.roll(Y, (2 * i, -2 * i), (0, 1)), np.roll(Cb, (i, -i), (0, 1)), np.roll(Cr, (i, -i), (0, 1)), layout) for i in range(f)])


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('layout,matrix,full', [('i420', 'bt709', False), ('i010', 'bt601', True)])
def test_yuv_recursive_stream(published, layout, matrix, full, mem):
    """'i420' / 'i010', T = 2: the samples are film_to_yuv420 of the float32 T = 2 stream on the frames dequantised by tests/yuv_ref.py
    (whose agreement with the device cut tests/test_yuv_gpu.py and tests/test_yuv10_gpu.py establish)."""
    import torch
    import yuv_ref
    R = yuv_ref.FORMATS[layout]
    opt, weights, eng = published
    h, w = 128, 192
    frames = _yuv_scene(layout, 3, h, w, seed=h + w)
    key = ('yuv', layout)
    if key not in _WANT:
        x = np.stack([R.yuv_in(fr, layout, matrix, full) for fr in frames])
        ref = _push_all(eng, x, 64, None, 'host', 2)
        want = []
        for mids in ref[1:]:
            dev = torch.from_numpy(mids).cuda()
            out = torch.empty((3, h * 3 // 2, w), dtype=torch.uint8 if layout == 'i420' else torch.int16, device='cuda')
            for k in range(3):
                eng.to_yuv420_device(dev[k].data_ptr(), out[k].data_ptr(), h, w, layout, matrix, full)
            torch.cuda.synchronize()
            want.append(out.cpu().numpy().view(frames.dtype))
        _WANT[key] = np.stack(want)
        _WANT[key].setflags(write=False)
    want = _WANT[key]
    got = _push_all(eng, frames, 64, None, mem, 2, pix=layout, matrix=matrix, full_range=full)
    assert got[0] is None
    for j in (1, 2):
        g = got[j].view(frames.dtype) if got[j].dtype != frames.dtype else got[j]
        assert g.shape == (3, h * 3 // 2, w)
        for k in range(3):
            bad = np.flatnonzero(g[k].ravel() != want[j - 1][k].ravel())
            assert bad.size == 0, (j, k, bad.size, bad[:8])
    assert len({m.tobytes() for m in want.reshape(6, -1)}) == 6


def test_recursive_stream_is_independent_of_other_calls(published):
    """Between pushes: three other shapes through film_interpolate (the stream's plan is evicted: three device plans are kept), every
    plan dropped, and "stream_times" set to another value - the open stream keeps its T and its bits."""
    opt, weights, eng = published
    h, w, align, block = 256, 256, 64, (2, 2)
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, (2, h, w, align, block), frames, 2, align, block)
    other = [_frames(2, a, b, seed=a) for a, b in ((64, 64), (64, 128), (128, 64))]
    try:
        with eng.open_stream(h, w, align=align, block_shape=block, times=2) as st:
            assert st.times == 2 and st.per_push == 3
            assert st.push(frames[0]) is None
            assert np.array_equal(st.push(frames[1]), want[0])
            for o in other:
                eng.interpolate_frames(o[:1], o[1:])
            assert np.array_equal(st.push(frames[2]), want[1])
            eng.set_option('stream_times', 3)                        # affects the next open only
            assert np.array_equal(st.push(frames[3]), want[2])     # (carried again, no re-extraction)
            eng.set_option('fuse', 0)
            eng.set_option('fuse', 31)
            assert np.array_equal(st.push(frames[4]), want[3])
            st.reset()
            assert st.push(frames[0]) is None
            for o in other:
                eng.interpolate_frames(o[:1], o[1:])
            assert np.array_equal(st.push(frames[1]), want[0])
    finally:
        eng.set_option('stream_times', 1)
    with eng.open_stream(h, w, align=align, block_shape=block) as st:      # times = 1 by default: one frame per push, as ever
        assert st.push(frames[0]) is None
        assert np.array_equal(st.push(frames[1]), want[0][1])


def test_recursive_stream_reset_and_null_mid(published):
    """reset: 0 frames, then 2^T - 1 again.  A NULL `mid` on a primed push: FILM_ERR_INVALID and an unprimed stream."""
    from film_hip.engine import FILM_ERR_INVALID
    opt, weights, eng = published
    h, w = 256, 256
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, (2, h, w, None, None), frames, 2, None, None)
    lib, hnd = eng._lib, eng._h
    produced = ctypes.c_int(7)
    with eng.open_stream(h, w, times=2) as st:
        assert st.push(frames[0]) is None
        assert np.array_equal(st.push(frames[1]), want[0])
        st.reset()
        assert st.push(frames[2]) is None
        assert np.array_equal(st.push(frames[3]), want[2])
        assert lib.film_stream_push(hnd, frames[4].ctypes.data, None, ctypes.byref(produced), 0, None) == FILM_ERR_INVALID
        assert produced.value == 0 and lib.film_last_error(hnd).decode() == 'NULL argument'
        assert st.push(frames[3]) is None
        out = np.empty((3, h, w, 3), np.float32)
        assert st.push(frames[4], out=out) is out and np.array_equal(out, want[3])
        with pytest.raises(ValueError):
            st.push(frames[4], out=np.empty((h, w, 3), np.float32))


def test_recursive_stream_scene_cut(published):
    """'u8', T = 2, "scene_cut" = 250: frames 0, 1 | 2, 3 with a designed cut (the second scene holds the first one's bytes halved: D
    computed here).  The cut push produces nothing and reports D; the push after it produces 2^T - 1 frames inside the new scene."""
    opt, weights, eng = published
    h, w = 256, 256
    a = _frames_u8(2, h, w, seed=5)
    b = _frames_u8(2, h, w, seed=5) // 2
    seq = [a[0], a[1], b[0], b[1]]
    S = 3 * h * w
    hist = lambda fr: np.stack([np.bincount(fr[..., c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)   # noqa: E731
    D = int(np.abs(hist(seq[2]) - hist(seq[1])).sum())
    assert 1000 * D >= 250 * 2 * S and np.array_equal(hist(seq[0]), hist(seq[1])) and np.array_equal(hist(seq[2]), hist(seq[3]))
    try:
        with eng.open_stream(h, w, pix='u8', times=2) as st:
            plain = [st.push(f) for f in (seq[2], seq[3])][1]
        with eng.open_stream(h, w, pix='u8', times=2, scene_cut=250) as st:
            assert st.push(seq[0]) is None and st.cut_info() == (-1, S, 0)
            first = st.push(seq[1])
            assert first is not None and first.shape == (3, h, w, 3) and st.cut_info() == (0, S, 0)
            assert st.push(seq[2]) is None and st.cut_info() == (D, S, 1)
            after = st.push(seq[3])
            assert st.cut_info() == (0, S, 0)
            assert after is not None and np.array_equal(after, plain)
    finally:
        eng.set_option('scene_cut', 0)


def test_recursive_stream_profile(published):
    """profile = 1: a steady T = 2 push lists the ops of its three pair runs in schedule order - two extractions' worth of image_pyramid /
    feat_ ops (the pushed frame's and the depth-1 mid's), three pair tails."""
    opt, weights, eng = published
    h, w, align, block, tiles = 256, 256, 64, (2, 2), 4
    frames = _frames(F, h, w, seed=h + w)
    want = _recursion(eng, (2, h, w, align, block), frames, 2, align, block)
    is_x = lambda t: t.startswith(('image_pyramid', 'feat_'))   # noqa: E731
    eng.set_option('profile', 1)
    try:
        with eng.open_stream(h, w, align=align, block_shape=block, times=2) as st:
            assert st.push(frames[0]) is None
            first = [o['tag'] for o in eng.profile()['ops']]
            p0 = eng.stream_pair_plan(tiles, 128, 128, 2, 1, 0, True)
            assert first == [o['tag'] for o in p0['ops'][:p0['n_extract']]] and all(is_x(t) for t in first)
            for j, slot in ((1, 1), (2, 0)):
                assert np.array_equal(st.push(frames[j]), want[j - 1])
                prof = eng.profile()
                tags = [o['tag'] for o in prof['ops']]
                steps = eng.stream_schedule(2, slot)['steps']
                plans = [eng.stream_pair_plan(tiles, 128, 128, 2, t['left'], t['right'], t['extract']) for t in steps]
                assert tags == [o['tag'] for p in plans for o in p['ops']]
                assert [p['n_extract'] > 0 for p in plans] == [True, True, False]
                assert sum(is_x(t) for t in tags) == 2 * len(first)
                tail = plans[2]['ops'][-1]['tag']
                assert not is_x(tail) and tags.count(tail) == 3
                assert sum(c['launches'] for c in prof['classes'].values()) == len(tags)
    finally:
        eng.set_option('profile', 0)


@pytest.mark.parametrize('colour', ['420jpeg', '420p10'])
def test_video_cli_times_to_interpolate(published, tmp_path, monkeypatch, colour):
    """A 4-frame 64 x 64 .y4m (8-bit and C420p10) through eval.video_cli --times_to_interpolate 2: 13 frames out, the inputs verbatim
    at the multiples of 4, the mids the stream API's, the header rate x 4."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m
    opt, weights, eng = published
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, **kw):
        it = real.__new__(real)
        it._options, it._engine = eng.options, eng
        it._align, it._block_shape = align or None, block_shape or None
        return it

    layout, kw = ('i420', {}) if colour == '420jpeg' else ('i010', {'colour': '420p10'})
    n = 4
    frames = _yuv_scene(layout, n, 64, 64, seed=5)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    tokens = y4m.header_tokens(64, 64, (24, 1), **kw)
    with open(src, 'wb') as f:
        wr = y4m.Y4MWriter(f, tokens)
        for fr in frames:
            wr.write(fr)
    with eng.open_stream(64, 64, align=64, pix=layout, matrix='bt601', times=2) as st:
        mids = [st.push(fr) for fr in frames][1:]
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    assert cli.main(['--input', str(src), '--output', str(dst), '--matrix', 'bt601', '--times_to_interpolate', '2']) == (n - 1) * 4 + 1
    with open(dst, 'rb') as f:
        r = y4m.Y4MReader(f, depths=(8, 10))
        got = list(r)
    assert r.tokens == ['W64', 'H64', 'F96:1'] + tokens[3:]
    assert len(got) == (n - 1) * 4 + 1
    for i in range(n):
        assert np.array_equal(got[4 * i], frames[i]), i
    for i in range(n - 1):
        for k in range(3):
            assert np.array_equal(got[4 * i + 1 + k], mids[i][k]), (i, k)
    assert len({g.tobytes() for g in got}) == len(got)
