"""GPU tests of selected mid-frames in a frame stream (film_stream_select; FilmStream.select): a primed push writes only the selected
positions of its 2^T - 1, packed in temporal order, every one bit-identical to the frame at that position of a FULL push of the same
frames - from host and device memory, on both executors, untiled and in padded tiles, with overlapped tiles, with 8-bit and 4:2:0
frames - and what goes with it: the caller's buffer behind the selected frames stays untouched, the selection outlives reset and scene
cuts, the profile lists the pruned runs, and eval.video_cli --fps writes the frames of --times_to_interpolate at the snapped instants.

(No in-process "graph" = 1 cases: profiles/r06_hipgraph_crash_diagnosis.md.)
"""
import numpy as np
import pytest

from test_stream_recursion_gpu import _frames, _frames_u8, _yuv_scene

pytestmark = pytest.mark.gpu

N = 4            # frames per case, pushed round and round: 0 1 2 3 0 1 ... (the pair (3, 0) is a pair like any other)
SENTINEL = -7.25
GUARD = 2        # frames of SENTINEL behind the selected ones in a device push's buffer


@pytest.fixture(scope='module')
def published():
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    w = W.make_synthetic_weights(PUBLISHED, seed=0)
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(w)
    yield eng
    eng.close()


_FULL = {}


def _full(eng, key, frames, times, align, block, pix='f32', **kw):
    """{first frame of the pair: [2^T - 1, ...] frames} of FULL host pushes of frames 0 1 2 ... n - 1 0 through a stream that is never
    given a selection.  Computed once per key, shared, never written to."""
    if key not in _FULL:
        h, w = (frames.shape[1] * 2 // 3, frames.shape[2]) if frames.ndim == 3 else frames.shape[1:3]
        order = list(range(len(frames))) + [0]
        with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, times=times, **kw) as st:
            assert st.selection == tuple(range(1, 1 << times))
            outs = [st.push(frames[i]) for i in order]
        assert outs[0] is None
        want = {}
        for i, o in zip(order[:-1], outs[1:]):
            o = o[None] if times == 1 else o
            assert o.shape[0] == (1 << times) - 1
            o.setflags(write=False)
            want[i] = o
        assert len({m.tobytes() for o in want.values() for m in o}) == len(frames) * ((1 << times) - 1)     # (a stale frame would show)
        _FULL[key] = want
    return _FULL[key]


def _push_selected(eng, frames, selections, times, align, block, mem, pix='f32', **kw):
    """Pushes frames 0 1 2 ... round and round, push j + 1 with selections[j]; returns [(first frame of the pair, selection, frames)].
    mem 'device': every push writes into a tensor of len(selection) frames followed by GUARD frames of SENTINEL, which must stay."""
    h, w = (frames.shape[1] * 2 // 3, frames.shape[2]) if frames.ndim == 3 else frames.shape[1:3]
    got = []
    with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, times=times, **kw) as st:
        if mem == 'device':
            import torch
            dev = [torch.from_numpy(np.array(f).view(np.int16) if f.dtype == np.uint16 else np.array(f)).cuda() for f in frames]
            stream = torch.cuda.current_stream().cuda_stream
            sentinel = SENTINEL if pix == 'f32' else 0x55
            assert st.push_device(dev[0].data_ptr(), 0, stream) in (0, False)
        else:
            assert st.push(frames[0]) is None
        for j, sel in enumerate(selections):
            i = (j + 1) % len(frames)
            st.select(sel)
            want_sel = tuple(range(1, 1 << times)) if sel is None else tuple(sorted(set(sel)))
            assert st.selection == want_sel
            k = len(want_sel)
            if mem == 'device':
                buf = torch.full((k + GUARD,) + tuple(dev[i].shape), sentinel, dtype=dev[i].dtype, device='cuda')
                n = st.push_device(dev[i].data_ptr(), buf.data_ptr(), stream)
                torch.cuda.synchronize()
                assert int(n) == k, (j, sel, n)
                out = buf.cpu().numpy()
                assert (out[k:] == np.array(sentinel, out.dtype)).all(), (j, sel)      # nothing but the selection reaches the caller
                out = out[:k].view(frames.dtype) if out.dtype != frames.dtype else out[:k]
            else:
                out = st.push(frames[i])
                if k == 0:
                    assert out is None
                    out = np.empty((0,) + frames.shape[1:], frames.dtype)
                elif times == 1:
                    out = out[None]
                assert out.shape == (k,) + frames.shape[1:] and out.dtype == frames.dtype, (j, sel)
            got.append(((i - 1) % len(frames), want_sel, out))
    return got


def _assert_selected(got, want):
    for first, sel, out in got:
        assert len(out) == len(sel)
        for k, p in enumerate(sel):
            bad = np.flatnonzero(out[k].ravel() != want[first][p - 1].ravel())
            assert bad.size == 0, (first, sel, p, bad.size, bad[:8])


T2 = [(), (1,), (2,), (1, 2), (3,), (1, 3), (2, 3), (1, 2, 3), None]                   # all eight masks, then a full push
T3 = [(3, 6), (2, 5), (1,), (7,), (4,), (6,), (5,), (), None]
SHAPES = [(256, 256, None, None), (192, 320, 64, (1, 2))]                              # the second one pads: 192 x 160 patches -> 192 x 192


@pytest.mark.parametrize('graph', [2, 0])
@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('h,w,align,block', SHAPES)
@pytest.mark.parametrize('times,selections', [(2, T2), (3, T3)])
def test_selected_pushes_are_the_full_push_frames(published, times, selections, h, w, align, block, mem, graph):
    eng = published
    frames = _frames(N, h, w, seed=h + w)
    want = _full(eng, (times, h, w), frames, times, align, block)
    eng.set_option('graph', graph)
    try:
        got = _push_selected(eng, frames, selections, times, align, block, mem)
    finally:
        eng.set_option('graph', 2)
    assert [len(s) for _, s, _ in got] == [len(s) if s is not None else (1 << times) - 1 for s in selections]
    _assert_selected(got, want)


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('pix', ['u8', 'i420', 'i010'])
def test_selected_pushes_of_quantised_streams(published, pix, mem):
    """T = 3 with {3, 6} / {2, 5}: the quantised frames of the full push of the same stream - what is fed back stayed float32."""
    eng = published
    if pix == 'u8':
        h, w, kw = 256, 256, {}
        frames = _frames_u8(N, h, w, seed=31)
    else:
        kw = dict(matrix='bt709', full_range=False) if pix == 'i420' else dict(matrix='bt601', full_range=True)
        h, w = 128, 192
        frames = _yuv_scene(pix, N, h, w, seed=h + w)
    want = _full(eng, (pix,), frames, 3, 64, None, pix, **kw)
    got = _push_selected(eng, frames, [(3, 6), (2, 5), (3, 6), (2, 5), None], 3, 64, None, mem, pix, **kw)
    _assert_selected(got, want)


def test_selected_push_with_overlapped_tiles(published):
    """256 x 256 in 2 x 2 tiles that overlap by (8, 8) (align 96), T = 2 with {3}: the undelivered depth-1 frame that is fed back is the
    blended one."""
    eng = published
    frames = _frames(N, 256, 256, seed=77)
    eng.set_block_overlap((8, 8))
    try:
        assert eng.tiling(256, 256, align=96, block_shape=(2, 2))['overlap_h'] == 8
        want = _full(eng, ('overlap',), frames, 2, 96, (2, 2))
        got = _push_selected(eng, frames, [(3,), (3,), None], 2, 96, (2, 2), 'host')
        got_dev = _push_selected(eng, frames, [(3,), (3,), None], 2, 96, (2, 2), 'device')
    finally:
        eng.set_block_overlap(0)
    plain = _full(eng, ('no overlap',), frames, 2, 96, (2, 2))
    assert not np.array_equal(plain[0][2], want[0][2])          # (the overlap was in force)
    _assert_selected(got, want)
    _assert_selected(got_dev, want)


def test_selection_state(published):
    """The refusals on an open stream; the selection outlives reset(); an empty selection takes a NULL `mid` and carries the pushed
    frame's extraction to the next push; DeviceStream.select; a T = 1 stream keeps its bare frame."""
    import ctypes
    import torch
    from film_hip.engine import FILM_ERR_INVALID, FilmError
    from film_hip.torch_io import DeviceInterpolator
    eng = published
    h, w = 256, 256
    frames = _frames(N, h, w, seed=h + w)
    want = _full(eng, (3, h, w), frames, 3, None, None)
    with eng.open_stream(h, w, times=3) as st:
        with pytest.raises(FilmError) as e:
            eng._check(eng._lib.film_stream_select(eng._h, 1 << 7))
        assert e.value.code == FILM_ERR_INVALID and 'mask' in str(e.value)
        with pytest.raises(ValueError):
            st.select([8])
        assert st.selection == tuple(range(1, 8))
        st.select([6, 3, 6])
        assert st.selection == (3, 6)
        assert st.push(frames[0]) is None
        out = np.empty((2, h, w, 3), np.float32)
        assert st.push(frames[1], out=out) is out and np.array_equal(out[0], want[0][2]) and np.array_equal(out[1], want[0][5])
        with pytest.raises(ValueError):
            st.push(frames[2], out=np.empty((7, h, w, 3), np.float32))
        st.reset()
        assert st.selection == (3, 6) and st.push(frames[1]) is None
        got = st.push(frames[2])
        assert got.shape == (2, h, w, 3) and np.array_equal(got[0], want[1][2]) and np.array_equal(got[1], want[1][5])
        st.select([])
        produced = ctypes.c_int(7)
        assert eng._lib.film_stream_push(eng._h, frames[3].ctypes.data, None, ctypes.byref(produced), 0, None) == 0 and produced.value == 0
        st.select(None)
        assert np.array_equal(st.push(frames[0]), want[3])
    with DeviceInterpolator(eng).stream(h, w, times=3) as ds:
        dev = [torch.from_numpy(f).cuda() for f in frames]
        assert ds.push(dev[0]) is None
        ds.select([2, 5])
        assert ds.selection == (2, 5)
        got = ds.push(dev[1])
        assert tuple(got.shape) == (2, h, w, 3) and np.array_equal(got.cpu().numpy(), want[0][[1, 4]])
        ds.select([])
        assert ds.push(dev[2]) is None
        ds.select(None)
        assert np.array_equal(ds.push(dev[3]).cpu().numpy(), want[2])
    one = _full(eng, (1, h, w), frames, 1, None, None)
    with eng.open_stream(h, w) as st:
        assert st.push(frames[0]) is None
        st.select([])
        assert st.push(frames[1]) is None
        st.select([1])
        got = st.push(frames[2])
        assert got.shape == (h, w, 3) and np.array_equal(got, one[1][0])


def test_selection_and_scene_cut(published):
    """'u8', T = 2, "scene_cut" = 250, selection {1, 3}: frames 0, 1 | 2, 3 with the designed cut of test_recursive_stream_scene_cut.  The
    cut push returns nothing, the push after it delivers the selection inside the new scene, and the selection is what it was."""
    eng = published
    h, w = 256, 256
    a = _frames_u8(2, h, w, seed=5)
    b = _frames_u8(2, h, w, seed=5) // 2
    seq = [a[0], a[1], b[0], b[1]]
    try:
        with eng.open_stream(h, w, pix='u8', times=2) as st:
            plain = [st.push(f) for f in (a[0], a[1])][1], [st.push(f) for f in (b[0], b[1])][1]
        with eng.open_stream(h, w, pix='u8', times=2, scene_cut=250) as st:
            st.select([1, 3])
            assert st.push(seq[0]) is None and st.cut_info()[2] == 0
            first = st.push(seq[1])
            assert first.shape == (2, h, w, 3) and np.array_equal(first, plain[0][[0, 2]]) and st.cut_info()[2] == 0
            assert st.push(seq[2]) is None and st.cut_info()[2] == 1
            assert st.selection == (1, 3)
            after = st.push(seq[3])
            assert st.cut_info()[2] == 0 and after.shape == (2, h, w, 3) and np.array_equal(after, plain[1][[0, 2]])
    finally:
        eng.set_option('scene_cut', 0)


def test_selected_push_profile(published):
    """profile = 1, T = 3: the op tags of a {6} push are the plans that stream_schedule(3, slot, select=[6]) names, one after the other -
    an extraction-only step contributes ops[:n_extract] - with two pair tails against the seven of a full push."""
    eng = published
    h, w, align, block, tiles = 256, 256, 64, (2, 2), 4
    frames = _frames(N, h, w, seed=h + w)
    want = _full(eng, ('profile',), frames, 3, align, block)
    is_x = lambda t: t.startswith(('image_pyramid', 'feat_'))   # noqa: E731
    eng.set_option('profile', 1)
    try:
        with eng.open_stream(h, w, align=align, block_shape=block, times=3) as st:
            assert st.push(frames[0]) is None
            n_x = len(eng.profile()['ops'])
            for j, slot, sel in ((1, 1, (6,)), (2, 0, (6,)), (3, 1, None)):
                st.select(sel)
                got = st.push(frames[j])
                tags = [o['tag'] for o in eng.profile()['ops']]
                steps = eng.stream_schedule(3, slot, select=sel or range(1, 8))['steps']
                expect = []
                for t in steps:
                    p = eng.stream_pair_plan(tiles, 128, 128, 3, t['left'], t['right'], t['extract'])
                    assert p['n_extract'] == (n_x if t['extract'] else 0)
                    expect += [o['tag'] for o in (p['ops'] if t['run'] == 'pair' else p['ops'][:p['n_extract']])]
                assert tags == expect
                tail = eng.stream_pair_plan(tiles, 128, 128, 3, 0, 1, False)['ops'][-1]['tag']
                assert not is_x(tail)
                if sel:
                    assert [(t['run'], t['index']) for t in steps] == [('pair', 4), ('extract', 4), ('pair', 6)]
                    assert tags.count(tail) == 2 and sum(is_x(t) for t in tags) == 2 * n_x
                    assert np.array_equal(got[0], want[j - 1][5])
                else:
                    assert tags.count(tail) == 7 and sum(is_x(t) for t in tags) == 4 * n_x
                    assert np.array_equal(got, want[j - 1])
    finally:
        eng.set_option('profile', 0)


@pytest.mark.parametrize('colour', ['420jpeg', '420p10'])
def test_video_cli_fps(published, tmp_path, monkeypatch, capsys, colour):
    """A 4-frame 64 x 64 24 fps .y4m (8-bit and C420p10) through eval.video_cli --fps 60 --times_to_interpolate 3: eight frames at F60:1,
    every one the frame of a --times_to_interpolate 3 run at its snapped grid index g = 0 3 6 10 13 16 19 22."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m
    eng = published
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, **kw):
        it = real.__new__(real)
        it._options, it._engine = eng.options, eng
        it._align, it._block_shape = align or None, block_shape or None
        return it

    layout, kw = ('i420', {}) if colour == '420jpeg' else ('i010', {'colour': '420p10'})
    n = 4
    frames = _yuv_scene(layout, n, 64, 64, seed=5)
    src, dst, ref = tmp_path / 'in.y4m', tmp_path / 'out.y4m', tmp_path / 'ref.y4m'
    tokens = y4m.header_tokens(64, 64, (24, 1), **kw)
    with open(src, 'wb') as f:
        wr = y4m.Y4MWriter(f, tokens)
        for fr in frames:
            wr.write(fr)
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    assert cli.main(['--input', str(src), '--output', str(ref), '--matrix', 'bt601', '--times_to_interpolate', '3']) == (n - 1) * 8 + 1
    capsys.readouterr()
    grid = [0, 3, 6, 10, 13, 16, 19, 22]
    assert cli.main(['--input', str(src), '--output', str(dst), '--matrix', 'bt601', '--times_to_interpolate', '3', '--fps', '60']) == len(grid)
    err = capsys.readouterr().err
    assert '4 frames in, 8 frames out' in err and 'snap error max 0.0500' in err and '12 pair runs against 21' in err
    with open(ref, 'rb') as f:
        every = list(y4m.Y4MReader(f, depths=(8, 10)))
    with open(dst, 'rb') as f:
        r = y4m.Y4MReader(f, depths=(8, 10))
        got = list(r)
    assert r.tokens == ['W64', 'H64', 'F60:1'] + tokens[3:]
    assert len(every) == 25 and len(got) == len(grid)
    for j, g in enumerate(grid):
        assert np.array_equal(got[j], every[g]), (j, g)
    assert len({g.tobytes() for g in got}) == len(got)
