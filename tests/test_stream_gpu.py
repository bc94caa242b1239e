"""GPU tests of the frame streams (film_stream_*): a steady-state push against film_interpolate on the same pair, bit for bit - from host
and device memory, on both executors, tiled, padded, with overlapped tiles, with 8-bit frames - and the stream's independence of
whatever else the handle does between two pushes, reset, the profile, the error path and the CLI's --stream mode.

(No in-process "graph" = 1 cases: profiles/r06_hipgraph_crash_diagnosis.md.)
"""
import ctypes
import filecmp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 5    # frames per case: both orientations of the stream plan run twice


def _frames(f, h, w, seed):
    """f frames of a scene moving by (2, -3) px per frame (+ noise), float32 [f, h, w, 3]."""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3), dtype=np.float32)
    out = [np.roll(base, (2 * i, -3 * i), axis=(0, 1)) + rng.normal(0, 0.01, base.shape).astype(np.float32) for i in range(f)]
    return np.stack(out).astype(np.float32)


def _frames_u8(f, h, w, seed):
    """f uint8 frames that hold every byte value in every channel (a ramp over the first pixels of rows 0 .. in each frame)."""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    ramp = np.arange(256, dtype=np.uint8)
    for i in range(f):
        flat = fr[i].reshape(-1, 3)
        for c in range(3):
            flat[17 * i + 5:17 * i + 5 + 256, c] = np.roll(ramp, 40 * c + i)
    assert all(len(np.unique(fr[i, ..., c])) == 256 for i in range(f) for c in range(3))
    return fr


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


def _pairs(eng, key, frames, align, block):
    """film_interpolate on every consecutive pair: computed once per case, shared, never written to."""
    if key not in _WANT:
        want = eng.interpolate_frames(frames[:-1], frames[1:], align=align, block_shape=block)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def _push_all(eng, frames, align, block, mem, pix='f32'):
    """Pushes every frame through a fresh stream; returns the list of results (None for the first)."""
    h, w = frames.shape[1:3]
    if mem == 'host':
        with eng.open_stream(h, w, align=align, block_shape=block, pix=pix) as st:
            return [st.push(f) for f in frames]
    import torch
    from film_hip.torch_io import DeviceInterpolator
    it = DeviceInterpolator(eng, align=align, block_shape=list(block) if block else None)
    with it.stream(h, w, pix) as st:
        outs = [st.push(torch.from_numpy(f).cuda()) for f in frames]
        torch.cuda.synchronize()
        return [None if o is None else o.cpu().numpy() for o in outs]


SHAPES = [(256, 256, None, None), (256, 256, 64, (2, 2)), (192, 320, 64, (1, 2))]   # the last one pads: 192 x 160 patches -> 192 x 192


@pytest.mark.parametrize('graph', [2, 0])
@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('h,w,align,block', SHAPES)
def test_stream_is_bit_identical_to_pairs(published, h, w, align, block, mem, graph):
    opt, weights, eng = published
    frames = _frames(F, h, w, seed=h + w)
    want = _pairs(eng, (h, w, align, block), frames, align, block)
    eng.set_option('graph', graph)
    try:
        got = _push_all(eng, frames, align, block, mem)
    finally:
        eng.set_option('graph', 2)
    assert got[0] is None
    for j in range(F - 1):
        assert got[j + 1].shape == (h, w, 3) and np.isfinite(got[j + 1]).all()
        assert np.array_equal(got[j + 1], want[j]), (j, float(np.abs(got[j + 1] - want[j]).max()))


@pytest.mark.parametrize('overlap', [(8, 8), (-1, -1)])
def test_stream_with_overlapped_tiles(published, overlap):
    """256 x 256 in 2 x 2 tiles that overlap (align 96: a 128-pixel patch has 64 pixels of padding, so -1 resolves to 32)."""
    opt, weights, eng = published
    frames = _frames(3, 256, 256, seed=77)
    eng.set_block_overlap(overlap)
    try:
        til = eng.tiling(256, 256, align=96, block_shape=(2, 2))
        assert til['overlap_h'] == (8 if overlap[0] > 0 else 32) and til['padded_h'] == 192
        want = eng.interpolate_frames(frames[:-1], frames[1:], align=96, block_shape=(2, 2))
        got = _push_all(eng, frames, 96, (2, 2), 'host')
        got_dev = _push_all(eng, frames, 96, (2, 2), 'device')
    finally:
        eng.set_block_overlap(0)
    assert got[0] is None and got_dev[0] is None
    for j in range(2):
        assert np.array_equal(got[j + 1], want[j]), j
        assert np.array_equal(got_dev[j + 1], want[j]), j


def _cut_reference(x, bh, bw, th, tw):
    """[H,W,3] -> [bh*bw, th, tw, 3]: the reference's patches, each zero-padded to th x tw with the patch at (pad // 2, pad // 2)."""
    h, w = x.shape[:2]
    ph, pw = h // bh, w // bw
    oy, ox = (th - ph) // 2, (tw - pw) // 2
    out = np.zeros((bh * bw, th, tw, 3), x.dtype)
    for ty in range(bh):
        for tx in range(bw):
            out[ty * bw + tx, oy:oy + ph, ox:ox + pw] = x[ty * ph:(ty + 1) * ph, tx * pw:(tx + 1) * pw]
    return out


def test_u8_cut_kernel_is_exact(published):
    """The 8-bit cut alone, read back through the img0 tap after a first push: every byte value becomes exactly numpy's float32
    quotient u8 / 255, at every alignment of its 4-byte groups (a 250-pixel row is 750 bytes, the second tile column starts 375 bytes
    in: rows start at byte offsets 0, 2, 3 and 1 modulo 4), and the padding is zero."""
    opt, weights, eng = published
    ramp = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ramp.astype(np.float32) / 255, ramp.astype(np.float32) / np.float32(255.0))
    for h, w, align, block, th, tw in [(100, 250, 64, (2, 2), 64, 128), (64, 64, None, None, 64, 64)]:
        x = _frames_u8(1, h, w, seed=w)[0]
        with eng.open_stream(h, w, align=align, block_shape=block, pix='u8') as st:
            assert st.push(x) is None
            img0 = eng.tap('img0')
        bh, bw = block or (1, 1)
        assert img0.shape == (2 * bh * bw, th, tw, 3)
        want = _cut_reference(x.astype(np.float32) / 255, bh, bw, th, tw)
        assert np.array_equal(img0[:bh * bw], want)
        seen = np.unique(img0[:bh * bw])
        assert np.array_equal(seen, np.unique(ramp.astype(np.float32) / 255))


@pytest.mark.parametrize('h,w,align,block', [(100, 250, 64, (2, 2)), (256, 256, None, None)])
def test_u8_stream_equals_quantised_float_stream(published, h, w, align, block):
    """The bytes of an 8-bit stream == util.to_uint8 of the float stream fed u8 / 255 (and of film_interpolate on those frames)."""
    from eval import util
    opt, weights, eng = published
    u8 = _frames_u8(3, h, w, seed=h)
    x = u8.astype(np.float32) / 255
    ref = _push_all(eng, x, align, block, 'host')
    pairs = eng.interpolate_frames(x[:-1], x[1:], align=align, block_shape=block)
    for mem in ('host', 'device'):
        got = _push_all(eng, u8, align, block, mem, pix='u8')
        assert got[0] is None
        for j in (1, 2):
            assert got[j].dtype == np.uint8 and got[j].shape == (h, w, 3)
            assert np.array_equal(got[j], util.to_uint8(ref[j])), (mem, j)
            assert np.array_equal(got[j], util.to_uint8(pairs[j - 1])), (mem, j)


@pytest.mark.parametrize('overlap', [(8, 8), (-1, -1)])
def test_u8_stream_with_overlapped_tiles(published, overlap):
    """The production route into frame_u8_to_tiles_kernel<true> (stream_cut with FILM_PIX_U8 and an overlap): 256 x 256 in 2 x 2
    overlapped tiles, align 96.  The bytes == util.to_uint8 of film_interpolate on u8 / 255 with the same overlap, from host and from
    device memory."""
    from eval import util
    opt, weights, eng = published
    u8 = _frames_u8(3, 256, 256, seed=91)
    x = u8.astype(np.float32) / 255
    eng.set_block_overlap(overlap)
    try:
        til = eng.tiling(256, 256, align=96, block_shape=(2, 2))
        assert til['overlap_h'] == til['overlap_w'] == (8 if overlap[0] > 0 else 32) and til['padded_h'] == 192
        pairs = eng.interpolate_frames(x[:-1], x[1:], align=96, block_shape=(2, 2))
        got = {mem: _push_all(eng, u8, 96, (2, 2), mem, pix='u8') for mem in ('host', 'device')}
    finally:
        eng.set_block_overlap(0)
    plain = eng.interpolate_frames(x[:1], x[1:2], align=96, block_shape=(2, 2))
    assert not np.array_equal(util.to_uint8(plain[0]), util.to_uint8(pairs[0]))      # (the overlap was in force)
    for mem in ('host', 'device'):
        assert got[mem][0] is None
        for j in (1, 2):
            assert got[mem][j].dtype == np.uint8 and got[mem][j].shape == (256, 256, 3)
            assert np.array_equal(got[mem][j], util.to_uint8(pairs[j - 1])), (mem, j)


def test_stream_is_independent_of_other_calls(published):
    """Between pushes: three other shapes through film_interpolate (the stream's plan is evicted: three device plans are kept) and
    "fuse" 31 -> 0 -> 31 (every plan is dropped).  The next pushes still equal the pair calls - the stream extracts the frame it kept."""
    opt, weights, eng = published
    h, w, align, block = 256, 256, 64, (2, 2)
    frames = _frames(F, h, w, seed=h + w)
    want = _pairs(eng, (h, w, align, block), frames, align, block)
    other = [_frames(2, a, b, seed=a) for a, b in ((64, 64), (64, 128), (128, 64))]
    with eng.open_stream(h, w, align=align, block_shape=block) as st:
        assert st.push(frames[0]) is None
        assert np.array_equal(st.push(frames[1]), want[0])
        for o in other:
            eng.interpolate_frames(o[:1], o[1:])
        assert np.array_equal(st.push(frames[2]), want[1])
        assert np.array_equal(st.push(frames[3]), want[2])     # (carried again, no re-extraction)
        eng.set_option('fuse', 0)
        eng.set_option('fuse', 31)
        assert np.array_equal(st.push(frames[4]), want[3])
        # a first push, then eviction before the second one
        st.reset()
        assert st.push(frames[0]) is None
        for o in other:
            eng.interpolate_frames(o[:1], o[1:])
        assert np.array_equal(st.push(frames[1]), want[0])


def test_stream_reset(published):
    opt, weights, eng = published
    h, w = 256, 256
    frames = _frames(F, h, w, seed=h + w)
    want = _pairs(eng, (h, w, None, None), frames, None, None)
    with eng.open_stream(h, w) as st:
        assert st.push(frames[0]) is None
        assert np.array_equal(st.push(frames[1]), want[0])
        st.reset()
        assert st.push(frames[2]) is None
        assert np.array_equal(st.push(frames[3]), want[2])
        assert np.array_equal(st.push(frames[4]), want[3])


def test_stream_profile_lists_one_extraction(published):
    """profile = 1: a first push runs the extractor ops and nothing else; a steady-state push runs the whole plan of its orientation,
    every feat_* op once, on `tiles` images."""
    opt, weights, eng = published
    h, w, align, block, tiles = 256, 256, 64, (2, 2), 4
    frames = _frames(F, h, w, seed=h + w)
    want = _pairs(eng, (h, w, align, block), frames, align, block)
    plans = [eng.stream_plan(tiles, 128, 128, s) for s in (0, 1)]
    eng.set_option('profile', 1)
    try:
        with eng.open_stream(h, w, align=align, block_shape=block) as st:
            assert st.push(frames[0]) is None
            first = [o['tag'] for o in eng.profile()['ops']]
            assert first == [o['tag'] for o in plans[0]['ops'][:plans[0]['n_extract']]]
            assert all(t.startswith(('image_pyramid', 'feat_')) for t in first)
            for j, slot in ((1, 1), (2, 0)):
                assert np.array_equal(st.push(frames[j]), want[j - 1])
                tags = [o['tag'] for o in eng.profile()['ops']]
                assert tags == [o['tag'] for o in plans[slot]['ops']]
                feat = [o for o in plans[slot]['ops'] if o['tag'].startswith('feat_')]
                assert feat and all(o['NB'] == tiles for o in feat)
                assert len({o['tag'] for o in feat}) == len(feat) == sum(t.startswith('feat_') for t in tags)
    finally:
        eng.set_option('profile', 0)


def test_stream_error_path_and_states(published):
    """A push with a NULL frame after a good push fails and leaves the stream unprimed: the next push produces nothing, the one after
    it is correct.  Also: a second open, a bad mem_kind, open before film_finalize."""
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID, FILM_ERR_STATE
    opt, weights, eng = published
    h, w = 256, 256
    frames = _frames(F, h, w, seed=h + w)
    want = _pairs(eng, (h, w, None, None), frames, None, None)
    lib, hnd = eng._lib, eng._h
    out = np.empty((h, w, 3), np.float32)
    produced = ctypes.c_int(7)
    with eng.open_stream(h, w) as st:
        with pytest.raises(FilmError) as e:
            eng.open_stream(h, w)
        assert e.value.code == FILM_ERR_STATE and 'already open' in str(e.value)
        assert st.push(frames[0]) is None
        assert np.array_equal(st.push(frames[1]), want[0])
        assert lib.film_stream_push(hnd, None, out.ctypes.data, ctypes.byref(produced), 0, None) == FILM_ERR_INVALID
        assert produced.value == 0 and lib.film_last_error(hnd).decode() == 'NULL argument'
        assert st.push(frames[2]) is None
        assert np.array_equal(st.push(frames[3]), want[2])
        assert lib.film_stream_push(hnd, frames[4].ctypes.data, out.ctypes.data, ctypes.byref(produced), 7, None) == FILM_ERR_INVALID
        assert lib.film_last_error(hnd).decode() == 'bad mem_kind'
        assert st.push(frames[3]) is None
        assert np.array_equal(st.push(frames[4]), want[3])
    with pytest.raises(FilmError) as e:     # closed
        st.push(frames[0])
    assert e.value.code == FILM_ERR_STATE
    raw = FilmEngine(opt, device=0)
    try:
        with pytest.raises(FilmError) as e:
            raw.open_stream(h, w)
        assert e.value.code == FILM_ERR_STATE
    finally:
        raw.close()


def test_cli_stream_writes_the_same_files(published, tmp_path, monkeypatch):
    """--stream --times_to_interpolate 1 on four 96 x 128 PNGs: the same frame_*.png files, byte for byte, as the default path - also
    with 2 x 2 blocks."""
    from eval import interpolator as interpolator_lib
    from eval import interpolator_cli as cli
    from eval import util
    opt, weights, eng = published
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, precision=0, **kw):
        it = real.__new__(real)
        it._options, it._engine = eng.options, eng
        it._align, it._block_shape = align or None, block_shape or None
        return it

    frames = np.clip(_frames(4, 96, 128, seed=3), 0, 1)
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    try:
        for blocks in ([], ['--block_height', '2', '--block_width', '2']):
            dirs = {}
            for name in ('pairs', 'stream'):
                d = tmp_path / f'{name}{len(blocks)}' / 'clip'
                d.mkdir(parents=True)
                for i, f in enumerate(frames):
                    util.write_image(str(d / f'f_{i}.png'), f)
                dirs[name] = d
            cli.main(['--pattern', str(dirs['pairs'].parent / '*'), '--times_to_interpolate', '1'] + blocks)
            cli.main(['--pattern', str(dirs['stream'].parent / '*'), '--times_to_interpolate', '1', '--stream'] + blocks)
            a = sorted(os.listdir(dirs['pairs'] / 'interpolated_frames'))
            b = sorted(os.listdir(dirs['stream'] / 'interpolated_frames'))
            assert a == b == [f'frame_{i:03d}.png' for i in range(3 * 2 + 1)]
            for f in a:
                assert filecmp.cmp(dirs['pairs'] / 'interpolated_frames' / f, dirs['stream'] / 'interpolated_frames' / f, shallow=False), f
    finally:
        monkeypatch.setattr(interpolator_lib, 'Interpolator', real)
