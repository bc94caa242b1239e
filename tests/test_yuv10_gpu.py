"""GPU tests of the 10-bit Y'CbCr 4:2:0 path (FILM_PIX_I010 / FILM_PIX_P010), bit for bit against the numpy restatement tests/yuv_ref.py
(include/film_hip.h, "The 10-bit 4:2:0 arithmetic"): frame_yuv10_to_tiles_kernel alone through film_debug_yuv_cut on designed data with guard
bands (tests/test_yuv10_cpu.py shows which instance and branch every case reaches and that the comparison finds each planted fault);
rgb_to_yuv10_kernel alone through film_to_yuv420; the two 10-bit instances of frame_histogram_kernel through film_frame_histogram and
through a stream with "scene_cut"; 10-bit frame streams on the TINY net from host and device memory; eval/video_cli.py on a small
C420p10 file.  No tolerance anywhere."""
import numpy as np
import pytest

import tile_map_ref as T
import yuv_ref as R

FMT = R.FORMATS['i010']
LAYOUTS = FMT.layouts
COLOURS = [(m, f) for m in ('bt709', 'bt601') for f in (False, True)]      # the four colour settings of the 4:2:0 tests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    """A handle with a device and NO weights: the kernels alone need none."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    e = FilmEngine(TINY, device=0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def tiny():
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    e = FilmEngine(TINY, device=0)
    e.set_weights(W.make_synthetic_weights(TINY, seed=0))
    yield e
    e.close()


def _up(words):
    """uint16 words -> a CUDA tensor of the same bits (int16: every torch has it)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int16).copy()).cuda()


def _down(t):
    return t.cpu().numpy().view(np.uint16)


# ---- the cut alone ------------------------------------------------------------------------------------------------------------------------
class GpuBackend:
    """film_debug_yuv_cut as a backend of yuv_ref.Format.check_cut: both allocations go up as torch tensors (guard | payload | guard in ONE
    allocation each), the entry point gets the payloads' addresses, both come back."""

    def __init__(self, eng):
        self.eng = eng

    def __call__(self, frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full):
        import torch
        ft, tt = _up(frames_alloc), torch.from_numpy(np.array(tiles_alloc)).cuda()
        fp, tp = ft.data_ptr() + 2 * FMT.guard, tt.data_ptr() + 4 * T.GUARD
        assert fp % 4 == 0 and tp % 16 == 0 and ft.numel() % 2 == 0
        self.eng.debug_yuv_cut(fp, tp, case.B, case.H, case.W, case.align, case.block, tile0, ntiles, pix=layout, matrix=matrix, full_range=full)
        torch.cuda.synchronize()
        return _down(ft), tt.cpu().numpy()


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_cut(eng, case, layout):
    """All four colour settings, every range of every partition: tiles_dev[0 : ntiles] == the restatement on the bits, the padding +0.0,
    the rest of the tile tensor, its guards and the frames untouched, the same bits from the same call again."""
    eng.set_block_overlap(case.overlap)
    try:
        geo = eng.tiling(case.H, case.W, case.align, case.block)
        backend = GpuBackend(eng)
        findings = [f'[{name}] {m}' for matrix, full in COLOURS for name, ranges in R.ranges_of(case, geo).items()
                    for m in FMT.check_cut(backend, case, geo, layout, matrix, full, ranges, seed=17)]
    finally:
        eng.set_block_overlap(0)
    assert not findings, f'{len(findings)} findings:\n' + '\n'.join(findings[:12])


# ---- film_to_yuv420 alone -------------------------------------------------------------------------------------------------------------------
def _rgb(h, w, seed):
    """float32 [h,w,3] in [-0.2, 1.2] with exact 0 and 1, values below 0 and above 1, and flat 2 x 2 blocks among the noise."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (h, w, 3)).astype(np.float32)
    x[:2, -2:] = rng.uniform(0, 1, 3).astype(np.float32)
    x[0, 0] = (0, 1, -3)
    x[-1, -1] = (7, 0.5, 1)
    assert (x < 0).any() and (x > 1).any()
    return x


@pytest.mark.parametrize('offset', [0, 1], ids=lambda o: f'dst+{2 * o}')
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('h,w', [(2, 2), (16, 18), (30, 50)])
def test_to_yuv420(eng, h, w, layout, offset):
    """dst 4-byte aligned (whole words where the rows allow) and 2 bytes behind that (samples): the frame == the restatement, the guard
    bands around it and the source untouched, for all four colour settings."""
    import torch
    n = h * w * 3 // 2
    src = _rgb(h, w, seed=h + w)
    st = torch.from_numpy(src).cuda()
    for ci, (matrix, full) in enumerate(COLOURS):
        alloc = np.random.default_rng(ci).integers(0, 65536, FMT.guard + offset + n + FMT.guard).astype(np.uint16)
        dt = _up(alloc)
        assert dt.data_ptr() % 4 == 0 and st.data_ptr() % 16 == 0
        eng.to_yuv420_device(st.data_ptr(), dt.data_ptr() + 2 * (FMT.guard + offset), h, w, layout, matrix, full)
        torch.cuda.synchronize()
        got = _down(dt)
        want = np.array(alloc)
        want[FMT.guard + offset:FMT.guard + offset + n] = FMT.yuv_out(src, layout, matrix, full).ravel()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (matrix, full, bad.size, bad[:8] - FMT.guard - offset, got[bad[:8]], want[bad[:8]])
    assert np.array_equal(st.cpu().numpy().view(np.uint32), src.view(np.uint32))


# ---- the histogram --------------------------------------------------------------------------------------------------------------------------
HIST_GUARD = 16     # guard words around the 768 counters


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('h,w', [(30, 50), (2, 2)])
def test_histogram(h, w, layout):
    """film_frame_histogram == numpy bincount of code >> 2 per plane, on designed frames (random junk in the ignored bits) inside guard
    words whose code is in no plane, with the frame starting 0, 4, 8 and 12 bytes behind a 16-byte boundary: no guard word counted, the
    counters' guards untouched, the same counters from a second call, the frame unmodified; and through torch_io.frame_histogram."""
    import torch
    from film_hip.engine import frame_histogram_device
    from film_hip.torch_io import frame_histogram
    frame = np.array(FMT.designed_frames(1, h, w, seed=h + w, layout=layout)[0])
    codes = FMT.code(frame, layout)
    frame[(codes >> 2) == 77] = FMT.store(320, layout)          # bin 77 is the guard's: codes 308 .. 311
    guard_word = int(FMT.store(309, layout)) | (0x0400 if layout == 'i010' else 0x0020)
    want = FMT.histogram(frame, layout)
    assert want[:, 77].sum() == 0 and want.sum(1).tolist() == [h * w, h * w // 4, h * w // 4]
    for offset_words in (0, 1, 2, 3):
        front, back = 32 + 2 * offset_words, 32
        alloc = np.concatenate([np.full(front, guard_word, np.uint16), frame.ravel(), np.full(back, guard_word, np.uint16)])
        ft = _up(alloc)
        assert ft.data_ptr() % 16 == 0
        noise = np.random.default_rng(5).integers(1, 2 ** 32, 768 + 2 * HIST_GUARD, dtype=np.uint32)
        ht = torch.from_numpy(noise.view(np.int32).copy()).cuda()
        for rep in range(2):
            frame_histogram_device(ft.data_ptr() + 2 * front, h, w, ht.data_ptr() + 4 * HIST_GUARD, layout)
            torch.cuda.synchronize()
            got = ht.cpu().numpy().view(np.uint32)
            counters = got[HIST_GUARD:HIST_GUARD + 768].astype(np.int64).reshape(3, 256)
            bad = np.argwhere(counters != want)
            assert bad.size == 0, (layout, h, w, offset_words, rep, len(bad), bad[:6].tolist(), counters[tuple(bad[:6].T)].tolist(), want[tuple(bad[:6].T)].tolist())
            assert np.array_equal(got[:HIST_GUARD], noise[:HIST_GUARD]) and np.array_equal(got[-HIST_GUARD:], noise[-HIST_GUARD:])
        assert np.array_equal(_down(ft), alloc)
    for t in [_up(frame)] + ([torch.from_numpy(frame.copy()).cuda()] if hasattr(torch, 'uint16') else []):      # int16 as a bit pattern; uint16 where torch has it
        got = frame_histogram(t, layout)
        torch.cuda.synchronize()
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)


# ---- the stream, on the TINY net -----------------------------------------------------------------------------------------------------------
STREAMS = {      # name: (frames, h, w, align, block, (matrix, full_range))
    '64x64': (4, 64, 64, None, None, ('bt709', False)),
    '100x250-b2x2': (4, 100, 250, 64, (2, 2), ('bt601', True)),       # 125-pixel patches: an odd column origin
}
_WANT = {}


def _scene(f, h, w, seed):
    """f I010 frames (clean words) of a scene that moves by (2, -2) px per frame, with every code in the Y plane."""
    base = FMT.designed_frames(1, h, w, seed)[0]
    Y, Cb, Cr = (FMT.code(p, 'i010').astype(np.uint16) for p in FMT.unpack(base, 'i010'))
    return np.stack([FMT.pack(np.roll(Y, (2 * i, -2 * i), (0, 1)), np.roll(Cb, (i, -i), (0, 1)), np.roll(Cr, (i, -i), (0, 1)), 'i010') for i in range(f)])


def _want(tiny, name):
    """(I010 frames, expected I010 mids): yuv_out(interpolate_frames(yuv_in(prev), yuv_in(cur))), computed once per case and shared."""
    if name not in _WANT:
        f, h, w, align, block, (matrix, full) = STREAMS[name]
        frames = _scene(f, h, w, seed=h + w)
        x = np.stack([FMT.yuv_in(fr, 'i010', matrix, full) for fr in frames])
        mids = tiny.interpolate_frames(x[:-1], x[1:], align=align, block_shape=block)
        assert np.isfinite(mids).all()
        want = np.stack([FMT.yuv_out(m, 'i010', matrix, full) for m in mids])
        frames.setflags(write=False); want.setflags(write=False)
        _WANT[name] = frames, want
    return _WANT[name]


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', list(STREAMS))
def test_stream(tiny, name, layout, mem):
    """Every push's mid == yuv_out(interpolate_frames(yuv_in(previous), yuv_in(frame))), code for code - also the push after "fuse" 31 -> 0
    -> 31 dropped every plan (the stream cuts the 10-bit frame it kept again).  The frames pushed carry junk in the ignored bits; the P010
    results are the I010 results shifted, with the ignored bits zero."""
    f, h, w, align, block, (matrix, full) = STREAMS[name]
    frames, want = _want(tiny, name)
    if layout == 'p010':
        frames = np.stack([R.convert_layout(fr, 'i010', 'p010') for fr in frames])
        want = np.stack([R.convert_layout(m, 'i010', 'p010') for m in want])
        assert np.array_equal(FMT.unpack(want[0], 'p010')[0], FMT.unpack(_want(tiny, name)[1][0], 'i010')[0] << 6)
    frames = np.stack([FMT.with_junk(fr, layout, 7 + i) for i, fr in enumerate(frames)])
    assert (frames != np.stack([R.convert_layout(fr, layout, layout) for fr in frames])).any()

    def drop_plans():
        tiny.set_option('fuse', 0)
        tiny.set_option('fuse', 31)

    if mem == 'host':
        with tiny.open_stream(h, w, align=align, block_shape=block, pix=layout, matrix=matrix, full_range=full) as st:
            assert st.shape == (h * 3 // 2, w) and st.dtype is np.uint16
            got = []
            for i, fr in enumerate(frames):
                if i == 2:
                    drop_plans()
                got.append(st.push(fr))
    else:
        import torch
        from film_hip.torch_io import DeviceInterpolator
        it = DeviceInterpolator(tiny, align=align, block_shape=list(block) if block else None)
        with it.stream(h, w, layout, matrix, full) as st:
            outs = []
            for i, fr in enumerate(frames):
                if i == 2:
                    torch.cuda.synchronize()
                    drop_plans()
                # int16 as a bit pattern; the last frame as uint16 where the installed torch has it
                t = torch.from_numpy(np.array(fr)).cuda() if i == f - 1 and hasattr(torch, 'uint16') else _up(fr)
                outs.append(st.push(t))
                assert outs[-1] is None or outs[-1].dtype == t.dtype        # results come back in the dtype that was pushed
            torch.cuda.synchronize()
            got = [None if o is None else o.cpu().numpy().view(np.uint16) for o in outs]
    assert got[0] is None
    for j in range(f - 1):
        g = got[j + 1]
        assert g.dtype == np.uint16 and g.shape == (h * 3 // 2, w)
        bad = np.flatnonzero(g.ravel() != want[j].ravel())
        assert bad.size == 0, (j, bad.size, bad[:8], g.ravel()[bad[:8]], want[j].ravel()[bad[:8]])
    assert len({m.tobytes() for m in want}) == f - 1       # (the mids differ from each other: a stale result would show)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_stream_scene_cut_reports_the_restatements_distance(tiny, layout):
    """A 10-bit stream with "scene_cut" set: D and S of cut_info are those of the restatement's histograms (bin = code >> 2), the rule
    1000 D >= k * 2 S decides, and a cut push produces nothing."""
    h, w = 64, 64
    frames = _scene(3, h, w, seed=9)
    other = FMT.pack(*[(FMT.code(p, 'i010') // 2).astype(np.uint16) for p in FMT.unpack(frames[0], 'i010')], 'i010')      # halved codes: a different histogram
    seq = [frames[0], frames[1], other, frames[2]]
    if layout == 'p010':
        seq = [R.convert_layout(fr, 'i010', 'p010') for fr in seq]
    seq = [FMT.with_junk(fr, layout, i) for i, fr in enumerate(seq)]
    hists = [FMT.histogram(fr, layout) for fr in seq]
    D = [int(np.abs(hists[i] - hists[i - 1]).sum()) for i in range(1, 4)]
    S = h * w * 3 // 2
    k = 300
    assert 1000 * D[0] < k * 2 * S <= 1000 * D[1] and 1000 * D[2] >= k * 2 * S       # frame 1 continues the scene, `other` and frame 2 each start one
    try:
        with tiny.open_stream(h, w, pix=layout, scene_cut=k) as st:
            assert st.push(seq[0]) is None and st.cut_info() == (-1, S, 0)
            assert st.push(seq[1]) is not None and st.cut_info() == (D[0], S, 0)
            assert st.push(seq[2]) is None and st.cut_info() == (D[1], S, 1)
            assert st.push(seq[3]) is None and st.cut_info() == (D[2], S, 1)
    finally:
        tiny.set_option('scene_cut', 0)


# ---- the Y4M tool --------------------------------------------------------------------------------------------------------------------------
def test_video_cli(tiny, tmp_path, monkeypatch):
    """A 5-frame 64 x 64 C420p10 .y4m through eval.video_cli: 9 frames out, the 5 originals verbatim, the mids equal to the stream's, F doubled."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, **kw):
        it = real.__new__(real)
        it._options, it._engine = tiny.options, tiny
        it._align, it._block_shape = align or None, block_shape or None
        return it

    frames = _scene(5, 64, 64, seed=5)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    tokens = y4m.header_tokens(64, 64, (24, 1), colour='420p10')
    with open(src, 'wb') as f:
        w = y4m.Y4MWriter(f, tokens)
        for fr in frames:
            w.write(fr)
    with tiny.open_stream(64, 64, align=64, pix='i010', matrix='bt601') as st:
        mids = [st.push(fr) for fr in frames][1:]
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    assert cli.main(['--input', str(src), '--output', str(dst), '--matrix', 'bt601']) == 9
    with open(dst, 'rb') as f:
        r = y4m.Y4MReader(f, depths=(8, 10))
        got = list(r)
    assert r.tokens == ['W64', 'H64', 'F48:1'] + tokens[3:] and r.depth == 10
    assert len(got) == 9 and all(g.dtype == np.uint16 for g in got)
    for i in range(5):
        assert np.array_equal(got[2 * i], frames[i]), i
    for i in range(4):
        assert np.array_equal(got[2 * i + 1], mids[i]), i
    assert not np.array_equal(mids[0], mids[1])
    want = FMT.yuv_out(tiny.interpolate_frames(FMT.yuv_in(frames[0], 'i010', 'bt601')[None], FMT.yuv_in(frames[1], 'i010', 'bt601')[None], align=64)[0], 'i010', 'bt601')
    assert np.array_equal(mids[0], want)
