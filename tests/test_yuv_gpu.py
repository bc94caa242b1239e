"""GPU tests of the 8-bit Y'CbCr 4:2:0 path, bit for bit against the numpy restatement tests/yuv_ref.py (include/film_hip.h, "The 4:2:0
arithmetic"): frame_yuv420_to_tiles_kernel alone through film_debug_yuv_cut on designed data with guard bands (tests/test_yuv_cpu.py
shows which instance and branch every case reaches and that the comparison finds each planted fault); rgb_to_yuv420_kernel alone through
film_to_yuv420; 4:2:0 frame streams on the TINY net from host and device memory; eval/video_cli.py on a small .y4m file."""
import numpy as np
import pytest

import tile_map_ref as T
import yuv_ref as R

FMT = R.FORMATS['i420']
LAYOUTS = FMT.layouts      # ('i420', 'nv12')
COLOURS = [(m, f) for m in ('bt709', 'bt601') for f in (False, True)]      # the four colour settings of the 4:2:0 tests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    """A handle with a device and NO weights: the two kernels need none."""
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


# ---- the cut alone ------------------------------------------------------------------------------------------------------------------------
class GpuBackend:
    """film_debug_yuv_cut as a backend of yuv_ref.Format.check_cut: both allocations go up as torch tensors (guard | payload | guard in ONE
    allocation each), the entry point gets the payloads' addresses, both come back."""

    def __init__(self, eng):
        self.eng = eng

    def __call__(self, frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full):
        import torch
        ft, tt = torch.from_numpy(np.array(frames_alloc)).cuda(), torch.from_numpy(np.array(tiles_alloc)).cuda()
        fp, tp = ft.data_ptr() + T.GUARD_U8, tt.data_ptr() + 4 * T.GUARD
        assert fp % 4 == 0 and tp % 16 == 0 and ft.numel() % 4 == 0
        self.eng.debug_yuv_cut(fp, tp, case.B, case.H, case.W, case.align, case.block, tile0, ntiles, pix=layout, matrix=matrix, full_range=full)
        torch.cuda.synchronize()
        return ft.cpu().numpy(), tt.cpu().numpy()


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


@pytest.mark.parametrize('offset', [0, 1, 2], ids=lambda o: f'dst+{o}')
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('h,w', [(2, 2), (16, 18), (30, 50)])
def test_to_yuv420(eng, h, w, layout, offset):
    """dst 4-byte aligned (whole words where the rows allow) and 1 / 2 bytes behind that (bytes): the frame == the restatement, the guard
    bands around it and the source untouched, for all four colour settings."""
    import torch
    n = h * w * 3 // 2
    src = _rgb(h, w, seed=h + w)
    st = torch.from_numpy(src).cuda()
    for ci, (matrix, full) in enumerate(COLOURS):
        alloc = np.random.default_rng(ci).integers(0, 256, T.GUARD_U8 + offset + n + T.GUARD_U8, dtype=np.uint8)
        dt = torch.from_numpy(alloc).cuda()
        assert dt.data_ptr() % 4 == 0 and st.data_ptr() % 16 == 0
        eng.to_yuv420_device(st.data_ptr(), dt.data_ptr() + T.GUARD_U8 + offset, h, w, layout, matrix, full)
        torch.cuda.synchronize()
        got = dt.cpu().numpy()
        want = np.array(alloc)
        want[T.GUARD_U8 + offset:T.GUARD_U8 + offset + n] = FMT.yuv_out(src, layout, matrix, full).ravel()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (matrix, full, bad.size, bad[:8] - T.GUARD_U8 - offset, got[bad[:8]], want[bad[:8]])
    assert np.array_equal(st.cpu().numpy().view(np.uint32), src.view(np.uint32))


# ---- the stream, on the TINY net -----------------------------------------------------------------------------------------------------------
STREAMS = {      # name: (frames, h, w, align, block, block_overlap, (matrix, full_range))
    '64x64': (4, 64, 64, None, None, 0, ('bt709', False)),
    '100x250-b2x2': (4, 100, 250, 64, (2, 2), 0, ('bt601', True)),       # 125-pixel patches: an odd column origin
    '256x256-b2x2-free-overlap': (3, 256, 256, 96, (2, 2), -1, ('bt709', True)),
}
_WANT = {}


def _scene(f, h, w, seed):
    """f I420 frames of a scene that moves by (2, -2) px per frame, with every byte value in the Y plane."""
    base = FMT.designed_frames(1, h, w, seed)[0]
    Y, Cb, Cr = FMT.unpack(base, 'i420')
    return np.stack([FMT.pack(np.roll(Y, (2 * i, -2 * i), (0, 1)), np.roll(Cb, (i, -i), (0, 1)), np.roll(Cr, (i, -i), (0, 1)), 'i420') for i in range(f)])


def _want(tiny, name):
    """(I420 frames, expected I420 mids): yuv_out(interpolate_frames(yuv_in(prev), yuv_in(cur))), computed once per case and shared."""
    if name not in _WANT:
        f, h, w, align, block, overlap, (matrix, full) = STREAMS[name]
        frames = _scene(f, h, w, seed=h + w)
        x = np.stack([FMT.yuv_in(fr, 'i420', matrix, full) for fr in frames])
        tiny.set_block_overlap(overlap)
        try:
            mids = tiny.interpolate_frames(x[:-1], x[1:], align=align, block_shape=block)
        finally:
            tiny.set_block_overlap(0)
        assert np.isfinite(mids).all()
        want = np.stack([FMT.yuv_out(m, 'i420', matrix, full) for m in mids])
        frames.setflags(write=False); want.setflags(write=False)
        _WANT[name] = frames, want
    return _WANT[name]


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', list(STREAMS))
def test_stream(tiny, name, layout, mem):
    """Every push's mid == yuv_out(interpolate_frames(yuv_in(previous), yuv_in(frame))), byte for byte - also the push after "fuse" 31 -> 0
    -> 31 dropped every plan (the stream cuts the 4:2:0 frame it kept again); the NV12 bytes are the I420 bytes re-interleaved."""
    f, h, w, align, block, overlap, (matrix, full) = STREAMS[name]
    frames, want = _want(tiny, name)
    if layout == 'nv12':
        frames = np.stack([R.convert_layout(fr, 'i420', 'nv12') for fr in frames])
        want = np.stack([R.convert_layout(m, 'i420', 'nv12') for m in want])

    def drop_plans():
        tiny.set_option('fuse', 0)
        tiny.set_option('fuse', 31)

    tiny.set_block_overlap(overlap)
    try:
        if mem == 'host':
            with tiny.open_stream(h, w, align=align, block_shape=block, pix=layout, matrix=matrix, full_range=full) as st:
                assert st.shape == (h * 3 // 2, w) and st.dtype is np.uint8
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
                    outs.append(st.push(torch.from_numpy(np.array(fr)).cuda()))
                torch.cuda.synchronize()
                got = [None if o is None else o.cpu().numpy() for o in outs]
    finally:
        tiny.set_block_overlap(0)
    assert got[0] is None
    for j in range(f - 1):
        g = got[j + 1]
        assert g.dtype == np.uint8 and g.shape == (h * 3 // 2, w)
        bad = np.flatnonzero(g.ravel() != want[j].ravel())
        assert bad.size == 0, (j, bad.size, bad[:8], g.ravel()[bad[:8]], want[j].ravel()[bad[:8]])
    assert len({m.tobytes() for m in want}) == f - 1       # (the mids differ from each other: a stale result would show)


# ---- the Y4M tool --------------------------------------------------------------------------------------------------------------------------
def test_video_cli(tiny, tmp_path, monkeypatch):
    """A 5-frame 64 x 64 .y4m through eval.video_cli: 9 frames out, the 5 originals verbatim, the mids equal to the stream's, F doubled."""
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
    tokens = y4m.header_tokens(64, 64, (24, 1))
    with open(src, 'wb') as f:
        w = y4m.Y4MWriter(f, tokens)
        for fr in frames:
            w.write(fr)
    with tiny.open_stream(64, 64, align=64, pix='i420', matrix='bt601') as st:
        mids = [st.push(fr) for fr in frames][1:]
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    assert cli.main(['--input', str(src), '--output', str(dst), '--matrix', 'bt601']) == 9
    with open(dst, 'rb') as f:
        r = y4m.Y4MReader(f)
        got = list(r)
    assert r.tokens == ['W64', 'H64', 'F48:1'] + tokens[3:]
    assert len(got) == 9
    for i in range(5):
        assert np.array_equal(got[2 * i], frames[i]), i
    for i in range(4):
        assert np.array_equal(got[2 * i + 1], mids[i]), i
    assert not np.array_equal(mids[0], mids[1])
