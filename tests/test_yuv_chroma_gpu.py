"""GPU tests of the planar 4:2:2 / 4:4:4 layouts (FILM_PIX_I422 / I444 / I210 / I410) and of the BT.2020 matrix flag, bit for bit against the
numpy restatement tests/yuv_ref.py (include/film_hip.h, "The 4:2:2 and 4:4:4 arithmetic"): the cut alone through film_debug_yuv_cut on
designed data with guard bands (tests/test_yuv_chroma_cpu.py shows which instance and branch every case reaches and that the comparison
finds each planted fault); the quantiser alone through film_to_yuv; the histogram through film_frame_histogram; frame streams on the TINY
net from host and device memory, with a selection and with "scene_cut"; eval/video_cli.py on a small C444p10 file.  No tolerance anywhere."""
import numpy as np
import pytest

import tile_map_ref as T
import yuv_ref as R

pytestmark = pytest.mark.gpu
NEW = R.NEW_LAYOUTS
COLOURS = [(m, f) for m in R.MATRICES for f in (False, True)]      # the six colour settings


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


def _up(samples):
    """uint8 / uint16 samples -> a CUDA tensor of the same bits (16-bit: int16, which every torch has)."""
    import torch
    a = np.ascontiguousarray(samples)
    return torch.from_numpy((a.view(np.int16) if a.dtype == np.uint16 else a).copy()).cuda()


def _down(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---- the cut alone ------------------------------------------------------------------------------------------------------------------------
class GpuBackend:
    """film_debug_yuv_cut as a backend of yuv_ref.Format.check_cut: both allocations go up as torch tensors (guard | payload | guard in ONE
    allocation each, the frames' a whole number of 32-bit words), the entry point gets the payloads' addresses, both come back."""

    def __init__(self, eng, fmt):
        self.eng, self.fmt = eng, fmt

    def __call__(self, frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full):
        import torch
        f = self.fmt
        ft, tt = _up(frames_alloc), torch.from_numpy(np.array(tiles_alloc)).cuda()
        fp, tp = ft.data_ptr() + f.dtype.itemsize * f.guard, tt.data_ptr() + 4 * T.GUARD
        assert fp % 4 == 0 and tp % 16 == 0 and ft.numel() % f.per_word == 0
        self.eng.debug_yuv_cut(fp, tp, case.B, case.H, case.W, case.align, case.block, tile0, ntiles, pix=layout, matrix=matrix, full_range=full)
        torch.cuda.synchronize()
        return _down(ft, f.dtype), tt.cpu().numpy()


@pytest.mark.parametrize('layout,case', [(lay, c) for lay in NEW for c in R.cases_of(lay)], ids=lambda v: v if isinstance(v, str) else v.name)
def test_cut(eng, layout, case):
    """All six colour settings, every range of every partition: tiles_dev[0 : ntiles] == the restatement on the bits, the padding +0.0,
    the rest of the tile tensor, its guards and the frames untouched, the same bits from the same call again."""
    f = R.FORMATS[layout]
    eng.set_block_overlap(case.overlap)
    try:
        geo = eng.tiling(case.H, case.W, case.align, case.block)
        backend = GpuBackend(eng, f)
        findings = [f'[{name}] {m}' for matrix, full in COLOURS for name, ranges in R.ranges_of(case, geo).items()
                    for m in f.check_cut(backend, case, geo, layout, matrix, full, ranges, seed=17)]
    finally:
        eng.set_block_overlap(0)
    assert not findings, f'{len(findings)} findings:\n' + '\n'.join(findings[:12])


# ---- film_to_yuv alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', R.OUT_OFFSETS, ids=lambda o: f'dst+{o}')
@pytest.mark.parametrize('layout,hw', [(lay, hw) for lay in NEW + ('i420', 'p010') for hw in R.out_sizes(lay)], ids=str)
def test_to_yuv(eng, layout, hw, offset):
    """dst on a 4-byte boundary (whole words where the rows allow) and one sample behind it, input outside [0, 1]: the frame == the
    restatement, the guard bands around it and the source untouched - all six colour settings for the new layouts, 'bt2020nc' for I420 and
    P010 (through film_to_yuv and through film_to_yuv420)."""
    import torch
    f = R.FORMATS[layout]
    h, w = hw
    n = f.samples(h, w)
    src = R.designed_rgb(h, w, seed=h + w)
    assert (src < 0).any() and (src > 1).any()
    st = torch.from_numpy(src).cuda()
    colours = COLOURS if layout in NEW else [('bt2020nc', False), ('bt2020nc', True)]
    for ci, (matrix, full) in enumerate(colours):
        size = -(-(2 * f.guard + offset + n) // f.per_word) * f.per_word
        alloc = np.random.default_rng(ci).integers(0, 1 << 8 * f.dtype.itemsize, size).astype(f.dtype)
        want = np.array(alloc)
        want[f.guard + offset:f.guard + offset + n] = f.yuv_out(src, layout, matrix, full).ravel()
        for call in (eng.to_yuv_device,) + (() if layout in NEW else (eng.to_yuv420_device,)):
            dt = _up(alloc)
            assert dt.data_ptr() % 4 == 0 and st.data_ptr() % 16 == 0
            call(st.data_ptr(), dt.data_ptr() + f.dtype.itemsize * (f.guard + offset), h, w, layout, matrix, full)
            torch.cuda.synchronize()
            got = _down(dt, f.dtype)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (matrix, full, bad.size, bad[:8] - f.guard - offset, got[bad[:8]], want[bad[:8]])
    assert np.array_equal(st.cpu().numpy().view(np.uint32), src.view(np.uint32))


def test_to_yuv420_refuses_the_new_layouts(eng):
    from film_hip.engine import FilmError
    for layout in NEW:
        with pytest.raises(FilmError):
            eng.to_yuv420_device(4096, 4096, 4, 4, layout)


# ---- the histogram --------------------------------------------------------------------------------------------------------------------------
HIST_GUARD = 16     # guard words around the 768 counters


@pytest.mark.parametrize('layout,hw', [(lay, hw) for lay in NEW for hw in ((30, 50), R.smallest(lay), (33, 51) if lay in ('i444', 'i410') else (33, 50))], ids=str)
def test_histogram(layout, hw):
    """film_frame_histogram == numpy bincount per plane (10 bits: of code >> 2), on designed frames inside guard samples whose code is in no
    plane, with the frame starting 0, 4, 8 and 12 bytes behind a 16-byte boundary: no guard sample counted (a 4:4:4 frame of odd size ends
    inside a word), the plane sums [HW, C, C], the counters' guards untouched, the same counters from a second call, the frame unmodified;
    and through torch_io.frame_histogram."""
    import torch
    from film_hip.engine import frame_histogram_device
    from film_hip.torch_io import frame_histogram
    f = R.FORMATS[layout]
    h, w = hw
    shift = f.depth - 8
    frame = np.array(f.designed_frames(1, h, w, h + w, layout)[0])
    frame[(f.code(frame, layout) >> shift) == 77] = 80 << shift          # bin 77 is the guard's
    guard_sample = (77 << shift) | (1 if shift else 0) | (0x0400 if shift else 0)
    want = f.histogram(frame, layout)
    ch, cw = f.chroma_shape(h, w)
    assert want[:, 77].sum() == 0 and want.sum(1).tolist() == [h * w, ch * cw, ch * cw]
    n = f.samples(h, w)
    for offset_words in (0, 1, 2, 3):
        front = (32 + offset_words) * f.per_word
        back = 32 * f.per_word + (-n) % f.per_word      # (the allocation: whole 32-bit words)
        alloc = np.concatenate([np.full(front, guard_sample, f.dtype), frame.ravel(), np.full(back, guard_sample, f.dtype)])
        ft = _up(alloc)
        assert ft.data_ptr() % 16 == 0 and alloc.size % f.per_word == 0
        noise = np.random.default_rng(5).integers(1, 2 ** 32, 768 + 2 * HIST_GUARD, dtype=np.uint32)
        ht = torch.from_numpy(noise.view(np.int32).copy()).cuda()
        for rep in range(2):
            frame_histogram_device(ft.data_ptr() + f.dtype.itemsize * front, h, w, ht.data_ptr() + 4 * HIST_GUARD, layout, 'bt2020nc')
            torch.cuda.synchronize()
            got = ht.cpu().numpy().view(np.uint32)
            counters = got[HIST_GUARD:HIST_GUARD + 768].astype(np.int64).reshape(3, 256)
            bad = np.argwhere(counters != want)
            assert bad.size == 0, (layout, h, w, offset_words, rep, len(bad), bad[:6].tolist(), counters[tuple(bad[:6].T)].tolist(), want[tuple(bad[:6].T)].tolist())
            assert np.array_equal(got[:HIST_GUARD], noise[:HIST_GUARD]) and np.array_equal(got[-HIST_GUARD:], noise[-HIST_GUARD:])
        assert np.array_equal(_down(ft, f.dtype), alloc)
    if n % f.per_word == 0:      # (a tensor of the frame alone is a whole number of words)
        for t in [_up(frame)] + ([torch.from_numpy(frame.copy()).cuda()] if f.depth == 10 and hasattr(torch, 'uint16') else []):
            got = frame_histogram(t, layout)
            torch.cuda.synchronize()
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)


# ---- the stream, on the TINY net -----------------------------------------------------------------------------------------------------------
STREAMS = {      # name: (frames, h, w, align, block, (matrix, full_range), layouts)
    '64x64': (4, 64, 64, None, None, ('bt2020nc', False), NEW),
    '99x250-b3x2': (3, 99, 250, 64, (3, 2), ('bt601', True), ('i422', 'i210')),          # 33 x 125 patches: odd origins in both axes, an odd H
    '99x249-b3x3': (3, 99, 249, 64, (3, 3), ('bt2020nc', True), ('i444', 'i410')),       # 33 x 83 patches, an odd W
}
_WANT = {}


def _scene(layout, n, h, w, seed):
    """n frames (clean codes) of a scene that moves by (2, -2) px per frame, designed codes in every plane."""
    f = R.FORMATS[layout]
    Y, Cb, Cr = (f.code(p, layout).astype(f.dtype) for p in f.unpack(f.designed_frames(1, h, w, seed, layout)[0], layout))
    cy, cx = 2 >> f.sy, 2 >> f.sx
    return np.stack([f.pack(np.roll(Y, (2 * i, -2 * i), (0, 1)), np.roll(Cb, (cy * i, -cx * i), (0, 1)), np.roll(Cr, (cy * i, -cx * i), (0, 1)), layout) for i in range(n)])


def _want(tiny, name, layout):
    """(frames, expected mids): yuv_out(interpolate_frames(yuv_in(prev), yuv_in(cur))), computed once per case and layout and shared."""
    if (name, layout) not in _WANT:
        n, h, w, align, block, (matrix, full), _ = STREAMS[name]
        f = R.FORMATS[layout]
        frames = _scene(layout, n, h, w, seed=h + w)
        x = np.stack([f.yuv_in(fr, layout, matrix, full) for fr in frames])
        mids = tiny.interpolate_frames(x[:-1], x[1:], align=align, block_shape=block)
        assert np.isfinite(mids).all()
        want = np.stack([f.yuv_out(m, layout, matrix, full) for m in mids])
        frames.setflags(write=False); want.setflags(write=False)
        _WANT[name, layout] = frames, want
    return _WANT[name, layout]


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('name,layout', [(name, lay) for name, v in STREAMS.items() for lay in v[6]])
def test_stream(tiny, name, layout, mem):
    """Every push's mid == yuv_out(interpolate_frames(yuv_in(previous), yuv_in(frame))), code for code - also the push after "fuse" 31 -> 0
    -> 31 dropped every plan (the stream cuts the frame it kept again).  Ten-bit frames carry junk in the ignored bits."""
    n, h, w, align, block, (matrix, full), _ = STREAMS[name]
    f = R.FORMATS[layout]
    frames, want = _want(tiny, name, layout)
    frames = np.stack([f.with_junk(fr, layout, 7 + i) for i, fr in enumerate(frames)])
    shape = (f.rows(h), w)

    def drop_plans():
        tiny.set_option('fuse', 0)
        tiny.set_option('fuse', 31)

    if mem == 'host':
        with tiny.open_stream(h, w, align=align, block_shape=block, pix=layout, matrix=matrix, full_range=full) as st:
            assert st.shape == shape and st.dtype is f.dtype.type
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
                t = torch.from_numpy(np.array(fr)).cuda() if i == n - 1 and f.depth == 10 and hasattr(torch, 'uint16') else _up(fr)
                outs.append(st.push(t))
                assert outs[-1] is None or outs[-1].dtype == t.dtype        # results come back in the dtype that was pushed
            torch.cuda.synchronize()
            got = [None if o is None else o.cpu().numpy().view(f.dtype) for o in outs]
    assert got[0] is None
    for j in range(n - 1):
        g = got[j + 1]
        assert g.dtype == f.dtype and g.shape == shape
        bad = np.flatnonzero(g.ravel() != want[j].ravel())
        assert bad.size == 0, (j, bad.size, bad[:8], g.ravel()[bad[:8]], want[j].ravel()[bad[:8]])
    assert len({m.tobytes() for m in want}) == n - 1       # (the mids differ from each other: a stale result would show)


def test_stream_select_on_i210(tiny):
    """A times = 2 stream with select([1, 3]) on 'i210': each frame == film_to_yuv of the float32 frame that pairwise film_interpolate calls
    on float32 parents give - the selected frames are quantised only on the way out, their parent (position 2) never is."""
    import torch
    layout, (matrix, full), h, w = 'i210', ('bt2020nc', False), 64, 64
    f = R.FORMATS[layout]
    frames = _scene(layout, 2, h, w, seed=11)
    x0, x1 = (f.yuv_in(fr, layout, matrix, full)[None] for fr in frames)
    m2 = tiny.interpolate_frames(x0, x1)
    floats = [tiny.interpolate_frames(x0, m2)[0], tiny.interpolate_frames(m2, x1)[0]]
    want = []
    for m in floats:
        st, dt = torch.from_numpy(m).cuda(), _up(np.zeros(f.samples(h, w), f.dtype))
        tiny.to_yuv_device(st.data_ptr(), dt.data_ptr(), h, w, layout, matrix, full)
        torch.cuda.synchronize()
        want.append(_down(dt, f.dtype).reshape(f.rows(h), w))
        assert np.array_equal(want[-1], f.yuv_out(m, layout, matrix, full))
    with tiny.open_stream(h, w, pix=layout, matrix=matrix, full_range=full, times=2) as st:
        st.select([1, 3])
        assert st.push(frames[0]) is None
        got = st.push(frames[1])
    assert got.shape == (2, f.rows(h), w) and got.dtype == f.dtype
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not np.array_equal(want[0], want[1])


def test_stream_scene_cut_on_i444(tiny):
    """An 'i444' stream with "scene_cut" set: D and S = 3 H W of cut_info are those of the restatement's histograms, the rule
    1000 D >= k * 2 S decides, and a cut push produces nothing."""
    layout, h, w = 'i444', 64, 64
    f = R.FORMATS[layout]
    frames = _scene(layout, 3, h, w, seed=9)
    other = f.pack(*[(p // 2).astype(f.dtype) for p in f.unpack(frames[0], layout)], layout)      # halved codes: a different histogram
    seq = [frames[0], frames[1], other, frames[2]]
    hists = [f.histogram(fr, layout) for fr in seq]
    D = [int(np.abs(hists[i] - hists[i - 1]).sum()) for i in range(1, 4)]
    S = 3 * h * w
    k = 300
    assert 1000 * D[0] < k * 2 * S <= 1000 * D[1] and 1000 * D[2] >= k * 2 * S
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
    """A 3-frame 33 x 63 C444p10 .y4m through eval.video_cli --chroma any --matrix bt2020nc: 5 frames out, the originals verbatim, the mids
    equal to the restatement's, F doubled."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, **kw):
        it = real.__new__(real)
        it._options, it._engine = tiny.options, tiny
        it._align, it._block_shape = align or None, block_shape or None
        return it

    layout, h, w = 'i410', 33, 63
    f = R.FORMATS[layout]
    frames = _scene(layout, 3, h, w, seed=5)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    tokens = y4m.header_tokens(w, h, (24, 1), colour='444p10')
    with open(src, 'wb') as fo:
        wr = y4m.Y4MWriter(fo, tokens)
        for fr in frames:
            wr.write(fr)
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    with pytest.raises(y4m.Y4MError):
        cli.main(['--input', str(src), '--output', str(dst), '--matrix', 'bt2020nc'])
    assert cli.main(['--input', str(src), '--output', str(dst), '--chroma', 'any', '--matrix', 'bt2020nc']) == 5
    with open(dst, 'rb') as fi:
        r = y4m.Y4MReader(fi, depths=(8, 10), chroma=('420', '422', '444'))
        got = list(r)
    assert r.tokens == [f'W{w}', f'H{h}', 'F48:1'] + tokens[3:] and r.pix == layout
    assert len(got) == 5 and all(g.dtype == np.uint16 and g.shape == (3 * h, w) for g in got)
    x = np.stack([f.yuv_in(fr, layout, 'bt2020nc') for fr in frames])
    mids = tiny.interpolate_frames(x[:-1], x[1:], align=64)
    for i in range(3):
        assert np.array_equal(got[2 * i], frames[i]), i
    for i in range(2):
        assert np.array_equal(got[2 * i + 1], f.yuv_out(mids[i], layout, 'bt2020nc')), i
    assert not np.array_equal(got[1], got[3])
