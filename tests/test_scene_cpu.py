"""CPU tests of the scene-cut detector (include/film_hip.h, "Scene cuts"): known answers of the numpy restatement tests/scene_ref.py that
tests/test_scene_gpu.py compares the kernel and the streams with; the rule at its boundary; the two entry points, the option and every
refusal of film_frame_histogram on a plan-only handle; the frame hold of eval/video_cli.py; and three faults planted in a numpy model of the
kernel, each found by the comparison the GPU test makes.  No GPU."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import scene_ref as S
from conftest import ROOT


# ---- known answers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pix', S.LAYOUTS)
def test_identical_rolled_and_disjoint_frames(pix):
    h, w = 30, 50
    n = S.samples(h, w, pix)
    a = S.to_layout(S.designed_codes(n, 1), h, w, pix)
    ha = S.histogram(a, pix)
    assert ha.shape == (3, 256) and ha.dtype == np.int64
    assert ha.sum(1).tolist() == ([h * w] * 3 if pix in ('u8', 'f32') else [h * w, h * w // 4, h * w // 4])     # every plane sums to its samples
    assert S.distance(ha, S.histogram(a.copy(), pix)) == 0
    if pix in ('u8', 'f32'):
        rolled = np.roll(a, (3, -7), (0, 1))
    else:                                # the Y plane rolled as a picture, the chroma bytes of each plane among themselves
        pl = S.planes(a, pix)
        y = np.roll(pl[0].reshape(h, w), (3, -7), (0, 1)).ravel()
        cb, cr = np.roll(pl[1], 5), np.roll(pl[2], 11)
        c = np.concatenate([cb, cr]) if pix == 'i420' else np.stack([cb, cr], -1).ravel()
        rolled = np.concatenate([y, c]).reshape(a.shape)
    assert not np.array_equal(rolled, a) and S.distance(ha, S.histogram(rolled, pix)) == 0
    c0, c1 = S.to_layout(np.full(n, 17), h, w, pix), S.to_layout(np.full(n, 200), h, w, pix)
    D = S.distance(S.histogram(c0, pix), S.histogram(c1, pix))
    assert D == 2 * n and S.is_cut(D, n, 1000)


@pytest.mark.parametrize('pix', S.LAYOUTS)
def test_quarter_change_scene(pix):
    """The frames of the stream tests: D = 0 inside a scene, exactly S / 2 across the cut, 255 unused in scene A."""
    fr = S.scene_frames(pix)
    n = S.samples(64, 64, pix)
    hs = [S.histogram(f, pix) for f in fr]
    assert hs[0][:, 255].sum() == 0 and hs[0][:, :16].sum() == 0 and hs[0][:, 236:].sum() == 0
    assert [S.distance(hs[i], hs[i + 1]) for i in range(5)] == [0, 0, n // 2, 0, 0] and n % 4 == 0
    assert not np.array_equal(fr[0], fr[1]) and not np.array_equal(fr[3], fr[4])
    assert S.is_cut(n // 2, n, 250) and not S.is_cut(n // 2, n, 251)


def test_nv12_equals_i420_of_the_reinterleaved_frame():
    h, w = 16, 18
    nv = S.to_layout(S.designed_codes(S.samples(h, w, 'nv12'), 2), h, w, 'nv12')
    y, cb, cr = S.planes(nv, 'nv12')
    i4 = np.concatenate([y, cb, cr]).reshape(nv.shape)
    assert not np.array_equal(i4, nv)
    assert np.array_equal(S.histogram(nv, 'nv12'), S.histogram(i4, 'i420'))
    assert not np.array_equal(S.histogram(nv, 'nv12'), S.histogram(nv, 'i420'))       # (the layouts differ on the same bytes)


def test_f32_follows_film_to_uint8s_rule():
    u8 = S.designed_codes(5 * 7 * 3, 3).reshape(5, 7, 3)
    assert np.array_equal(S.histogram(u8.astype(np.float32) / np.float32(255), 'f32'), S.histogram(u8, 'u8'))
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(S.quantise(every.astype(np.float32) / np.float32(255)), every)
    # below 0 -> 0, above 1 -> 255, NaN-free; at (v + 0.5) / 255 the value x * 255 is within an ulp of the tie v + 0.5: the rule's own float32 answer
    assert S.quantise(np.float32([-0.0, -1e-9, -3, -np.inf])).tolist() == [0, 0, 0, 0]
    assert S.quantise(np.float32([1, 1 + 1e-6, 7, np.inf])).tolist() == [255, 255, 255, 255]
    v = np.arange(255, dtype=np.float64)
    x = ((v + 0.5) / 255).astype(np.float32)
    prod = x * np.float32(255)                                     # one float32 rounding
    want = np.floor(prod.astype(np.float64) + 0.5)                 # + 0.5 is exact or rounds to even in float32 ...
    want32 = (prod + np.float32(0.5)).astype(np.uint8)             # ... which this is
    got = S.quantise(x)
    assert np.array_equal(got, want32) and (np.abs(got.astype(np.float64) - want) <= 1).all()
    assert set((got.astype(np.int64) - v.astype(np.int64)).tolist()) <= {0, 1}      # a tie lands on one of its two neighbours
    assert S.quantise(np.float32(0.4999 / 255)) == 0 and S.quantise(np.float32(0.5001 / 255)) == 1


def test_rule_at_its_boundary():
    n = 3 * 64 * 64
    assert S.is_cut(n // 2, n, 250) is True and S.is_cut(n // 2, n, 251) is False
    assert S.is_cut(n // 2 - 1, n, 250) is False and S.is_cut(n // 2 + 1, n, 250) is True
    assert S.is_cut(2 * n, n, 1000) and not S.is_cut(2 * n - 1, n, 1000) and S.is_cut(1, n, 1) is False and S.is_cut(25, n, 1)
    big = 3 * (2 ** 31 - 1)                  # the largest S the entry point admits: the products stay inside int64
    assert 1000 * 2 * big < 2 ** 63 and S.is_cut(2 * big, big, 1000) and not S.is_cut(2 * big - 1, big, 1000)
    for k in (0, 1001):
        with pytest.raises(AssertionError):
            S.is_cut(1, n, k)


# ---- the C-ABI on a plan-only handle --------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_loadable():
    from film_hip import engine
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    assert re.search(r'^int film_frame_histogram\(const void\* frame_dev, int H, int W, int pix, uint32_t\* hist_dev, void\* stream\);', header, re.M)
    assert re.search(r'^int film_stream_cut_info\(film_t\* h, int64_t\* distance, int64_t\* samples, int\* cut\);', header, re.M)
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    lib = engine.load_library()
    for sym in ('film_frame_histogram', 'film_stream_cut_info'):
        assert re.search(rf'\b{sym};', mapfile) and sym in engine.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    assert len(lib.film_frame_histogram.argtypes) == 6 and len(lib.film_stream_cut_info.argtypes) == 4


def test_header_states_what_is_unmeasured_and_unseen():
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    for text in (header, readme):
        low = text.lower()
        assert 'unmeasured' in low and 'alike histograms' in low and 'fades' in low and 'flashes' in low
    assert re.search(r'"scene_cut" k', header) and '1000 D >= k * 2 S' in header


def test_scene_cut_option_range():
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    try:
        for ok in (0, 1000, 250, 0):
            eng.set_option('scene_cut', ok)
        for bad in (-1, 1001):
            with pytest.raises(FilmError) as e:
                eng.set_option('scene_cut', bad)
            assert e.value.code == FILM_ERR_INVALID and e.value.msg.startswith('scene_cut'), e.value.msg
    finally:
        eng.close()


def test_histogram_refusals_come_before_any_device_call():
    """A pointer that is never dereferenced, in a process that may have no device: every refused call returns FILM_ERR_INVALID."""
    from film_hip import engine
    from film_hip.engine import FILM_ERR_INVALID
    lib = engine.load_library()
    P = ctypes.c_void_p(4096)

    def call(frame=P, H=30, W=50, pix=1, hist=P):
        return lib.film_frame_histogram(frame, H, W, pix, hist, None)

    assert call(frame=None) == FILM_ERR_INVALID and call(hist=None) == FILM_ERR_INVALID
    for H, W in ((0, 50), (30, 0), (-1, 50), (30, -4)):
        assert call(H=H, W=W) == FILM_ERR_INVALID, (H, W)
    for H, W in ((1 << 16, 1 << 15), (46341, 46341), (2 ** 31 - 1, 2)):      # H * W >= 2^31
        assert call(H=H, W=W) == FILM_ERR_INVALID, (H, W)
        assert call(H=H, W=W, pix=0) == FILM_ERR_INVALID, (H, W)
    for pix in (2, -1, 15, 18, 16 | 0x200, 17 | 0x1000, 0 | 0x100, 1 | 0x400):
        assert call(pix=pix) == FILM_ERR_INVALID, pix
    for pix in (16, 17, 16 | 0x100, 17 | 0x400):                        # 4:2:0 needs even sizes
        for H, W in ((31, 48), (32, 47), (31, 47)):
            assert call(H=H, W=W, pix=pix) == FILM_ERR_INVALID, (pix, H, W)
    for off in (1, 2, 3):
        for pix in (0, 1, 16, 17):
            assert call(frame=ctypes.c_void_p(4096 + off), H=32, W=48, pix=pix) == FILM_ERR_INVALID, (off, pix)


def test_cut_info_without_a_stream_is_a_state_error():
    from film_hip.engine import FilmEngine, FILM_ERR_STATE
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    try:
        d, n, c = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int(7)
        assert eng._lib.film_stream_cut_info(eng._h, ctypes.byref(d), ctypes.byref(n), ctypes.byref(c)) == FILM_ERR_STATE
        assert eng._lib.film_stream_cut_info(eng._h, None, None, None) == FILM_ERR_STATE
        assert (d.value, n.value, c.value) == (7, 7, 7)
    finally:
        eng.close()


# ---- eval/video_cli.py: the frame hold ----------------------------------------------------------------------------------------------------------
def test_video_cli_holds_the_frame_before_a_cut():
    from eval import video_cli as cli
    from film_hip import y4m
    assert cli.build_parser().parse_args(['--input', 'i', '--output', 'o']).scene_cut == 0
    assert cli.build_parser().parse_args(['--input', 'i', '--output', 'o', '--scene_cut', '250']).scene_cut == 250

    class Stream:
        def __init__(self, cut_at): self.prev, self.i, self.cut_at = None, -1, cut_at
        def __enter__(self): return self
        def __exit__(self, *exc): pass
        def push(self, frame):
            self.i += 1
            mid = None if self.prev is None or self.i == self.cut_at else ((self.prev.astype(np.int32) + frame) // 2).astype(np.uint8)
            self.prev = frame
            return mid

    class It:
        def __init__(self, cut_at): self.cut_at, self.kw = cut_at, None
        def open_stream(self, h, w, pix, matrix, full_range, **kw):
            self.kw = kw
            return Stream(self.cut_at if kw.get('scene_cut') else None)

    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (6, 6, 6), dtype=np.uint8)        # six 4 x 6 I420 frames
    tokens = y4m.header_tokens(6, 4, (25, 1))
    data = io.BytesIO()
    wr = y4m.Y4MWriter(data, tokens)
    for f in frames:
        wr.write(f)

    def run(scene_cut):
        it, out, cuts = It(3), io.BytesIO(), []
        kw = {'scene_cut': scene_cut, 'cuts': cuts} if scene_cut else {}
        n = cli.double_frame_rate(it, y4m.Y4MReader(io.BytesIO(data.getvalue())), out, 'bt709', None, **kw)
        got = list(y4m.Y4MReader(io.BytesIO(out.getvalue())))
        assert n == len(got)
        return it, got, cuts

    it0, plain, _ = run(0)
    assert it0.kw == {} and len(plain) == 11                     # (without the flag the stream is opened as before)
    it1, held, cuts = run(250)
    assert it1.kw == {'scene_cut': 250} and cuts == [3]
    assert len(held) == 11
    assert np.array_equal(held[5], frames[2])                    # the hold: the input before the cut, verbatim
    assert not np.array_equal(plain[5], frames[2])
    for i in range(11):
        if i != 5:
            assert np.array_equal(held[i], plain[i]), i
    for i in range(6):
        assert np.array_equal(held[2 * i], frames[i]), i


# ---- planted faults in a model of the kernel ------------------------------------------------------------------------------------------------------
def _gpu_comparison(got, frame, pix):
    """What tests/test_scene_gpu.py asserts of the 768 counters."""
    return np.array_equal(np.asarray(got, np.int64).reshape(3, 256), S.histogram(frame, pix))


def test_kernel_model_agrees_and_planted_faults_are_found():
    for pix in S.LAYOUTS:
        for h, w in ((1, 1), (2, 2), (5, 7), (16, 18), (30, 50)):
            if pix in S.YUV and (h % 2 or w % 2):
                continue
            frame = S.to_layout(S.designed_codes(S.samples(h, w, pix), h * w), h, w, pix)
            for head in (0, 4, 12) if pix != 'f32' else (0, 1, 3):
                assert _gpu_comparison(S.kernel_model(frame, pix, head=head), frame, pix), (pix, h, w, head)
    # 1: the last partial 16-byte vector dropped - every shape of the GPU test whose bytes are no multiple of 16 shows it
    for pix, (h, w) in (('u8', (1, 1)), ('u8', (5, 7)), ('i420', (2, 2)), ('nv12', (30, 50)), ('f32', (5, 7)), ('u8', (30, 50))):
        frame = S.to_layout(S.designed_codes(S.samples(h, w, pix), 9), h, w, pix)
        assert (frame.size * (4 if pix == 'f32' else 1)) % 16
        assert not _gpu_comparison(S.kernel_model(frame, pix, 'drop_tail'), frame, pix), (pix, h, w)
    # 2: Cb and Cr swapped for NV12 - designed data, whose codes have unequal counts, and random bytes show it; a constant frame cannot
    for h, w in ((2, 2), (16, 18), (30, 50)):
        frame = S.to_layout(S.designed_codes(S.samples(h, w, 'nv12'), 5), h, w, 'nv12')
        assert not _gpu_comparison(S.kernel_model(frame, 'nv12', 'swap_cbcr'), frame, 'nv12'), (h, w)
    # 3: truncation instead of + 0.5 for F32 - frames u8 / 255.0f HIDE it (x * 255 lands on the integer for every code), which is why the GPU
    # test's F32 frames carry half-way and out-of-range values (scene_ref.f32_test_frame is that data)
    u = S.to_layout(S.designed_codes(16 * 18 * 3, 6), 16, 18, 'f32')
    assert _gpu_comparison(S.kernel_model(u, 'f32', 'truncate'), u, 'f32')
    for h, w in ((1, 1), (2, 2), (5, 7), (16, 18), (30, 50)):
        x = S.f32_test_frame(h, w, seed=h + w)
        assert _gpu_comparison(S.kernel_model(x, 'f32'), x, 'f32')
        assert not _gpu_comparison(S.kernel_model(x, 'f32', 'truncate'), x, 'f32'), (h, w)
