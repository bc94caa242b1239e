"""GPU tests of frame streams that drop duplicate frames (options "dup_hi" / "dup_lo" / "dup_frac"; include/film_hip.h, "Duplicate frames"),
on the TINY net: a push judged a duplicate reports dup = 1 and the restatement's statistics (tests/frame_diff_ref.py), produces nothing,
leaves `out` and the stream untouched, and the next real push returns the bits of a plain stream that never saw the dropped frames - from
host and device memory, for an RGB, an 8-bit and a 10-bit Y'CbCr layout, with recursion and a selection, and beside option "scene_cut"; and
the eval.video_cli --dedup command end to end."""
import io

import numpy as np
import pytest

import frame_diff_ref as R
from film_hip import pixfmt

pytestmark = pytest.mark.gpu

H = W = 256
LAYOUTS = ('u8', 'i420', 'p010')


@pytest.fixture(scope='module')
def tiny():
    from film_hip import weights as Wt
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    e = FilmEngine(TINY, device=0)
    e.set_weights(Wt.make_synthetic_weights(TINY, seed=0))
    yield e
    e.close()


def _options_off(eng):
    for key, v in (('dup_hi', -1), ('dup_lo', 0), ('dup_frac', 1000), ('scene_cut', 0)):
        eng.set_option(key, v)


_FRAMES = {}


def _frames(pix):
    """A, A' (A with ONE sample of the Y / R plane moved by one code), B, and A rolled along its rows (the same samples per plane: histogram
    distance 0) - and C, which shares no code with A (histogram distance 2 S)."""
    if pix not in _FRAMES:
        rng = np.random.default_rng(17)
        lay = pixfmt.BY_NAME[pix]
        shape = pixfmt.frame_shape(pix, H, W)
        top, sh = (1 << (lay.depth or 8)), (6 if pix == 'p010' else 0)

        def codes(lo, hi):
            return (rng.integers(lo * top // 256, hi * top // 256, shape) << sh).astype(lay.dtype)

        a, b, c = codes(16, 120), codes(16, 120), codes(140, 236)
        a1 = R.with_sample(a, pix, 0, 77, 131, 1)
        fr = dict(A=a, A1=a1, B=b, C=c, Aroll=np.ascontiguousarray(np.roll(a, 6, axis=1)))
        for f in fr.values():
            f.setflags(write=False)
        assert R.frame_diff(a, a1, pix)[0][:3] == [1, 1, 1]
        _FRAMES[pix] = fr
    return _FRAMES[pix]


def _run(eng, pix, mem, frames, dedup=None, times=1, select=None, scene_cut=0, guard_out_at=None):
    """Pushes the frames through a fresh stream; returns (results, dup_info and cut_info after every push, the pre-filled `out` of push
    guard_out_at).  The engine's options are off again afterwards."""
    got, dups, cuts, guarded = [], [], [], None
    _options_off(eng)
    try:
        if mem == 'host':
            with eng.open_stream(H, W, pix=pix, scene_cut=scene_cut, times=times, dedup=dedup) as st:
                if select is not None:
                    st.select(select)
                for i, fr in enumerate(frames):
                    out = None
                    if i == guard_out_at:
                        out = np.full(st.shape if times == 1 else (len(st.selection),) + st.shape, 9, st.dtype)
                        guarded = out
                    r = st.push(fr, out)
                    got.append(None if r is None else np.array(r))
                    dups.append(st.dup_info())
                    cuts.append(st.cut_info())
        else:
            import torch
            from film_hip.torch_io import DeviceInterpolator
            with DeviceInterpolator(eng).stream(H, W, pix, scene_cut=scene_cut, times=times, dedup=dedup) as st:
                if select is not None:
                    st.select(select)
                outs = []
                for fr in frames:
                    x = np.array(fr)
                    outs.append(st.push(torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda()))
                    dups.append(st.dup_info())
                    cuts.append(st.cut_info())
                torch.cuda.synchronize()
                got = [None if o is None else o.cpu().numpy().view(frames[0].dtype) for o in outs]
    finally:
        _options_off(eng)
    return got, dups, cuts, guarded


_PLAIN = {}


def _plain(eng, pix):
    """The reference streams without the option, computed once per layout (host memory) and shared."""
    if pix not in _PLAIN:
        f = _frames(pix)
        three, dups, _, _ = _run(eng, pix, 'host', [f['A'], f['A1'], f['B']])
        assert dups == [(None, 0)] * 3                                     # dup_hi = -1: no comparison is ever made
        two, _, _, _ = _run(eng, pix, 'host', [f['A'], f['B']])
        deep, _, _, _ = _run(eng, pix, 'host', [f['A'], f['B']], times=2, select=(1, 3))
        assert [g is None for g in three] == [True, False, False] and two[1] is not None and deep[1].shape[0] == 2
        assert len({three[1].tobytes(), three[2].tobytes(), two[1].tobytes(), deep[1][0].tobytes(), deep[1][1].tobytes()}) == 5   # a stale result would show
        _PLAIN[pix] = dict(A_A1=three[1], A1_B=three[2], A_B=two[1], A_B_deep=deep[1])
    return _PLAIN[pix]


def _same(a, b):
    return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _stats(s):
    return None if s is None else np.asarray(s).tolist()


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('pix', LAYOUTS)
def test_exact_duplicates_are_dropped(tiny, pix, mem):
    """dedup = 0 on A, A, A', B: the second push is dropped; A' differs in one sample and is kept; the results are those of a plain stream
    pushed A, A', B."""
    f, want = _frames(pix), _plain(tiny, pix)
    got, dups, cuts, guarded = _run(tiny, pix, mem, [f['A'], f['A'], f['A1'], f['B']], dedup=0, guard_out_at=1)
    assert [g is None for g in got] == [True, True, False, False]
    assert [d for _, d in dups] == [0, 1, 0, 0]
    assert dups[0][0] is None                                               # the first push: no comparison
    assert _stats(dups[1][0]) == R.frame_diff(f['A'], f['A'], pix) and [s[:3] for s in _stats(dups[1][0])] == [[0, 0, 0]] * 3
    assert _stats(dups[2][0]) == R.frame_diff(f['A'], f['A1'], pix)
    assert _stats(dups[3][0]) == R.frame_diff(f['A1'], f['B'], pix)
    assert _same(got[2], want['A_A1']) and _same(got[3], want['A1_B'])
    assert all(c[0] == -1 and c[2] == 0 for c in cuts)                      # scene_cut is off
    if mem == 'host':
        assert guarded is not None and (guarded == 9).all()                 # the dropped push left `out` as it was


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('pix', LAYOUTS)
def test_near_duplicates_are_dropped_and_the_first_of_the_run_is_carried(tiny, pix, mem):
    """dedup = (2, 1, 0): the one block of A' at s = 1 code (10 bits: s = 1 <= 1 * 4) is neither above hi nor over lo, so A' is dropped too,
    and B is compared and interpolated with A - the first of the run -, not with A'."""
    f, want = _frames(pix), _plain(tiny, pix)
    m = R.scale(pix)
    assert R.is_duplicate(f['A'], f['A1'], pix, 2, 1, 0) and not R.is_duplicate(f['A'], f['A1'], pix, 0) and not R.is_duplicate(f['A'], f['B'], pix, 2, 1, 0)
    got, dups, _, guarded = _run(tiny, pix, mem, [f['A'], f['A'], f['A1'], f['B']], dedup=(2, 1, 0), guard_out_at=2)
    assert [g is None for g in got] == [True, True, True, False]
    assert [d for _, d in dups] == [0, 1, 1, 0]
    assert _stats(dups[2][0]) == R.frame_diff(f['A'], f['A1'], pix, lo=m) and _stats(dups[2][0])[0][:3] == [1, 1, 0]
    assert _stats(dups[3][0]) == R.frame_diff(f['A'], f['B'], pix, lo=m) != R.frame_diff(f['A1'], f['B'], pix, lo=m)
    assert _same(got[3], want['A_B']) and not _same(got[3], want['A1_B'])
    if mem == 'host':
        assert guarded is not None and (guarded == 9).all()


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('pix', LAYOUTS)
def test_dropped_pushes_with_recursion_and_a_selection(tiny, pix, mem):
    """times = 2 with positions 1 and 3 selected: the dropped pushes leave the selection and the slots alone, the push of B returns the two
    frames of a plain stream pushed A, B."""
    f, want = _frames(pix), _plain(tiny, pix)
    got, dups, _, _ = _run(tiny, pix, mem, [f['A'], f['A'], f['A1'], f['B']], dedup=(2, 1, 0), times=2, select=(1, 3))
    assert [g is None for g in got] == [True, True, True, False] and [d for _, d in dups] == [0, 1, 1, 0]
    assert got[3].shape[0] == 2 and _same(got[3], want['A_B_deep'])


@pytest.mark.parametrize('mem', ['host', 'device'])
@pytest.mark.parametrize('pix', ('u8', 'i420'))
def test_duplicates_are_decided_before_cuts(tiny, pix, mem):
    """scene_cut = 1000 beside dedup = 0 on A, A, A rolled, C: the duplicate takes no histogram and reports no comparison; the next push is
    compared with A's histogram (distance 0: the same samples), and C, which shares no code with A, is a cut."""
    f = _frames(pix)
    lay = pixfmt.BY_NAME[pix]
    n = H * W * 3 if lay.depth is None else H * W + 2 * (H >> lay.sy) * (W >> lay.sx)
    got, dups, cuts, _ = _run(tiny, pix, mem, [f['A'], f['A'], f['Aroll'], f['C']], dedup=0, scene_cut=1000)
    assert [d for _, d in dups] == [0, 1, 0, 0]
    assert cuts == [(-1, n, 0), (-1, n, 0), (0, n, 0), (2 * n, n, 1)], cuts
    assert [g is None for g in got] == [True, True, False, True]
    plain, _, _, _ = _run(tiny, pix, 'host', [f['A'], f['Aroll']])
    assert _same(got[2], plain[1])


def test_without_the_option_nothing_is_compared_or_dropped(tiny):
    """dedup = None with "dup_hi" at -1: A, A gives the mid-frame of two identical frames, as always."""
    f = _frames('u8')
    got, dups, _, _ = _run(tiny, 'u8', 'host', [f['A'], f['A'], f['B']])
    assert [g is None for g in got] == [True, False, False] and dups == [(None, 0)] * 3
    dedup, _, _, _ = _run(tiny, 'u8', 'host', [f['A'], f['A'], f['B']], dedup=0)
    assert dedup[1] is None and _same(dedup[2], _plain(tiny, 'u8')['A_B'])
    assert _same(got[2], dedup[2])           # (A, A, B plain: the carried frame of the last push is A either way)


def test_video_cli_dedup(tiny, tmp_path, monkeypatch, capsys):
    """eval.video_cli --fps 48 --times_to_interpolate 2 --dedup 0 on a 64 x 64 24 fps .y4m A A B C: the span of two intervals is spread over
    the full push of B, then B, position 2 of the push of C, and C - seven frames, each the bytes of a frame of --times_to_interpolate 2 on
    A B C; and on A B C the flag changes no byte."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, **kw):
        it = real.__new__(real)
        it._options, it._engine = tiny.options, tiny
        it._align, it._block_shape = align or None, block_shape or None
        return it

    a, b, c = np.random.default_rng(23).integers(0, 256, (3, 96, 64), dtype=np.uint8)        # 64 x 64 I420 frames of random codes

    def video(name, frames):
        with open(tmp_path / name, 'wb') as f:
            wr = y4m.Y4MWriter(f, y4m.header_tokens(64, 64, (24, 1)))
            for fr in frames:
                wr.write(fr)
        return str(tmp_path / name)

    def run(src, name, *flags):
        n = cli.main(['--input', src, '--output', str(tmp_path / name), '--times_to_interpolate', '2', *flags])
        return n, (tmp_path / name).read_bytes(), capsys.readouterr().err

    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    aabc, abc = video('aabc.y4m', [a, a, b, c]), video('abc.y4m', [a, b, c])
    _options_off(tiny)
    try:
        n_ref, ref, _ = run(abc, 'ref.y4m')
        n, got, err = run(aabc, 'out.y4m', '--fps', '48', '--dedup', '0')
        _options_off(tiny)                       # (handle options: the next command runs without them)
        plain = run(abc, 'plain.y4m', '--fps', '48')
        same = run(abc, 'same.y4m', '--fps', '48', '--dedup', '0')
    finally:
        _options_off(tiny)
    every, frames = list(y4m.Y4MReader(io.BytesIO(ref))), list(y4m.Y4MReader(io.BytesIO(got)))
    assert n_ref == len(every) == 9 and len({e.tobytes() for e in every}) == 9
    assert n == len(frames) == 7 and '1 duplicate input frames dropped' in err
    for j, g in enumerate((0, 1, 2, 3, 4, 6, 8)):
        assert frames[j].tobytes() == every[g].tobytes(), (j, g)
    assert plain[0] == same[0] == 5 and same[1] == plain[1] and '0 duplicate input frames dropped' in same[2]
