"""CPU tests of retiming over stretched intervals (film_hip/retime.py, Retime.span) and of eval/video_cli.py --dedup: span() against a brute
force in fractions.Fraction, n = 1 against grid(), and the command on scripted duplicate patterns through a stand-in stream that records
what was selected for every push - frame count, header, which frames are verbatim, the hold on a cut, the trailing run, and the bytes of a
video without duplicates with and without the flag.  No GPU."""
import io
from fractions import Fraction

import numpy as np
import pytest

from film_hip import retime
from standin_stream import It as _It, between as _between

RATES = [((24, 1), (60, 1)), ((25, 1), (60, 1)), ((24000, 1001), (60000, 1001)), ((24, 1), (48, 1))]


def _round_half_even(x: Fraction) -> int:
    f = x.numerator // x.denominator
    r = x - f
    return f + (r > Fraction(1, 2) or (r == Fraction(1, 2) and f & 1))


def _brute_span(rate_in, rate_out, times, k, n):
    """The definition, output by output: u_j = j * (a d) / (b c); in the span iff k <= u_j < k + n; g = round((u_j - k) 2^T / n)."""
    (a, b), (c, d) = rate_in, rate_out
    step = Fraction(a * d, b * c)
    j = 0
    while j * step < k:
        j += 1
    j0, grid = j, []
    while j * step < k + n:
        grid.append(_round_half_even((j * step - k) * (1 << times) / n))
        j += 1
    return j0, tuple(grid)


@pytest.mark.parametrize('rate_in, rate_out', RATES)
def test_span_against_the_definition(rate_in, rate_out):
    for times in (1, 2, 3, 4):
        try:
            rt = retime.Retime(rate_in, rate_out, times)
        except ValueError:
            assert Fraction(*rate_out) / Fraction(*rate_in) > 1 << times          # (24 -> 60 at T = 1: refused, as without spans)
            continue
        for n in (1, 2, 3, 4, 5):
            for k in (0, 1, 2, 5, 11, 12, 1000, 1001):
                sp = rt.span(k, n)
                assert (sp.j, sp.grid) == _brute_span(rate_in, rate_out, times, k, n), (times, k, n)
                assert all(0 <= g <= 1 << times for g in sp.grid) and list(sp.grid) == sorted(sp.grid)
                for i, g in enumerate(sp.grid):                                   # the snap error, in input intervals
                    num, den = rt.span_error(k, n, sp.j + i)
                    u = (sp.j + i) * Fraction(rate_in[0] * rate_out[1], rate_in[1] * rate_out[0])
                    assert den > 0 and Fraction(num, den) == k + Fraction(g * n, 1 << times) - u
                    assert abs(Fraction(num, den)) <= Fraction(n, 2 << times)
        # consecutive spans tile the outputs: none lost, none twice
        j, k = 0, 0
        for n in (1, 3, 1, 1, 5, 2, 4, 1):
            sp = rt.span(k, n)
            assert sp.j == j
            j, k = j + len(sp.grid), k + n
        assert rt.span(k, 1).j == j
    with pytest.raises(ValueError):
        retime.Retime(rate_in, rate_out, 4).span(0, 0)
    with pytest.raises(ValueError):
        retime.Retime(rate_in, rate_out, 4).span(-1, 1)


@pytest.mark.parametrize('rate_in, rate_out', RATES)
def test_spans_of_one_interval_walk_the_frames_of_the_grid(rate_in, rate_out):
    """n = 1: the sequence of frames of g_j, frame for frame - (input index, position) per output, position 0 being the input frame itself."""
    for times in (2, 3, 4) if rate_out != (48, 1) else (1, 2, 3, 4):
        rt = retime.Retime(rate_in, rate_out, times)
        top = 1 << times
        old, j = [], 0
        while rt.grid(j) >> times < 40:
            old.append((rt.grid(j) >> times, rt.grid(j) & (top - 1)))
            j += 1
        new = []
        for k in range(40):
            sp = rt.span(k, 1)
            assert sp.j == len(new)
            new += [(k + 1, 0) if g == top else (k, g) for g in sp.grid]
        n = min(len(old), len(new)) - 1
        assert n > 40 and old[:n] == new[:n]
        assert [rt.grid(j) for j in range(n)] == [(k << times) + g for k, g in new[:n]]


# ---- eval/video_cli.py --dedup on a stand-in stream --------------------------------------------------------------------------------------------
def _video(pattern, rate=(24, 1)):
    """A 4 x 6 I420 video whose frame i is picture pattern[i]: equal letters are equal frames."""
    from film_hip import y4m
    rng = np.random.default_rng(5)
    pics = {c: rng.integers(0, 256, (6, 6), dtype=np.uint8) for c in sorted(set(pattern))}
    frames = [pics[c] for c in pattern]
    data = io.BytesIO()
    wr = y4m.Y4MWriter(data, y4m.header_tokens(6, 4, rate))
    for f in frames:
        wr.write(f)
    return frames, data.getvalue()


def _convert(data, rate_out, times, dedup, scene_cut=0, cut_at=None):
    from eval import video_cli as cli
    from film_hip import y4m
    it, out, cuts, stats = _It(cut_at), io.BytesIO(), [], {}
    rd = y4m.Y4MReader(io.BytesIO(data))
    n = cli.convert_frame_rate(it, rd, out, rate_out, 'bt709', None, scene_cut, cuts, times, stats, dedup=dedup)
    back = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    got = list(back)
    assert n == len(got)
    return it, back, got, cuts, stats, out.getvalue()


def _expected(frames, kept, rate_in, rate_out, times, cut_at=None):
    """What the definition writes for kept frames k_0 < k_1 < ...: per output the frame of its span and grid index; the outputs at or behind
    the last kept frame are that frame."""
    rt = retime.Retime(rate_in, rate_out, times)
    top, out = 1 << times, []
    for k, k1 in zip(kept, kept[1:]):
        j0, grid = _brute_span(rate_in, rate_out, times, k, k1 - k)
        assert j0 == len(out)
        at = _between(frames[k], frames[k1], times)
        for g in grid:
            out.append(frames[k] if g == 0 or (g < top and k1 == cut_at) else at[g])
    while len(out) < rt.outputs(len(frames)):
        out.append(frames[kept[-1]])
    return out


def _kept(pattern):
    return [i for i, c in enumerate(pattern) if i == 0 or c != pattern[i - 1]]


PATTERNS = ['ABCDE', 'AABCD', 'AABBCCDD', 'AAABBCCCDD', 'ABBBBBC', 'ABCCC', 'AAAA', 'A', 'AB', 'ABCDEEEEEF']


@pytest.mark.parametrize('rate_out, times', [((60, 1), 3), ((60, 1), 4), ((48, 1), 1), ((48, 1), 3), ((30, 1), 3)])
@pytest.mark.parametrize('pattern', PATTERNS)
def test_video_cli_dedup_on_scripted_patterns(pattern, rate_out, times):
    frames, data = _video(pattern)
    kept = _kept(pattern)
    it, rd, got, _, stats, _ = _convert(data, rate_out, times, (0, 0, 1000))
    plain = _convert(data, rate_out, times, None)
    assert it.kw.get('dedup') == (0, 0, 1000) and 'dedup' not in plain[0].kw
    assert len(got) == len(plain[2]) and rd.tokens == plain[1].tokens               # the frame count and the header of the plain command
    want = _expected(frames, kept, (24, 1), rate_out, times)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (pattern, j)
    assert stats['duplicates'] == len(pattern) - len(kept)
    # what was selected for every push that closed a span: the positions of span(k, n), once each, and nothing else ran
    top = 1 << times
    closing = [(k1, tuple(sorted({g for g in _brute_span((24, 1), rate_out, times, k, k1 - k)[1] if 0 < g < top}))) for k, k1 in zip(kept, kept[1:])]
    assert it.stream.pushes == closing
    repeats = sum(len(g) - len(set(g)) for g in (_brute_span((24, 1), rate_out, times, k, k1 - k)[1] for k, k1 in zip(kept, kept[1:])))
    assert stats['repeats'] == repeats
    if len(kept) == len(pattern):                                                   # no duplicate: byte for byte the plain command
        assert _convert(data, rate_out, times, (0, 0, 1000))[5] == plain[5]


def test_video_cli_dedup_verbatim_frames_hold_and_trailing_run():
    pattern = 'AABBBCDD'
    frames, data = _video(pattern)
    kept = _kept(pattern)                        # 0, 2, 5, 6
    assert kept == [0, 2, 5, 6]
    # twice the input rate on a grid of 1/8: the span of two (three) intervals gets four (six) outputs at g = 0, 2, 4, 6 (0, 1, 3, 4, 5, 7)
    it, rd, got, _, stats, _ = _convert(data, (48, 1), 3, (0, 0, 1000))
    assert len(got) == 15 and 'F48:1' in rd.tokens
    assert it.stream.pushes == [(2, (2, 4, 6)), (5, (1, 3, 4, 5, 7)), (6, (4,))]
    for j, k in ((0, 0), (4, 2), (10, 5), (12, 6), (13, 6), (14, 6)):               # verbatim: the kept frames, and the trailing run as the last kept one
        assert np.array_equal(got[j], frames[k]), j
    at = _between(frames[2], frames[5], 3)
    assert [np.array_equal(got[4 + i], at[g]) for i, g in enumerate((0, 1, 3, 4, 5, 7))] == [True] * 6
    assert stats['duplicates'] == 4 and stats['repeats'] == 0
    # on the shallowest grid the stretched spans share grid indices: four (six) outputs on g = 0, 1, 2 - selected once, written once per output
    it1, _, got1, _, stats1, _ = _convert(data, (48, 1), 1, (0, 0, 1000))
    assert len(got1) == 15 and it1.stream.pushes == [(2, (1,)), (5, (1,)), (6, (1,))] and stats1['repeats'] == 1 + 3
    mid = _between(frames[2], frames[5], 1)[1]
    assert [np.array_equal(got1[4 + i], f) for i, f in enumerate((frames[2], frames[2], mid, mid, mid, frames[5]))] == [True] * 6      # g = 0 0 1 1 1 2
    with pytest.raises(ValueError):
        _convert(data, (60, 1), 1, (0, 0, 1000))                                    # (a rate the grid cannot hold is refused as without the flag)
    # a scene cut on the frame that closes a span holds the span's FIRST frame in place of every position
    it, _, held, cuts, _, _ = _convert(data, (48, 1), 3, (0, 0, 1000), scene_cut=250, cut_at=5)
    assert cuts == [5] and it.kw == {'dedup': (0, 0, 1000), 'scene_cut': 250, 'times': 3} and len(held) == 15
    for j in range(15):
        assert np.array_equal(held[j], frames[2] if 4 <= j < 10 else got[j]), j
    assert np.array_equal(held[10], frames[5])


@pytest.mark.parametrize('rate_in, rate_out, times', [((24, 1), (60, 1), 3), ((25, 1), (60, 1), 4), ((24000, 1001), (60000, 1001), 3), ((24, 1), (48, 1), 1),
                                                      ((24, 1), (48, 1), 3), ((30, 1), (24, 1), 3)])
def test_video_without_duplicates_is_written_byte_for_byte(rate_in, rate_out, times):
    for scene_cut, cut_at in ((0, None), (250, 2), (250, 1)):
        _, data = _video('ABCDEFG', rate_in)
        with_flag = _convert(data, rate_out, times, (0, 0, 1000), scene_cut, cut_at)
        without = _convert(data, rate_out, times, None, scene_cut, cut_at)
        assert with_flag[5] == without[5] and with_flag[3] == without[3]
        assert with_flag[4]['duplicates'] == 0 and with_flag[4]['pair_runs'] == without[4]['pair_runs']
        assert with_flag[4]['snap_max'] == pytest.approx(without[4]['snap_max'])


def test_the_earlier_name_of_the_dedup_conversion_is_kept():
    """convert_frame_rate_dedup(it, reader, out, rate_out, dedup, ...), the interface before the one driver: the same bytes, cuts and statistics."""
    from eval import video_cli as cli
    from film_hip import y4m
    _, data = _video('AABBBCDD')
    it, out, cuts, stats = _It(5), io.BytesIO(), [], {}
    n = cli.convert_frame_rate_dedup(it, y4m.Y4MReader(io.BytesIO(data)), out, (48, 1), (0, 0, 1000), 'bt709', None, 250, cuts, 3, stats)
    want = _convert(data, (48, 1), 3, (0, 0, 1000), scene_cut=250, cut_at=5)
    assert n == 15 and (out.getvalue(), cuts, stats, it.kw, it.stream.pushes) == (want[5], want[3], want[4], want[0].kw, want[0].stream.pushes)


def test_dedup_flag_needs_fps_and_parses(tmp_path, monkeypatch):
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli

    def no_model(*a, **kw):
        raise AssertionError('the model must not be loaded')
    monkeypatch.setattr(interpolator_lib, 'Interpolator', no_model)
    _, data = _video('AAB')
    src = tmp_path / 'in.y4m'
    src.write_bytes(data)
    with pytest.raises(SystemExit) as e:
        cli.main(['--input', str(src), '--output', str(tmp_path / 'o.y4m'), '--dedup', '0'])
    assert '--dedup needs --fps' in str(e.value)
    for bad in ('x', '1:2:3:4', '-1', '16321', '0:16321', '0:0:1001', ''):
        with pytest.raises(SystemExit) as e:
            cli.main(['--input', str(src), '--output', str(tmp_path / 'o.y4m'), '--fps', '48', '--dedup=' + bad])
        assert '--dedup' in str(e.value), bad
    assert cli.parse_dedup('0') == (0, 0, 1000) and cli.parse_dedup('768:320') == (768, 320, 1000) and cli.parse_dedup('768:320:330') == (768, 320, 330)
    ap = cli.build_parser()
    assert ap.parse_args(['--input', 'i', '--output', 'o']).dedup is None and 'HI[:LO[:FRAC]]' in ap.format_help()


def test_video_cli_main_with_dedup(tmp_path, monkeypatch, capsys):
    """The command end to end on the stand-in: --fps 48 --times_to_interpolate 3 --dedup 0, the stderr line names what was dropped."""
    from eval import interpolator as interpolator_lib
    from eval import video_cli as cli
    from film_hip import y4m
    its = []

    def fake(*a, **kw):
        its.append(_It())
        return its[-1]
    monkeypatch.setattr(interpolator_lib, 'Interpolator', fake)
    frames, data = _video('AABBBCDD')
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    n = cli.main(['--input', str(src), '--output', str(dst), '--fps', '48', '--times_to_interpolate', '3', '--dedup', '0'])
    err = capsys.readouterr().err
    assert n == 15 and '4 duplicate input frames dropped' in err and '--dedup 0:0:1000' in err
    got = list(y4m.Y4MReader(io.BytesIO(dst.read_bytes())))
    want = _expected(frames, [0, 2, 5, 6], (24, 1), (48, 1), 3)
    assert len(got) == 15 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert its[0].kw == {'times': 3, 'dedup': (0, 0, 1000)}


def test_the_one_loop_writes_what_the_three_loops_wrote():
    """tests/golden/video_cli_digests.json was written by tools/make_video_cli_golden.py from the commit that had one frame loop per mode
    (--times_to_interpolate, --fps, --fps --dedup): per case the bytes written, the return value, the cuts, what open_stream got, every
    select() and every push that ran, and the statistics to the last bit are still those."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('make_video_cli_golden', os.path.join(root, 'tools', 'make_video_cli_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want, got = json.load(open(tool.PATH)), json.loads(json.dumps(tool.records()))
    assert len(want) >= 100 and sorted(got) == sorted(want)
    for name in sorted(want):
        assert sorted(got[name]) == sorted(want[name]), name
        for key in want[name]:
            assert got[name][key] == want[name][key], (name, key)
