"""CPU tests of selected mid-frames in a frame stream (film_stream_select, film_stream_select_schedule_json), of the timing of a
frame-rate conversion (film_hip/retime.py) and of eval.video_cli --fps, WITHOUT a GPU.

A selection (bit i - 1 of the mask: position i of the 2^T - 1 of a push) prunes the push to C, the selected positions and their ancestors
in the recursion.  Here the pruned schedule is simulated for every mask of T <= 3 and seeded random ones of T = 4, 5, 6, executed by the
numpy interpreter (tests/plan_interp.py) over one persistent arena against the full schedule's frames, and the timing tables of the
common conversions are pinned.
"""
import ctypes
import io
import os
import random
import re

import numpy as np
import pytest

from standin_stream import It as _It, between as _between
from test_sequence_cpu import _tiny_engine

H, W = 32, 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(times):
    """{position: (depth, parent position or None)} of the recursion between positions 0 and 2^times, written down from the definition:
    the mid-frame of the frames at positions lo and hi lies at (lo + hi) / 2, its children are the mids of (lo, mid) and (mid, hi)."""
    tree = {}

    def walk(lo, hi, depth, parent):
        if hi - lo < 2:
            return
        mid = (lo + hi) // 2
        tree[mid] = (depth, parent)
        walk(lo, mid, depth + 1, mid)
        walk(mid, hi, depth + 1, mid)

    walk(0, 1 << times, 1, None)
    return tree


def _closure(tree, positions):
    c = set()
    for i in positions:
        while i is not None and i not in c:
            c.add(i)
            i = tree[i][1]
    return c


def _positions(mask):
    return [i + 1 for i in range(64) if mask >> i & 1]


def _plan_only_engine():
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    return FilmEngine(TINY, device=-1)


# ---- the symbols, the refusals, the default ---------------------------------------------------------------------------------------------
def test_select_symbols_and_refusals():
    from film_hip import engine
    from film_hip.engine import FILM_ERR_INVALID, FILM_ERR_STATE
    eng = _plan_only_engine()
    lib, hnd = eng._lib, eng._h
    names = ('film_stream_select', 'film_stream_select_schedule_json')
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    vmap = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    for n in names:
        assert re.search(r'^int ' + n + r'\(film_t\* h,', header, re.M), n
        assert re.search(r'\b' + n + ';', vmap), n
        assert n in engine.EXPORTED_SYMBOLS and hasattr(lib, n)
    need = ctypes.c_int64()
    query = lambda times, slot, mask: lib.film_stream_select_schedule_json(hnd, times, slot, mask, None, 0, ctypes.byref(need))   # noqa: E731
    assert lib.film_stream_select(None, 1) == FILM_ERR_INVALID
    assert lib.film_stream_select_schedule_json(None, 1, 0, 1, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert lib.film_stream_select(hnd, 1) == FILM_ERR_STATE                      # no open stream
    assert 'no open stream' in lib.film_last_error(hnd).decode()
    assert query(3, 0, 0b1010101) == 0 and need.value > 100
    for times in (0, 7):
        assert query(times, 0, 1) == FILM_ERR_INVALID
        assert 'times' in lib.film_last_error(hnd).decode()
    for slot in (-1, 2):
        assert query(2, slot, 1) == FILM_ERR_INVALID
        assert 'slot' in lib.film_last_error(hnd).decode()
    for times in range(1, 7):
        n = (1 << times) - 1
        assert query(times, 1, (1 << n) - 1) == 0 and query(times, 0, 0) == 0
        for bit in {n, 63}:                                                       # the first bit past the positions, and the last of the word
            assert query(times, 0, 1 << bit) == FILM_ERR_INVALID, (times, bit)
            assert 'mask' in lib.film_last_error(hnd).decode()
    for bad in ([0], [8], [1.5]):                                                 # the wrapper names positions, 1 .. 2^T - 1
        with pytest.raises(ValueError):
            eng.stream_schedule(3, 0, select=bad)
    eng.close()


@pytest.mark.parametrize('times', [1, 2, 3, 4, 5, 6])
def test_full_selection_is_the_full_schedule(times):
    eng = _plan_only_engine()
    for slot in (0, 1):
        full = eng.stream_schedule(times, slot)
        assert all(set(t) == {'left', 'right', 'extract', 'index', 'depth', 'feed'} for t in full['steps'])     # (as it always was)
        for select in (range(1, 1 << times), list(range(1, 1 << times)) * 2):
            sel = eng.stream_schedule(times, slot, select=select)
            assert sel['mask'] == (1 << ((1 << times) - 1)) - 1
            assert {k: v for k, v in sel.items() if k not in ('mask', 'steps')} == {k: v for k, v in full.items() if k != 'steps'}
            assert all(t['deliver'] == 1 and t['run'] == 'pair' for t in sel['steps'])
            assert [{k: v for k, v in t.items() if k not in ('deliver', 'run')} for t in sel['steps']] == full['steps']
    eng.close()


# ---- the pruned schedule, by simulation -------------------------------------------------------------------------------------------------
def _simulate(eng, times, slot, mask, tree, full_order):
    """A push of B (position 2^T, into `slot`) after A (position 0, extracted, in the other slot) with selection `mask`."""
    pos = _positions(mask)
    sch = eng.stream_schedule(times, slot, select=pos)
    ctx = (times, slot, pos)
    assert (sch['times'], sch['slot'], sch['slots'], sch['produced'], sch['mask']) == (times, slot, times + 1, len(pos), mask), ctx
    steps = sch['steps']
    C = _closure(tree, pos)
    has_child = {i for i in C if any(tree[j][1] == i for j in C)}
    pairs = [t for t in steps if t['run'] == 'pair']
    assert all(t['run'] in ('pair', 'extract') and t['deliver'] in (0, 1) for t in steps), ctx
    assert [t['index'] for t in pairs] == [i for i in full_order if i in C], ctx            # exactly C, once each, in today's order
    assert [t['index'] for t in steps if t['deliver']] == [i for i in full_order if i in pos], ctx
    assert sum(t['extract'] for t in steps) == 1 + len(has_child), ctx
    holds = {1 - slot: 0, slot: 1 << times}          # slot -> position of the frame it holds
    extracted = {1 - slot}                            # slots whose pyramids belong to the frame they hold
    extracted_frames = {0}                            # positions that have been extracted, ever
    for n, t in enumerate(steps):
        where = ctx + (n, t)
        assert t['left'] != t['right'] and 0 <= t['left'] <= times and 0 <= t['right'] <= times, where
        if t['run'] == 'extract':
            assert (t['extract'], t['deliver'], t['feed']) == (1, 0, -1), where
            assert holds.get(t['right']) == t['index'] and t['right'] not in extracted, where
            assert t['depth'] == (tree[t['index']][0] if t['index'] in tree else 0), where
        else:
            d = 1 << (times - t['depth'])
            assert tree[t['index']][0] == t['depth'], where
            assert holds.get(t['left']) == t['index'] - d and holds.get(t['right']) == t['index'] + d, where + (holds,)
            assert t['left'] in extracted, where
            assert (t['right'] in extracted) == (not t['extract']), where
            assert t['deliver'] == (t['index'] in pos), where
            assert t['feed'] == (1 + t['depth'] if t['index'] in has_child else -1), where
        if t['extract']:
            assert holds[t['right']] not in extracted_frames, where                              # no frame is extracted twice
            extracted_frames.add(holds[t['right']])
            extracted.add(t['right'])
        if t['feed'] >= 0:
            assert t['feed'] >= 2, where               # no step writes an input slot
            holds[t['feed']] = t['index']
            extracted.discard(t['feed'])
    assert holds[slot] == 1 << times and holds[1 - slot] == 0 and slot in extracted, ctx
    return len(pairs), sum(t['extract'] for t in steps)


def test_pruned_schedule_by_simulation():
    """Every mask of T <= 3 and 200 seeded random masks each of T = 4, 5, 6, on both slots: the pair steps are C in today's order, the
    delivered ones the mask, every pair finds its parents in its slots with the left one extracted and the right one extracted iff the
    step does not do it, nothing is extracted twice, extractions = 1 + the members of C with a child in C, no step writes an input
    slot, and the pushed frame ends up extracted where it was put.  film_hip.retime states the same costs."""
    from film_hip import retime
    eng = _plan_only_engine()
    rng = random.Random(20)
    for times in range(1, 7):
        n = (1 << times) - 1
        tree = _tree(times)
        assert sorted(tree) == list(range(1, n + 1))
        masks = list(range(1 << n)) if times <= 3 else [rng.getrandbits(n) >> rng.choice((0, 0, n // 2, n - 3)) for _ in range(200)]
        for slot in (0, 1):
            full_order = [t['index'] for t in eng.stream_schedule(times, slot)['steps']]
            for mask in masks:
                got = _simulate(eng, times, slot, mask, tree, full_order)
                assert got == retime.push_cost(times, _positions(mask)), (times, mask)
                assert list(retime.closure(times, _positions(mask))) == sorted(_closure(tree, _positions(mask)))
    # the two pushes of 24 -> 60 at T = 3: four pair runs and three extractions each, against seven and four
    assert retime.push_cost(3, (3, 6)) == (4, 3) and retime.push_cost(3, (2, 5)) == (4, 3) and retime.push_cost(3, range(1, 8)) == (7, 4)
    sch = eng.stream_schedule(3, 1, select=[6])                              # the right child alone: an extraction-only step before it
    assert [(t['run'], t['index'], t['left'], t['right']) for t in sch['steps']] == [('pair', 4, 0, 1), ('extract', 4, 0, 2), ('pair', 6, 2, 1)]
    eng.close()


# ---- the interpreter --------------------------------------------------------------------------------------------------------------------
def test_selected_pushes_in_the_interpreter(tiny_weights):
    """T = 3, seven frames, masks {3, 6}, {2, 5}, {6}, {5}, {} and the full one push after push through one persistent arena, beside
    full pushes of the same frames through another: every delivered frame has the bits of the full push's frame at its position - the
    full push after the empty one too, so the extraction it carried over survived."""
    import plan_interp as pi
    times, tiles = 3, 1
    eng = _tiny_engine(tiny_weights)
    packed = eng.export_layouts()
    key = pi.blob_key(packed)
    rng = np.random.default_rng(31)
    frames = [rng.random((tiles, H, W, 3), dtype=np.float32) for _ in range(7)]
    selections = [(3, 6), (2, 5), (6,), (5,), (), tuple(range(1, 8))]
    plans = {}

    def plan_of(left, right, extract):
        k = (left, right, extract)
        if k not in plans:
            plans[k] = eng.stream_pair_plan(tiles, H, W, times, left, right, extract)
        return plans[k]

    base = plan_of(1, 0, 1)
    bufs = {b['name']: b for b in base['buffers']}
    img0, fsz = bufs['img0'], frames[0].size

    def run(selections):
        """{(push, position): frame} of the delivered frames (selections None: full pushes, by film_stream_schedule_json)."""
        arena = np.zeros(base['arena_floats'], np.float32)
        got, slot, runs = {}, 0, 0

        def put(s, fr):
            arena[img0['off'] + s * fsz:img0['off'] + (s + 1) * fsz] = fr.ravel()

        for i, fr in enumerate(frames):
            put(slot, fr)
            if i == 0:
                steps = [dict(left=1, right=0, extract=1, run='extract')]
            elif selections is None:
                steps = eng.stream_schedule(times, slot)['steps']
            else:
                steps = eng.stream_schedule(times, slot, select=selections[i - 1])['steps']
            for t in steps:
                p = plan_of(t['left'], t['right'], t['extract'])
                pair = t.get('run', 'pair') == 'pair'
                assert p['n_extract'] > 0 or pair
                for op in p['ops'] if pair else p['ops'][:p['n_extract']]:
                    pi.run_op(op, arena, packed, bufs, verify_key=key)
                if not pair:
                    continue
                runs += 1
                out = pi.tap(p, arena, 'out').copy()
                if t.get('deliver', 1):
                    got[i, t['index']] = out
                if t['feed'] >= 0:
                    put(t['feed'], out)
            slot = 1 - slot
        return got, runs

    want, full_runs = run(None)
    got, runs = run(selections)
    assert full_runs == 6 * 7 and runs == 4 + 4 + 2 + 3 + 0 + 7
    assert sorted(got) == sorted((i + 1, p) for i, sel in enumerate(selections) for p in sel)
    for k, frame in got.items():
        assert np.array_equal(frame, want[k]), k
    eng.close()


# ---- retime -----------------------------------------------------------------------------------------------------------------------------
def test_retime_properties():
    """For every a, b in 1 .. 39 (u_j = j a / b) and T in 1 .. 6 with a 2^T >= b: the g_j are strictly increasing and every snap error is at
    most 2^-(T + 1) input intervals; a finer output rate is refused."""
    from fractions import Fraction
    from math import gcd
    from film_hip import retime
    for times in range(1, 7):
        for a in range(1, 40):
            for b in range(1, 40):
                if a << times < b:
                    with pytest.raises(ValueError) as e:
                        retime.Retime((a, 1), (b, 1), times)
                    assert 'times the input rate' in str(e.value)
                    continue
                rt = retime.Retime((a, 1), (b, 1), times)
                period = b // gcd(a, b)
                g = [rt.grid(j) for j in range(period + 2)]
                assert g[0] == 0 and all(x < y for x, y in zip(g, g[1:])), (a, b, times)
                assert g[period] == (a // gcd(a, b)) << times                                  # (the pattern repeats from here)
                for j in range(period + 1):
                    num, den = rt.error(j)
                    err = Fraction(g[j], 1 << times) - Fraction(j * a, b)
                    assert den > 0 and Fraction(num, den) == err
                    assert abs(err) <= Fraction(1, 2 << times), (a, b, times, j)
                    if abs(err) == Fraction(1, 2 << times):
                        assert g[j] % 2 == 0                                                   # a tie goes to the even grid index
    assert retime.Retime((24000, 1001), (60000, 1001), 3).grid(5) == retime.Retime((24, 1), (60, 1), 3).grid(5) == 16
    for text, want in (('60', (60, 1)), ('60000:1001', (60000, 1001)), ('60000/1001', (60000, 1001)), ('50:2', (25, 1))):
        assert retime.parse_rate(text) == want
    for bad in ('', '0', '59.94', '-24', '60:0', '1:2:3', 'abc'):
        with pytest.raises(ValueError):
            retime.parse_rate(bad)


def _table(rate_in, rate_out, times, n):
    """From the definition: output j is position g_j & (2^T - 1) behind input frame g_j >> T, position 0 being the frame itself."""
    from film_hip import retime
    rt = retime.Retime(rate_in, rate_out, times)
    rows, j = [(False, ())] * n, 0
    while rt.grid(j) >> times < n:
        k, i = rt.grid(j) >> times, rt.grid(j) & ((1 << times) - 1)
        rows[k] = (rows[k][0], rows[k][1] + (i,)) if i else (True, rows[k][1])
        j += 1
    return rows, rt


def test_retime_tables():
    """(is input frame k written, the positions of the push of frame k + 1) per interval, T = 3."""
    Y, N = True, False
    rows, rt = _table((24, 1), (60, 1), 3, 4)
    assert [rt.grid(j) for j in range(6)] == [0, 3, 6, 10, 13, 16]
    assert rows == [(Y, (3, 6)), (N, (2, 5)), (Y, (3, 6)), (N, (2, 5))]
    assert _table((24000, 1001), (60000, 1001), 3, 4)[0] == rows
    # 25 -> 60: u_j = 5 j / 12, g_j = round(10 j / 3) = 0 3 7 10 13 17 20 23 27 30 33 37 40
    assert _table((25, 1), (60, 1), 3, 5)[0] == [(Y, (3, 7)), (N, (2, 5)), (N, (1, 4, 7)), (N, (3, 6)), (N, (1, 5))]
    # 24 -> 30: u_j = 4 j / 5, g_j = round(32 j / 5) = 0 6 13 19 26 32: four of five input frames are not written
    assert _table((24, 1), (30, 1), 3, 5)[0] == [(Y, (6,)), (N, (5,)), (N, (3,)), (N, (2,)), (Y, (6,))]
    # 50 -> 60: u_j = 5 j / 6, g_j = round(20 j / 3) = 0 7 13 20 27 33 40
    assert _table((50, 1), (60, 1), 3, 5)[0] == [(Y, (7,)), (N, (5,)), (N, (4,)), (N, (3,)), (N, (1,))]
    # 30 -> 24: u_j = 5 j / 4, g_j = 10 j: an interval without any output
    assert _table((30, 1), (24, 1), 3, 5)[0] == [(Y, ()), (N, (2,)), (N, (4,)), (N, (6,)), (N, ())]
    for times in (1, 3, 6):
        full, rt = _table((25, 1), (25 << times, 1), times, 3)
        assert full == [(Y, tuple(range(1, 1 << times)))] * 3 and rt.outputs(5) == (4 << times) + 1
        same, rt = _table((30000, 1001), (30000, 1001), times, 3)
        assert same == [(Y, ())] * 3 and rt.outputs(5) == 5 and all(rt.error(j)[0] == 0 for j in range(5))
    rt = _table((24, 1), (60, 1), 3, 1)[1]
    assert [rt.outputs(n) for n in (0, 1, 2, 3, 5)] == [0, 1, 3, 6, 11]      # (outputs past the last input frame are dropped)


def test_set_rate():
    from film_hip import y4m
    tokens = y4m.header_tokens(6, 4, (24, 1))
    got = y4m.set_rate(tokens, (120000, 2002))
    assert [t for t in got if t[:1] == 'F'] == ['F60000:1001']
    assert [t for t in got if t[:1] != 'F'] == [t for t in tokens if t[:1] != 'F']
    assert y4m.set_rate(['W6', 'H4'], (60, 1)) == ['W6', 'H4', 'F60:1']
    for bad in ((0, 1), (1, 0)):
        with pytest.raises(ValueError):
            y4m.set_rate(tokens, bad)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
def _video(n, rate, tokens=None):
    from film_hip import y4m
    frames = np.random.default_rng(5).integers(0, 256, (n, 6, 6), dtype=np.uint8)        # 4 x 6 I420 frames
    data = io.BytesIO()
    wr = y4m.Y4MWriter(data, tokens or y4m.header_tokens(6, 4, rate))
    for f in frames:
        wr.write(f)
    return frames, data.getvalue()


def test_video_cli_fps():
    from eval import video_cli as cli
    from film_hip import y4m
    ap = cli.build_parser()
    assert ap.parse_args(['--input', 'i', '--output', 'o']).fps is None
    assert ap.parse_args(['--input', 'i', '--output', 'o', '--fps', '60000/1001']).fps == '60000/1001'
    assert ap.parse_args(['--input', 'i', '--output', 'o', '--fps', '60']).times_to_interpolate == 1
    assert '3 or 4' in ap.format_help()
    frames, data = _video(5, (24, 1))

    def convert(rate_out, times, scene_cut=0, cut_at=None, data=data):
        it, out, cuts, stats = _It(cut_at), io.BytesIO(), [], {}
        n = cli.convert_frame_rate(it, y4m.Y4MReader(io.BytesIO(data)), out, rate_out, 'bt709', None, scene_cut, cuts, times, stats)
        rd = y4m.Y4MReader(io.BytesIO(out.getvalue()))
        got = list(rd)
        assert n == len(got)
        return it, rd, got, cuts, stats, out.getvalue()

    # 24 -> 60 on the grid of 1/8: g = 0 3 6 10 13 16 19 22 26 29 32
    it, rd, got, _, stats, _ = convert((60, 1), 3)
    grid = [0, 3, 6, 10, 13, 16, 19, 22, 26, 29, 32]
    assert it.kw == {'times': 3} and len(got) == len(grid) and 'F60:1' in rd.tokens and sum(t[:1] == 'F' for t in rd.tokens) == 1
    for j, g in enumerate(grid):
        k, i = g >> 3, g & 7
        want = frames[k] if i == 0 else _between(frames[k], frames[k + 1], 3)[i]
        assert np.array_equal(got[j], want), (j, g)
    assert it.stream.selects == [(3, 6), (2, 5), (3, 6), (2, 5)]
    assert stats['pair_runs'] == 16 and stats['pair_runs_full'] == 28
    assert stats['snap_max'] == pytest.approx(0.05) and stats['snap_mean'] == pytest.approx((0 + 2 + 1 + 1 + 2) * 2 / 5 / 8 / 11)
    # 24 -> 30: the input frames between the landings are not written
    _, rd, got, _, _, _ = convert((30, 1), 3)
    assert len(got) == 6 and 'F30:1' in rd.tokens
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[5], frames[4])
    assert not any(np.array_equal(g, f) for g in got[1:5] for f in frames)
    # the dyadic rates write the bytes of --times_to_interpolate T, held frames included, without ever touching the selection
    for times in (1, 2, 3):
        for scene_cut in (0, 250):
            it, _, got, cuts, stats, raw = convert((24 << times, 1), times, scene_cut, 2)
            ref_it, ref_out, ref_cuts = _It(2), io.BytesIO(), []
            cli.double_frame_rate(ref_it, y4m.Y4MReader(io.BytesIO(data)), ref_out, 'bt709', None, scene_cut, ref_cuts, times)
            assert raw == ref_out.getvalue() and cuts == ref_cuts == ([2] if scene_cut else []) and it.kw == ref_it.kw
            assert it.stream.selects == [] and len(got) == (4 << times) + 1 and stats['snap_max'] == 0
    odd, odd_data = _video(3, None, ['W6', 'H4', 'F48:2', 'C420jpeg'])                 # (a header whose rate is not reduced)
    ref_out = io.BytesIO()
    cli.double_frame_rate(_It(), y4m.Y4MReader(io.BytesIO(odd_data)), ref_out, times=2)
    assert convert((96, 1), 2, data=odd_data)[5] == ref_out.getvalue()
    # a cut holds the previous input frame once per selected position: the count and the rate stay
    it, _, held, cuts, _, _ = convert((60, 1), 3, 250, 2)
    assert it.kw == {'scene_cut': 250, 'times': 3} and cuts == [2] and len(held) == len(grid)
    plain = convert((60, 1), 3)[2]
    for j, g in enumerate(grid):
        assert np.array_equal(held[j], frames[1] if g >> 3 == 1 and g & 7 else plain[j]), j
    # a cut in an interval that selects nothing is still reported (30 -> 24: interval 0 has no position)
    assert convert((24, 1), 3, 250, 1, data=_video(5, (30, 1))[1])[3] == [1]
    # the refusals
    with pytest.raises(ValueError) as e:
        convert((60, 1), 3, data=_video(2, None, ['W6', 'H4', 'C420jpeg'])[1])
    assert 'F token' in str(e.value)
    with pytest.raises(ValueError) as e:
        convert((60, 1), 1)                                                           # 60 > 2 x 24
    assert 'times the input rate' in str(e.value)


def test_video_cli_fps_refuses_before_the_model_loads(tmp_path, monkeypatch):
    from eval import video_cli as cli

    def no_model(*a, **kw):
        raise AssertionError('the model must not be loaded')

    monkeypatch.setattr(cli.interpolator_lib, 'Interpolator', no_model)
    rated, unrated = tmp_path / 'rated.y4m', tmp_path / 'unrated.y4m'
    rated.write_bytes(_video(2, (24, 1))[1])
    unrated.write_bytes(_video(2, None, ['W6', 'H4', 'C420jpeg'])[1])
    out = str(tmp_path / 'out.y4m')
    for argv, word in ((['--input', str(unrated), '--fps', '60', '--times_to_interpolate', '3'], 'F token'),
                       (['--input', str(rated), '--fps', '60'], 'times the input rate'),
                       (['--input', str(rated), '--fps', '59.94', '--times_to_interpolate', '3'], 'N:D'),
                       (['--input', str(rated), '--fps', '60', '--times_to_interpolate', '7'], '1 .. 6')):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ['--output', out])
        assert word in str(e.value), argv
    with pytest.raises(AssertionError):                                               # (what is accepted goes on to the model)
        cli.main(['--input', str(rated), '--output', out, '--fps', '60', '--times_to_interpolate', '3'])
