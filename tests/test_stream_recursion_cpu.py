"""CPU tests of recursive mid-frames in a frame stream (engine option "stream_times" = T; film_stream_pair_plan_json,
film_stream_schedule_json) WITHOUT a GPU.

A T-stream plan has T + 1 frame slots in its per-image buffers: slots 0 and 1 take turns for the input frames, slot 1 + d holds the
depth-d mid-frame that is fed back.  One primed push runs 2^T - 1 pair runs, each an ORIENTATION (left slot, right slot, extract or
not) of that plan over one workspace.  Here the schedule of a push is simulated, the orientations are compared with each other and
with the T = 1 stream plan, checked for bounds and lane ordering, and executed by the numpy interpreter (tests/plan_interp.py,
unchanged) over ONE persistent arena, push after push.
"""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from conftest import oracle_options
from test_sequence_cpu import _check_bounds, _check_lanes, _tiny_engine, _view_pixels

H, W = 32, 48
WRITE_KEYS = ('out', 'out2', 'pw_out', 'img_out')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_image(name):
    return name.startswith('feat') or name.startswith('img')


def _writes(op):
    """[(view, pixels)] of everything the op writes (a conv with a fused 1x1 head does not write `out`)."""
    px = _view_pixels(op)
    res = []
    for key in WRITE_KEYS:
        v = op.get(key)
        if not v or not v.get('buf') or px.get(key, 0) <= 0:
            continue
        if key == 'out' and (op.get('pw_out') or {}).get('buf'):
            continue
        res.append((v, px[key]))
    return res


# ---- the option, the symbols, the refusals ------------------------------------------------------------------------------------------------
def test_stream_times_option_and_symbols(tiny_weights):
    from film_hip import engine
    from film_hip.engine import FilmError, FILM_ERR_INVALID
    eng = _tiny_engine(tiny_weights)
    for ok in (1, 6, 1):
        eng.set_option('stream_times', ok)
    for bad in (0, 7):
        with pytest.raises(FilmError) as e:
            eng.set_option('stream_times', bad)
        assert e.value.code == FILM_ERR_INVALID and 'stream_times' in str(e.value) and '1 .. 6' in str(e.value)
    names = ('film_stream_pair_plan_json', 'film_stream_schedule_json')
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    vmap = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    for n in names:
        assert re.search(r'^int ' + n + r'\(film_t\* h,', header, re.M), n
        assert re.search(r'\b' + n + ';', vmap), n
        assert n in engine.EXPORTED_SYMBOLS and hasattr(eng._lib, n)
    eng.close()


def test_pair_plan_and_schedule_refusals(tiny_weights):
    from film_hip.engine import FILM_ERR_INVALID
    eng = _tiny_engine(tiny_weights)
    lib, hnd = eng._lib, eng._h
    need = ctypes.c_int64()
    pair = lambda *a: lib.film_stream_pair_plan_json(hnd, *a, None, 0, ctypes.byref(need))   # noqa: E731
    assert lib.film_stream_pair_plan_json(None, 1, H, W, 1, 0, 1, 1, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert lib.film_stream_schedule_json(None, 1, 0, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert pair(1, H, W, 2, 0, 1, 1) == 0 and need.value > 100
    for times in (0, 7):
        assert pair(1, H, W, times, 0, 1, 1) == FILM_ERR_INVALID
        assert lib.film_stream_schedule_json(hnd, times, 0, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert pair(1, H, W, 2, 1, 1, 1) == FILM_ERR_INVALID                      # left == right
    for left, right in ((3, 0), (0, 3), (-1, 0), (0, -1)):                   # slots of times = 2: 0 .. 2
        assert pair(1, H, W, 2, left, right, 1) == FILM_ERR_INVALID, (left, right)
    assert pair(1, H, W, 1, 0, 2, 1) == FILM_ERR_INVALID                      # slots of times = 1: 0 .. 1
    assert pair(0, H, W, 2, 0, 1, 1) == FILM_ERR_INVALID
    assert pair(1, 30, W, 2, 0, 1, 1) == FILM_ERR_INVALID                     # not divisible by 8
    for slot in (-1, 2):
        assert lib.film_stream_schedule_json(hnd, 2, slot, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    # film_stream_plan_json keeps its refusal, whatever the option says
    eng.set_option('stream_times', 3)
    assert lib.film_stream_plan_json(hnd, 1, H, W, 2, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert 'slot must be 0 or 1' in lib.film_last_error(hnd).decode()
    eng.close()


@pytest.mark.parametrize('tiles', [1, 2])
def test_times_one_is_the_stream_plan(tiny_weights, tiles):
    """times = 1, left = 1 - s, right = s, extract = 1: the ops and buffers of film_stream_plan_json(slot = s) - which itself does not
    change when "stream_times" is set."""
    eng = _tiny_engine(tiny_weights)
    before = [eng.stream_plan(tiles, H, W, s) for s in (0, 1)]
    eng.set_option('stream_times', 3)
    for s in (0, 1):
        assert eng.stream_plan(tiles, H, W, s) == before[s]
        pair = eng.stream_pair_plan(tiles, H, W, 1, 1 - s, s, True)
        assert pair['ops'] == before[s]['ops'] and pair['buffers'] == before[s]['buffers']
        assert pair['arena_floats'] == before[s]['arena_floats'] and pair['n_extract'] == before[s]['n_extract']
        assert (pair['kind'], pair['slots'], pair['left'], pair['right'], pair['tiles']) == ('stream', 2, 1 - s, s, tiles)
    eng.close()


# ---- the schedule of a push ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slot', [0, 1])
@pytest.mark.parametrize('times', [1, 2, 3, 4])
def test_schedule_by_simulation(times, slot):
    """A push of B (position 2^T, into `slot`) after A (position 0, in the other slot): every index once, 2^(T-1) extractions, every
    step finds its two parents in its slots - extracted exactly when it does not extract them itself - and B stays where it was put."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    sch = eng.stream_schedule(times, slot)
    n = (1 << times) - 1
    assert (sch['times'], sch['slot'], sch['slots'], sch['produced']) == (times, slot, times + 1, n)
    steps = sch['steps']
    assert sorted(t['index'] for t in steps) == list(range(1, n + 1))
    assert sum(t['extract'] for t in steps) == 1 << (times - 1)
    assert steps[0]['extract'] == 1 and (steps[0]['left'], steps[0]['right']) == (1 - slot, slot)
    holds = {1 - slot: 0, slot: 1 << times}          # slot -> position of the frame it holds
    extracted = {1 - slot}                            # slots whose pyramids belong to the frame they hold (A: carried from the push before)
    for i, t in enumerate(steps):
        d = 1 << (times - t['depth'])
        assert 1 <= t['depth'] <= times and t['index'] % (2 * d) == d, t
        assert t['left'] != t['right'] and 0 <= t['left'] <= times and 0 <= t['right'] <= times
        assert holds.get(t['left']) == t['index'] - d and holds.get(t['right']) == t['index'] + d, (i, t, holds)
        assert t['left'] in extracted, (i, t)
        assert (t['right'] in extracted) == (not t['extract']), (i, t)    # no frame is extracted twice, none is read unextracted
        extracted.add(t['right'])
        assert t['feed'] == (1 + t['depth'] if t['depth'] < times else -1), t
        if t['feed'] >= 0:
            assert t['feed'] >= 2                      # a mid-frame never lands on an input slot
            holds[t['feed']] = t['index']              # (a later step that still needed the old frame fails the check above)
            extracted.discard(t['feed'])
    assert holds[slot] == 1 << times and slot in extracted
    # the last-depth mids are fed nowhere; every other one is extracted exactly once, by its left child
    assert all((t['feed'] < 0) == (t['depth'] == times) for t in steps)
    eng.close()


# ---- the orientations ---------------------------------------------------------------------------------------------------------------------
def _orientations(eng, times):
    seen = []
    for slot in (0, 1):
        for t in eng.stream_schedule(times, slot)['steps']:
            key = (t['left'], t['right'], t['extract'])
            if key not in seen:
                seen.append(key)
    return seen


@pytest.mark.parametrize('tiles', [1, 2])
def test_orientations_share_one_workspace(tiny_weights, tiles):
    times = 3
    eng = _tiny_engine(tiny_weights)
    keys = _orientations(eng, times)
    assert any(e for _, _, e in keys) and any(not e for _, _, e in keys)
    first = None
    for left, right, extract in keys:
        plan = eng.stream_pair_plan(tiles, H, W, times, left, right, extract)
        assert (plan['kind'], plan['slots'], plan['left'], plan['right'], plan['B']) == ('stream', times + 1, left, right, tiles)
        first = first or plan
        assert plan['buffers'] == first['buffers'] and plan['arena_floats'] == first['arena_floats']
        bufs = {b['name']: b for b in plan['buffers']}
        assert bufs['img0']['N'] == (times + 1) * tiles and bufs['feat0']['N'] == (times + 1) * tiles
        ne = plan['n_extract']
        assert (ne > 0) == bool(extract) and ne < len(plan['ops'])
        for op in plan['ops'][:ne]:
            assert op['NB'] == tiles and op['tag'].startswith(('image_pyramid', 'feat_')), op['tag']
            wr = _writes(op)
            assert wr
            for v, px in wr:
                b = bufs[v['buf']]
                part = b['floats'] // (times + 1)
                lo = b['off'] + right * part
                end = v['off'] + (px - 1) * v['stride'] + v['C']
                assert lo <= v['off'] and end <= lo + part, (op['tag'], v, b, right)
        assert not any(op['tag'].startswith(('image_pyramid', 'feat_')) for op in plan['ops'][ne:])
        for op in plan['ops'][ne:]:
            for v, _ in _writes(op):
                assert not _per_image(v['buf']), (op['tag'], v['buf'])
        # what is not the extraction does not depend on whether there is one (but for the indices of the ops waited for)
        twin = eng.stream_pair_plan(tiles, H, W, times, left, right, not extract)
        strip = lambda ops: [{k: v for k, v in op.items() if k != 'xdeps'} for op in ops]   # noqa: E731
        assert strip(plan['ops'][ne:]) == strip(twin['ops'][twin['n_extract']:])
        assert _check_bounds(plan) > 100
        assert _check_lanes(plan) > 0
        assert all(0 <= d < i for i, op in enumerate(plan['ops']) for d in op['xdeps'])   # a plan of its own: no wait for an op it lacks
    eng.close()


def test_plan_cache_keeps_slot_counts_apart():
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    asked = {'t1': lambda: eng.stream_pair_plan(2, H, W, 1, 1, 0, True), 't3': lambda: eng.stream_pair_plan(2, H, W, 3, 1, 0, True),
             'st0': lambda: eng.stream_plan(2, H, W, 0), 't3n': lambda: eng.stream_pair_plan(2, H, W, 3, 2, 1, False),
             'seq': lambda: eng.sequence_plan(1, 2, H, W)}
    first = {}
    for order in (('t1', 't3', 'st0', 't3n', 'seq'), ('t3n', 'seq', 't3', 'st0', 't1'), ('st0', 't3', 't1', 'seq', 't3n')):
        for k in order:
            got = asked[k]()
            assert first.setdefault(k, got) == got, k
    img0 = lambda p: next(b for b in p['buffers'] if b['name'] == 'img0')['N']   # noqa: E731
    assert (img0(first['t1']), img0(first['t3']), img0(first['t3n']), img0(first['st0'])) == (4, 8, 8, 4)
    assert first['t1']['ops'] == first['st0']['ops'] and first['t1']['arena_floats'] < first['t3']['arena_floats']
    assert first['t3n']['n_extract'] == 0 and first['seq']['kind'] == 'sequence'
    eng.close()


# ---- the interpreter ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fuse', [None, 0])
@pytest.mark.parametrize('tiles', [1, 2])
def test_recursive_pushes_in_the_interpreter(tiny_weights, tiles, fuse):
    """Frames A, B, C with T = 2, then again with T = 3, each through one persistent arena along the schedule; the feedback is the copy
    of `out` into img0's slot.  Every generated frame is within 1e-5 (the bound of test_stream_carry_in_the_interpreter for one pair:
    each frame is compared with the oracle on the interpreter's OWN two parents, so no error compounds) of the oracle's forward, and
    every feat* / img* slice a step does not fill keeps its bits."""
    from film_hip.options import TINY
    from oracle import film_oracle as fo
    import plan_interp as pi
    eng = _tiny_engine(tiny_weights, fuse)
    packed = eng.export_layouts()
    key = pi.blob_key(packed)
    rng = np.random.default_rng(11 + tiles)
    frames = [rng.random((tiles, H, W, 3), dtype=np.float32) for _ in range(3)]
    for times in (2, 3):
        S = times + 1
        plans = {}

        def plan_of(left, right, extract):
            k = (left, right, extract)
            if k not in plans:
                plans[k] = eng.stream_pair_plan(tiles, H, W, times, left, right, extract)
            return plans[k]

        base = plan_of(1, 0, 1)
        bufs = {b['name']: b for b in base['buffers']}
        per_image = [b for b in base['buffers'] if _per_image(b['name'])]
        arena = np.zeros(base['arena_floats'], np.float32)
        img0 = bufs['img0']
        fsz = frames[0].size

        def put(slot, fr):
            arena[img0['off'] + slot * fsz:img0['off'] + (slot + 1) * fsz] = fr.ravel()

        def snapshot():
            return {b['name']: arena[b['off']:b['off'] + b['floats']].reshape(S, -1).copy() for b in per_image}

        def unchanged(before, filled):
            for b in per_image:
                now = arena[b['off']:b['off'] + b['floats']].reshape(S, -1)
                for sl in range(S):
                    if sl == filled and b['name'] != 'img0':     # (img0 is only read: the frame was put there before the step)
                        continue
                    assert np.array_equal(now[sl], before[b['name']][sl]), (b['name'], sl, filled)

        held = {}
        slot = 0
        n_out = 0
        for i, fr in enumerate(frames):
            put(slot, fr)
            held[slot] = fr
            if i == 0:
                p = plan_of(1, 0, 1)
                before = snapshot()
                for op in p['ops'][:p['n_extract']]:
                    pi.run_op(op, arena, packed, bufs, verify_key=key)
                unchanged(before, 0)
            else:
                for t in eng.stream_schedule(times, slot)['steps']:
                    p = plan_of(t['left'], t['right'], t['extract'])
                    before = snapshot()
                    for op in p['ops']:
                        pi.run_op(op, arena, packed, bufs, verify_key=key)
                    unchanged(before, t['right'] if t['extract'] else -1)
                    out = pi.tap(p, arena, 'out').copy()
                    want = fo.film_forward(held[t['left']], held[t['right']], tiny_weights, oracle_options(TINY))
                    assert out.shape == want.shape
                    assert np.abs(out - want).max() < 1e-5, (times, i, t)
                    n_out += 1
                    if t['feed'] >= 0:
                        put(t['feed'], out)
                        held[t['feed']] = out
            slot = 1 - slot
        assert n_out == 2 * ((1 << times) - 1)
    eng.close()


# ---- Y4M and the CLI ----------------------------------------------------------------------------------------------------------------------
def test_multiply_rate():
    from film_hip import y4m
    tokens = y4m.header_tokens(6, 4, (30000, 1001))
    assert y4m.multiply_rate(tokens, 1) == list(tokens)
    assert y4m.multiply_rate(tokens, 2) == y4m.double_rate(tokens)
    got = y4m.multiply_rate(tokens, 8)
    assert [t for t in got if t[:1] == 'F'] == ['F240000:1001']
    assert [t for t in got if t[:1] != 'F'] == [t for t in tokens if t[:1] != 'F']
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            y4m.multiply_rate(tokens, bad)


def test_video_cli_times_to_interpolate():
    """--times_to_interpolate parses; with a stand-in stream that averages frames: (n - 1) * 4 + 1 frames in temporal order, the header
    rate x 4, inputs verbatim at multiples of 4, and a cut holds the previous frame three times."""
    from eval import video_cli as cli
    from film_hip import y4m
    ap = cli.build_parser()
    assert ap.parse_args(['--input', 'i', '--output', 'o']).times_to_interpolate == 1
    assert ap.parse_args(['--input', 'i', '--output', 'o', '--times_to_interpolate', '3']).times_to_interpolate == 3
    with pytest.raises(SystemExit):
        cli.main(['--input', '/nonexistent.y4m', '--output', 'o', '--times_to_interpolate', '7'])

    def avg(a, b):
        return ((a.astype(np.int32) + b) // 2).astype(np.uint8)

    class Stream:
        def __init__(self, times, cut_at): self.prev, self.i, self.times, self.cut_at = None, -1, times, cut_at
        def __enter__(self): return self
        def __exit__(self, *exc): pass
        def push(self, frame):
            self.i += 1
            mid = None
            if self.prev is not None and self.i != self.cut_at:
                m = avg(self.prev, frame)
                mid = m if self.times == 1 else np.stack([avg(self.prev, m), m, avg(m, frame)])
            self.prev = frame
            return mid

    class It:
        def __init__(self, cut_at): self.cut_at, self.kw = cut_at, None
        def open_stream(self, h, w, pix, matrix, full_range, **kw):
            self.kw = kw
            return Stream(kw.get('times', 1), self.cut_at if kw.get('scene_cut') else None)

    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (5, 6, 6), dtype=np.uint8)        # five 4 x 6 I420 frames
    data = io.BytesIO()
    wr = y4m.Y4MWriter(data, y4m.header_tokens(6, 4, (25, 1)))
    for f in frames:
        wr.write(f)

    def run(times, scene_cut=0):
        it, out, cuts = It(2), io.BytesIO(), []
        kw = dict({'scene_cut': scene_cut, 'cuts': cuts} if scene_cut else {}, **({'times': times} if times != 1 else {}))
        n = cli.double_frame_rate(it, y4m.Y4MReader(io.BytesIO(data.getvalue())), out, 'bt709', None, **kw)
        rd = y4m.Y4MReader(io.BytesIO(out.getvalue()))
        got = list(rd)
        assert n == len(got)
        return it, rd, got, cuts

    it1, rd1, one, _ = run(1)
    assert it1.kw == {} and len(one) == 9 and 'F50:1' in rd1.tokens            # (times = 1: the stream is opened as before)
    it2, rd2, four, _ = run(2)
    assert it2.kw == {'times': 2} and len(four) == 17 and 'F100:1' in rd2.tokens
    for j in range(4):
        a, b = frames[j], frames[j + 1]
        m = avg(a, b)
        for k, want in enumerate((a, avg(a, m), m, avg(m, b))):
            assert np.array_equal(four[4 * j + k], want), (j, k)
    assert np.array_equal(four[16], frames[4])
    it3, _, held, cuts = run(2, 250)
    assert it3.kw == {'scene_cut': 250, 'times': 2} and cuts == [2] and len(held) == 17
    for k in range(17):
        want = frames[1] if k in (5, 6, 7) else four[k]               # input 2 starts a new scene: input 1 is held three times
        assert np.array_equal(held[k], want), k
    with pytest.raises(ValueError):
        cli.double_frame_rate(It(None), y4m.Y4MReader(io.BytesIO(data.getvalue())), io.BytesIO(), times=0)
