"""CPU tests of tile groups in a frame stream (include/film_hip.h, "Tile groups"), WITHOUT a GPU.

A stream whose frame does not fit one invocation runs every step of a push as G runs of one plan of n tiles, and a carry buffer holds per
(group, frame slot) what a pair run reads of an extracted frame.  film_stream_group_schedule_json prints the list the push walks: per step
and group the restores from the carry, where the extracted frame comes from, the run, the save and the joined tiles.  Here that list is
SIMULATED - a model of what the plan's slots and the carry hold, written down from the definition - for every selection of T <= 3, both
slots and the groupings (tiles, n) = (4, 1), (4, 2), (5, 2), (5, 3); three planted faults must each be caught by the same simulator.
"""
import copy
import ctypes
import os
import re

import pytest

H, W = 32, 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPINGS = ((4, 1), (4, 2), (5, 2), (5, 3))
NAMES = ('film_stream_layout_json', 'film_stream_group_schedule_json', 'film_debug_segment_copy')


@pytest.fixture(scope='module')
def eng():
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    return FilmEngine(TINY, device=-1)


def _positions(mask):
    return [i + 1 for i in range(64) if mask >> i & 1]


class Fault(AssertionError):
    pass


def _need(cond, what, entry):
    if not cond:
        raise Fault(f'{what}: {entry}')


def simulate(sched, prev_slot_valid=True):
    """Walks the entries of a group schedule over a model of the device: carry[(group, slot)] = (level, frame) with level 'img0' (a feed-cut left
    the tiles) or 'all' (a save left the pyramids), plan[slot] = (level, group, frame, stamp, dirty) - stamp = the (step, group) that put it
    there, dirty = extracted and not yet saved.  frame: the position between the two inputs (0: the earlier frame, 2^T: the pushed one).
    Raises Fault at the first entry that reads what is not there."""
    T, slot, tiles, n, G = sched['times'], sched['slot'], sched['tiles'], sched['group_tiles'], sched['groups']
    assert G == -(-tiles // n) and sched['slots'] == T + 1
    grouped = G > 1
    carry, plan = {}, {}
    if grouped and prev_slot_valid:
        for g in range(G):
            carry[(g, 1 - slot)] = ('all', 0)
    elif prev_slot_valid:
        plan[1 - slot] = ('all', 0, 0, None, False)
    joined = {}
    by_step = {}
    for e in sched['steps']:
        by_step.setdefault(e['step'], []).append(e['group'])
    _need(all(v == list(range(G)) for v in by_step.values()), 'every step runs its groups in order', by_step)
    _need(sorted(by_step) == list(range(len(by_step))), 'steps are numbered in order', by_step)
    order = [(e['step'], e['group']) for e in sched['steps']]
    _need(order == sorted(order), 'outer = the steps, inner = the groups', order)

    def put(s, value, e):
        old = plan.get(s)
        _need(not (old and old[4]), f'slot {s} of the plan is reused before its extracted state was saved', e)
        plan[s] = value

    for e in sched['steps']:
        g, stamp = e['group'], (e['step'], e['group'])
        r = min(n, tiles - g * n)
        _need((e['tile0'], e['ntiles']) == (g * n, r), 'the tile range of the group', e)
        _need(e['last'] == int(g == G - 1), 'last', e)
        pair, extract, left, right = e['run'] == 'pair', bool(e['extract']), e['left'], e['right']
        _need(pair or extract, 'a run that does nothing', e)
        _need(grouped or (not e['restore'] and e['save'] == -1), 'one group: no restore, no save', e)
        for s in e['restore']:
            st = carry.get((g, s))
            _need(st is not None and st[0] == 'all', f'restore of slot {s} from a carry entry no save made valid', e)
            put(s, ('all', g, st[1], stamp, False), e)
        if e['cut'] == 'keep':
            _need(extract and right < 2, 'only a pushed frame is cut from keep', e)
            put(right, ('img0', g, 1 << T, stamp, False), e)
        elif e['cut'] == 'carry':
            st = carry.get((g, right))
            _need(grouped and extract and st is not None and st[0] == 'img0', 'img0 restore from a carry entry no feed-cut made valid', e)
            put(right, ('img0', g, st[1], stamp, False), e)
        elif e['cut'] == 'plan':
            st = plan.get(right)
            _need(not grouped and extract and st is not None and st[0] == 'img0', 'one group: the fed-back tiles are in the plan', e)
        else:
            _need(e['cut'] == 'none' and not extract, 'an extraction needs a source', e)
        if extract:
            st = plan.get(right)
            _need(st is not None and st[0] == 'img0' and st[1] == g and (not grouped or st[3] == stamp), 'the extraction reads tiles that were not put there for it', e)
            plan[right] = ('all', g, st[2], stamp, grouped)
        if pair:
            half = 1 << (T - e['depth'])
            for s, frame in ((left, e['index'] - half), (right, e['index'] + half)):
                st = plan.get(s)
                _need(st is not None and st[0] == 'all' and st[1] == g, f'the pair run reads slot {s}, which does not hold an extracted frame of this group', e)
                _need(not grouped or st[3] == stamp, f'the pair run reads slot {s}, which was not restored in this step and group', e)
                _need(st[2] == frame, f'the pair run reads frame {st[2]} in slot {s}, its parent is {frame}', e)
        else:
            _need(plan[right][2] == e['index'], 'an extraction-only step extracts the frame at its index', e)
        if e['save'] >= 0:
            st = plan.get(e['save'])
            _need(e['save'] == right and st is not None and st[0] == 'all' and st[1] == g and st[4], 'a save of what this run did not extract', e)
            carry[(g, e['save'])] = ('all', st[2])
            plan[e['save']] = st[:4] + (False,)
        if pair:
            _need(len(e['join']) == 2, 'a pair run joins its tiles', e)
            _need(e['join'] == [g * n, r], 'the join covers the tiles of the group', e)
            seen = joined.setdefault(e['step'], [])
            seen.extend(range(e['join'][0], e['join'][0] + e['join'][1]))
        else:
            _need(e['join'] == [], 'an extraction joins nothing', e)
        if e['last'] and pair:
            _need(sorted(joined[e['step']]) == list(range(tiles)), 'every tile is joined exactly once', joined[e['step']])
        want_feed = 'none' if e['feed'] < 0 or not e['last'] else 'carry' if grouped else 'plan'
        _need(e['feed_to'] == want_feed, 'feed_to', e)
        if e['feed_to'] == 'carry':
            for c in range(G):
                carry[(c, e['feed'])] = ('img0', e['index'])
        elif e['feed_to'] == 'plan':
            put(e['feed'], ('img0', 0, e['index'], None, False), e)
    for s, st in plan.items():
        _need(not st[4], f'slot {s} was extracted and never saved', st)
    if grouped:   # the next push finds the pushed frame in the carry, every group of it
        for g in range(G):
            _need(carry.get((g, slot)) == ('all', 1 << T), 'the pushed frame is in the carry when the push ends', (g, slot))
    return carry


STEP_KEYS = ('left', 'right', 'extract', 'index', 'depth', 'feed', 'deliver', 'run')


def _collapsed(sched):
    return [{k: e[k] for k in STEP_KEYS} for e in sched['steps'] if e['group'] == 0]


def test_symbols_are_declared_exported_and_listed():
    from film_hip import engine
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    vmap = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    kernels = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_kernels.h')).read()
    stubs = open(os.path.join(ROOT, 'tools', 'sanitize', 'launch_stubs.cpp')).read()
    lib = engine.load_library()
    for n in NAMES:
        assert re.search(r'^int ' + n + r'\(', header, re.M), n
        assert re.search(r'\b' + n + ';', vmap), n
        assert n in engine.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert re.search(r'^hipError_t film_launch_segment_copy\(', kernels, re.M)
    assert 'film_launch_segment_copy(' in stubs                      # (the host-only build keeps linking)
    assert 'a stream neither chunks a frame' not in header and 'Tile groups' in header


def test_refusals(eng):
    from film_hip.engine import FILM_ERR_INVALID, FILM_ERR_STATE
    lib, hnd = eng._lib, eng._h
    need = ctypes.c_int64()
    q = lambda tiles, times, slot, mask, n: lib.film_stream_group_schedule_json(hnd, tiles, H, W, times, slot, mask, n, None, 0, ctypes.byref(need))   # noqa: E731
    assert q(4, 2, 0, 0b111, 2) == 0 and need.value > 100
    assert q(0, 2, 0, 0b111, 2) == FILM_ERR_INVALID and q(4, 2, 0, 0b111, 0) == FILM_ERR_INVALID
    assert q(4, 0, 0, 1, 2) == FILM_ERR_INVALID and q(4, 2, 2, 1, 2) == FILM_ERR_INVALID
    assert q(4, 2, 0, 0b1000, 2) == FILM_ERR_INVALID and 'mask' in lib.film_last_error(hnd).decode()
    assert lib.film_stream_layout_json(hnd, None, 0, ctypes.byref(need)) == FILM_ERR_STATE
    assert lib.film_stream_layout_json(None, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    seg = (ctypes.c_int64 * 3)(0, 0, 4)
    assert lib.film_debug_segment_copy(seg, 33, 16, 16, None) == FILM_ERR_INVALID        # more than 32 segments
    assert lib.film_debug_segment_copy(seg, 1, None, 16, None) == FILM_ERR_INVALID       # a NULL pointer
    assert lib.film_debug_segment_copy(seg, 1, 18, 16, None) == FILM_ERR_INVALID         # a pointer that is no float's
    assert lib.film_debug_segment_copy((ctypes.c_int64 * 3)(0, -1, 4), 1, 16, 16, None) == FILM_ERR_INVALID
    assert lib.film_debug_segment_copy(None, 0, None, None, None) == 0                    # an empty table copies nothing


@pytest.mark.parametrize('tiles,n', GROUPINGS)
def test_group_schedule_simulates_for_every_selection(eng, tiles, n):
    for times in (1, 2, 3):
        for mask in range(1 << ((1 << times) - 1)):
            for slot in (0, 1):
                sched = eng.stream_group_schedule(tiles, H, W, times, slot, n, select=_positions(mask))
                assert (sched['times'], sched['slot'], sched['mask'], sched['tiles'], sched['group_tiles']) == (times, slot, mask, tiles, n)
                assert sched['produced'] == bin(mask).count('1')
                simulate(sched)
                # collapsing the groups gives stream_schedule's list
                want = eng.stream_schedule(times, slot, select=_positions(mask))['steps']
                assert _collapsed(sched) == [{k: s[k] for k in STEP_KEYS} for s in want], (times, mask, slot)
                assert len(sched['steps']) == len(want) * sched['groups']


def test_first_push_extracts_every_group_into_the_carry(eng):
    # a first push is the push of an empty selection on a stream that carries nothing: nothing may be restored
    for tiles, n in GROUPINGS:
        sched = eng.stream_group_schedule(tiles, H, W, 2, 0, n, select=[])
        assert all(e['run'] == 'extract' and e['restore'] == [] and e['cut'] == 'keep' and e['save'] == 0 for e in sched['steps'])
        simulate(sched, prev_slot_valid=False)


def test_one_group_is_the_stream_schedule_without_restore_or_save(eng):
    for times in (1, 2, 3):
        for mask in (0, 1, (1 << ((1 << times) - 1)) - 1, 1 << ((1 << times) - 2)):
            for n in (4, 7):                                # as many tiles as the frame has, and more
                sched = eng.stream_group_schedule(4, H, W, times, 1, n, select=_positions(mask))
                assert sched['groups'] == 1 and sched['group_tiles'] == 4
                assert all(e['restore'] == [] and e['save'] == -1 and e['cut'] != 'carry' and e['feed_to'] != 'carry' for e in sched['steps'])
                assert _collapsed(sched) == [{k: s[k] for k in STEP_KEYS} for s in eng.stream_schedule(times, 1, select=_positions(mask))['steps']]
                simulate(sched)


def test_carry_buffers_are_what_a_pair_run_reads_and_never_writes(eng):
    for times, n in ((1, 2), (3, 3)):
        plan = eng.stream_pair_plan(n, H, W, times, 1, 0, extract=False)
        assert plan['n_extract'] == 0
        reads, writes = set(), set()
        for op in plan['ops']:
            rd = [s['v'] for s in op['segs']] if op['kind'] == 'conv_mfma' else [op['in'], op['in2']]
            rd += [op['in3'], op['img_in'], op['pack_b'], op['pack_f']]
            wr = [op['pw_out'] if op['pw_out']['buf'] else op['out'], op['out2'], op['img_out']]
            reads |= {v['buf'] for v in rd if v['buf']}
            writes |= {v['buf'] for v in wr if v['buf']}
        want = [b['name'] for b in plan['buffers'] if b['N'] == (times + 1) * n and b['name'] in reads and b['name'] not in writes]
        sched = eng.stream_group_schedule(5, H, W, times, 0, n)
        assert sched['carry'] == want and 'img0' in want and len(want) >= 2
        assert all(re.fullmatch(r'(img|feat)\d+', name) for name in want)          # today: the image and feature pyramids


def _grouped(eng, tiles=5, n=2, times=2, slot=1):
    return eng.stream_group_schedule(tiles, H, W, times, slot, n)


def test_planted_missing_save_is_caught(eng):
    sched = _grouped(eng)
    simulate(sched)
    victims = [i for i, e in enumerate(sched['steps']) if e['save'] >= 0]
    assert len(victims) >= 6                                # (the pushed frame and the depth-1 mid, three groups each)
    for i in victims:
        bad = copy.deepcopy(sched)
        bad['steps'][i]['save'] = -1
        with pytest.raises(Fault):
            simulate(bad)


def test_planted_restore_from_the_wrong_slot_is_caught(eng):
    sched = _grouped(eng)
    victims = [i for i, e in enumerate(sched['steps']) if e['restore']]
    assert victims
    for i in victims:
        for k in range(len(sched['steps'][i]['restore'])):
            for wrong in range(sched['slots']):
                if wrong == sched['steps'][i]['restore'][k]:
                    continue
                bad = copy.deepcopy(sched)
                bad['steps'][i]['restore'][k] = wrong
                with pytest.raises(Fault):
                    simulate(bad)


def test_planted_join_of_n_tiles_in_the_short_group_is_caught(eng):
    for tiles, n in ((5, 2), (5, 3)):
        sched = _grouped(eng, tiles, n)
        short = [i for i, e in enumerate(sched['steps']) if e['ntiles'] < n and e['join']]
        assert short
        for i in short:
            bad = copy.deepcopy(sched)
            bad['steps'][i]['join'][1] = n
            with pytest.raises(Fault):
                simulate(bad)
