"""The per-op isolation run (tests/test_ops_gpu.py) covers every kernel variant the plans of the real workloads hold - checked on plan-only
handles, without a GPU (tests/op_cases.py: signature, candidates, workload_plans, uncovered).  A new planner rule or kernel family whose
variant no small case plans fails here, with the signature and an example op.  The same for the real-valued regime of the resampling kinds
(op_harness.REAL_KINDS): the cases plan every such variant of the workloads, every such op of the cases passes that regime on the
numpy backend, and the designed flows of a warp reach every class of query point they were designed for."""
import numpy as np
import pytest

import op_cases as OC
import op_harness as OH
from op_cases import CASES, NEW_CASES

# conv_wino2d_kernel tile shapes (film_kernels.h, Wino2dTile; a tile code holds the shape in its low four bits, +16: the XCD workgroup order)
W2D_8x64, W2D_8x32, W2D_8x32_S2, W2D_16x64, W2D_16x32, W2D_16x32_S2 = range(6)


def test_every_workload_variant_is_planned_by_a_case():
    missing = OC.uncovered(CASES + NEW_CASES)
    assert not missing, f'{len(missing)} kernel variants of the workload plans are in no case of the isolation run:\n' + OC.format_uncovered(missing)


def _case_ops_of_the_resampling_kinds():
    """(case id, op index, op) of what the isolation run checks on real-valued inputs: the distinct ops (op_harness.dedup_key) of the
    five resampling kinds in every plan of CASES, and in a plan of NEW_CASES those no earlier case covers."""
    cases = CASES + NEW_CASES
    for n, case in enumerate(cases):
        ops = OC.case_plan(*case)['ops']
        only = None if n < len(CASES) else {OH.dedup_key(ops[i]) for i in OC.ops_no_earlier_case_covers(cases, n)}
        seen = set()
        for i, op in enumerate(ops):
            key = OH.dedup_key(op)
            if op['kind'] in OH.REAL_KINDS and key not in seen and (only is None or key in only):
                seen.add(key)
                yield OC._case_id(*case), i, op


def test_every_resampling_op_of_the_workloads_runs_on_real_data():
    """tests/test_ops_gpu.py requires it of what it ran (_RAN_REAL); here: the cases plan it, and each op gets its input sets."""
    have = OC.Covered()
    kinds = set()
    for _, _, op in _case_ops_of_the_resampling_kinds():
        have.add(OC.signature(op), OC.candidates(op))
        kinds.add(op['kind'])
    assert kinds == set(OH.REAL_KINDS)
    missing = {}
    for label, op in OC.workload_ops():
        if op['kind'] in OH.REAL_KINDS and not have.covers(op):
            missing.setdefault(OC.signature(op), (label, op['tag'], f'{op["H"]}x{op["W"]}'))
    assert not missing, OC.format_uncovered(missing)


def _first_occurrences():
    """{case id: op indices}: an op that an earlier case holds at the same index with the same descriptor gets the same input sets (the
    harness seeds them with the index) on the same geometry - it is the same test, and runs once."""
    seen, out = set(), {}
    for case, i, op in _case_ops_of_the_resampling_kinds():
        if (i, OH.dedup_key(op)) not in seen:
            seen.add((i, OH.dedup_key(op)))
            out.setdefault(case, []).append(i)
    return out


@pytest.mark.parametrize('case', CASES + NEW_CASES, ids=[OC._case_id(*c) for c in CASES + NEW_CASES])
def test_every_resampling_op_of_the_cases_passes_on_real_data_without_a_gpu(case):
    """Every op of the five kinds that the isolation run holds to the float32 oracle, on the numpy backend: the input sets are made and
    run, no NaN comes out, and the float32 oracle stays within the a-priori float64 bounds on every set with finite flows."""
    idx = _first_occurrences().get(OC._case_id(*case), [])
    plan = OC.case_plan(*case)
    h = OH.Harness(OH.NumpyBackend(plan, None), plan, None, False)      # (these kinds read no weights)
    fails = [f for i in idx for f in h.check_op(i)]
    assert not fails, '\n'.join(map(str, fails[:20]))
    assert len(h.real_records) >= len(idx)
    for r in h.real_records:
        assert r.differ == 0 and (not r.has_f64 or r.ratio_oracle <= 1.0), r


def test_edge_flows_reach_every_class_of_q_on_every_warp_op():
    """The `edges` set of every warp op of the listed cases, for every flow the op reads directly (in2, pack_b, pack_f) and on both axes,
    puts at least one pixel into each class of op_harness.Q_CLASSES - read from the oracle's own q (fo.warp_query) in float32 and in
    float64, not from the targets the flows were solved for.  Behind the fused resize the flow is derived (in3): that op has no `edges`
    set and meets, through the random flows of `normal*s`, the classes that are intervals of q (Q_CLASSES_OF_A_DERIVED_FLOW: below the
    frame, in its last cell, beyond it, alpha clamped at either end) - asserted on the levels of at least 16 x 16 pixels, where one
    pixel in eight far away is enough of them; an integer q and a q that float32 rounds onto one are points no derived flow hits."""
    n_direct = n_derived = 0
    small = set()
    for case, i, op in _case_ops_of_the_resampling_kinds():
        if op['kind'] != 'warp':
            continue
        sets = {s.name.split('*')[0]: s for s in OH.input_sets(op, i, False)}       # (the harness seeds with seed + index, seed = 0)
        assert not any(np.isnan(a).any() for s in sets.values() for a in s.values.values())
        assert set(sets) == {'normal', 'huge'} | (set() if OH._has(op, 'in3') else {'edges'})
        assert sets['normal'].finite and not sets['huge'].finite
        for name, a in sets['huge'].values.items():
            if name not in OH.FLOW_VIEWS + ('in3',):
                assert np.isfinite(a).all(), (case, op['tag'], name)        # (the sources stay finite)
            elif a.size >= 100:     # (one lattice period: ten values on every fifth component)
                assert np.isinf(a).any() == (name != 'in3'), (case, op['tag'], name)
                assert np.abs(a[np.isfinite(a)]).max() == np.float32(3e38 if name != 'in3' else 8e37), (case, op['tag'], name)
        if OH._has(op, 'in3'):
            counts = OH.warp_classes(op, sets['normal'].values)
            assert set(counts) == {('in3', 'y'), ('in3', 'x')}
            if op['H'] >= 16 and op['W'] >= 16:
                n_derived += 1
                for key, c in counts.items():
                    assert all(c[k] > 0 for k in OH.Q_CLASSES_OF_A_DERIVED_FLOW), (case, op['tag'], key, c)
            continue
        n_direct += 1
        assert sets['edges'].finite
        counts = OH.warp_classes(op, sets['edges'].values)
        assert {n for n, _ in counts} == {n for n, *_ in OH.in_views(op) if n in OH.FLOW_VIEWS}
        for key, c in counts.items():
            assert (c > 0).all(), (case, op['tag'], key, dict(zip(OH.Q_CLASSES, c)))
        small.add((op['NB'], op['H'], op['W']))
    assert n_direct >= 20 and n_derived >= 10
    assert (2, 2, 2) in small and (1, 5, 11) in small      # (eight pixels are enough; a ragged level)


def _conv(sig):
    return sig[1], sig[2], sig[7]       # family, Ctot, ksplit


def _warp(sig):
    return sig[0], tuple(c for _, c in sig[9]), sig[13], sig[15], sig[16]    # kind, view channels, in3, src_brot, flow_brot


# What only the workload plans hold, by the NEW_CASES entry that plans it on a small frame:
#   the deep layers of the flow predictor and the fusion on conv_wino2d_kernel UNSPLIT (72 x 120 and 144 x 240 levels of a 1080p tile),
#   the coarsest (9 x 15) level of a 576 x 960 tile: conv_buf_kernel, K = 9 x 1920 over 8 ranges, a batch-remapped segment,
#   the per-direction warps of the stream and sequence plans (no batch rotation): with the fused x2 resize of the flow (in3 / out2) at 960,
#   448 and - on the 128 x 224 level of a 256 x 448 stream - 192 channels, with a plain flow (in2) at 192 and 64 channels.
ONLY_IN = {
    0: {('W2D', 1920, 1), ('W2D', 896, 1), ('W2D', 2448, 1), ('W2D', 1168, 1)},
    1: {('BUF', 1920, 8)},
    2: {('warp', (960, 2, 960, 2), True, False, False), ('warp', (448, 2, 448, 2), True, False, False), ('warp', (192, 2, 192, 2), True, False, False)},
    3: {('warp', (192, 2, 192), False, False, False), ('warp', (64, 2, 64), False, False, False)},
}


def _named(missing):
    return {_conv(s) if s[0] == 'conv_mfma' else _warp(s) for s in missing}


def test_removing_the_new_cases_is_noticed():
    missing = OC.uncovered(CASES)
    assert len(_named(missing)) == len(missing)     # (what is asserted below tells the signatures apart)
    assert _named(missing) == set().union(*ONLY_IN.values()), OC.format_uncovered(missing)
    # their segments: two 960- / 448-channel halves (+ 16 + the skip), the second half batch-remapped on the 9 x 15 level only
    segs = {_conv(s): s[8] for s in missing if s[0] == 'conv_mfma'}
    assert segs[('W2D', 1920, 1)] == ((960, False, False), (960, False, False))
    assert segs[('W2D', 896, 1)] == ((448, False, False), (448, False, False))
    assert segs[('W2D', 2448, 1)] == ((960, False, False), (960, False, False), (16, False, False), (512, False, False))
    assert segs[('W2D', 1168, 1)] == ((448, False, False), (448, False, False), (16, False, False), (256, False, False))
    assert segs[('BUF', 1920, 8)] == ((960, False, False), (960, False, True))
    for i, want in ONLY_IN.items():      # each entry is needed for exactly its own variants
        rest = NEW_CASES[:i] + NEW_CASES[i + 1:]
        missing = OC.uncovered(CASES + rest)
        assert _named(missing) == want, f'without {NEW_CASES[i]}:\n' + OC.format_uncovered(missing)


def test_every_new_case_has_ops_no_earlier_case_covers():
    cases = CASES + NEW_CASES
    for i in range(len(CASES), len(cases)):
        idx = OC.ops_no_earlier_case_covers(cases, i)
        ops = OC.case_plan(*cases[i])['ops']
        assert idx and len(idx) <= 12, (cases[i], [ops[j]['tag'] for j in idx])      # (a few seconds on the GPU: a handful of ops)
    # the unsplit conv_wino2d layers run on levels that admit every one of the six tiles, in both workgroup orders
    ops = OC.case_plan(*NEW_CASES[0])['ops']
    idx = OC.ops_no_earlier_case_covers(cases, len(CASES))
    assert {_conv(OC.signature(ops[j])) for j in idx} == ONLY_IN[0]
    for j in idx:
        assert {c & 15 for c in ops[j]['cands']} == set(range(6)) and len(ops[j]['cands']) == 12, ops[j]['tag']


def _w2d_shapes(h, w, cout, pw):
    """wino2d_candidates (film_tune.cpp) restated: the 16 x 16 arrangements where their tiles pad the level no more than the 8 x 32 ones."""
    pad_r = -(-w // 32) * -(-h // 8)
    pad_s = -(-w // 16) * -(-h // 16)
    sq = pad_s <= pad_r
    shapes = []
    if pw or cout % 64 == 0:
        shapes += [W2D_8x64] + ([W2D_16x64] if sq else [])
    if not pw:
        shapes += [W2D_8x32, W2D_8x32_S2] + ([W2D_16x32, W2D_16x32_S2] if sq else [])
    return sq, shapes


def test_plan_json_lists_the_candidates_of_every_op():
    plan = dict(OC.workload_plans())['plan(4,576,960)']
    levels = set()
    for op in plan['ops']:
        if op['kind'] != 'conv_mfma':
            assert op['cands'] == [], op['tag']
            continue
        assert len(op['cands']) >= 1 and len(set(op['cands'])) == len(op['cands']), op['tag']
        if OH.family(op) == 'W2D':
            sq, want = _w2d_shapes(op['H'], op['W'], op['Cout'], OH._has(op, 'pw_out'))
            assert [c & 15 for c in op['cands'][0::2]] == want and [c & 15 for c in op['cands'][1::2]] == want, (op['tag'], op['cands'])
            assert all(b == a + 16 for a, b in zip(op['cands'][0::2], op['cands'][1::2])), op['cands']      # (each shape in both workgroup orders)
            levels.add((op['H'], op['W'], sq))
            assert sq == any((c & 15) in (W2D_16x64, W2D_16x32, W2D_16x32_S2) for c in op['cands'])
    # one level with the square tiles and one without, as the rule says: 9 x 15 = 135 squares against 18 x 8 = 144 rows, 5 x 8 = 40 against 9 x 4 = 36
    assert (144, 240, True) in levels and (72, 120, False) in levels, levels
    assert not any((h, w, not sq) in levels for h, w, sq in levels)
