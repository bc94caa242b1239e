"""The per-op isolation run (tests/test_ops_gpu.py) covers every kernel variant the plans of the real workloads hold - checked on plan-only
handles, without a GPU (tests/op_cases.py: signature, candidates, workload_plans, uncovered).  A new planner rule or kernel family whose
variant no small case plans fails here, with the signature and an example op."""
import op_cases as OC
import op_harness as OH
from op_cases import CASES, NEW_CASES

# conv_wino2d_kernel tile shapes (film_kernels.h, Wino2dTile; a tile code holds the shape in its low four bits, +16: the XCD workgroup order)
W2D_8x64, W2D_8x32, W2D_8x32_S2, W2D_16x64, W2D_16x32, W2D_16x32_S2 = range(6)


def test_every_workload_variant_is_planned_by_a_case():
    missing = OC.uncovered(CASES + NEW_CASES)
    assert not missing, f'{len(missing)} kernel variants of the workload plans are in no case of the isolation run:\n' + OC.format_uncovered(missing)


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
