"""Every planned kernel launch in isolation (tests/op_harness.py) on the GPU: one op at a time on a workspace the test filled, through
film_debug_arena / film_debug_run_op - ownership of every float it did not have to write, independence of the background, equal bits
from every tile candidate, and the value against the float64 reference of the op on the same inputs (bit for bit on small integers
for the exact families, within 2 x the float32 restatement's own error on the points the restatement is evaluated at otherwise).
The resampling kinds (pool, flow_up, flow_add, pack_flow, warp) are exact on the small integers too, and on real-valued inputs - random
fields, flows solved onto every clamp of the warp, flows up to +-inf - every value they store must be the float32 oracle's
(plan_interp.run_op on a float32 arena), with an a-priori bound against float64 beside it; a fused pool or sum of a conv-like op must
be its unfused op of what the same launch stored.

Two engines per plan: one with integer weights (op_harness.make_integer_weights: the exact regime and the designed impulse sets), one
with the seeded synthetic weights (the rounding regime on random normal activations at three dynamic ranges, and the real-valued
regime of the resampling kinds).  Autotune is off: the
test runs every candidate of every conv op itself.  FILM_OP_ERRORS=<file> makes the run write its error table there (the source of
profiles/op_isolation_errors.md).

The case lists and the definition of "covered" live in tests/op_cases.py: the kernel variants the plans of the real workloads hold and
the small plans above do not (unsplit deep conv_wino2d layers, the 9 x 15 level's split, the per-direction warps) run through NEW_CASES,
only the ops no earlier case covers (test_workload_variants_in_isolation), with the same checks."""
import os
import time

import numpy as np
import pytest

from conftest import has_extra_families, needs_extra_families

import op_cases as OC
import op_harness as OH
from op_cases import CASES, EXTRA_CASES, NEW_CASES, _case_id, _config

pytestmark = pytest.mark.gpu
_T0 = time.time()

_KINDS, _FAMILIES, _CASES_RUN, _TABLE, _COUNTS = set(), set(), set(), [], []
_RAN = OC.Covered()  # signature (op_cases.signature) and candidate codes of every op that ran
_RAN_REAL = OC.Covered()    # ... of every op of the resampling kinds that ran on the real-valued input sets
_REAL_TABLE = []
_PLANNED = set()    # every conv family any op of any plan of this run uses (from the plan JSON: what the bound libraries hold and select)
DEFAULT_FAMILIES = {'BUF', 'C3', 'W2D', 'W43', 'FOLD4', 'FOLD2'}
EXTRA_FAMILIES = {'HALO', 'SPLIT6', 'SPLIT3', 'WINO', 'WINOX3', 'FOLDX3'}
ALL_KINDS = {'conv_mfma', 'conv_pw', 'flow_head', 'pool', 'warp', 'flow_up', 'flow_add', 'pack_flow'}


def _run_case(cfg, key, options, only=None):
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    opt = _config(cfg)
    t0 = time.time()
    fails, total = [], 0
    for integer in (True, False):
        eng = FilmEngine(opt, device=0)
        try:
            eng.set_option('autotune', 0)
            for k, v in options.items():
                eng.set_option(k, v)
            eng.set_weights(OH.make_integer_weights(opt) if integer else W.make_synthetic_weights(opt, seed=0))
            eng.debug_arena_read(key, 0, 1)            # creates the device plan (and packs the weight layouts it needs)
            plan = eng.sequence_plan(key[0] // key[3], key[3], key[1], key[2]) if len(key) > 3 else eng.plan(*key)
            packed = eng.export_layouts()
            if integer:
                OH.assert_exact_regime(plan, packed)
            h = OH.Harness(OH.GpuBackend(eng, key), plan, packed, integer)
            # ops of ONE plan that share their descriptor (op_harness.dedup_key) run once; nothing else is skipped
            ops = distinct = h.distinct_ops()
            if only is not None:    # (test_workload_variants_in_isolation: indices into the plan as a plan-only handle states it - the same plan)
                want = [(OC.signature(op), op['cands']) for op in OC.case_plan(cfg, key, options)['ops']]
                assert [(OC.signature(op), op['cands']) for op in plan['ops']] == want, 'the device plan differs from the plan-only one'
                seen = {OH.dedup_key(plan['ops'][i]) for i in only}
                ops = [i for i in distinct if OH.dedup_key(plan['ops'][i]) in seen]
            _PLANNED.update(OH.family(op) for op in plan['ops'] if op['kind'] == 'conv_mfma')
            for i in ops:
                op = plan['ops'][i]
                fails += h.check_op(i)
                _KINDS.add(op['kind'])
                if op['kind'] == 'conv_mfma':
                    _FAMILIES.add(OH.family(op))
                    n = h.n_candidates[i]       # (what film_debug_run_op reported for the op)
                    assert h.ran_candidates[i] == n >= 1, f'{op["tag"]}: {h.ran_candidates[i]} of {n} candidates ran'
                    assert n == len(op['cands']), f'{op["tag"]}: the plan lists {op["cands"]}, film_debug_run_op has {n} candidates'
                _RAN.add(OC.signature(op), OC.candidates(op))
                if not integer and op['kind'] in OH.REAL_KINDS:
                    _RAN_REAL.add(OC.signature(op), OC.candidates(op))
            total = len(plan['ops'])
            for r in h.records:
                _TABLE.append((_case_id(cfg, key, options), r))
            for r in h.real_records:
                _REAL_TABLE.append((_case_id(cfg, key, options), r))
            if integer:
                _COUNTS.append((_case_id(cfg, key, options), total, len(distinct), len(ops), eng.version()))
                print(f'{_case_id(cfg, key, options)}: {total} ops in the plan, {len(ops)} of {len(distinct)} distinct ones run')
        finally:
            eng.close()
    print(f'{_case_id(cfg, key, options)}: {time.time() - t0:.1f} s')
    _CASES_RUN.add(_case_id(cfg, key, options))
    assert not fails, f'{len(fails)} checks failed:\n' + '\n'.join(str(f) for f in fails[:40])


@pytest.mark.parametrize('cfg,key,options', CASES, ids=[_case_id(*c) for c in CASES])
def test_every_op_in_isolation(cfg, key, options):
    _run_case(cfg, key, options)


@needs_extra_families
@pytest.mark.parametrize('cfg,key,options', EXTRA_CASES, ids=[_case_id(*c) for c in EXTRA_CASES])
def test_every_op_in_isolation_extra_families(cfg, key, options):
    _run_case(cfg, key, options)


@pytest.mark.parametrize('cfg,key,options', NEW_CASES, ids=[_case_id(*c) for c in NEW_CASES])
def test_workload_variants_in_isolation(cfg, key, options):
    """The kernel variants only the plans of real workloads hold (op_cases.workload_plans), on the small plans of NEW_CASES that plan them
    too: the ops of the case whose signature and candidate list no earlier case of CASES + NEW_CASES covers, checked like every other op."""
    cases = CASES + NEW_CASES
    only = OC.ops_no_earlier_case_covers(cases, cases.index((cfg, key, options)))
    assert only, 'every op of the case is covered by an earlier one: the case adds nothing'
    _run_case(cfg, key, options, only=only)


def test_debug_entry_points_refuse_what_the_header_says(tiny_weights):
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_INVALID
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=0)
    eng.set_option('autotune', 0)
    eng.set_weights(tiny_weights)
    key = (1, 32, 32)
    plan = eng.plan(*key)
    n = plan['arena_floats']
    assert eng.debug_arena_read(key, n - 4, 4).shape == (4,)
    for off, cnt in ((n - 3, 4), (-1, 2), (n + 1, 0)):
        with pytest.raises(FilmError) as e:
            eng.debug_arena_read(key, off, cnt)
        assert e.value.code == FILM_ERR_INVALID
    conv = next(i for i, op in enumerate(plan['ops']) if op['kind'] == 'conv_mfma')
    other = next(i for i, op in enumerate(plan['ops']) if op['kind'] != 'conv_mfma')
    nc = eng.debug_run_op(key, conv, -1)
    assert nc >= 1 and eng.debug_run_op(key, other, -1) == 0
    for index, cand in ((conv, nc), (conv, -2), (other, 0), (len(plan['ops']), -1), (-1, -1)):
        with pytest.raises(FilmError) as e:
            eng.debug_run_op(key, index, cand)
        assert e.value.code == FILM_ERR_INVALID
    # both set the plan film_get_tap reads
    x = np.arange(32 * 32 * 3, dtype=np.float32)
    eng.debug_arena_write(key, next(b for b in plan['buffers'] if b['name'] == 'img0')['off'], x)
    assert np.array_equal(eng.tap('img0')[0].ravel(), x)
    eng.close()


def test_coverage_of_the_isolation_run():
    """Every op kind, every conv family of the bound library (and of the extra-families library when it has been built) and every
    candidate (asserted per op above) has run - and every kernel variant (op_cases.signature, with a superset of its tile candidates) of
    every op the plans of the real workloads hold (op_cases.workload_plans, on a plan-only handle).  Needs the whole file to have run in
    this session."""
    want = {_case_id(*c) for c in CASES + NEW_CASES}
    extra_built = has_extra_families() or os.path.isfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                    'frame-interpolation_amd', 'film_hip', 'libfilm_hip_extra.so'))
    if extra_built:
        want |= {_case_id(*c) for c in EXTRA_CASES}
    assert want <= _CASES_RUN, f'run the whole file: {sorted(want - _CASES_RUN)} did not run (or failed before the end)'
    assert ALL_KINDS <= _KINDS, ALL_KINDS - _KINDS
    # every family a plan of this run selected has run (derived from the plans' family codes: a family added to the library later is
    # required as soon as a listed option set reaches it) - and the listed option sets reach every family the libraries hold today
    assert _PLANNED <= _FAMILIES, _PLANNED - _FAMILIES
    fams = DEFAULT_FAMILIES | (EXTRA_FAMILIES if extra_built else set())
    assert fams <= _PLANNED, fams - _PLANNED
    missing, missing_real = {}, {}
    for label, op in OC.workload_ops():
        if not _RAN.covers(op):
            missing.setdefault(OC.signature(op), (label, op['tag'], f'{op["H"]}x{op["W"]}'))
        if op['kind'] in OH.REAL_KINDS and not _RAN_REAL.covers(op):
            missing_real.setdefault(OC.signature(op), (label, op['tag'], f'{op["H"]}x{op["W"]}'))
    assert not missing, f'{len(missing)} kernel variants of the workload plans did not run in isolation:\n' + OC.format_uncovered(missing)
    assert not missing_real, (f'{len(missing_real)} variants of the resampling kinds in the workload plans did not run on real-valued inputs:\n' +
                              OC.format_uncovered(missing_real))
    # every op of those kinds ran every input set made for it, and no output value differed from the float32 oracle
    assert _REAL_TABLE and {r.kind for _, r in _REAL_TABLE} == set(OH.REAL_KINDS)
    assert {r.input_set.split('*')[0] for _, r in _REAL_TABLE if r.kind == 'warp'} == {'normal', 'edges', 'huge'}
    path = os.environ.get('FILM_OP_ERRORS')
    if path:
        _write_table(path)


def _write_table(path):
    rows = {}
    for case, r in _TABLE:
        k = (r.family, r.K, r.input_set.split('*')[0])
        cur = rows.setdefault(k, [0, 0.0, 0.0, 0.0, 'every op: restatement and kernel both exact (e = 0)', 0.0])
        cur[0] += 1
        cur[5] = max(cur[5], r.e_full)
        if r.e_ref == r.e_ref and r.e_ref > 0:
            ratio = r.e_got / r.e_ref
            if ratio >= cur[3]:
                cur[1], cur[2], cur[3], cur[4] = r.e_ref, r.e_got, ratio, f'{case}: {r.tag}'
    with open(path, 'w') as f:
        f.write('# Per-op isolation run: rounding error of every kernel family against its float32 restatement\n\n')
        f.write('Written by tests/test_ops_gpu.py (FILM_OP_ERRORS).  e = max |got - float64| / (2^-24 S); e_ref: the float32 restatement of the\n'
                'kernel\'s accumulation structure on a sample of the output, e_gpu: the kernel on the same sample, e_full: the kernel on the\n'
                'whole output (held to 4 x e_ref; the sample IS the whole output for the ops the restatement can afford to cover).  One line per family, K = ksize^2 Ctot and input set: the op\n'
                'with the largest e_gpu / e_ref of `ops` tested ones.  The test requires ratio <= 2.\n\n')
        f.write('| family | K | input set | ops | e_ref | e_gpu | ratio | largest e_full | worst op |\n|---|---|---|---|---|---|---|---|---|\n')
        for (fam, K, s), (n, er, eg, ratio, tag, ef) in sorted(rows.items()):
            shown = f'{ratio:.2f}' if er > 0 else '-'
            f.write(f'| {fam} | {K} | {s} | {n} | {er:.2f} | {eg:.2f} | {shown} | {ef:.2f} | {tag} |\n')
        f.write('\n## The resampling kinds on real-valued inputs\n\n'
                'pool, flow_up, flow_add, pack_flow and warp against the float32 oracle (plan_interp.run_op on a float32 arena), value for value:\n'
                '`differ` must be 0.  e = |got - float64| where e / bound is largest, bound = the a-priori bound there (op_harness.f64_bounds: one\n'
                'rounding per operation of the oracle; required: e <= bound, for the kernel and for the float32 oracle); the `huge` flows include\n'
                '+-inf and have no float64 column.\n\n'
                '| kind | input set | ops | values | differ | largest e / bound | e | bound | float32 oracle: largest e / bound |\n|---|---|---|---|---|---|---|---|---|\n')
        real = {}
        for case, r in _REAL_TABLE:
            cur = real.setdefault((r.kind, r.input_set.split('*')[0]), [0, 0, 0, -1.0, 0.0, 0.0, 0.0, r.has_f64])
            cur[0] += 1
            cur[1] += r.size
            cur[2] += r.differ
            cur[6] = max(cur[6], r.ratio_oracle)
            if r.ratio > cur[3]:
                cur[3], cur[4], cur[5] = r.ratio, r.e, r.bound
        for (kind, s), (n, size, differ, ratio, e, bound, orc, has) in sorted(real.items()):
            f.write(f'| {kind} | {s} | {n} | {size} | {differ} | ' + (f'{ratio:.3f} | {e:.3g} | {bound:.3g} | {orc:.3f} |\n' if has else '- | - | - | - |\n'))
        f.write('\n## Ops per plan\n\n| plan | ops | distinct ops run | library |\n|---|---|---|---|\n')
        for case, total, distinct, run, ver in _COUNTS:
            f.write(f'| {case} | {total} | {run if run == distinct else f"{run} of {distinct}"} | {ver} |\n')
        f.write(f'\nWall time of the file: {time.time() - _T0:.0f} s.\n')
