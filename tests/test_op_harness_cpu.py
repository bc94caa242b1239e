"""The per-op isolation harness (tests/op_harness.py) without a GPU: over the numpy backend (plan_interp.run_op on a float32 arena)
every op of a plan passes in the exact regime, and every planted fault is reported by the check that is there for it, at the op and
the place it was planted.  Also: the two debug entry points are declared and exported, the float64 run_op chain reproduces run_plan,
and the float32 restatements stay below the a-priori bound of a chunked sum."""
import os
import re

import numpy as np
import pytest

import op_harness as OH
import plan_interp as PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = (3, 64, 24)


def test_debug_entry_points_are_declared_and_exported():
    from film_hip import engine
    from film_hip.engine import FilmEngine, FilmError, FILM_ERR_NO_DEVICE
    from film_hip.options import TINY
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    assert re.search(r'^int film_debug_arena\(film_t\* h, int B, int H, int W, int tiles, int64_t offset, int64_t count, float\* data, '
                     r'int write\);', header, re.M)
    assert re.search(r'^int film_debug_run_op\(film_t\* h, int B, int H, int W, int tiles, int index, int candidate, int\* n_candidates\);',
                     header, re.M)
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    for name in ('film_debug_arena', 'film_debug_run_op'):
        assert re.search(rf'\b{name};', mapfile) and name in engine.EXPORTED_SYMBOLS
        assert getattr(engine.load_library(), name) is not None
    eng = FilmEngine(TINY, device=-1)       # plan-only handles have no workspace to show and nothing to launch on
    for call in (lambda: eng.debug_arena_read((1, 32, 32), 0, 1), lambda: eng.debug_run_op((1, 32, 32), 0)):
        with pytest.raises(FilmError) as e:
            call()
        assert e.value.code == FILM_ERR_NO_DEVICE
    eng.close()


def _plan(opt, key, integer, options=()):
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    eng = FilmEngine(opt, device=-1)
    for k, v in options:
        eng.set_option(k, v)
    eng.set_weights(OH.make_integer_weights(opt) if integer else W.make_synthetic_weights(opt, seed=0))
    eng.set_option('pack_groups', 4)     # every layout copy, so that run_plan can check all of them
    plan = eng.plan(*key)
    packed = eng.export_layouts()
    eng.close()
    return plan, packed


@pytest.fixture(scope='module')
def tiny_int():
    from film_hip.options import TINY
    return _plan(TINY, KEY, True)


@pytest.fixture(scope='module')
def tiny_float():
    from film_hip.options import TINY
    return _plan(TINY, KEY, False)


def _check_all(plan, packed):
    OH.assert_exact_regime(plan, packed)
    h = OH.Harness(OH.NumpyBackend(plan, packed), plan, packed, True)
    ops = h.distinct_ops()
    fails = [f for i in ops for f in h.check_op(i)]
    assert not fails, '\n'.join(map(str, fails[:20]))
    for i in ops:
        if plan['ops'][i]['kind'] == 'conv_mfma':
            assert h.ran_candidates[i] == 2
    return h, ops


def test_every_tiny_op_passes_in_the_exact_regime(tiny_int):
    plan, packed = tiny_int
    h, ops = _check_all(plan, packed)
    kinds = {plan['ops'][i]['kind'] for i in ops}
    assert {'conv_mfma', 'conv_pw', 'flow_head', 'pool', 'warp'} <= kinds
    assert {'BUF', 'C3', 'W2D', 'FOLD4'} <= {OH.family(plan['ops'][i]) for i in ops}
    # the F(4,3)-based ops are not exact on integers: they were held to the restatement, and that is on record
    assert {r.family for r in h.records} == {'W2D'} and all(np.isfinite(r.e_ref) and r.e_got <= OH.FACTOR * r.e_ref for r in h.records)


def test_every_published_64x64_op_passes_in_the_exact_regime():
    from film_hip.options import PUBLISHED
    plan, packed = _plan(PUBLISHED, (1, 64, 64), True)
    h, ops = _check_all(plan, packed)
    assert len(ops) < len(plan['ops'])      # (the shared predictor / extractor layers: deduplicated)
    assert max(op.get('ksplit', 1) for op in plan['ops']) == 16


def test_every_unfused_direct_op_passes_in_the_exact_regime():
    """fuse = 0 brings the op kinds a default plan fuses away (flow_up, flow_add, pack_flow), winograd = 0 / wino2d = 0 the direct
    kernel on every level, fold2x2 = 2 the four-phase form."""
    from film_hip.options import TINY
    plan, packed = _plan(TINY, (2, 32, 48), True, (('fuse', 0), ('winograd', 0), ('wino2d', 0), ('fold2x2', 2)))
    h, ops = _check_all(plan, packed)
    assert {'flow_up', 'flow_add', 'pack_flow'} <= {plan['ops'][i]['kind'] for i in ops}
    assert {OH.family(plan['ops'][i]) for i in ops if plan['ops'][i]['kind'] == 'conv_mfma'} == {'BUF', 'C3', 'FOLD2'}
    assert not h.records


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
class Faulty(OH.NumpyBackend):
    """The numpy backend with one fault planted in op `target`."""

    def __init__(self, plan, packed, fault, target):
        super().__init__(plan, packed)
        self.fault, self.target = fault, target

    def run(self, index, candidate):
        if index != self.target:
            return super().run(index, candidate)
        op, a, f = self.plan['ops'][index], self.arena, self.fault
        nb, h, w = op['NB'], op['H'], op['W']
        out = PI._view(a, op['out'], nb, h, w)
        lo, hi = OH.extent(op['out'], nb, h, w)
        if f == 'drop_last_k_chunk':                # the last 8 channels of the first segment never reach the sum
            seg = PI._view(a, op['segs'][0]['v'], nb, h, w)
            saved = seg[..., -8:].copy()
            seg[..., -8:] = 0
            n = super().run(index, candidate)
            seg[..., -8:] = saved
            return n
        if f in ('halo_from_next_image', 'leaky_before_bias'):
            x = PI.conv_input(op, a)
            ct, co = op['Ctot'], op['Cout']
            wt = np.ascontiguousarray(self.packed[op['w_off']:op['w_off'] + 9 * ct * co].reshape(co, 3, 3, ct).transpose(1, 2, 3, 0))
            bias = self.packed[op['b_off']:op['b_off'] + co]
            pre = PI.fo.conv2d_same(x, wt, None)
            if f == 'halo_from_next_image':         # the zero beyond the bottom-right corner read from the first pixel of the next image
                for n in range(nb - 1):
                    pre[n, h - 1, w - 1] += x[n + 1, 0, 0] @ wt[2, 2]
                out[...] = PI.fo.leaky_relu(pre + bias)
            else:
                out[...] = PI.fo.leaky_relu(pre) + bias
            return 2
        n = super().run(index, candidate)
        if f == 'shift_last_tile_column':           # the last 4-pixel tile column stored one pixel to the right
            x0 = (w - 1) // 4 * 4
            out[:, :, x0:] = np.roll(out[:, :, x0:], 1, axis=2)
        elif f == 'store_behind_view':
            a[hi] = 7.0
        elif f == 'modify_input':
            a[op['segs'][0]['v']['off'] + 5] += 1.0
        elif f == 'depends_on_background':
            out[1, 2, 3, 4] += a[self.background_offset] * np.float32(2.0 ** -8)
        elif f == 'one_ulp':
            out[1, 2, 3, 4] = np.nextafter(out[1, 2, 3, 4], np.float32(np.inf))
        elif f == 'splitk_order' and candidate == 1:    # the split-K partial sums of the K ranges added in the reverse order
            x = PI.conv_input(op, a)
            ks, ct, co, S = op['ksize'], op['Ctot'], op['Cout'], op['ksplit']
            wt = np.ascontiguousarray(self.packed[op['w_off']:op['w_off'] + ks * ks * ct * co].reshape(co, ks, ks, ct).transpose(1, 2, 3, 0))
            edges = [j * ct // S for j in range(S + 1)]
            parts = [PI.fo.conv2d_same(np.ascontiguousarray(x[..., lo:hi]), np.ascontiguousarray(wt[:, :, lo:hi]), None) for lo, hi in zip(edges, edges[1:])]
            acc = parts[-1]
            for part in parts[-2::-1]:
                acc = acc + part
            y = acc + self.packed[op['b_off']:op['b_off'] + co]
            out[...] = PI.fo.leaky_relu(y) if op['leaky'] else y
        return n


def _target(plan, **want):
    """First 3x3 leaky conv op on the direct kernel with three images of at least 12 pixels a row, and what else is asked."""
    for i, op in enumerate(plan['ops']):
        if (op['kind'] == 'conv_mfma' and OH.family(op) == 'BUF' and op['ksize'] == 3 and op['leaky'] and op['NB'] >= 3 and op['W'] >= 12 and
                not any(sg['up'] or sg['bmod'] for sg in op['segs']) and all(op.get(k, 1) >= v for k, v in want.items())):
            return i
    raise AssertionError('no such op in the plan')


def _planted(plan, packed, fault, target, integer=True):
    be = Faulty(plan, packed, fault, target)
    h = OH.Harness(be, plan, packed, integer)
    op = plan['ops'][target]
    touched = OH._merge([OH.extent(v, nb, hh, ww) for _, v, nb, hh, ww in OH.in_views(op) + OH.out_views(op)])
    be.background_offset = next(o for o in range(64, plan['arena_floats']) if not any(lo - 8 <= o < hi + 8 for lo, hi in touched))
    fails = h.check_op(target)
    assert fails and all(f.op == target and f.tag == op['tag'] for f in fails)
    # the neighbours of the op are clean: the fault is reported at the op it was planted in, and only there
    for other in (target - 1, target + 1):
        assert not h.check_op(other), other
    return fails, op


def test_a_shifted_last_tile_column_is_found(tiny_int):
    plan, packed = tiny_int
    fails, op = _planted(plan, packed, 'shift_last_tile_column', _target(plan))
    assert {f.check for f in fails} == {'value'}
    assert all(f.view == 'out' and f.coord[2] >= (op['W'] - 1) // 4 * 4 for f in fails)
    assert {f.input_set for f in fails} == {'dense-int', 'impulses'}    # (the impulses on both sides of that seam see it too)


def test_a_dropped_last_k_chunk_is_found(tiny_int):
    plan, packed = tiny_int
    t = _target(plan)
    fails, op = _planted(plan, packed, 'drop_last_k_chunk', t)
    assert {f.check for f in fails} == {'value'}
    # the one-hot impulses at the last channel of the segment name it without the dense set
    assert any(f.input_set == 'impulses' for f in fails) and any(f.input_set == 'dense-int' for f in fails)
    assert op['segs'][0]['v']['C'] - 1 in OH._boundary_channels(op)


def test_a_halo_read_from_the_next_image_is_found(tiny_int):
    plan, packed = tiny_int
    fails, op = _planted(plan, packed, 'halo_from_next_image', _target(plan))
    assert {f.check for f in fails} == {'value'}
    assert all(f.coord[1:3] == (op['H'] - 1, op['W'] - 1) and f.coord[0] < op['NB'] - 1 for f in fails)


def test_a_store_behind_the_output_view_is_found(tiny_int):
    plan, packed = tiny_int
    t = _target(plan)
    fails, op = _planted(plan, packed, 'store_behind_view', t)
    assert {f.check for f in fails} == {'ownership'}
    assert all(f.coord == (OH.extent(op['out'], op['NB'], op['H'], op['W'])[1],) for f in fails)


def test_a_modified_input_is_found(tiny_int):
    plan, packed = tiny_int
    fails, op = _planted(plan, packed, 'modify_input', _target(plan))
    assert {f.check for f in fails} == {'ownership'}
    assert all(f.coord == (op['segs'][0]['v']['off'] + 5,) and 'seg0 pixel (n 0, y 0, x 0), float 5' in f.where for f in fails)


def test_a_value_that_depends_on_the_background_is_found(tiny_int):
    plan, packed = tiny_int
    fails, op = _planted(plan, packed, 'depends_on_background', _target(plan))
    assert 'independence' in {f.check for f in fails}
    assert all(f.coord == (1, 2, 3, 4) for f in fails if f.check in ('independence', 'value'))


def test_split_k_parts_added_in_another_order_fail_the_candidate_comparison_only(tiny_float):
    """Candidate 1 adds the K-range partial sums of a split-K op in the reverse order: as good a float32 sum as candidate 0's (the value
    check passes), other bits (the candidate comparison does not)."""
    plan, packed = tiny_float
    t = next(i for i, op in enumerate(plan['ops']) if op['kind'] == 'conv_mfma' and op.get('ksplit', 1) > 1 and OH.family(op) == 'BUF')
    assert not OH.Harness(OH.NumpyBackend(plan, packed), plan, packed, False).check_op(t)
    fails = OH.Harness(Faulty(plan, packed, 'splitk_order', t), plan, packed, False).check_op(t)
    assert fails and {f.check for f in fails} == {'candidates'}
    assert all(f.candidate == 1 and f.op == t for f in fails)


def test_the_leaky_slope_before_the_bias_is_found(tiny_int):
    plan, packed = tiny_int
    fails, op = _planted(plan, packed, 'leaky_before_bias', _target(plan))
    assert {f.check for f in fails} == {'value'}


def test_one_ulp_in_one_output_is_found(tiny_int):
    plan, packed = tiny_int
    fails, op = _planted(plan, packed, 'one_ulp', _target(plan))
    assert {f.check for f in fails} == {'value'}
    assert all(f.coord == (1, 2, 3, 4) and f.view == 'out' for f in fails)


# ---- the references ------------------------------------------------------------------------------------------------------------------
def test_float64_op_chain_reproduces_run_plan(tiny_float):
    import inputs as TI
    plan, packed = tiny_float
    x0, x1 = TI.frame_pair(KEY[0], KEY[1], KEY[2], seed=5)
    a32 = PI.run_plan(plan, packed, x0, x1)
    a64 = np.zeros(plan['arena_floats'], np.float64)
    img0 = next(b for b in plan['buffers'] if b['name'] == 'img0')
    a64[img0['off']:img0['off'] + x0.size] = x0.ravel()
    a64[img0['off'] + x0.size:img0['off'] + 2 * x0.size] = x1.ravel()
    for op in plan['ops']:
        PI.run_op(op, a64, packed)
    for b in plan['buffers']:
        g, r = a32[b['off']:b['off'] + b['floats']], a64[b['off']:b['off'] + b['floats']]
        assert np.abs(g - r).max() <= 1e-4 * (1 + np.abs(r).max()), b['name']
    assert np.abs(PI.tap(plan, a32, 'out') - PI.tap(plan, a64, 'out')).max() < 1e-4


def test_restatement_errors_are_finite_and_below_the_a_priori_bound(tiny_float):
    """A chunked float32 sum of K products (+ bias, + activation) rounds at most K + 2 times, each by at most 2^-24 of a partial sum that
    S bounds: e_ref <= K + 2 = 9 Ctot + 2 for the direct restatement.  (It is a random walk: the measured values are a few units.)"""
    plan, packed = tiny_float
    h = OH.Harness(OH.NumpyBackend(plan, packed), plan, packed, False)
    fails = [f for i in h.distinct_ops() for f in h.check_op(i)]
    assert not fails, '\n'.join(map(str, fails[:10]))      # (the numpy backend - torch's float32 convolution - passes the rounding regime too)
    assert {r.family for r in h.records} >= {'BUF', 'C3', 'W2D', 'FOLD4', 'conv_pw', 'flow_head'}
    for r in h.records:
        assert np.isfinite(r.e_ref) and np.isfinite(r.e_got) and r.e_ref > 0, r
        if r.family in ('BUF', 'C3', 'conv_pw'):
            assert r.e_ref <= r.K + 2, r
