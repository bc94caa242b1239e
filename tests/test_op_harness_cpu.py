"""The per-op isolation harness (tests/op_harness.py) without a GPU: over the numpy backend (plan_interp.run_op on a float32 arena)
every op of a plan passes in the exact regime, and every planted fault is reported by the check that is there for it, at the op and
the place it was planted - the faults of the resampling kinds (a reordered pool sum, lerps contracted to an fma, a conversion before the
clamp ...) by the real-valued regime, with on record which of them the small-integer set cannot see.  Also: the two debug entry points are declared and exported, the float64 run_op chain reproduces run_plan,
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
        if f in REAL_FAULTS:
            n = super().run(index, candidate)
            with np.errstate(all='ignore'):
                self._real_fault(op, f)
            return n
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

    def _real_fault(self, op, f):
        """The faults of the resampling kinds (and of a fused pool): the op has run; its `out` (the fused pool: `out2`) is overwritten
        with what the faulty kernel would have stored."""
        a, fo = self.arena, PI.fo
        nb, h, w = op['NB'], op['H'], op['W']
        if f == 'pool_tree':                        # (a + b) + (c + d) instead of ((a + b) + c) + d
            x = np.ascontiguousarray(PI._view(a, op['in'], nb, h, w))
            s = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])
            PI._view(a, op['out'], nb, h // 2, w // 2)[...] = s * np.float32(0.25)
        elif f == 'flow_up_fma':                    # a + (b - a) t with the product and the sum rounded once
            x = np.float32(2) * np.ascontiguousarray(PI._view(a, op['in'], nb, h, w))
            ylo, yhi, yl = fo._resize_axis_weights(h, 2 * h, np.float32)
            xlo, xhi, xl = fo._resize_axis_weights(w, 2 * w, np.float32)
            xl, yl = xl[None, None, :, None], yl[None, :, None, None]
            top = _fma(x[:, ylo][:, :, xhi] - x[:, ylo][:, :, xlo], xl, x[:, ylo][:, :, xlo])
            bot = _fma(x[:, yhi][:, :, xhi] - x[:, yhi][:, :, xlo], xl, x[:, yhi][:, :, xlo])
            PI._view(a, op['out'], nb, 2 * h, 2 * w)[...] = _fma(bot - top, yl, top)
        elif f == 'pool_before_activation':         # the fused pool of a conv op taken from the values in front of the leaky relu
            x = PI.conv_input(op, a)
            ct, co = op['Ctot'], op['Cout']
            wt = np.ascontiguousarray(self.packed[op['w_off']:op['w_off'] + 9 * ct * co].reshape(co, 3, 3, ct).transpose(1, 2, 3, 0))
            pre = fo.conv2d_same(x, wt, self.packed[op['b_off']:op['b_off'] + co], None)
            PI._view(a, op['out2'], nb, h // 2, w // 2)[...] = fo.avg_pool2x2(pre)
        elif f == 'one_ulp_real':
            out = PI._view(a, op['out'], nb, h, w)
            out[0, 1, 1, 0] = np.nextafter(out[0, 1, 1, 0], np.float32(np.inf))
        else:                                       # a warp: `out` again, from the flow the op used
            src = np.roll(np.ascontiguousarray(PI._view(a, op['in'], nb, h, w)), -op.get('src_brot', 0), axis=0)
            if OH._has(op, 'in3'):
                flow = np.ascontiguousarray(PI._view(a, op['out2'], nb, h, w))
            else:
                flow = np.roll(np.ascontiguousarray(PI._view(a, op['in2'], nb, h, w)), -op.get('flow_brot', 0), axis=0)
            PI._view(a, op['out'], nb, h, w)[...] = _warp_variant(src, np.float32(op['fscale']) * flow, f)


def _fma(a, b, c):
    """float32 a * b + c with the product and the sum in float64, rounded once."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


REAL_FAULTS = ('pool_tree', 'flow_up_fma', 'pool_before_activation', 'one_ulp_real', 'warp_fma', 'floor_int32', 'clamp_last',
               'alpha_unclamped', 'swap_flow')


def _warp_variant(src, flow, fault):
    """fo.warp(src, flow) in float32 (flow = (x, y), already scaled) with one fault:
    warp_fma         every lerp t * (b - a) + a as one fma
    floor_int32      floor(q) converted to int32 first (out of range: INT32_MIN, what the conversion instruction gives), then clamped
    clamp_last       the lower index clamped to size - 1 instead of size - 2, the upper corner clamped to size - 1
    alpha_unclamped  alpha = q - floor, not clipped to [0, 1]
    swap_flow        the x component of the flow moves y and the other way round"""
    n, h, w, _ = src.shape
    if fault == 'swap_flow':
        flow = flow[..., ::-1]
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    qy, qx = gy[None] + flow[..., 1], gx[None] + flow[..., 0]

    def axis(q, size):
        fl = np.floor(q)
        if fault == 'floor_int32':
            i = np.where(np.isfinite(fl) & (np.abs(fl) < 2.0 ** 31), fl, -2.0 ** 31).astype(np.int64)
            fl = np.clip(i, 0, size - 2).astype(np.float32)
        else:
            fl = np.minimum(np.maximum(fl, 0), size - (1 if fault == 'clamp_last' else 2))
        al = q - fl
        if fault != 'alpha_unclamped':
            al = np.clip(al, 0, 1)
        lo = fl.astype(np.int64)
        return lo, np.minimum(lo + 1, size - 1), al[..., None].astype(np.float32)
    (y0, y1, ay), (x0, x1, ax) = axis(qy, h), axis(qx, w)
    b = np.arange(n)[:, None, None]
    lerp = (lambda t, p, q: _fma(t, q - p, p)) if fault == 'warp_fma' else (lambda t, p, q: t * (q - p) + p)
    top = lerp(ax, src[b, y0, x0], src[b, y0, x1])
    bot = lerp(ax, src[b, y1, x0], src[b, y1, x1])
    return lerp(ay, top, bot)


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


# ---- the resampling kinds on real data ----------------------------------------------------------------------------------------------
UNFUSED = ((2, 32, 48), (('fuse', 0),))      # flow_up, flow_add, pack_flow and the plain warps as ops of their own


@pytest.fixture(scope='module')
def unfused_int():
    from film_hip.options import TINY
    return _plan(TINY, UNFUSED[0], True, UNFUSED[1])


@pytest.fixture(scope='module')
def unfused_float():
    from film_hip.options import TINY
    return _plan(TINY, UNFUSED[0], False, UNFUSED[1])


def _real_ops(plan):
    return [i for i, op in enumerate(plan['ops']) if op['kind'] in OH.REAL_KINDS]


@pytest.mark.parametrize('which', ['tiny', 'unfused'])
def test_every_resampling_op_passes_on_real_data(which, tiny_float, unfused_float):
    """plan_interp.run_op in float32 IS the oracle the bits are held to: what this run shows is that the float32 oracle stays within
    the a-priori float64 bounds on every input set with finite flows, that every set runs, and that the `huge` flows give no NaN."""
    plan, packed = tiny_float if which == 'tiny' else unfused_float
    h = OH.Harness(OH.NumpyBackend(plan, packed), plan, packed, False)
    ops = [i for i in h.distinct_ops() if i in set(_real_ops(plan))]
    fails = [f for i in ops for f in h.check_op(i)]
    assert not fails, '\n'.join(map(str, fails[:20]))
    kinds = {r.kind for r in h.real_records}
    assert kinds == ({'pool', 'warp'} if which == 'tiny' else set(OH.REAL_KINDS))
    for r in h.real_records:
        assert r.differ == 0 and r.size > 0
        assert r.has_f64 == (r.input_set != 'huge') and (not r.has_f64 or r.ratio == r.ratio_oracle <= 1.0), r
    sets = lambda tag: {r.input_set.split('*')[0] for r in h.real_records if r.tag == tag}      # noqa: E731
    for i in ops:
        op = plan['ops'][i]
        want = {'normal'} if op['kind'] != 'warp' else {'normal', 'huge'} | (set() if OH._has(op, 'in3') else {'edges'})
        assert sets(op['tag']) == want, op['tag']
    # the bounds bind: the oracle uses a good part of them (they are sums of worst cases: a third to nine tenths is what a maximum
    # over some 1e4 outputs reaches), so that an error of a few ulps would exceed them
    assert max(r.ratio for r in h.real_records if r.kind == 'warp') > 0.3 and max(r.ratio for r in h.real_records if r.kind == 'pool') > 0.3


def test_the_unfaulted_warp_variant_is_the_oracle():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((2, 7, 9, 5), dtype=np.float32)
    flow = rng.standard_normal((2, 7, 9, 2), dtype=np.float32) * np.float32(4)
    assert np.array_equal(_warp_variant(src, flow, None), PI.fo.warp(src, flow))


def _first(plan, kind, **want):
    return next(i for i, op in enumerate(plan['ops']) if op['kind'] == kind and all(OH._has(op, k) == v for k, v in want.items()))


# fault -> (plan, op, the real-valued sets that must report it, whether dense-int reports it)
REAL_PLANTED = {
    'pool_tree': ('tiny', lambda p: max(i for i, op in enumerate(p['ops']) if op['kind'] == 'pool'), {'normal'}, False),
    'pool_tree/c3': ('tiny', lambda p: _first(p, 'pool') + 1, {'normal'}, False),
    'warp_fma': ('tiny', lambda p: _first(p, 'warp', in3=False, img_out=False), {'normal', 'edges', 'huge'}, False),
    'warp_fma/fused': ('tiny', lambda p: _first(p, 'warp', in3=True), {'normal', 'huge'}, False),
    'flow_up_fma': ('unfused', lambda p: _first(p, 'flow_up'), {'normal'}, False),
    'floor_int32': ('tiny', lambda p: _first(p, 'warp', in3=False, img_out=False), {'huge'}, False),
    'clamp_last': ('tiny', lambda p: _first(p, 'warp', in3=False, img_out=False), {'normal', 'edges', 'huge'}, False),
    'alpha_unclamped': ('tiny', lambda p: _first(p, 'warp', in3=False, img_out=True), {'normal', 'edges', 'huge'}, True),
    'swap_flow': ('unfused', lambda p: _first(p, 'warp', in3=False), {'normal', 'edges', 'huge'}, True),
    'pool_before_activation': ('tiny', lambda p: next(i for i, op in enumerate(p['ops']) if op['kind'] == 'conv_mfma' and OH._has(op, 'out2')),
                               {'normal'}, True),
    'one_ulp_real': ('unfused', lambda p: _first(p, 'warp', in3=False), {'normal', 'edges', 'huge'}, True),
}


@pytest.mark.parametrize('name', list(REAL_PLANTED))
def test_a_fault_in_a_resampling_kernel_is_found_on_real_data(name, tiny_int, tiny_float, unfused_int, unfused_float):
    """Each fault is reported by the value check of the real-valued regime, at the op it is planted in and only there, by the input sets
    listed - and whether the small-integer set of the exact regime sees it is on record: a reordered pool sum and a lerp contracted to
    an fma have the same bits on dyadic data (the gap the real-valued regime closes), and so has a conversion before the clamp (no
    integer flow reaches 2^31) and a lower index on the last row (src[size - 1] against 1 * (b - a) + a: equal when that is exact)."""
    which, pick, want_sets, want_dense = REAL_PLANTED[name]
    fault = name.split('/')[0]
    (plan_i, packed_i), (plan_f, packed_f) = (tiny_int, tiny_float) if which == 'tiny' else (unfused_int, unfused_float)
    t = pick(plan_f)
    op = plan_f['ops'][t]
    assert OH.dedup_key(plan_i['ops'][t]) == OH.dedup_key(op)
    h = OH.Harness(Faulty(plan_f, packed_f, fault, t), plan_f, packed_f, False)
    fails = h.check_op(t)
    assert fails and all(f.check == 'value' and f.op == t and f.tag == op['tag'] for f in fails), '\n'.join(map(str, fails[:10]))
    assert {f.input_set.split('*')[0] for f in fails} == want_sets
    assert {f.view for f in fails} == ({'out2'} if fault == 'pool_before_activation' else {'out'})
    if fault == 'pool_before_activation':
        assert any('fused epilogue' in f.detail for f in fails)
    elif fault == 'one_ulp_real':
        assert all(f.coord == (0, 1, 1, 0) for f in fails)
    elif fault != 'floor_int32':      # a difference in bits names both errors against float64 (the `huge` set has no float64 side)
        assert any('e(got)' in f.detail and 'e(oracle)' in f.detail for f in fails)
    for other in (t - 1, t + 1):
        assert not h.check_op(other), other
    dense = OH.Harness(Faulty(plan_i, packed_i, fault, t), plan_i, packed_i, True).check_op(t)
    assert all(f.check == 'value' and f.op == t for f in dense)
    assert bool(dense) == want_dense, '\n'.join(map(str, dense[:10]))


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
