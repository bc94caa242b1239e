"""Test-only: runs ONE op of an execution plan on a workspace the test controls and checks what it wrote - and what it did not.

A backend is three functions over the plan's workspace: write(offset, float32 array), run(op index, candidate) -> number of tile
candidates of the op, read(offset, count).  GpuBackend drives the engine's debug entry points (film_debug_arena, film_debug_run_op);
NumpyBackend runs tests/plan_interp.run_op on a float32 numpy arena, so the harness itself (and the faults it must catch,
tests/test_op_harness_cpu.py) is tested without a GPU.

For one op, Harness.check_op
  1. fills the whole workspace with a background of finite pseudo-random floats of magnitude ~1e3 (no Inf / NaN: the kernels document
     that they rely on finite x 0),
  2. writes designed inputs into the op's input views only,
  3. runs the op with every tile candidate and reads back,
  4. ownership: every float outside the op's output views and its split-K scratch is bit-identical to what was uploaded (the whole
     workspace up to 64 MiB, else the input views and a >= 1 MiB band on each side of every output view),
  5. independence: with another background and the same inputs the output views are bit-identical,
  6. candidates: every candidate gives the bits of candidate 0,
  7. value: against plan_interp.run_op in float64 on the same inputs -
     exact regime (small-integer inputs, weights, biases; every partial sum is a float32 number): bit for bit, for the op kinds and
     kernel families in EXACT_FAMILIES;
     rounding regime (everything else, and the random-float input set): e = |got - ref64| / (2^-24 S), S = the same op over
     |x|, |w|, |b|.  The float32 restatement of the kernel's accumulation structure (plan_interp.restate_f32) is evaluated on a
     sample of the output (the points the input set was designed around, the corners, random blocks; a product-by-product float32 sum of
     the whole output of a deep layer costs minutes on the CPU): on THOSE points max e of the backend must not exceed 2 x max e of
     the restatement - the same op, the same inputs, the same outputs.  (A maximum over the whole output against a maximum over a
     sample does not compare like with like: e has a long tail, and every kernel family, torch's own CPU convolution included,
     exceeded 2 x by 10-60 % that way.)  Where the restatement is affordable over the whole output (FULL_COST) it covers it; beyond,
     the whole output is held to WHOLE_FACTOR = 4 x the restatement's maximum on the sample;
     real-valued regime of the resampling kinds (REAL_KINDS: pool, flow_up, flow_add, pack_flow, warp - in the pass that is not integer;
     the weights do not matter to them): every output view equals, value for value, plan_interp.run_op on a FLOAT32 arena - the
     oracle states these ops one numpy operation at a time in the array's dtype, so that is the kernels' documented arithmetic with
     one rounding per operation: the summation order of the pools, no fma in the lerps, the clamp in float before the conversion.
     Input sets (input_sets): `normal*s` (random sources, flows of a few pixels that are not dyadic, one in eight up to two frame
     sizes away), and for a warp `edges` (flows solved so that q lands on and next to every clamp: Q_CLASSES, _edge_flows) and `huge`
     (flows of 1e6 .. 3e38 and +-inf).  On the sets with finite flows the output and the float32 oracle are also both held to an
     a-priori bound against float64 (f64_bounds), and a difference in bits is reported with both errors: "rounded differently" against
     "wrong" at a glance,
  8. fused epilogues (the pass that is not integer): a conv op's fused pool is avg_pool2x2 of the `out` the same launch stored, a flow
     head's fused sum is `out` + in2, both in float32, bit for bit.

It does not poison the background with NaN, and the F(4,3)-based kernels (conv_wino43_kernel, conv_wino2d_kernel: their 1/6, 1/12,
1/24 weight transforms are rounded) and the bf16 split modes (restated with the split conv_split_impl.h defines) are held to
the rounding limit only.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Tuple

import numpy as np

import plan_interp as PI

ULP = 2.0 ** -24
WHOLE_ARENA_BYTES = 64 << 20
BAND_FLOATS = (1 << 20) // 4
EXACT_KINDS = ('conv_pw', 'flow_head', 'pool', 'flow_up', 'flow_add', 'pack_flow', 'warp')
EXACT_FAMILIES = ('BUF', 'C3', 'HALO', 'WINO', 'FOLD4', 'FOLD2')      # conv families held to bit-exactness on integer operands
REAL_KINDS = ('pool', 'flow_up', 'flow_add', 'pack_flow', 'warp')     # the resampling kinds: held to the float32 oracle's bits on real data
# The restatement costs a float64 multiply-add per product on the CPU: it covers the whole output of an op up to FULL_COST
# multiply-adds (most ops of the small plans), a sample of SAMPLE_COST beyond.
FULL_COST = 3e8
SAMPLE_COST = 1.5e8
# Beyond the sample the kernel is held to WHOLE_FACTOR x the restatement's maximum ON the sample: the issue's factor 2, and 2 for the
# growth of a maximum from the sample (>= 1e4 values) to the whole output (<= 1e7 values) - the error is a sum of many roundings, its
# maximum grows like sqrt(2 ln N): x 1.3 from 1e4 to 1e7 values; the transform kernels' e has a longer tail (it is a ratio to S).
# One dropped product of a dense K-term sum is 2^24 / K units (3e4 at K = 576) against limits of 10 .. 100.
WHOLE_FACTOR = 4.0
FACTOR = 2.0        # e_gpu <= FACTOR * e_ref: the kernel's order and fma contraction INSIDE a K step is all the restatement leaves out


def family(op: dict) -> str:
    """Kernel family of a conv op from the plan's family codes (film_internal.h, family_codes)."""
    if op['kind'] != 'conv_mfma':
        return op['kind']
    if op.get('c3'):
        return 'C3'
    if op.get('halo'):
        return 'HALO'
    if op.get('split') == 1:
        return 'SPLIT6'
    if op.get('split') == 2:
        return 'FOLDX3' if op.get('fold') else 'SPLIT3'
    if op.get('wino'):
        return {1: 'WINO', 2: 'WINOX3', 3: 'W43', 4: 'W2D'}[op['wino']]
    if op.get('fold') == 3:
        return 'FOLD4'
    if op.get('fold') == 2:
        return 'FOLD2'
    return 'BUF'


def _has(op, name):
    return bool(op.get(name, {}).get('buf'))


def in_views(op: dict) -> List[Tuple[str, dict, int, int, int]]:
    """(name, view, nb, h, w) of everything the op reads from the workspace."""
    k, nb, h, w = op['kind'], op['NB'], op['H'], op['W']
    if k == 'conv_mfma':
        out = []
        for i, sg in enumerate(op['segs']):
            hs, ws = (h // 2, w // 2) if sg['up'] else (h, w)
            out.append((f'seg{i}', sg['v'], sg['bmod'] or nb, hs, ws))
        return out
    if k in ('conv_pw', 'flow_head'):
        return [('in', op['in'], 1, 1, op['n'])] + ([('in2', op['in2'], 1, 1, op['n'])] if _has(op, 'out2') else [])
    if k in ('pool', 'flow_up'):
        return [('in', op['in'], nb, h, w)]
    if k == 'flow_add':
        return [('in', op['in'], 1, 1, op['n'] // 2), ('in2', op['in2'], 1, 1, op['n'] // 2)]
    if k == 'pack_flow':
        return [('in', op['in'], 1, 1, op['n']), ('in2', op['in2'], 1, 1, op['n'])]
    assert k == 'warp', k
    out = [('in', op['in'], nb, h, w)]
    out.append(('in3', op['in3'], nb, h // 2, w // 2) if _has(op, 'in3') else ('in2', op['in2'], nb, h, w))
    if _has(op, 'img_out'):
        mb = op.get('misc_nb', 0) or nb
        out += [('img_in', op['img_in'], 2 * mb, h, w), ('pack_b', op['pack_b'], mb, h, w), ('pack_f', op['pack_f'], mb, h, w)]
    return out


def out_views(op: dict) -> List[Tuple[str, dict, int, int, int]]:
    """(name, view, nb, h, w) of everything the op writes (a fused RGB head leaves `out` unwritten)."""
    k, nb, h, w = op['kind'], op['NB'], op['H'], op['W']
    if k == 'conv_mfma':
        if _has(op, 'pw_out'):
            return [('pw_out', op['pw_out'], nb, h, w)]
        f = 2 if op.get('fold') else 1
        return [('out', op['out'], nb, f * h, f * w)] + ([('out2', op['out2'], nb, h // 2, w // 2)] if _has(op, 'out2') else [])
    if k in ('conv_pw', 'flow_head', 'pack_flow'):
        return [('out', op['out'], 1, 1, op['n'])] + ([('out2', op['out2'], 1, 1, op['n'])] if _has(op, 'out2') else [])
    if k == 'pool':
        return [('out', op['out'], nb, h // 2, w // 2)]
    if k == 'flow_up':
        return [('out', op['out'], nb, 2 * h, 2 * w)]
    if k == 'flow_add':
        return [('out', op['out'], 1, 1, op['n'] // 2)]
    out = [('out', op['out'], nb, h, w)]
    if _has(op, 'in3'):
        out.append(('out2', op['out2'], nb, h, w))
    if _has(op, 'img_out'):
        out.append(('img_out', op['img_out'], op.get('misc_nb', 0) or nb, h, w))
    return out


def extent(v: dict, nb: int, h: int, w: int) -> Tuple[int, int]:
    return v['off'], v['off'] + (nb * h * w - 1) * v['stride'] + v['C']


def dedup_key(op: dict):
    """Ops of one plan that agree in all of this run the same kernel on the same geometry: tested once."""
    segs = tuple((sg['v']['C'], sg['v']['stride'], sg['up'], sg['bmod'], sg['boff']) for sg in op.get('segs', []))
    views = tuple((n, v['C'], v['stride']) for n, v, *_ in in_views(op) + out_views(op))
    return (op['kind'], family(op), op['NB'], op['H'], op['W'], op['Ctot'], op['Cout'], op['ksize'], segs, op.get('ksplit', 1), op.get('fold', 0),
            _has(op, 'out2'), _has(op, 'pw_out'), _has(op, 'img_out'), _has(op, 'in3'), op['leaky'], op.get('n', 0), views,
            op.get('src_brot', 0), op.get('flow_brot', 0), op.get('fscale', 0))


# ----------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------
def make_integer_weights(opt, seed: int = 0) -> Dict[str, np.ndarray]:
    """The names and shapes of make_synthetic_weights with EVEN kernels in {-2, 0, 2} (the F(2,3) weight transform halves sums of
    them, the difference form of the folded 2x2 adds them: all integers) and biases in -3 .. 3.  The 1x1 layer in front of every flow
    head holds multiples of 5 instead: its leaky-relu output 0.2f * 5 m rounds to the integer m (0.2f = 0.2 (1 + 2^-26): the product
    is m (1 + 2^-26), within half an ulp of m), so the second layer of the fused flow_head kernel sums integers too."""
    from film_hip import weights as W
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape, _ in W.weight_specs(opt):
        mul = 5 if (name.startswith('predict_flow') and shape[0] == 1 and shape[3] != 2) else 1
        out[name + '/kernel'] = (rng.integers(-1, 2, shape) * 2 * mul).astype(np.float32)
        out[name + '/bias'] = (rng.integers(-3, 4, (shape[3],)) * mul).astype(np.float32)
    return out


def assert_exact_regime(plan: dict, packed: np.ndarray) -> None:
    """|x| <= 3 and |w| <= 3 (15 in the flow-head layers) keep every partial sum of every layer an integer below 2^24, in every weight
    layout an exact-regime kernel reads: the copies hold integers only, and 9 Ctot 9 (the folded form: 4 Ctot 144) stays below 2^24."""
    for op in plan['ops']:
        if op['kind'] == 'conv_mfma' and family(op) in EXACT_FAMILIES:
            ct, co, ks = op['Ctot'], op['Cout'], op['ksize']
            assert 9 * ct * 9 < 2 ** 24 and 4 * ct * 144 < 2 ** 24, op['tag']
            fam = family(op)
            off, n = {'BUF': (op['w_off'], ks * ks * ct * co), 'FOLD2': (op['w_off'], 9 * ct * co), 'C3': (op['w_off'], 48 * co),
                      'HALO': (op['wh_off'], 9 * ct * co), 'WINO': (op['ww_off'], 12 * ct * co), 'FOLD4': (op['wf4_off'], 4 * ct * co)}[fam]
            wv = packed[off:off + n]
            assert off >= 0 and np.array_equal(wv, np.round(wv)) and np.abs(wv).max() <= 12, f'{op["tag"]}: the {fam} weight copy is not exact'
        elif op['kind'] in ('conv_pw', 'flow_head'):
            assert 15 * 3 * op['Ctot'] + 15 < 2 ** 24


# ----------------------------------------------------------------------------------------------
# designed inputs
# ----------------------------------------------------------------------------------------------
def _seam_points(op: dict) -> List[Tuple[int, int, int]]:
    """(n, y, x) on the op's input grid: the corners, the edge midpoints and both sides of every seam of every tile of the op's kernel
    family (x seams every 16 pixels cover the 16 / 32 / 64 / 128-pixel patches, y seams every 2 rows up to 16 the 2 / 4 / 8 / 16-row
    ones; conv_buf_kernel and conv_c3_kernel tile the flat pixel index by 64 / 128 / 256)."""
    nb, h, w = op['NB'], op['H'], op['W']
    pts = set()
    for n in {0, nb - 1}:
        for y in {0, h // 2, h - 1}:
            for x in {0, w // 2, w - 1}:
                pts.add((n, y, x))
    fam = family(op)
    if fam in ('BUF', 'C3', 'FOLD2'):
        m = nb * h * w
        for s in range(64, m, 64):
            for i in (s - 1, s):
                pts.add((i // (h * w), i // w % h, i % w))
    else:
        ys = [y for y in (2, 4, 8, 16) if y < h] + [y for y in range(16, h, 16)]
        for s in range(16, w, 16):
            for y in {0, h - 1, *[min(v, h - 1) for v in ys[:2]]}:
                pts.update({(0, y, s - 1), (nb - 1, y, s)})
        for t in ys:
            for x in {0, w - 1, min(16, w - 1)}:
                pts.update({(nb - 1, t - 1, x), (0, t, x)})
    return sorted(pts)[:4096]


def _boundary_channels(op: dict) -> List[int]:
    """First and last channel of every input segment, both sides of the 8- and 16-channel K chunks next to them, and both sides of
    every split-K range boundary (ranges are whole chunks: the multiples of 8 and 16 around j Ctot / ksplit)."""
    ct = op['Ctot']
    cs, c0 = set(), 0
    for sg in op['segs']:
        c = sg['v']['C']
        cs.update({c0, c0 + c - 1, c0 + min(7, c - 1), c0 + min(8, c - 1), c0 + min(15, c - 1), c0 + min(16, c - 1), c0 + max(c - 9, 0), c0 + max(c - 17, 0)})
        c0 += c
    ks = op.get('ksplit', 1)
    for j in range(1, ks):
        b = j * ct // ks
        for a in (b, b // 8 * 8, b // 16 * 16, -(-b // 8) * 8, -(-b // 16) * 16):
            cs.update({max(a - 1, 0), min(a, ct - 1)})
    return sorted(c for c in cs if 0 <= c < ct)


@dataclasses.dataclass
class InputSet:
    name: str
    exact: bool                       # small integers: every partial sum is a float32 number
    values: Dict[str, np.ndarray]     # input view name -> [nb, h, w, C] float32
    poi: List[Tuple[int, int, int]]   # (n, y, x) the set was designed around
    finite: bool = True               # no infinite flow: the float64 bound of the resampling kinds applies


# ----------------------------------------------------------------------------------------------
# the resampling kinds on real data: designed flows, and the a-priori bound against float64
# ----------------------------------------------------------------------------------------------
FLOW_VIEWS = ('in2', 'pack_b', 'pack_f')     # the flows a warp reads directly (in3 is the coarse flow behind the fused x2 resize)
HUGE_FLOWS = (1e6, 2.0 ** 31, 1e30, 3e38)
# q classes of one axis of a warp (warp_classes); `edges` puts at least one pixel into each, for every directly read flow
Q_CLASSES = ('floor(q) < 0', 'q an integer inside the frame', 'size-2 < q < size-1', 'q = size-1', 'q > size-1', 'alpha clamped to 0',
             'alpha clamped to 1', 'float32 q and exact q floor differently')
# ... and what the random flows of `normal*s` reach behind the fused resize, where the flow is derived and cannot be solved for: every
# class that is an interval of q.  An integer q, and a q within half an ulp below one, are points: a derived flow does not hit them.
Q_CLASSES_OF_A_DERIVED_FLOW = (0, 2, 4, 5, 6)


def _flow_scale(op: dict, name: str) -> float:
    return op['fscale'] if name in ('in2', 'in3') else 0.5


def _edge_variants(size: int, coord: np.ndarray, fscale: float) -> np.ndarray:
    """[variant, pixel] float32 flows of one axis: q = coord + fscale * flow aimed at every target (-1, 0, 0.5, 1, size - 2, size - 1, size, 2 size) and at its neighbours one
    and two ulps to either side, for both meanings of "one ulp": the float32 neighbours t of the target, flow = (t - coord) / fscale
    rounded once (they are the q next to the target that float32 can hold), and the float32 neighbours of the flow solved for the
    target itself (their exact q lies between two float32 numbers: float32 q is rounded back onto one of them, which is how it comes
    to floor differently from the exact q).  A neighbour of zero would be a denormal: those variants keep the flow of the target."""
    c = coord.astype(np.float64)
    out = []
    for base in (-1.0, 0.0, 0.5, 1.0, size - 2.0, size - 1.0, float(size), 2.0 * size):
        f0 = ((base - c) / fscale).astype(np.float32)
        out.append(f0)
        for k in (-2, -1, 1, 2):
            t = np.float32(base)
            for _ in range(abs(k)):
                t = np.nextafter(t, np.float32(np.inf if k > 0 else -np.inf))
            out.append(((np.float64(t) - c) / fscale).astype(np.float32) if base != 0 else f0)
            f = f0.copy()
            for _ in range(abs(k)):
                f = np.nextafter(f, np.float32(np.inf if k > 0 else -np.inf))
            out.append(np.where(f0 != 0, f, f0))
    return np.stack(out)


def _axis_classes(q32: np.ndarray, q64: np.ndarray, size: int) -> np.ndarray:
    """[..., len(Q_CLASSES)] bool: the classes of Q_CLASSES that float32 q (and, for the last, the exact q next to it) falls into."""
    fl = np.floor(q32)
    a = q32 - np.minimum(np.maximum(fl, 0), size - 2)       # alpha before its clamp
    return np.stack([fl < 0, (q32 == fl) & (q32 >= 0) & (q32 <= size - 1), (q32 > size - 2) & (q32 < size - 1), q32 == size - 1, q32 > size - 1,
                     a < 0, a > 1, fl != np.floor(q64)], axis=-1)


def _edge_flows(rng, nb: int, h: int, w: int, fscale: float) -> np.ndarray:
    """[nb, h, w, 2] float32 flow (x, y) whose q covers every class of Q_CLASSES on both axes (a level has at least 2 x 2 pixels and a
    launch at least one image), the variants of _edge_variants spread over rows, columns and images.  A few pixels are given
    the variant that puts a class on record that no pixel holds yet; every other pixel walks through the variant list."""
    n = nb * h * w
    ys, xs = np.divmod(np.arange(n) % (h * w), w)
    flow = np.zeros((n, 2), np.float32)
    for comp, (size, coord) in enumerate(((w, xs), (h, ys))):
        var = _edge_variants(size, coord, fscale)                   # [V, n]
        c = coord.astype(np.float32)
        with np.errstate(all='ignore'):
            q32 = c + np.float32(fscale) * var
            q64 = c.astype(np.float64) + np.float64(fscale) * var.astype(np.float64)
        cls = _axis_classes(q32, q64, size)                        # [V, n, classes]
        step = int(rng.integers(1, len(var)))
        pick = (np.arange(n) * 5 + step) % len(var)                 # (5 and the 72 variants are coprime)
        order = rng.permutation(n)
        held = np.zeros(len(Q_CLASSES), bool)
        fixed = 0
        while not held.all():
            assert fixed < n, 'more classes than pixels'
            i = order[fixed]
            gain = (cls[:, i] & ~held).sum(axis=1)
            if gain.any():
                pick[i] = int(np.argmax(gain))
            held |= cls[pick[i], i]
            fixed += 1
        # (the pixels behind `fixed` keep their walk: they can only add to what is held)
        flow[:, comp] = var[pick, np.arange(n)]
    return flow.reshape(nb, h, w, 2)


def warp_queries(op: dict, values: Dict[str, np.ndarray], dtype) -> List[Tuple[str, np.ndarray, np.ndarray]]:
    """(flow view, qy, qx) of every flow a warp op samples with, per flow pixel: the oracle's own query points (fo.warp_query of the
    oracle's own flow statements, plan_interp.run_op) in `dtype`."""
    fo = PI.fo
    nb, h, w = op['NB'], op['H'], op['W']
    out = []
    for name, v, nbv, hv, wv in in_views(op):
        if name == 'in3':
            flow = fo.resize_bilinear(np.float32(2) * values[name].astype(dtype), (h, w))
        elif name in FLOW_VIEWS:
            flow = values[name].astype(dtype)
        else:
            continue
        with np.errstate(all='ignore'):
            qy, qx = fo.warp_query(-(np.float32(_flow_scale(op, name)) * flow)[..., ::-1])
        out.append((name, qy, qx))
    return out


def warp_classes(op: dict, values: Dict[str, np.ndarray]) -> Dict[Tuple[str, str], np.ndarray]:
    """{(flow view, axis): number of pixels in each class of Q_CLASSES}, from the oracle's q in float32 and in float64."""
    out = {}
    for (name, qy, qx), (_, ry, rx) in zip(warp_queries(op, values, np.float32), warp_queries(op, values, np.float64)):
        out[(name, 'y')] = _axis_classes(qy, ry, op['H']).reshape(-1, len(Q_CLASSES)).sum(axis=0)
        out[(name, 'x')] = _axis_classes(qx, rx, op['W']).reshape(-1, len(Q_CLASSES)).sum(axis=0)
    return out


# One float32 operation rounds by at most U = 2^-24 of its result.  A lerp as the oracle states it - three operations, d = b - a,
# p = d t, r = a + p (or p + a), 0 <= t <= 1 exact - on operands of magnitude <= M that carry an error <= e: the exact lerp of the
# operands carries <= e (a convex combination); |d| <= 2 M' (M' = M + e) rounds by <= 2 U M'; |p| <= 2 M' (1 + U) by <= 2 U M' (1 + U);
# |a + p| <= M' (1 + 4 U + 2 U^2) by U times that: e' <= e + LERP U M', LERP = 5 + 6 U + 2 U^2.
LERP = 5 + 6 * ULP + 2 * ULP ** 2


def _lerp_bound(M, e=0.0):
    return e + LERP * ULP * (M + e)


def _flow_up_bound(x64: np.ndarray, size) -> np.ndarray:
    """flow_up / the fused resize: 2 x is exact and the lerp weights are the same float32 numbers in either precision, so the error is
    the roundings of the three lerps (top and bottom along x, then along y) on M = the largest magnitude of the four corners."""
    fo = PI.fo
    h, w = x64.shape[1:3]
    ylo, yhi, _ = fo._resize_axis_weights(h, size[0], np.float64)
    xlo, xhi, _ = fo._resize_axis_weights(w, size[1], np.float64)
    a = np.abs(2.0 * x64)
    M = np.maximum(np.maximum(a[:, ylo][:, :, xlo], a[:, ylo][:, :, xhi]), np.maximum(a[:, yhi][:, :, xlo], a[:, yhi][:, :, xhi]))
    return _lerp_bound(M, _lerp_bound(M))


def _warp_bound(src64: np.ndarray, qy: np.ndarray, qx: np.ndarray, dy, dx) -> np.ndarray:
    """A warp of src64 [nb, h, w, C] at the exact query points (qy, qx) [nb, h, w] that float32 knows to within (dy, dx): bilinear
    interpolation with clamped indices and weights is a continuous function of q, linear inside a cell with the corner differences
    as slopes, across cell borders and across both clamps - so float32 q moves the exact result by at most dx Dx + dy Dy, D = the
    largest difference of neighbouring corners over the cells q +- d touches (two per axis when q lies within d of a border: a
    different floor on the two sides is covered, not excluded).  Its weights are then exact functions of float32 q (q - floor(q) is
    exact, the clamps round monotonically), and the three lerps round as in _lerp_bound on M = the largest corner magnitude of those
    cells (a corner outside them has the weight 0: the lerp returns the other corner bit for bit)."""
    nb, h, w, _ = src64.shape
    b = np.arange(nb)[:, None, None]

    def cells(q, d, size):
        lo = np.clip(np.floor(q - d), 0, size - 2).astype(np.int64)
        hi = np.clip(np.floor(q + d), 0, size - 2).astype(np.int64)
        return lo, lo + 1, hi + 1
    rows, cols = cells(qy, dy, h), cells(qx, dx, w)
    v = [[src64[b, r, c] for c in cols] for r in rows]
    M = np.max([np.abs(v[i][j]) for i in range(3) for j in range(3)], axis=0)
    Dx = np.max([np.abs(v[i][j + 1] - v[i][j]) for i in range(3) for j in range(2)], axis=0)
    Dy = np.max([np.abs(v[i + 1][j] - v[i][j]) for i in range(2) for j in range(3)], axis=0)
    return dx[..., None] * Dx + dy[..., None] * Dy + _lerp_bound(M, _lerp_bound(M))


def f64_bounds(op: dict, values: Dict[str, np.ndarray], ref64: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """{output view: a-priori bound on |float32 result - float64 result|} of an op of the resampling kinds, elementwise, from one
    rounding of at most U = 2^-24 (relative) per float32 operation of the oracle's statements:
      flow_add    one addition: U |result|
      pack_flow   one multiplication (by 0.5: exact): U |result|; the zero channels: 0
      pool        three additions, each partial sum at most S = |a| + |b| + |c| + |d| (times (1 + U) per earlier rounding), then
                  the exact x 0.25: 0.25 S ((1 + U)^3 - 1)
      flow_up     _flow_up_bound
      warp        _warp_bound with d = U |q| (q = coord + fscale flow is one rounded addition: fscale is 1 or 0.5); behind the
                  fused resize the flow itself carries e = _flow_up_bound: d = fscale e (1 + U) + U |q|, and out2 is held to e"""
    k, nb, h, w = op['kind'], op['NB'], op['H'], op['W']
    v64 = {name: a.astype(np.float64) for name, a in values.items()}
    if k in ('flow_add', 'pack_flow'):
        return {'out': ULP * np.abs(ref64['out'])}
    if k == 'pool':
        a = np.abs(v64['in'][:, :h // 2 * 2, :w // 2 * 2])
        S = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
        return {'out': 0.25 * S * ((1 + ULP) ** 3 - 1)}
    if k == 'flow_up':
        return {'out': _flow_up_bound(v64['in'], (2 * h, 2 * w))}
    assert k == 'warp', k
    assert op['fscale'] in (1.0, 0.5), 'fscale flow is taken to be exact'
    out = {}
    q = {name: (qy, qx) for name, qy, qx in warp_queries(op, values, np.float64)}
    if 'in3' in q:
        e = _flow_up_bound(v64['in3'], (h, w))
        out['out2'] = e
        qy, qx = q['in3']
        s = op['fscale'] * (1 + ULP)
        dy, dx = s * e[..., 1] + ULP * np.abs(qy), s * e[..., 0] + ULP * np.abs(qx)
    else:
        qy, qx = (np.roll(a, -op.get('flow_brot', 0), axis=0) for a in q['in2'])
        dy, dx = ULP * np.abs(qy), ULP * np.abs(qx)
    out['out'] = _warp_bound(np.roll(v64['in'], -op.get('src_brot', 0), axis=0), qy, qx, dy, dx)
    if 'pack_b' in q:
        mb = values['pack_b'].shape[0]
        bound = np.zeros(ref64['img_out'].shape)
        for c0, name, ims in ((0, 'pack_b', v64['img_in'][:mb]), (3, 'pack_f', v64['img_in'][mb:])):
            qy, qx = q[name]
            bound[..., c0:c0 + 3] = _warp_bound(ims, qy, qx, ULP * np.abs(qy), ULP * np.abs(qx))
        bound[..., 6:10] = ULP * np.abs(ref64['img_out'][..., 6:10])
        out['img_out'] = bound
    return out


def _conv_concat_to_views(op: dict, x: np.ndarray) -> Dict[str, np.ndarray]:
    """Splits a designed [NB, H, W, Ctot] conv input into the op's segment views (batch remaps and nearest-x2 segments take what the
    FIRST output batch / the even pixels see: the rest of their designed values is dropped, the reference reads the views)."""
    out, c0 = {}, 0
    for i, (name, v, nbv, hs, ws) in enumerate(in_views(op)):
        sg = op['segs'][i]
        part = x[..., c0:c0 + v['C']]
        if sg['up']:
            part = part[:, ::2, ::2]
        if sg['bmod']:
            full = np.zeros((nbv, hs, ws, v['C']), np.float32)
            idx = (np.arange(op['NB']) + sg['boff']) % sg['bmod']
            full[idx] = part[:, :hs, :ws]
            part = full
        out[name] = np.ascontiguousarray(part[:, :hs, :ws], dtype=np.float32)
        c0 += v['C']
    return out


def input_sets(op: dict, seed: int, integer_weights: bool) -> List[InputSet]:
    rng = np.random.default_rng(seed)
    k, nb, h, w = op['kind'], op['NB'], op['H'], op['W']
    ivs = in_views(op)
    sets = []
    if not integer_weights:
        # rounding regime: random normal activations at the dynamic ranges of a trained net (1, 1e2, 1e3: tests/test_gpu_r3.py)
        scale = (1.0, 100.0, 1000.0)[seed % 3]
        vals = {name: (rng.standard_normal((nbv, hv, wv, v['C']), dtype=np.float32) * np.float32(scale)) for name, v, nbv, hv, wv in ivs}
        if k != 'warp':
            return [InputSet(f'normal*{scale:g}', False, vals, [])]
        # a warp's flows: a few pixels, not dyadic; about one pixel in eight up to two frame sizes away
        flows = [(name, nbv, hv, wv) for name, v, nbv, hv, wv in ivs if name in FLOW_VIEWS + ('in3',)]
        for name, nbv, hv, wv in flows:
            f = rng.standard_normal((nbv, hv, wv, 2), dtype=np.float32) * np.float32(3.0)
            far = rng.random((nbv, hv, wv)) < 0.125
            f[far] = (rng.uniform(-2, 2, (int(far.sum()), 2)) * (w, h)).astype(np.float32)
            vals[name] = f / np.float32(_flow_scale(op, name) * (2 if name == 'in3' else 1))
        sets.append(InputSet(f'normal*{scale:g}', False, dict(vals), []))
        if any(name in FLOW_VIEWS for name, *_ in flows):
            ev = dict(vals)
            for name, nbv, hv, wv in flows:
                if name in FLOW_VIEWS:
                    ev[name] = _edge_flows(rng, nbv, hv, wv, _flow_scale(op, name))
            sets.append(InputSet('edges', False, ev, []))
        # huge: +-1e6, 2^31, 1e30, 3e38 and, on the flows read directly, +-inf on every fifth flow component; the coarse flow of
        # the fused resize stops at 8e37 (flow_up_at doubles it and subtracts two such values: 3.2e38 is still finite)
        hv_ = dict(vals)
        for name, nbv, hv, wv in flows:
            mags = HUGE_FLOWS + (np.inf,) if name in FLOW_VIEWS else HUGE_FLOWS[:3] + (8e37,)
            lattice = np.array([s * m for m in mags for s in (1, -1)], np.float32)
            f = vals[name].copy().reshape(-1)
            j = np.arange(0, f.size, 5)
            f[j] = lattice[(j // 5) % len(lattice)]
            hv_[name] = f.reshape(vals[name].shape)
        sets.append(InputSet('huge', False, hv_, [], finite=False))
        # the flow a fused warp samples the features with IS one of the flows it packs (in2 and pack_b / pack_f share their buffer):
        # the values of a set are what the views hold once all of them are written, in the order check_op writes them
        lo, hi = min(extent(v, *s)[0] for _, v, *s in ivs), max(extent(v, *s)[1] for _, v, *s in ivs)
        tmp = np.zeros(hi - lo, np.float32)
        for iset in sets:
            for name, v, *s in ivs:
                PI._view(tmp, dict(v, off=v['off'] - lo), *s)[...] = iset.values[name]
            iset.values = {name: PI._view(tmp, dict(v, off=v['off'] - lo), *s).copy() for name, v, *s in ivs}
        return sets
    if k == 'conv_mfma':
        ct = op['Ctot']
        sets.append(InputSet('dense-int', True, _conv_concat_to_views(op, rng.integers(-3, 4, (nb, h, w, ct)).astype(np.float32)), []))
        x = np.zeros((nb, h, w, ct), np.float32)
        pts, chs = _seam_points(op), _boundary_channels(op)
        for i, (n, y, xx) in enumerate(pts):            # one impulse per point, walking through the boundary channels
            x[n, y, xx, chs[i % len(chs)]] = (1, -2, 3, -1, 2, -3)[i % 6]
        for i, c in enumerate(chs):                     # and every boundary channel at one interior and one corner pixel
            x[(i // 2) % nb, h // 2, w // 2, c] = 3 - (i % 3)
            x[nb - 1, h - 1, w - 1, c] += 1
        sets.append(InputSet('impulses', True, _conv_concat_to_views(op, x), pts))
        return sets
    vals = {name: rng.integers(-3, 4, (nbv, hv, wv, v['C'])).astype(np.float32) for name, v, nbv, hv, wv in ivs}
    if k == 'warp':
        # flows in quarter pixels (after fscale), up to well outside the frame; the bilinear weights are then multiples of 1/4 (of 1/32
        # behind the fused x2 upsample of a coarse flow in half pixels) and every product a short dyadic number
        q = np.float32(0.25 / (op['fscale'] or 1.0))
        for name, v, nbv, hv, wv in ivs:
            if name in ('in2', 'pack_b', 'pack_f'):
                f = rng.integers(-12, 13, (nbv, hv, wv, v['C']))
                f[:, ::5, ::7] = rng.integers(-4 * max(hv, wv) - 8, 4 * max(hv, wv) + 9, f[:, ::5, ::7].shape)
                f[:, 1::4, 1::4] = 4 * rng.integers(-3, 4, f[:, 1::4, 1::4].shape)      # integer-pixel flows
                vals[name] = f.astype(np.float32) * (np.float32(0.5) if name != 'in2' else q)
            elif name == 'in3':
                f = rng.integers(-6, 7, (nbv, hv, wv, v['C']))
                f[:, ::3, ::4] = rng.integers(-2 * max(hv, wv) - 4, 2 * max(hv, wv) + 5, f[:, ::3, ::4].shape)
                vals[name] = f.astype(np.float32) * np.float32(0.5)
    sets.append(InputSet('dense-int', True, vals, []))
    return sets


# ----------------------------------------------------------------------------------------------
# backends
# ----------------------------------------------------------------------------------------------
class NumpyBackend:
    """plan_interp.run_op on a float32 arena; conv ops pretend to have two (identical) tile candidates."""

    def __init__(self, plan: dict, packed: np.ndarray):
        self.plan, self.packed = plan, packed
        self.arena = np.zeros(plan['arena_floats'], np.float32)

    def write(self, off: int, data: np.ndarray) -> None:
        self.arena[off:off + data.size] = data

    def read(self, off: int, count: int) -> np.ndarray:
        return self.arena[off:off + count].copy()

    def run(self, index: int, candidate: int) -> int:
        op = self.plan['ops'][index]
        n = 2 if op['kind'] == 'conv_mfma' else 0
        assert -1 <= candidate < max(n, 1)
        PI.run_op(op, self.arena, self.packed)
        return n


class GpuBackend:
    """film_debug_arena / film_debug_run_op of an engine with a device; key = (B, H, W[, tiles])."""

    def __init__(self, engine, key):
        self.engine, self.key = engine, tuple(key)

    def write(self, off, data):
        self.engine.debug_arena_write(self.key, off, data)

    def read(self, off, count):
        return self.engine.debug_arena_read(self.key, off, count)

    def run(self, index, candidate):
        return self.engine.debug_run_op(self.key, index, candidate)


# ----------------------------------------------------------------------------------------------
# the checks
# ----------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Failure:
    check: str          # ownership | independence | candidates | value
    op: int
    tag: str
    input_set: str
    candidate: int
    where: str          # view / arena offset and coordinates
    detail: str = ''
    view: str = ''      # output view of a value / candidates / independence failure
    coord: tuple = ()   # (n, y, x, c) in that view; ownership: (arena offset,)

    def __str__(self):
        return f'op {self.op} ({self.tag}) [{self.input_set}, candidate {self.candidate}] {self.check}: {self.where} {self.detail}'


@dataclasses.dataclass
class Record:           # one line of the error table
    op: int
    tag: str
    family: str
    K: int
    input_set: str
    e_ref: float    # the restatement, on the sample
    e_got: float    # the backend, on the same sample
    e_full: float = 0.0     # the backend, on the whole output


@dataclasses.dataclass
class RealRecord:       # one op of the resampling kinds on one real-valued input set
    op: int
    tag: str
    kind: str
    input_set: str
    differ: int         # output values that are not the float32 oracle's
    size: int           # ... of so many
    has_f64: bool       # the set has finite flows: the float64 bound applies
    ratio: float = 0.0      # the backend: largest |got - float64| / bound ...
    e: float = 0.0          # ... |got - float64| there ...
    bound: float = 0.0      # ... and the bound there
    ratio_oracle: float = 0.0   # the float32 oracle: largest |oracle - float64| / bound


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tile_max(s: np.ndarray, th: int, tw: int) -> np.ndarray:
    """max of s [nb, h, w, c] over the aligned th x tw tiles of the grid, broadcast back."""
    nb, h, w, c = s.shape
    p = np.pad(s, ((0, 0), (0, -h % th), (0, -w % tw), (0, 0)))
    t = p.reshape(nb, p.shape[1] // th, th, p.shape[2] // tw, tw, c).max(axis=(2, 4), keepdims=True)
    return np.broadcast_to(t, (nb, p.shape[1] // th, th, p.shape[2] // tw, tw, c)).reshape(p.shape)[:, :h, :w]


# The outputs of one transform tile share their inputs and the nine taps of a channel pair share their transformed weights: a Winograd
# kernel's rounding error at an output is proportional to the operand magnitudes of the whole tile, not of that output's own nine
# products.  On the sparse integer sets (an impulse next to outputs whose own sum is empty, or under a tap whose weight is zero) the
# scale S of these families is therefore computed with every tap at the largest magnitude of the nine, and its maximum over the
# tile is taken: rows x pixels of one output tile.  Where even that is zero every product of the transform domain is zero.
TRANSFORM_TILE = {'W43': (1, 4), 'W2D': (2, 4), 'WINOX3': (1, 2)}


def _merge(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(a, b) for a, b in out]


class Harness:
    def __init__(self, backend, plan: dict, packed: np.ndarray, integer_weights: bool, seed: int = 0):
        self.be, self.plan, self.packed, self.int_w = backend, plan, packed, integer_weights
        self.n = plan['arena_floats']
        self.bufs = {b['name']: b for b in plan['buffers']}
        rng = np.random.default_rng(seed)
        # two backgrounds: finite, magnitude ~1e3, both signs
        self.bg = [(rng.standard_normal(self.n, dtype=np.float32) * np.float32(1e3)) for _ in range(2)]
        for b in self.bg:
            b[b == 0] = np.float32(1e3)
        self.arena64 = np.zeros(self.n, np.float64)
        self.arena32 = np.zeros(self.n, np.float32)     # the float32 oracle of the resampling kinds runs here
        self.real_records: List[RealRecord] = []
        self.cur = None                 # which background the backend holds
        self.records: List[Record] = []
        self.ran_candidates = {}        # op index -> number of candidates run
        self.n_candidates = {}          # op index -> number of candidates the backend reported
        self.seed = seed

    # -- helpers
    def _set_background(self, i: int) -> None:
        if self.cur != i:
            self.be.write(0, self.bg[i])
            self.cur = i

    def _scratch(self, op):
        b = self.bufs.get('splitk:' + op['tag']) if op.get('ksplit', 1) > 1 else None
        return [(b['off'], b['off'] + b['floats'])] if b else []

    def _checked_ranges(self, op, ivs, ovs):
        if self.n * 4 <= WHOLE_ARENA_BYTES:
            return [(0, self.n)]
        r = [extent(v, nb, h, w) for _, v, nb, h, w in ivs]
        for lo, hi in [extent(v, nb, h, w) for _, v, nb, h, w in ovs] + self._scratch(op):
            r.append((max(lo - BAND_FLOATS, 0), min(hi + BAND_FLOATS, self.n)))
        return _merge(r)

    def _locate(self, off: int, views) -> str:
        for name, v, nb, h, w in views:
            lo, hi = extent(v, nb, h, w)
            if lo <= off < hi:
                pix, c = divmod(off - v['off'], v['stride'])
                return f'arena[{off}] = {name} pixel (n {pix // (h * w)}, y {pix // w % h}, x {pix % w}), float {c} of its {v["stride"]}-float pitch (view: {v["C"]} channels)'
        b = next((b for b in self.plan['buffers'] if b['off'] <= off < b['off'] + b['floats']), None)
        return f'arena[{off}]' + (f' = buffer {b["name"]} + {off - b["off"]}' if b else ' (alignment gap)')

    def _reference(self, op, iset: InputSet, ivs, ovs, mag: bool, tap_max: bool = False, arena=None):
        """run_op in float64 (arena: in that arena's precision) on the designed inputs -> {output view name: array}.  mag: the magnitude
        companion.  tap_max (3x3 conv): ... with every tap's weight replaced by the largest magnitude among the nine taps of its
        (input, output) channel pair."""
        arena = self.arena64 if arena is None else arena
        for name, v, nb, h, w in ivs:
            PI._view(arena, v, nb, h, w)[...] = iset.values[name]
        if tap_max:
            ct, co = op['Ctot'], op['Cout']
            region = self.packed[op['w_off']:op['w_off'] + 9 * ct * co]
            saved = region.copy()
            wv = region.reshape(co, 9, ct)
            wv[...] = np.abs(wv).max(axis=1, keepdims=True)
        try:
            with np.errstate(all='ignore'):     # (the `huge` flows overflow on purpose)
                PI.run_op(op, arena, self.packed, mag=mag)
        finally:
            if tap_max:
                region[...] = saved
        return {name: PI._view(arena, v, nb, h, w).copy() for name, v, nb, h, w in ovs}

    def _sample(self, op, iset: InputSet, rng):
        """(blocks, channels) the restatement is evaluated at: the WHOLE output where that costs at most FULL_COST multiply-adds,
        else the corners, the designed points (spread evenly over the list: every image, row and seam kind) and random blocks."""
        nb, h, w = op['NB'], op['H'], op['W']
        if op['kind'] != 'conv_mfma':
            nb, h, w = 1, 1, op['n']
        co, fam = op['Cout'], family(op)
        nblocks = nb * ((h + 1) // 2) * ((w + 3) // 4)
        per_px = op['ksize'] ** 2 * op['Ctot'] * {'W2D': 3, 'W43': 4.5, 'SPLIT6': 6, 'SPLIT3': 3, 'FOLDX3': 3, 'WINOX3': 4.5}.get(fam, 1 if not op.get('fold') else 4)
        if nblocks * 8 * per_px * co <= FULL_COST:
            blk = {(n, y, x) for n in range(nb) for y in range(0, h, 2) for x in range(0, w, 4)}
            return np.array(sorted(blk), dtype=np.int64), np.arange(co)
        chans = np.arange(co) if co <= 128 else np.unique(np.concatenate([np.arange(0, co, co // 96), [co - 1]]))
        budget = int(np.clip(SAMPLE_COST // (8 * per_px * len(chans)), 16, 512))
        blk = {(n, y // 2 * 2, x // 4 * 4) for n in {0, nb - 1} for y in {0, h - 1} for x in {0, w - 1}}
        poi = iset.poi[::max(1, len(iset.poi) // max(budget // 2, 1))]
        for n, y, x in poi:
            blk.add((n, y // 2 * 2, x // 4 * 4))
        while len(blk) < budget + 8 and len(blk) < nblocks:
            blk.add((int(rng.integers(nb)), int(rng.integers((h + 1) // 2)) * 2, int(rng.integers((w + 3) // 4)) * 4))
        return np.array(sorted(blk), dtype=np.int64), chans

    # -- one op
    def _first_bad(self, bad):
        return tuple(int(t[0]) for t in np.nonzero(bad))

    def _check_real(self, index, op, iset, cand, got, ref32, ref64, bounds, fails) -> None:
        """The resampling kinds on real data.  Bits: every output view equals the float32 oracle (run_op on a float32 arena: the
        kernels' documented arithmetic, one rounding per operation), compared by value (+0 == -0; a NaN differs).  Float64 (input
        sets with finite flows): |got - ref64| and |oracle - ref64| both within f64_bounds."""
        differ = size = 0
        worst = (0.0, 0.0, 0.0, 0.0)      # (e / bound, e, bound) of the backend where that ratio is largest, and the oracle's ratio
        for name, g in got.items():
            r32, r64 = ref32[name], ref64[name]
            bad = ~(g == r32)
            differ, size = differ + int(bad.sum()), size + bad.size
            where = lambda i: f'{name}[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]'      # noqa: E731
            e_got = e_orc = None
            if bounds is not None:
                b = bounds[name]
                e_got, e_orc = np.abs(g.astype(np.float64) - r64), np.abs(r32.astype(np.float64) - r64)
                e_got[np.isnan(e_got)] = np.inf
                for who, e in (('got', e_got), ('the float32 oracle', e_orc)):
                    over = ~(e <= b)
                    if over.any():
                        i = self._first_bad(over)
                        fails.append(Failure('value', index, op['tag'], iset.name, cand, where(i), view=name, coord=i, detail=
                                             f'{who}: |{(g if who == "got" else r32)[i]!r} - float64 {r64[i]!r}| = {e[i]:.4g} > the a-priori bound {b[i]:.4g} '
                                             f'({int(over.sum())} of {over.size} exceed it)'))
                ratio = np.where(b > 0, e_got / np.where(b > 0, b, 1), np.where(e_got > 0, np.inf, 0))
                j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
                orc = float(np.where(b > 0, e_orc / np.where(b > 0, b, 1), np.where(e_orc > 0, np.inf, 0)).max())
                if ratio[j] >= worst[0]:
                    worst = (float(ratio[j]), float(e_got[j]), float(b[j]), max(worst[3], orc))
                else:
                    worst = worst[:3] + (max(worst[3], orc),)
            if bad.any():
                i = self._first_bad(bad)
                against = (f'; against float64 {r64[i]!r}: e(got) = {e_got[i]:.4g}, e(oracle) = {e_orc[i]:.4g}, bound {bounds[name][i]:.4g}'
                           if bounds is not None else '')
                fails.append(Failure('value', index, op['tag'], iset.name, cand, where(i), view=name, coord=i, detail=
                                     f'got {g[i]!r}, the float32 oracle {r32[i]!r} ({int(bad.sum())} of {bad.size} differ){against}'))
        self.real_records.append(RealRecord(index, op['tag'], op['kind'], iset.name, differ, size, bounds is not None, *worst))

    def _run_and_read(self, index, cand, up, touched, ranges, owned, ivs, ovs, iset, fails, check_ownership):
        op = self.plan['ops'][index]
        for lo, hi in touched:
            self.be.write(lo, up[lo:hi])
        ncand = self.be.run(index, cand)
        got = {}
        for lo, hi in (ranges if check_ownership else []):
            back = self.be.read(lo, hi - lo)
            bad = (_bits(back) != _bits(up[lo:hi])) & ~owned[lo:hi]
            if bad.any():       # ownership: everything outside the output views and the split-K scratch, bit for bit
                off = lo + int(np.flatnonzero(bad)[0])
                fails.append(Failure('ownership', index, op['tag'], iset.name, cand, self._locate(off, ivs + ovs), coord=(off,), detail=
                                     f'uploaded {up[off]!r}, read back {back[off - lo]!r} ({int(bad.sum())} floats changed)'))
            for name, v, nb, h, w in ovs:
                vlo, vhi = extent(v, nb, h, w)
                if lo <= vlo and vhi <= hi:
                    got[name] = PI._view(back, dict(v, off=vlo - lo), nb, h, w).copy()
        for name, v, nb, h, w in ovs:
            if name not in got:
                vlo, vhi = extent(v, nb, h, w)
                got[name] = PI._view(self.be.read(vlo, vhi - vlo), dict(v, off=0), nb, h, w).copy()
        return ncand, got

    def check_op(self, index: int, candidates=None) -> List[Failure]:
        """Runs the op on every input set with every candidate (or those listed); returns what failed (empty: all checks hold)."""
        op = self.plan['ops'][index]
        ivs, ovs = in_views(op), out_views(op)
        fam = family(op)
        is_conv = op['kind'] == 'conv_mfma'
        conv_like = op['kind'] in ('conv_mfma', 'conv_pw', 'flow_head')
        exact_op = op['kind'] in EXACT_KINDS or fam in EXACT_FAMILIES
        fails: List[Failure] = []
        rng = np.random.default_rng(self.seed * 7919 + index)
        primary = self.cur or 0
        owned = np.zeros(self.n, bool)
        for _, v, nb, h, w in ovs:
            PI._view(owned, v, nb, h, w)[...] = True
        for lo, hi in self._scratch(op):
            owned[lo:hi] = True
        ranges = self._checked_ranges(op, ivs, ovs)
        touched = _merge([extent(v, nb, h, w) for _, v, nb, h, w in ivs + ovs] + self._scratch(op))
        self._set_background(primary)
        keep = []
        for si, iset in enumerate(input_sets(op, self.seed + index, self.int_w)):
            up = self.bg[primary]
            saved = [up[lo:hi].copy() for lo, hi in touched]
            for name, v, nb, h, w in ivs:
                PI._view(up, v, nb, h, w)[...] = iset.values[name]
            ref = self._reference(op, iset, ivs, ovs, mag=False)
            exact = iset.exact and exact_op
            real = not iset.exact and op['kind'] in REAL_KINDS
            limit = S = rs = ref32 = bounds = None
            if real:
                ref32 = self._reference(op, iset, ivs, ovs, mag=False, arena=self.arena32)
                bounds = f64_bounds(op, iset.values, ref) if iset.finite else None
            elif not exact:
                sparse = iset.exact and fam in TRANSFORM_TILE
                S = self._reference(op, iset, ivs, ovs, mag=True, tap_max=sparse)
                if sparse:
                    th, tw = TRANSFORM_TILE[fam]
                    S = {name: _tile_max(a, *((th, tw) if name != 'out2' else (max(th // 2, 1), tw // 2))) for name, a in S.items()}
                blocks, chans = self._sample(op, iset, rng)
                rs = PI.restate_f32(op, up, self.packed, blocks, chans)      # (reads the input views only)
                assert rs is not None, f'{fam}: no restatement'
                if True:
                    limit = 0.0
                    for name, (idx, vals) in rs.items():
                        cs = np.arange(vals.shape[1]) if vals.shape[1] == ref[name].shape[-1] else chans
                        r, s = ref[name][idx][:, cs], S[name][idx][:, cs]
                        d = np.abs(vals.astype(np.float64) - r)
                        assert not (d[s == 0] != 0).any(), 'the restatement differs where every operand is zero'
                        limit = max(limit, float((d[s > 0] / (ULP * s[s > 0])).max(initial=0.0)))
                    assert np.isfinite(limit)
            first, k, per_cand = None, 0, []
            while True:
                cand = (candidates[k] if candidates is not None else k) if is_conv else -1
                ncand, got = self._run_and_read(index, cand, up, touched, ranges, owned, ivs, ovs, iset, fails, True)
                per_cand.append(got)
                if not self.int_w and conv_like and 'out2' in got:
                    # the fused epilogue against its unfused op, on what THIS launch wrote: ConvParams::pool_out's stated order
                    # (pool_vec_kernel's), and the flow head's v = residual + upsampled flow - one float32 operation per statement
                    want = PI.fo.avg_pool2x2(got['out']) if is_conv else got['out'] + iset.values['in2']
                    bad = ~(got['out2'] == want)
                    if bad.any():
                        i = self._first_bad(bad)
                        what = 'avg_pool2x2(out)' if is_conv else 'out + in2'
                        fails.append(Failure('value', index, op['tag'], iset.name, cand, f'out2[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]', view='out2', coord=i, detail=
                                             f'fused epilogue: got {got["out2"][i]!r}, {what} of the same launch in float32 {want[i]!r} ({int(bad.sum())} of {bad.size} differ)'))
                if first is None:
                    first = got
                    e_got = e_full = 0.0
                    if real:
                        self._check_real(index, op, iset, cand, got, ref32, ref, bounds, fails)
                    for name, g in ([] if real else got.items()):
                        r = ref[name]
                        if exact:
                            bad = g.astype(np.float64) != r             # (+0 == -0; a NaN differs)
                            if bad.any():
                                i = self._first_bad(bad)
                                fails.append(Failure('value', index, op['tag'], iset.name, cand, f'{name}[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]', view=name, coord=i, detail=
                                                     f'got {g[i]!r}, exact {r[i]!r} ({int(bad.sum())} of {bad.size} differ)'))
                            continue
                        d = np.abs(g.astype(np.float64) - r)
                        d[np.isnan(d)] = np.inf
                        s = S[name]
                        e = np.where(s > 0, d / (ULP * np.where(s > 0, s, 1)), np.where(d > 0, np.inf, 0))
                        # the whole output against WHOLE_FACTOR x the restatement's error on its sample ...
                        bound = WHOLE_FACTOR * limit
                        full = float(e.max())
                        e_full = max(e_full, full)
                        if not (full <= bound):
                            i = tuple(int(t) for t in np.unravel_index(int(np.argmax(e)), e.shape))
                            fails.append(Failure('value', index, op['tag'], iset.name, cand, f'{name}[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]', view=name, coord=i, detail=
                                                 f'e = {full:.2f} > {WHOLE_FACTOR:g} x e_ref {limit:.2f} (whole output): got {g[i]!r}, float64 {r[i]!r}, S {s[i]:.4g}'))
                        # ... and, on the points the restatement was evaluated at, against the restatement's own error
                        if rs is not None and name in rs:
                            idx, vals = rs[name]
                            cs = np.arange(vals.shape[1]) if vals.shape[1] == r.shape[-1] else chans
                            es = e[idx][:, cs]
                            ratio = float(es.max(initial=0.0))
                            e_got = max(e_got, ratio)
                            if not (ratio <= FACTOR * limit):
                                j = np.unravel_index(int(np.argmax(es)), es.shape)
                                i = (int(idx[0][j[0]]), int(idx[1][j[0]]), int(idx[2][j[0]]), int(cs[j[1]]))
                                fails.append(Failure('value', index, op['tag'], iset.name, cand, f'{name}[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]', view=name, coord=i, detail=
                                                     f'e = {ratio:.2f} > {FACTOR:g} x e_ref {limit:.2f}: got {g[i]!r}, float64 {r[i]!r}, S {s[i]:.4g}'))
                    if not exact and not real:
                        self.records.append(Record(index, op['tag'], fam, op['ksize'] ** 2 * op['Ctot'], iset.name,
                                                   float('nan') if limit is None else limit, e_got, e_full))
                else:               # candidates: the bits of the first one
                    for name, g in got.items():
                        bad = _bits(g) != _bits(first[name])
                        if bad.any():
                            i = self._first_bad(bad)
                            fails.append(Failure('candidates', index, op['tag'], iset.name, cand, f'{name}[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]', view=name, coord=i, detail=
                                                 f'{g[i]!r} != {first[name][i]!r} of the first candidate ({int(bad.sum())} differ)'))
                k += 1
                if not is_conv or k >= (len(candidates) if candidates is not None else ncand):
                    break
            self.ran_candidates[index] = max(self.ran_candidates.get(index, 0), k)
            self.n_candidates[index] = ncand
            keep.append((iset, per_cand, k))
            for (lo, hi), sv in zip(touched, saved):    # the background as it was, here and in the backend
                up[lo:hi] = sv
                self.be.write(lo, sv)
        # independence: the other background, the same inputs (every input set, every candidate): the same bits, and the same ownership
        other = 1 - primary
        self._set_background(other)
        up = self.bg[other]
        for iset, per_cand, k in keep:
            saved = [up[lo:hi].copy() for lo, hi in touched]
            for name, v, nb, h, w in ivs:
                PI._view(up, v, nb, h, w)[...] = iset.values[name]
            for kk in range(k):
                cand = (candidates[kk] if candidates is not None else kk) if is_conv else -1
                _, got = self._run_and_read(index, cand, up, touched, ranges, owned, ivs, ovs, iset, fails, True)
                for name, g in got.items():
                    first = per_cand[kk]
                    bad = _bits(g) != _bits(first[name])
                    if bad.any():
                        i = self._first_bad(bad)
                        fails.append(Failure('independence', index, op['tag'], iset.name, cand, f'{name}[n {i[0]}, y {i[1]}, x {i[2]}, c {i[3]}]', view=name, coord=i, detail=
                                             f'{g[i]!r} with the second background, {first[name][i]!r} with the first ({int(bad.sum())} differ)'))
            for (lo, hi), sv in zip(touched, saved):
                up[lo:hi] = sv
                self.be.write(lo, sv)
        return fails

    def distinct_ops(self) -> List[int]:
        seen, out = set(), []
        for i, op in enumerate(self.plan['ops']):
            key = dedup_key(op)
            if key not in seen:
                seen.add(key)
                out.append(i)
        return out
