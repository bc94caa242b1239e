"""Test-only numpy interpreter of the engine's execution plan (film_plan_json).

The HIP engine plans a forward pass as a list of kernel launches over one workspace arena.  This
module executes that same op list on a numpy arena, giving every op the semantics its HIP kernel
implements (frame-interpolation_amd/csrc/*.hip).  It lets the CPU test-suite validate the planner
(buffer layout, concat-by-slices, batch remaps, upsample folding) and the weight packer
(channel permutation / zero padding) against the oracle WITHOUT a GPU.  It is test infrastructure:
nothing under frame-interpolation_amd/ imports it.
"""
from __future__ import annotations

import zlib

import numpy as np

from oracle import film_oracle as fo


_VERIFIED = set()


def _view(arena: np.ndarray, v: dict, nb: int, h: int, w: int) -> np.ndarray:
    s, e = v['stride'], arena.itemsize
    base = arena[v['off']:]
    need = ((nb * h * w - 1) * s + v['C'])
    assert need <= base.size, 'view exceeds arena'
    return np.lib.stride_tricks.as_strided(
        base, shape=(nb, h, w, v['C']), strides=(h * w * s * e, w * s * e, s * e, e), writeable=True)


def blob_key(packed: np.ndarray) -> int:
    """Key of the "weight copies verified" cache: the CONTENT of the blob (an id() can be recycled by a re-packed blob of the same size)."""
    return zlib.crc32(np.ascontiguousarray(packed).view(np.uint8))


def _leaky(y: np.ndarray) -> np.ndarray:
    """leaky-relu(0.2) as the kernels apply it: in float32, to the (rounded) pre-activation - also on a float64 arena, where the
    pre-activation of small-integer operands is exact and the result is then the float32 value the kernel must produce."""
    if y.dtype == np.float32:
        return fo.leaky_relu(y)
    return fo.leaky_relu(y.astype(np.float32)).astype(y.dtype)


def _conv(x, wt, bias, leaky, mag=False):
    """fo.conv2d_same in the dtype of x (float32 weights are widened for a float64 arena).  mag: the operand-magnitude companion -
    the same sum over |x|, |w|, |b| without the activation (the scale S of the rounding statistic, tests/op_harness.py)."""
    wt, bias = wt.astype(x.dtype), bias.astype(x.dtype)
    if mag:
        return fo.conv2d_same(np.abs(x), np.abs(wt), np.abs(bias), None)
    y = fo.conv2d_same(x, wt, bias, None)
    return _leaky(y) if leaky else y


def run_plan(plan: dict, packed: np.ndarray, x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    """Executes the plan; returns the arena (use `tap` to read named buffers)."""
    arena = np.zeros(plan['arena_floats'], dtype=np.float32)
    bufs = {b['name']: b for b in plan['buffers']}
    key = blob_key(packed)
    img0 = bufs['img0']
    n = x0.size
    arena[img0['off']:img0['off'] + n] = x0.ravel()
    arena[img0['off'] + n:img0['off'] + 2 * n] = x1.ravel()
    for op in plan['ops']:
        run_op(op, arena, packed, bufs, verify_key=key)
    return arena


def conv_input(op: dict, arena: np.ndarray) -> np.ndarray:
    """The concatenated [NB, H, W, Ctot] input of a plain (not C3, not folded) conv op: segments, batch remaps, nearest x2."""
    nb, h, w = op['NB'], op['H'], op['W']
    parts = []
    for sg in op['segs']:
        hs, ws = (h // 2, w // 2) if sg['up'] else (h, w)
        if sg['bmod']:
            src = _view(arena, sg['v'], sg['bmod'], hs, ws)
            idx = (np.arange(nb) + sg['boff']) % sg['bmod']
            src = src[idx]
        else:
            src = _view(arena, sg['v'], nb, hs, ws)
        if sg['up']:
            src = np.repeat(np.repeat(src, 2, axis=1), 2, axis=2)
        parts.append(src)
    return np.ascontiguousarray(np.concatenate(parts, axis=-1))


def run_op(op: dict, arena: np.ndarray, packed: np.ndarray, bufs: dict = None, verify_key=None, mag: bool = False) -> None:
    """Executes ONE op of a plan on `arena` (float32, or float64: the high-precision reference of the op on the same inputs; the packed
    weights stay the float32 values the kernels read).  verify_key (blob_key(packed)): also verify the layer's other weight copies, once
    per (blob, layer).  mag: the operand-magnitude companion of a conv-like op (see _conv); other kinds have none."""
    dt = arena.dtype.type
    A = (lambda a: np.abs(a)) if mag else (lambda a: a)
    blob_key = verify_key
    k = op['kind']
    nb, h, w = op['NB'], op['H'], op['W']
    if k == 'conv_mfma' and op.get('c3'):
        # first-layer mode: 3-channel image input, weights packed [12 tap slots][4][Cout]
        x = np.ascontiguousarray(_view(arena, op['segs'][0]['v'], nb, h, w))
        co = op['Cout']
        w48 = packed[op['w_off']:op['w_off'] + 48 * co].reshape(12, 4, co)
        assert not w48[9:].any() and not w48[:, 3].any(), 'padding rows of the C3 pack must be zero'
        wt = np.ascontiguousarray(w48[:9, :3]).reshape(3, 3, 3, co)
        bias = packed[op['b_off']:op['b_off'] + co]
        _view(arena, op['out'], nb, h, w)[...] = _conv(x, wt, bias, op['leaky'], mag)
    elif k == 'conv_mfma' and op.get('fold'):
        # nearest-x2 + 2x2 conv as four sub-pixel phases on the low-resolution grid (H, W); output 2H x 2W.
        # fold == 2: all phases in one op, phase q = py*2 + px, taps (a, b), a <= py, b <= px, raster order
        sg = op['segs'][0]
        assert op['fold'] in (2, 3) and len(op['segs']) == 1 and not sg['up'] and not sg['bmod'] and not op['leaky']
        x = np.ascontiguousarray(_view(arena, sg['v'], nb, h, w))
        ct, co = op['Ctot'], op['Cout']
        outv = _view(arena, op['out'], nb, 2 * h, 2 * w)
        if op['fold'] == 3:
            # conv_fold4_kernel: the difference form.  Weights [Cout/32][chunk8][plane 4][K half][32][4], planes S, Sx, Sy, W11;
            # G0 = S.I, G1 = Sx.Dx, G2 = Sy.Dy, G3 = W11.Dxy with Dx = I - I(x+1), Dy = I - I(y+1), Dxy = Dx - (I(y+1) - I(y+1,x+1))
            # (zero beyond the bottom / right edge); out = G0, G0 - G1, G0 - G2, ((G0 - G1) - G2) + G3 (+ bias)
            assert op['w_off'] == op['wf4_off'] and ct % 16 == 0 and co % 32 == 0
            w4 = packed[op['w_off']:op['w_off'] + 4 * ct * co].reshape(co // 32, ct // 8, 4, 2, 32, 4)
            w4 = A(w4.transpose(2, 1, 3, 5, 0, 4).reshape(4, ct, co).astype(dt))            # [plane][c = chunk*8 + half*4 + j][n = tile*32 + lane]
            sh = lambda a, b: np.pad(x[:, a:, b:], ((0, 0), (0, a), (0, b), (0, 0)))     # noqa: E731
            i00, i01, i10, i11 = x, sh(0, 1), sh(1, 0), sh(1, 1)
            dx = i00 - i01
            planes = [A(i00), A(dx), A(i00 - i10), A(dx - (i10 - i11))]
            g = [(pl.reshape(-1, ct) @ w4[q]).reshape(nb, h, w, co) for q, pl in enumerate(planes)]
            bias = A(packed[op['b_off']:op['b_off'] + co].astype(dt))
            if mag:     # every product of the difference form counts with its magnitude
                outv[:, 0::2, 0::2] = g[0] + bias
                outv[:, 0::2, 1::2] = (g[0] + g[1]) + bias
                outv[:, 1::2, 0::2] = (g[0] + g[2]) + bias
                outv[:, 1::2, 1::2] = (((g[0] + g[1]) + g[2]) + g[3]) + bias
                return
            outv[:, 0::2, 0::2] = g[0] + bias
            outv[:, 0::2, 1::2] = (g[0] - g[1]) + bias
            outv[:, 1::2, 0::2] = (g[0] - g[2]) + bias
            outv[:, 1::2, 1::2] = (((g[0] - g[1]) - g[2]) + g[3]) + bias
            return
        wfx = None
        # (a single op run without verification may see a blob whose layout group 4 is not packed: run_plan always checks the copy)
        if op.get('wfx_off', -1) >= 0 and (blob_key is not None or op['wfx_off'] + 9 * ct * co <= packed.size):
            # bf16x3 copy for conv_foldx3_kernel: [Cout][chunk16][9 (tap, phase) steps][plane][16] bf16
            raw = packed[op['wfx_off']:op['wfx_off'] + 9 * ct * co].view(np.uint16)
            wfx = (raw.astype(np.uint32) << 16).view(np.float32).reshape(co, ct // 16, 9, 2, 16).astype(np.float64).sum(axis=3)
            fold_step = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 1): 4, (1, 3): 5, (2, 2): 6, (2, 3): 7, (3, 3): 8}
        for q in range(4):
            py, px = q >> 1, q & 1
            taps = [(a, b) for a in range(py + 1) for b in range(px + 1)]
            off = op['w_off'] + op['fold_woff'][q]
            wt = packed[off:off + len(taps) * ct * co].reshape(co, len(taps), ct)
            acc = np.zeros((nb, h, w, co), dt)
            for t, (a, b) in enumerate(taps):
                if wfx is not None:
                    got = wfx[:, :, fold_step[(a * 2 + b, q)], :].reshape(co, ct)
                    want = wt[:, t].astype(np.float64)
                    assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -17), 'bf16x3 fold weight copy differs'
                sh = np.zeros_like(x)
                sh[:, :h - a, :w - b] = x[:, a:, b:]          # zero beyond the bottom / right edge
                acc += (A(sh).reshape(-1, ct) @ A(wt[:, t].T.astype(dt))).reshape(nb, h, w, co)
            acc += A(packed[op['b_off']:op['b_off'] + co].astype(dt))
            outv[:, py::2, px::2] = acc
    elif k == 'conv_mfma':
        x = conv_input(op, arena)
        ks, ct, co = op['ksize'], op['Ctot'], op['Cout']
        assert x.shape[-1] == ct
        # MFMA-conv layers are packed K-major: [Cout][tap][Ctot]
        wt = packed[op['w_off']:op['w_off'] + ks * ks * ct * co].reshape(co, ks, ks, ct)
        wt = np.ascontiguousarray(wt.transpose(1, 2, 3, 0))
        # the layer's other weight copies are verified once per (layout blob, layer): the shared sub-extractor / flow
        # predictor layers appear in many ops, and several plans are run over one blob
        vkey = (blob_key, packed.size, op['w_off'], op.get('wh_off', -1), op.get('ww_off', -1), op.get('w2d_off', -1), op.get('ws_off', -1), op.get('wx_off', -1))
        check = blob_key is not None and vkey not in _VERIFIED
        if blob_key is not None:
            _VERIFIED.add(vkey)
        if check and op.get('wh_off', -1) >= 0:
            # the layer's second copy for conv_halo_kernel, [Cout][chunk][tap][16], must hold the same weights
            wh = packed[op['wh_off']:op['wh_off'] + 9 * ct * co].reshape(co, ct // 16, 3, 3, 16)
            wh = wh.transpose(2, 3, 1, 4, 0).reshape(3, 3, ct, co)
            assert np.array_equal(wh, wt), 'halo weight copy differs'
            if op.get('halo') or op.get('split'):
                assert ks == 3 and not any(sg['up'] for sg in op['segs'])
        if check and op.get('ww_off', -1) >= 0:
            # Winograd copy [Cout][chunk of 8][nu*3+dy][8]: u0 = g0, u1 = ((g0+g2)+g1)/2, u2 = ((g0+g2)-g1)/2, u3 = g2
            ww = packed[op['ww_off']:op['ww_off'] + 12 * ct * co].reshape(co, ct // 8, 4, 3, 8)
            ww = ww.transpose(2, 3, 1, 4, 0).reshape(4, 3, ct, co)      # [nu][dy][c][n]
            g0, g1, g2 = wt[:, 0], wt[:, 1], wt[:, 2]                    # [dy][c][n]
            half = np.float32(0.5)
            want_u = np.stack([g0, ((g0 + g2) + g1) * half, ((g0 + g2) - g1) * half, g2])
            assert np.array_equal(ww, want_u), 'Winograd weight copy differs'
            if op.get('w43_off', -1) >= 0:
                # F(4,3) copy for conv_wino43_kernel: [Cout][chunk8][dy][nu 6][8], same float32 operation order as the packer
                w43 = packed[op['w43_off']:op['w43_off'] + 18 * ct * co].reshape(co, ct // 8, 3, 6, 8)
                w43 = w43.transpose(3, 2, 1, 4, 0).reshape(6, 3, ct, co)      # [nu][dy][c][n]
                f = np.float32
                c6, c12, c24 = f(1) / f(6), f(1) / f(12), f(1) / f(24)
                e, o = g0 * c24 + g2 * c6, g1 * c12
                want43 = np.stack([g0 * f(0.25), -((g0 + g2) + g1) * c6, -((g0 + g2) - g1) * c6, e + o, e - o, g2])
                assert np.array_equal(w43, want43), 'F(4,3) weight copy differs'
            if op.get('w2d_off', -1) >= 0:
                # nested copy for conv_wino2d_kernel: [Cout/32][chunk8][mu 4][nu 6][K half][32][4]; U = F(2,3) along dy of the
                # F(4,3)-transformed rows (want43[nu][dy]), same float32 operation order as the packer
                w2d = packed[op['w2d_off']:op['w2d_off'] + 24 * ct * co].reshape(co // 32, ct // 8, 4, 6, 2, 32, 4)
                w2d = w2d.transpose(2, 3, 1, 4, 6, 0, 5).reshape(4, 6, ct, co)      # [mu][nu][c = chunk*8 + half*4 + j][n = tile*32 + lane]
                u0, u1, u2 = want43[:, 0], want43[:, 1], want43[:, 2]               # [nu][c][n] per dy
                want2d = np.stack([u0, ((u0 + u2) + u1) * half, ((u0 + u2) - u1) * half, u2])
                assert np.array_equal(w2d, want2d), 'nested Winograd weight copy differs'
            if op.get('wx_off', -1) >= 0:
                # bf16x3 copy of the transformed weights: [Cout][chunk16][dy][j][h][plane][16] bf16, nu = 2h + j,
                # hi + mid within 2^-17 of the fp32 value (nearest split)
                n16 = 12 * ct * co * 2
                raw = packed[op['wx_off']:op['wx_off'] + n16 // 2].view(np.uint16)
                pl = (raw.astype(np.uint32) << 16).view(np.float32).reshape(co, ct // 16, 3, 2, 2, 2, 16)
                got_u = pl.astype(np.float64).sum(axis=5)                      # [n][chunk][dy][j][h][16]
                got_u = got_u.transpose(4, 3, 2, 1, 5, 0).reshape(2, 2, 3, ct, co)   # [h][j][dy][c][n]
                got_u = got_u.reshape(4, 3, ct, co)                            # nu = 2h + j
                assert np.all(np.abs(got_u - want_u) <= np.abs(want_u.astype(np.float64)) * 2.0 ** -17), 'bf16x3 Winograd weight copy differs'
        if check and op.get('ws_off', -1) >= 0:
            # bf16x6 copy: three bf16 planes [Cout][chunk][tap][plane][16] that add up to the weight EXACTLY
            n16 = 9 * ct * co * 3
            raw = packed[op['ws_off']:op['ws_off'] + (n16 + 1) // 2].view(np.uint16)[:n16]
            planes = (raw.astype(np.uint32) << 16).view(np.float32).reshape(co, ct // 16, 3, 3, 3, 16)
            ws = planes.astype(np.float64).sum(axis=4).transpose(2, 3, 1, 4, 0).reshape(3, 3, ct, co)
            assert np.array_equal(ws.astype(np.float32), wt) and np.array_equal(ws, wt.astype(np.float64)), 'bf16x6 split is not exact'
            # round-to-nearest pieces: the two planes bf16x3 uses are within 2^-17 of the weight
            two = planes.astype(np.float64)[:, :, :, :, :2].sum(axis=4).transpose(2, 3, 1, 4, 0).reshape(3, 3, ct, co)
            assert np.all(np.abs(two - wt) <= np.abs(wt.astype(np.float64)) * 2.0 ** -17), 'hi + mid is not a nearest split'
        bias = packed[op['b_off']:op['b_off'] + co]
        y = _conv(x, wt, bias, op['leaky'], mag)
        if op.get('pw_out', {}).get('buf'):     # fused 1x1 convolution (the RGB head): `out` is NOT written
            assert op.get('wino') in (3, 4) and co == 64 and op.get('ksplit', 1) <= 1 and not op.get('out2', {}).get('buf')
            c2 = op['pw_cout']
            w2 = packed[op['w2_off']:op['w2_off'] + co * c2].reshape(1, 1, co, c2)
            b2 = packed[op['b2_off']:op['b2_off'] + c2]
            _view(arena, op['pw_out'], nb, h, w)[...] = _conv(y, w2, b2, 0, mag)
            return
        _view(arena, op['out'], nb, h, w)[...] = y
        if op.get('out2', {}).get('buf'):       # fused AveragePooling2D(2, 2) of the output
            assert op.get('wino') in (3, 4) and h % 2 == 0 and w % 2 == 0
            _view(arena, op['out2'], nb, h // 2, w // 2)[...] = fo.avg_pool2x2(y)
    elif k == 'flow_head':
        m = op['n']
        x = np.ascontiguousarray(_view(arena, op['in'], 1, 1, m))
        ci = op['Ctot']
        w3 = packed[op['w_off']:op['w_off'] + ci * 16].reshape(1, 1, ci, 16)
        b3 = packed[op['b_off']:op['b_off'] + 16]
        w4 = packed[op['w2_off']:op['w2_off'] + 32].reshape(1, 1, 16, 2)
        b4 = packed[op['b2_off']:op['b2_off'] + 2]
        hid = _conv(x, w3, b3, 1, mag)
        _view(arena, op['out'], 1, 1, m)[...] = _conv(hid, w4, b4, 0, mag)
        if op.get('out2', {}).get('buf'):       # fused v = residual + upsampled flow
            _view(arena, op['out2'], 1, 1, m)[...] = _view(arena, op['out'], 1, 1, m) + A(_view(arena, op['in2'], 1, 1, m))
    elif k == 'conv_pw':
        m = op['n']
        x = np.ascontiguousarray(_view(arena, op['in'], 1, 1, m))
        ci, co = op['Ctot'], op['Cout']
        wt = packed[op['w_off']:op['w_off'] + ci * co].reshape(1, 1, ci, co)
        bias = packed[op['b_off']:op['b_off'] + co]
        _view(arena, op['out'], 1, 1, m)[...] = _conv(x, wt, bias, op['leaky'], mag)
        if op.get('out2', {}).get('buf'):       # flow head: fused v = residual + upsampled flow
            assert co == 2
            _view(arena, op['out2'], 1, 1, m)[...] = _view(arena, op['out'], 1, 1, m) + A(_view(arena, op['in2'], 1, 1, m))
    elif k == 'pool':
        x = np.ascontiguousarray(_view(arena, op['in'], nb, h, w))
        _view(arena, op['out'], nb, h // 2, w // 2)[...] = fo.avg_pool2x2(x)
    elif k == 'flow_up':
        x = np.ascontiguousarray(_view(arena, op['in'], nb, h, w))
        _view(arena, op['out'], nb, 2 * h, 2 * w)[...] = fo.resize_bilinear(np.float32(2) * x, (2 * h, 2 * w))
    elif k == 'flow_add':
        m = op['n'] // 2
        a = _view(arena, op['in'], 1, 1, m)
        b = _view(arena, op['in2'], 1, 1, m)
        _view(arena, op['out'], 1, 1, m)[...] = a + b
    elif k == 'warp':
        # one launch may carry both directions / both images of a level: the source (flow) batch of output batch n is
        # (n + src_brot) % nb ((n + flow_brot) % nb)
        src = np.roll(np.ascontiguousarray(_view(arena, op['in'], nb, h, w)), -op.get('src_brot', 0), axis=0)
        if op.get('in3', {}).get('buf'):        # fused tf.image.resize(2 * v) of the coarser level, stored to out2
            assert not op['in2']['buf'] and op['out2']['buf'] and not op.get('flow_brot', 0)
            coarse = np.ascontiguousarray(_view(arena, op['in3'], nb, h // 2, w // 2))
            flow = fo.resize_bilinear(np.float32(2) * coarse, (h, w))
            _view(arena, op['out2'], nb, h, w)[...] = flow
        else:
            flow = np.roll(np.ascontiguousarray(_view(arena, op['in2'], nb, h, w)), -op.get('flow_brot', 0), axis=0)
        _view(arena, op['out'], nb, h, w)[...] = fo.warp(src, np.float32(op['fscale']) * flow)
        if op.get('img_out', {}).get('buf'):    # fused sixteen miscellaneous channels of the aligned level
            mb = op.get('misc_nb', 0) or nb
            ims = np.ascontiguousarray(_view(arena, op['img_in'], 2 * mb, h, w))
            bf = np.ascontiguousarray(_view(arena, op['pack_b'], mb, h, w))
            ff = np.ascontiguousarray(_view(arena, op['pack_f'], mb, h, w))
            out = _view(arena, op['img_out'], mb, h, w)
            assert op['img_out']['C'] == 16 and op['fscale'] == 0.5
            out[..., 0:3] = fo.warp(ims[:mb], np.float32(0.5) * bf)    # image 0 <- backward flow
            out[..., 3:6] = fo.warp(ims[mb:], np.float32(0.5) * ff)    # image 1 <- forward flow
            out[..., 6:8] = bf * np.float32(0.5)
            out[..., 8:10] = ff * np.float32(0.5)
            out[..., 10:16] = 0
    elif k == 'pack_flow':
        m = op['n']
        bf = _view(arena, op['in'], 1, 1, m)
        ff = _view(arena, op['in2'], 1, 1, m)
        out = _view(arena, op['out'], 1, 1, m)
        out[..., 0:2] = bf * np.float32(0.5)
        out[..., 2:4] = ff * np.float32(0.5)
        out[..., 4:10] = 0
    else:
        raise ValueError(k)


# ----------------------------------------------------------------------------------------------
# float32 restatements of the kernels' accumulation structure (the yardstick of the rounding regime, tests/op_harness.py)
# ----------------------------------------------------------------------------------------------
MFMA_K = 2      # K step of v_mfma_f32_32x32x2_f32, the matrix instruction of every fp32 convolution kernel
# ... which adds its two products one after the other, each as a fused multiply-add rounded to float32: on an MI355X conv_buf_kernel
# and conv_pw_kernel return, bit for bit, what the chain acc = fma(x[k], w[k], acc) over k gives (K = 128 and 256, checked at the outputs
# of the first GPU run where a chunk-of-two restatement - both products exact, one rounding - was closer to the float64 sum than the
# kernel by more than 2 x).  The restatements therefore accumulate in chunks of ONE product (no longer than the K step).
ACC_STEP = 1

# the standard transforms of F(2,3) and F(4,3) (Lavin & Gray); the weight transforms G are what run_op verifies in the packed copies
_BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
_AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float32)
_BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]], np.float32)
_AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float32)


def chunked_sum_f32(X: np.ndarray, Wt: np.ndarray, kstep: int = ACC_STEP) -> np.ndarray:
    """acc[g, m, o] = sum_k X[g, m, k] * Wt[g, k, o] the way a matrix-core kernel accumulates it: float32, in K order, one chunk of
    `kstep` products (exact inside the chunk: float64) added per step and the sum rounded to float32 - kstep = 1 is the fma chain.
    <= K / kstep roundings per output."""
    import torch
    G, M, K = X.shape
    Co = Wt.shape[2]
    pad = -K % kstep
    if pad:
        X = np.concatenate([X, np.zeros((G, M, pad), X.dtype)], axis=2)
        Wt = np.concatenate([Wt, np.zeros((G, pad, Co), Wt.dtype)], axis=1)
    steps = (K + pad) // kstep
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).reshape(G, M, steps, kstep).permute(2, 0, 1, 3)     # [s, G, M, kstep]
    Wv = torch.from_numpy(np.ascontiguousarray(Wt, dtype=np.float32)).reshape(G, steps, kstep, Co).permute(1, 0, 2, 3)   # [s, G, kstep, Co]
    acc = torch.zeros((G, M, Co), dtype=torch.float32)
    slab = max(1, (1 << 23) // max(1, G * M * Co))
    for s0 in range(0, steps, slab):
        part = torch.matmul(Xt[s0:s0 + slab].double(), Wv[s0:s0 + slab].double())
        for i in range(part.shape[0]):
            acc = (acc.double() + part[i]).float()
    return acc.numpy()


def _fma(k: float, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float32 fma(k, a, b) for a small-integer k (the product is exact in float64, the sum is rounded once)."""
    return (np.float64(k) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def _f43_input(e: np.ndarray):
    """F(4,3) B^T along x of e [B, 6, C] as conv_wino2d_kernel forms it (xf_t / xf_v): six [B, C] planes."""
    d = [e[:, j] for j in range(6)]
    t0, t1, t2, t3 = _fma(-4, d[2], d[4]), _fma(-4, d[1], d[3]), d[4] - d[2], d[3] - d[1]
    return [_fma(4, d[0], _fma(-5, d[2], d[4])), t0 + t1, t0 - t1, _fma(2, t3, t2), _fma(-2, t3, t2), _fma(4, d[1], _fma(-5, d[3], d[5]))]


def _f43_output(m: np.ndarray):
    """F(4,3) A^T of the six planes m [6, B, C] as conv_wino2d_kernel's epilogue forms it: four [B, C] pixels."""
    s34, d34, d12, s12 = m[3] + m[4], m[3] - m[4], m[1] - m[2], m[1] + m[2]
    return [((m[0] + m[1]) + m[2]) + s34, _fma(2, d34, d12), _fma(4, s34, s12), d12 + _fma(8, d34, m[5])]


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), as a float32 (v_cvt_pk_bf16_f32)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(np.float32).reshape(x.shape)


def bf16_pieces(x: np.ndarray):
    """conv_split_impl.h: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); hi + mid + lo == x exactly."""
    hi = bf16_round(x)
    mid = bf16_round(x - hi)
    return hi, mid, bf16_round((x - hi) - mid)


def split_expand(X: np.ndarray, Wt: np.ndarray, nprod: int):
    """The bf16x6 / bf16x3 precision modes as conv_split_impl.h defines them: every operand in bf16 pieces, and per 16 K the products
    hi*hi, hi*mid, mid*hi (bf16x3) and hi*lo, lo*hi, mid*mid (bf16x6) - each exact in float32 - accumulated in float32.  Returns the
    operands of that longer sum, K' = nprod K, in the kernel's order [16-chunk][product][16]."""
    G, M, K = X.shape
    pad = -K % 16
    if pad:
        X = np.concatenate([X, np.zeros((G, M, pad), X.dtype)], axis=2)
        Wt = np.concatenate([Wt, np.zeros((G, pad, Wt.shape[2]), Wt.dtype)], axis=1)
    xp, wp = bf16_pieces(X), bf16_pieces(Wt)
    prods = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)][:nprod]
    nc = X.shape[2] // 16
    Xe = np.stack([xp[a].reshape(G, M, nc, 16) for a, _ in prods], axis=3).reshape(G, M, nc * nprod * 16)
    We = np.stack([wp[b].reshape(G, nc, 16, -1) for _, b in prods], axis=2).reshape(G, nc * nprod * 16, -1)
    return Xe, We


def _patches(x: np.ndarray, blocks: np.ndarray, ks: int) -> np.ndarray:
    """[B, 2 + ks - 1, 4 + ks - 1, C]: the zero-padded ('same') input window of each 2-row x 4-pixel output block (n, y0, x0)."""
    pt, pb = fo.same_padding(ks)
    xp = np.pad(x, ((0, 0), (pt, pb + 2), (pt, pb + 4), (0, 0)))
    n, y0, x0 = blocks[:, 0], blocks[:, 1], blocks[:, 2]
    yy = y0[:, None] + np.arange(2 + ks - 1)
    xx = x0[:, None] + np.arange(4 + ks - 1)
    return xp[n[:, None, None], yy[:, :, None], xx[:, None, :]]


def restate_f32(op: dict, arena: np.ndarray, packed: np.ndarray, blocks: np.ndarray, chans: np.ndarray):
    """The op in float32 with the kernel family's arithmetic structure, on a sample of its output: `blocks` [B, 3] = (n, y0, x0) of
    2-row x 4-pixel blocks of the op's H x W grid (y0 even, x0 % 4 == 0; pixels beyond the grid are dropped), `chans` the output
    channels.  Transformed weights come from the packed copy the kernel reads (verified by run_op), the input / output transforms are the standard ones in the
    operation order the kernel's header documents, channels are accumulated by chunked_sum_f32.  Returns {view name: ((n, y, x) index arrays, values [P, chans])},
    every family of the library has one (the bf16 split modes: split_expand)."""
    k = op['kind']
    nb, h, w = op['NB'], op['H'], op['W']
    f32 = np.float32
    B = len(blocks)
    if k in ('conv_pw', 'flow_head'):
        m = op['n']
        x = np.ascontiguousarray(_view(arena, op['in'], 1, 1, m))
        ci = op['Ctot']
        co = 16 if k == 'flow_head' else op['Cout']
        pat = _patches(x, blocks, 1).reshape(1, B * 8, ci)
        wt = packed[op['w_off']:op['w_off'] + ci * co].reshape(1, ci, co)
        y = chunked_sum_f32(pat, wt)[0] + packed[op['b_off']:op['b_off'] + co]
        if k == 'flow_head' or op['leaky']:
            y = fo.leaky_relu(y)
        if k == 'flow_head':
            y = chunked_sum_f32(y[None], packed[op['w2_off']:op['w2_off'] + 32].reshape(1, 16, 2))[0] + packed[op['b2_off']:op['b2_off'] + 2]
            chans = np.arange(2)
        else:
            y = y[:, chans]
        n_i = np.repeat(blocks[:, 0], 8)
        y_i = (blocks[:, 1, None, None] + np.arange(2)[None, :, None] + np.zeros((1, 1, 4), int)).reshape(-1)
        x_i = (blocks[:, 2, None, None] + np.arange(4)[None, None, :] + np.zeros((1, 2, 1), int)).reshape(-1)
        ok = (y_i < 1) & (x_i < m)
        idx = (n_i[ok], y_i[ok], x_i[ok])
        res = {'out': (idx, y[ok])}
        if op.get('out2', {}).get('buf'):
            add = np.ascontiguousarray(_view(arena, op['in2'], 1, 1, m))[idx]
            res['out2'] = (idx, y[ok] + add[:, chans] if k != 'flow_head' else y[ok] + add)
        return res
    assert k == 'conv_mfma'
    ct, co, ks = op['Ctot'], op['Cout'], op['ksize']
    bias = packed[op['b_off']:op['b_off'] + co]
    nprod = {1: 6, 2: 3}.get(op.get('split', 0) or (2 if op.get('wino') == 2 else 0), 0)      # bf16x6 / bf16x3: products per operand pair
    acc_sum = (lambda X, Wt: chunked_sum_f32(*split_expand(X, Wt, nprod))) if nprod else chunked_sum_f32
    if op.get('fold'):
        x = np.ascontiguousarray(_view(arena, op['segs'][0]['v'], nb, h, w))
        pat = _patches(x, blocks, 2)                                   # [B, 3, 5, ct]
        i00, i01, i10, i11 = pat[:, :2, :4], pat[:, :2, 1:5], pat[:, 1:3, :4], pat[:, 1:3, 1:5]
        y = np.zeros((B, 2, 4, 2, 2, len(chans)), f32)                  # [block][y][x][py][px][c]
        if op['fold'] == 3:
            w4 = packed[op['w_off']:op['w_off'] + 4 * ct * co].reshape(co // 32, ct // 8, 4, 2, 32, 4)
            w4 = w4.transpose(2, 1, 3, 5, 0, 4).reshape(4, ct, co)[:, :, chans]
            dx = i00 - i01
            planes = np.stack([i00, dx, i00 - i10, dx - (i10 - i11)]).reshape(4, B * 8, ct)
            g = chunked_sum_f32(planes, w4).reshape(4, B, 2, 4, len(chans))
            b = bias[chans]
            y[:, :, :, 0, 0] = g[0] + b
            y[:, :, :, 0, 1] = (g[0] - g[1]) + b
            y[:, :, :, 1, 0] = (g[0] - g[2]) + b
            y[:, :, :, 1, 1] = (((g[0] - g[1]) - g[2]) + g[3]) + b
        else:
            src = {(0, 0): i00, (0, 1): i01, (1, 0): i10, (1, 1): i11}
            for q in range(4):
                py, px = q >> 1, q & 1
                taps = [(a, b) for a in range(py + 1) for b in range(px + 1)]
                off = op['w_off'] + op['fold_woff'][q]
                wt = packed[off:off + len(taps) * ct * co].reshape(co, len(taps) * ct).T[None][:, :, chans]
                X = np.concatenate([src[t].reshape(B * 8, ct) for t in taps], axis=1)[None]
                y[:, :, :, py, px] = acc_sum(X, wt)[0].reshape(B, 2, 4, len(chans)) + bias[chans]
        n_i = np.broadcast_to(blocks[:, 0, None, None, None, None], y.shape[:5])
        ly = blocks[:, 1, None, None, None, None] + np.arange(2)[None, :, None, None, None]
        lx = blocks[:, 2, None, None, None, None] + np.arange(4)[None, None, :, None, None]
        y_i = np.broadcast_to(2 * ly + np.arange(2)[None, None, None, :, None], y.shape[:5])
        x_i = np.broadcast_to(2 * lx + np.arange(2)[None, None, None, None, :], y.shape[:5])
        ok = np.broadcast_to((ly < h) & (lx < w), y.shape[:5])
        return {'out': ((n_i[ok], y_i[ok], x_i[ok]), y[ok])}
    fused_pw = bool(op.get('pw_out', {}).get('buf'))
    yc = np.arange(co) if fused_pw else chans                           # (the fused 1x1 needs every channel of a pixel)
    if op.get('c3'):
        x = np.ascontiguousarray(_view(arena, op['segs'][0]['v'], nb, h, w))
        wt = np.ascontiguousarray(packed[op['w_off']:op['w_off'] + 48 * co].reshape(12, 4, co)[:9, :3]).reshape(3, 3, 3, co)
    else:
        x = conv_input(op, arena)
        wt = packed[op['w_off']:op['w_off'] + ks * ks * ct * co].reshape(co, ks, ks, ct).transpose(1, 2, 3, 0)
    pat = _patches(x, blocks, ks)
    wino = op.get('wino', 0)
    if wino == 4:       # conv_wino2d_kernel: F(4,3) along x nested in F(2,3) along y, one 4 x 6 input tile per 2 x 4 outputs
        w2d = packed[op['w2d_off']:op['w2d_off'] + 24 * ct * co].reshape(co // 32, ct // 8, 4, 6, 2, 32, 4)
        w2d = w2d.transpose(2, 3, 1, 4, 6, 0, 5).reshape(24, ct, co)[:, :, yc]
        # the operation order conv_wino2d_impl.h documents: y first on the raw rows, then x with fused multiply-adds (products by 2, 4, 5, 8
        # are exact in float64: one rounding per fma); the inverse along x per mu plane, then the two output rows
        d = [pat[:, r] for r in range(4)]
        E = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
        V = np.stack([np.stack(_f43_input(e), axis=1) for e in E], axis=1)      # [B, mu, nu, ct]
        M = chunked_sum_f32(np.ascontiguousarray(V.transpose(1, 2, 0, 3)).reshape(24, B, ct), w2d).reshape(4, 6, B, len(yc))
        P = [np.stack(_f43_output(M[mu]), axis=1) for mu in range(4)]           # per mu: [B, 4 (x), c]
        y = np.stack([(P[0] + P[1]) + P[2], (P[1] - P[2]) - P[3]], axis=1)
    elif wino == 3:     # conv_wino43_kernel: F(4,3) along x, the three kernel rows accumulated in the transform domain
        w43 = packed[op['w43_off']:op['w43_off'] + 18 * ct * co].reshape(co, ct // 8, 3, 6, 8)
        w43 = w43.transpose(3, 2, 1, 4, 0).reshape(6, 3 * ct, co)[:, :, yc]
        rows = np.stack([pat[:, r:r + 3] for r in range(2)], axis=1)      # [B, r, dy, 6, ct]
        # (the input and output forms conv_wino43_impl.h documents: products by 2, 4, 5, 8 are exact, one rounding per sum)
        V = np.stack(_f43_input(rows.reshape(B * 6, 6, ct))).reshape(6, B * 2, 3 * ct)
        M = chunked_sum_f32(V, w43)                                       # [nu, B * 2, c]
        y = np.stack(_f43_output(M), axis=1).reshape(B, 2, 4, len(yc))
    elif wino in (1, 2):     # conv_wino_kernel / conv_winox3_kernel (bf16x3 products): F(2,3) along x, two 1 x 2 tiles per block row
        ww = packed[op['ww_off']:op['ww_off'] + 12 * ct * co].reshape(co, ct // 8, 4, 3, 8)
        ww = ww.transpose(2, 3, 1, 4, 0).reshape(4, 3 * ct, co)[:, :, yc]
        tiles = np.stack([np.stack([pat[:, r:r + 3, 2 * t:2 * t + 4] for t in range(2)], axis=1) for r in range(2)], axis=1)   # [B, r, t, dy, 4, ct]
        V = np.einsum('nj,brtdjc->nbrtdc', _BT2, tiles).reshape(4, B * 4, 3 * ct)
        M = acc_sum(V, ww)
        y = np.einsum('qn,nmo->mqo', _AT2, M).reshape(B, 2, 4, len(yc))
    else:               # the direct sum, K-major [tap][channel]
        X = np.stack([pat[:, r:r + ks, q:q + ks].reshape(B, ks * ks * x.shape[-1]) for r in range(2) for q in range(4)], axis=1)
        y = acc_sum(X.reshape(1, B * 8, -1), wt.reshape(1, -1, co)[:, :, yc])[0].reshape(B, 2, 4, len(yc))
    y = (y + bias[yc]).astype(f32)
    if op['leaky']:
        y = fo.leaky_relu(y)
    n_i = np.broadcast_to(blocks[:, 0, None, None], (B, 2, 4))
    y_i = np.broadcast_to(blocks[:, 1, None, None] + np.arange(2)[None, :, None], (B, 2, 4))
    x_i = np.broadcast_to(blocks[:, 2, None, None] + np.arange(4)[None, None, :], (B, 2, 4))
    ok = (y_i < h) & (x_i < w)
    idx = (n_i[ok], y_i[ok], x_i[ok])
    if fused_pw:
        c2 = op['pw_cout']
        w2 = packed[op['w2_off']:op['w2_off'] + co * c2].reshape(1, co, c2)
        z = chunked_sum_f32(y.reshape(1, B * 8, co), w2)[0].reshape(B, 2, 4, c2) + packed[op['b2_off']:op['b2_off'] + c2]
        return {'pw_out': (idx, z[ok])}
    res = {'out': (idx, y[ok])}
    if op.get('out2', {}).get('buf'):       # fused AveragePooling2D(2, 2): the 2 x 2 windows inside the block
        s = ((y[:, 0, 0::2] + y[:, 0, 1::2]) + y[:, 1, 0::2]) + y[:, 1, 1::2]
        pn = np.broadcast_to(blocks[:, 0, None], (B, 2))
        py_ = np.broadcast_to(blocks[:, 1, None] // 2, (B, 2))
        px_ = blocks[:, 2, None] // 2 + np.arange(2)[None, :]
        okp = (2 * py_ + 1 < h) & (2 * px_ + 1 < w)
        res['out2'] = ((pn[okp], py_[okp], px_[okp]), (s * f32(0.25))[okp])
    return res


def tap(plan: dict, arena: np.ndarray, name: str) -> np.ndarray:
    b = next(x for x in plan['buffers'] if x['name'] == name)
    raw = arena[b['off']:b['off'] + b['floats']]
    if not b.get('planar'):
        return raw.reshape(b['N'], b['H'], b['W'], b['C']).copy()
    # three pixel-major planes (aligned-pyramid levels) -> [N, H, W, C], as film_get_tap returns them
    npix, parts, base = b['N'] * b['H'] * b['W'], [], 0
    for c in (b['planar'], b['planar'], b['C'] - 2 * b['planar']):
        parts.append(raw[base:base + npix * c].reshape(b['N'], b['H'], b['W'], c))
        base += npix * c
    return np.concatenate(parts, axis=-1)


# ----------------------------------------------------------------------------------------------
# Conversions between the engine's internal layouts and the reference's tensors
# ----------------------------------------------------------------------------------------------
def split_pair(x: np.ndarray, B: int):
    """[2B,...] batch (n = s*B + b) -> (first half, second half)."""
    return x[:B], x[B:]


def aligned_to_reference(a: np.ndarray, C: int) -> np.ndarray:
    """internal [feat0 C | feat1 C | img0 3 | img1 3 | bflow 2 | fflow 2 | 0x6] ->
    reference [img0 | feat0 | img1 | feat1 | bflow | fflow] (interpolator.py:167-183)."""
    f0, f1 = a[..., :C], a[..., C:2 * C]
    m = a[..., 2 * C:]
    return np.concatenate([m[..., 0:3], f0, m[..., 3:6], f1, m[..., 6:8], m[..., 8:10]], axis=-1)
