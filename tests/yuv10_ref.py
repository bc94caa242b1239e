"""Numpy restatement of the 10-bit Y'CbCr 4:2:0 arithmetic of include/film_hip.h ("The 10-bit 4:2:0 arithmetic"): the code of a stored
word, the conversion in (words -> float32 RGB, what frame_yuv10_to_tiles_kernel of csrc/frame_kernels.hip fuses into the tile cut), the
conversion out (float32 RGB -> words, rgb_to_yuv10_kernel there), I010 <-> P010, the cut of a 10-bit frame batch into tiles over the
geometry film_tiling_json reports, and the histogram of a 10-bit frame.  The matrix constants, the cases and the tile ranges are
tests/yuv_ref.py's, the tile bookkeeping tests/tile_map_ref.py's.  Every operation is float32 with one rounding (numpy does not fuse), so
every comparison against the kernels is on the bits.

A frame is a uint16 array [H * 3 // 2, W] of stored words: rows [0, H) are the Y plane; the H * W / 2 words behind it are Cb [H/2][W/2]
then Cr [H/2][W/2] (I010) or CbCr [H/2][W/2][2] (P010).  I010 keeps the 10-bit code in bits 0-9 of a word, P010 in bits 6-15; the other six
bits are ignored on the way in and written as zero on the way out.

A "backend" of check_cut is a callable
    backend(frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full) -> (frames_alloc', tiles_alloc')
on the two whole allocations (guard | payload | guard; the frames' a uint16 array); the GPU test's calls film_debug_yuv_cut, NumpyBackend
applies the restatement, optionally with one of FAULTS planted.
"""
import numpy as np

import tile_map_ref as T
from yuv_ref import CASES, COLOURS, constants, ranges_of      # noqa: F401  (the cases and ranges of the 8-bit cut test, re-exported)

LAYOUTS = ('i010', 'p010')
F = np.float32
GUARD_U16 = T.GUARD_U8 // 2       # words of guard band on each side of a 10-bit frame batch (the payload stays 4-byte aligned)


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def code(words, layout):
    """The 10-bit code of every stored word."""
    w = np.asarray(words).astype(np.uint32) & 0xffff
    return (w >> 6) if layout == 'p010' else (w & 1023)


def store(codes, layout):
    """The word a code is stored as: the ignored bits are zero."""
    c = np.asarray(codes).astype(np.uint16)
    assert int(c.max(initial=0)) <= 1023
    return (c << 6).astype(np.uint16) if layout == 'p010' else c


def with_junk(frame, layout, seed):
    """The same codes with random bits where the layout ignores them."""
    j = np.random.default_rng(seed).integers(0, 64, frame.shape).astype(np.uint16)
    return (store(code(frame, layout), layout) | (j if layout == 'p010' else (j << 10))).astype(np.uint16)


def tables(full):
    """(y[1024], c[1024]): the luma and chroma value of every code, IEEE float32 division."""
    v = np.arange(1024).astype(F)
    if full:
        return v / F(1023), (v - F(512)) / F(1023)
    return (v - F(64)) / F(876), (v - F(512)) / F(896)


def _clip01(v):
    return np.minimum(np.maximum(v, F(0)), F(1))


def _matrix(y, cb, cr, matrix):
    k = constants(matrix)
    R = y + k['a_r'] * cr
    B = y + k['a_b'] * cb
    G = (y - k['g_b'] * cb) - k['g_r'] * cr
    out = np.stack([_clip01(R), _clip01(G), _clip01(B)], -1)
    assert out.dtype == F
    return out


def samples_to_rgb(Y, Cb, Cr, matrix, full):
    """Codes of equal shape (chroma already replicated) -> float32 [..., 3]."""
    ty, tc = tables(full)
    return _matrix(ty[Y], tc[Cb], tc[Cr], matrix)


def unpack(frame, layout):
    """[H * 3 // 2, W] -> the stored words (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2]) (views)."""
    h3, W = frame.shape
    H = h3 * 2 // 3
    assert H % 2 == 0 and W % 2 == 0 and H * 3 // 2 == h3 and layout in LAYOUTS and frame.dtype == np.uint16
    flat = frame.reshape(-1)
    Y, c = flat[:H * W].reshape(H, W), flat[H * W:]
    if layout == 'i010':
        return Y, c[:H * W // 4].reshape(H // 2, W // 2), c[H * W // 4:].reshape(H // 2, W // 2)
    c = c.reshape(H // 2, W // 2, 2)
    return Y, c[..., 0], c[..., 1]


def pack(Y, Cb, Cr, layout):
    """Stored words -> one frame."""
    H, W = Y.shape
    c = np.concatenate([Cb.ravel(), Cr.ravel()]) if layout == 'i010' else np.stack([Cb, Cr], -1).ravel()
    return np.concatenate([Y.ravel(), c]).astype(np.uint16).reshape(H * 3 // 2, W)


def convert_layout(frame, src, dst):
    """I010 <-> P010 of one frame: the same codes, the ignored bits zero."""
    return pack(*[store(code(p, src), dst) for p in unpack(np.ascontiguousarray(frame), src)], dst)


def yuv_in(frame, layout, matrix='bt709', full=False):
    """One 10-bit 4:2:0 frame -> float32 [H,W,3]: pixel (y, x) takes the chroma sample (y >> 1, x >> 1)."""
    Y, Cb, Cr = (code(p, layout) for p in unpack(np.ascontiguousarray(frame), layout))
    rep = lambda c: c.repeat(2, 0).repeat(2, 1)       # noqa: E731
    return samples_to_rgb(Y, rep(Cb), rep(Cr), matrix, full)


def _q10(v):
    return (np.minimum(np.maximum(v, F(0)), F(1023)) + F(0.5)).astype(np.uint16)


def out_unquantised(rgb, matrix, full):
    """float32 [H,W,3] -> the float32 values right before q10(): (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2])."""
    k = constants(matrix)
    x = _clip01(np.asarray(rgb, F))
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Yf = (k['kr'] * R + k['kg'] * G) + k['kb'] * B
    cbf = (B - Yf) * k['s_b']
    crf = (R - Yf) * k['s_r']
    box = lambda c: ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * F(0.25)       # noqa: E731
    ys, yo, cs = (F(1023), F(0), F(1023)) if full else (F(876), F(64), F(896))
    vals = Yf * ys + yo, box(cbf) * cs + F(512), box(crf) * cs + F(512)
    assert all(v.dtype == F for v in vals)
    return vals


def yuv_out(rgb, layout, matrix='bt709', full=False):
    """float32 [H,W,3] -> one 10-bit 4:2:0 frame [H * 3 // 2, W]."""
    return pack(*[store(_q10(v), layout) for v in out_unquantised(rgb, matrix, full)], layout)


def histogram(frame, layout):
    """int64 [3][256]: plane p's samples in bin code >> 2 (include/film_hip.h, "Scene cuts")."""
    return np.stack([np.bincount((code(p, layout) >> 2).ravel(), minlength=256) for p in unpack(np.ascontiguousarray(frame), layout)]).astype(np.int64)


# ---- the cut --------------------------------------------------------------------------------------------------------------------------
# p010_as_i010 / i010_as_p010: the code rule of the other layout; ignored_bits_not_masked: the whole word taken as the value (I010: float(w);
# P010: float(w) / 64); eight_bit_scale_shifted: the divisors 219 << 2, 224 << 2, 255 << 2 - right for limited range, 1020 instead of 1023
# for full range (chroma centred on 128 << 2 = 512 either way); cb_cr_swapped; chroma_from_tile_coordinate: the pairing counted from the
# tile's first row / column.
FAULTS = ('p010_as_i010', 'i010_as_p010', 'ignored_bits_not_masked', 'eight_bit_scale_shifted', 'cb_cr_swapped', 'chroma_from_tile_coordinate')


def _rgb_of_words(Y, Cb, Cr, layout, matrix, full, fault):
    if fault == 'p010_as_i010' and layout == 'p010':
        layout = 'i010'
    elif fault == 'i010_as_p010' and layout == 'i010':
        layout = 'p010'
    if fault == 'ignored_bits_not_masked':
        v = [p.astype(F) / F(64) if layout == 'p010' else p.astype(F) for p in (Y, Cb, Cr)]
    else:
        v = [code(p, layout).astype(F) for p in (Y, Cb, Cr)]
    if full:
        d = F(1020) if fault == 'eight_bit_scale_shifted' else F(1023)
        y, cb, cr = v[0] / d, (v[1] - F(512)) / d, (v[2] - F(512)) / d
    else:
        y, cb, cr = (v[0] - F(64)) / F(876), (v[1] - F(512)) / F(896), (v[2] - F(512)) / F(896)
    return _matrix(y, cb, cr, matrix)


def cut(frames, geo, tile0, ntiles, layout, matrix, full, fault=None):
    """Tiles [tile0, tile0 + ntiles) of the 10-bit frame batch [B, H * 3 // 2, W] as float32 RGB [ntiles, TH, TW, 3] with +0.0 padding."""
    B, h3, W = frames.shape
    H = h3 * 2 // 3
    g = T._Geo(geo, (B, H, W))
    out = np.zeros((ntiles, g.TH, g.TW, 3), F)
    for k in range(ntiles):
        b, ty, tx = g.tile(tile0 + k)
        sy, sx = g.ys[ty], g.xs[tx]
        Y, Cb, Cr = unpack(np.ascontiguousarray(frames[b]), layout)
        if fault == 'cb_cr_swapped':
            Cb, Cr = Cr, Cb
        yy, xx = sy + np.arange(g.eh), sx + np.arange(g.ew)
        cy, cx = yy >> 1, xx >> 1
        if fault == 'chroma_from_tile_coordinate':
            cy, cx = (sy >> 1) + (np.arange(g.eh) >> 1), (sx >> 1) + (np.arange(g.ew) >> 1)
        out[k, g.oy:g.oy + g.eh, g.ox:g.ox + g.ew] = _rgb_of_words(Y[yy][:, xx], Cb[cy][:, cx], Cr[cy][:, cx], layout, matrix, full, fault)
    return out


def cut_via_frames(frames, geo, tile0, ntiles, layout, matrix, full):
    """The same through the frame-level conversion (table look-ups) and tile_map_ref's float cut: the two must agree."""
    rgb = np.stack([yuv_in(f, layout, matrix, full) for f in frames])
    return T.cut(rgb, geo, tile0, ntiles)


# ---- designed data and allocations ------------------------------------------------------------------------------------------------------
EXTREMES = (0, 1, 3, 4, 63, 64, 65, 511, 512, 513, 939, 940, 941, 959, 960, 961, 1019, 1020, 1022, 1023)


def designed_frames(b, h, w, seed, layout='i010'):
    """b frames: a Y plane of 1024 samples or more holds every code 0 .. 1023 (a rolled ramp); smaller planes share a strided ramp out among
    the frames of the batch; every plane starts with as many of EXTREMES as fit; the rest is random.  The bits the layout ignores are random
    junk (the same codes for both layouts: the frames of 'p010' are those of 'i010' converted, with junk of their own)."""
    rng = np.random.default_rng(seed)
    ramp = np.arange(1024)
    out = []
    for i in range(b):
        planes = []
        for pi, n in enumerate((h * w, h * w // 4, h * w // 4)):
            p = rng.integers(0, 1024, n)
            m = min(n, 1024)
            rolled = np.roll(ramp, 160 * pi + 28 * i)
            start = min(17 * i + 5, n - m)
            p[start:start + m] = rolled if m == 1024 else rolled[np.arange(m) * 1024 // m]
            ne = min(len(EXTREMES), n - (start + m) if n >= 1024 else n // 2)      # (never into a whole ramp)
            if n < 8:                                                    # (a 2 x 2 frame: the extremes take turns over the frames)
                ne = n
            if ne:
                p[n - ne:] = np.roll(EXTREMES, -3 * i - 7 * pi)[:ne]
            planes.append(p)
        fr = pack(store(planes[0].reshape(h, w), layout), store(planes[1].reshape(h // 2, w // 2), layout), store(planes[2].reshape(h // 2, w // 2), layout), layout)
        out.append(with_junk(fr, layout, seed * 31 + i))
    return np.stack(out)


def frames_view(alloc, case):
    n = case.B * case.H * case.W * 3 // 2
    return alloc[GUARD_U16:GUARD_U16 + n].reshape(case.B, case.H * 3 // 2, case.W)


def new_frames_alloc(case, layout, seed):
    """uint16 [guard | the frame batch | guard]: whole 32-bit words, the payload 4-byte aligned when the allocation is."""
    n = case.B * case.H * case.W * 3 // 2
    assert n % 2 == 0 and GUARD_U16 % 2 == 0
    a = np.random.default_rng(seed).integers(0, 65536, GUARD_U16 + n + GUARD_U16).astype(np.uint16)
    a[GUARD_U16:GUARD_U16 + n] = designed_frames(case.B, case.H, case.W, seed, layout).ravel()
    return a


class NumpyBackend:
    """The restatement as a backend, with at most one of FAULTS planted."""

    def __init__(self, geo_of, fault=None):
        assert fault is None or fault in FAULTS
        self.geo_of, self.fault = geo_of, fault

    def __call__(self, frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full):
        geo = self.geo_of(case)
        fr, tl = np.array(frames_alloc), np.array(tiles_alloc)
        T.tiles_view(tl, geo)[:ntiles] = cut(frames_view(fr, case), geo, tile0, ntiles, layout, matrix, full, self.fault)
        return fr, tl


def check_cut(backend, case, geo, layout, matrix, full, ranges, seed=0, twice=True):
    """Yields a message per finding (as yuv_ref.check_cut): for every range, on freshly filled allocations, tiles_dev[0 : ntiles] equals
    the restatement on the bits with +0.0 padding, the rest of the tile tensor (one tile more than the longest range), its guards and the
    frame allocation are untouched, and the same call again gives the same bits."""
    cap = max(nt for _, nt in ranges) + 1
    for i, (tile0, nt) in enumerate(ranges):
        fr0 = new_frames_alloc(case, layout, seed + 2 * i)
        tl0 = T.new_tiles_alloc(geo, cap, seed + 2 * i + 1)
        fr0.setflags(write=False); tl0.setflags(write=False)
        fr1, tl1 = backend(fr0, tl0, case, tile0, nt, layout, matrix, full)
        where = f'{case.name} {layout} {matrix}{" full" if full else ""} cut [{tile0}, {tile0 + nt})'
        ref = cut(frames_view(fr0, case), geo, tile0, nt, layout, matrix, full)
        want = np.array(tl0)
        T.tiles_view(want, geo)[:nt] = ref
        got = T.tiles_view(tl1, geo)[:nt]
        if not np.array_equal(np.asarray(fr1).view(np.uint16), fr0):
            yield f'{where}: the frames (or their guards) were written'
        if not T._same(got, ref):
            bad = np.argwhere(T.bits(got) != T.bits(ref))
            yield f'{where}: {len(bad)} tile floats differ, first at (tile, y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {ref[tuple(bad[0])]!r}'
        pad = np.ones(ref.shape, bool)
        pad[:, geo['pad_y']:geo['pad_y'] + geo['tile_h'], geo['pad_x']:geo['pad_x'] + geo['tile_w']] = False
        if T.bits(got)[pad].any():
            yield f'{where}: the padding is not +0.0'
        rest_got, rest_want = np.array(tl1), np.array(want)
        T.tiles_view(rest_got, geo)[:nt] = 0; T.tiles_view(rest_want, geo)[:nt] = 0
        if not T._same(rest_got, rest_want):
            yield f'{where}: written outside tiles [0, {nt}) of the tile tensor (the later tiles or the guards)'
        if twice:
            fr2, tl2 = backend(fr0, tl0, case, tile0, nt, layout, matrix, full)
            if not (np.array_equal(np.asarray(fr2).view(np.uint16), np.asarray(fr1).view(np.uint16)) and T._same(tl2, tl1)):
                yield f'{where}: the same call again gives other bits'


# ---- which branches of the kernels a call takes (restates the kernels' own conditions) ----------------------------------------------------
def branches(case, geo, layout, tile0, ntiles):
    """Names of the instance of frame_yuv10_to_tiles_kernel and of the branches the call takes, for a tile tensor whose first float is
    16-byte aligned and a frame batch whose first word is 4-byte aligned.  Addresses below count 16-bit words."""
    g = T._Geo(geo, (case.B, case.H, case.W))
    p010 = layout == 'p010'
    out = {f'frame_yuv10_to_tiles_kernel<{"true" if g.ovy | g.ovx else "false"}, {"true" if p010 else "false"}>'}
    row, groups = g.TW * 3, (g.TW + 3) // 4
    plane = g.H * g.W
    for k in range(ntiles):
        b, ty, tx = g.tile(tile0 + k)
        if g.ys[ty] & 1: out.add('odd row origin')
        if g.xs[tx] & 1: out.add('odd column origin')
        for y in range(g.TH):
            r = k * g.TH + y
            sy = y - g.oy
            for q in range(groups):
                xp0 = q * 4
                s0 = xp0 - g.ox
                if 0 <= sy < g.eh and s0 + 4 > 0 and s0 < g.ew:
                    fy, fx = g.ys[ty] + sy, g.xs[tx] + s0
                    if s0 >= 0 and s0 + 4 <= g.ew:
                        ya = b * plane * 3 // 2 + fy * g.W + fx
                        out.add('word path, Y in two aligned words' if ya % 2 == 0 else 'word path, Y across three words')
                        out.add('word path, odd column: three chroma samples' if fx & 1 else 'word path, even column: two chroma samples')
                        c0, nc = fx >> 1, ((fx + 3) >> 1) - (fx >> 1) + 1
                        if p010:
                            out.add(f'word path, {"three" if nc == 3 else "two"} CbCr pair words')
                        else:
                            ca = b * plane * 3 // 2 + plane + (fy >> 1) * (g.W // 2) + c0
                            out.add('word path, chroma across two words' if ca % 2 + nc > 2 else 'word path, chroma in one word')
                    else:
                        out.add('sample path')
                else:
                    out.add('padding group')
                vec = xp0 * 3 + 12 <= row and (r * row + xp0 * 3) % 4 == 0
                out.add('vector stores' if vec else 'scalar stores')
    return out


def out_branches(h, w, layout, dst_offset=0):
    """The same for rgb_to_yuv10_kernel on an h x w frame whose dst lies dst_offset BYTES (0 or 2) behind a 4-byte boundary (src 16-byte aligned)."""
    assert dst_offset in (0, 2)
    o = dst_offset // 2
    out = {f'rgb_to_yuv10_kernel<{"true" if layout == "p010" else "false"}>'}
    for y0 in range(0, h, 2):
        for x0 in range(0, w, 8):
            n = min(8, w - x0)
            for dy in (0, 1):
                out.add('vector loads' if n == 8 and (((y0 + dy) * w + x0) * 12) % 16 == 0 else 'scalar loads')
                out.add('Y word stores' if n == 8 and (o + (y0 + dy) * w + x0) % 2 == 0 else 'Y sample stores')
            if layout == 'p010':
                ok = n == 8 and (o + h * w + (y0 >> 1) * w + x0) % 2 == 0
            else:
                a = o + h * w + (y0 >> 1) * (w >> 1) + (x0 >> 1)
                ok = n == 8 and a % 2 == 0 and (a + h * w // 4) % 2 == 0
            out.add('chroma word stores' if ok else 'chroma sample stores')
    return out
