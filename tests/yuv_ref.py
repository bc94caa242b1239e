"""Numpy restatement of the Y'CbCr 4:2:0 arithmetic of include/film_hip.h ("The 4:2:0 arithmetic"): the per-byte tables, the conversion in
(samples -> float32 RGB, what frame_yuv_to_tiles_kernel of csrc/frame_kernels.hip fuses into the tile cut), the conversion out (float32 RGB
-> samples, rgb_to_yuv_kernel there), I420 <-> NV12, and the cut of a 4:2:0 frame batch into tiles over the geometry film_tiling_json reports.
Every operation is float32 with one rounding (numpy does not fuse), so every comparison against the kernels is on the bits.

A frame is an array [H * 3 // 2, W] of samples: rows [0, H) are the Y plane; the H * W / 2 samples behind it are Cb [H/2][W/2] then
Cr [H/2][W/2] (planar: I420, I010) or CbCr [H/2][W/2][2] (semi-planar: NV12, P010).

What does not depend on the depth of a sample is stated once, in Format: the plane bookkeeping, the conversions around a format's tables and
code rule, the cut, its comparison and the branches of the kernels.  This module instantiates it for 8-bit samples and exports that
instance's functions under their plain names; tests/yuv10_ref.py does the same for 10-bit codes in 16-bit words.

The tile bookkeeping is tests/tile_map_ref.py's.  A "backend" of check_cut is a callable
    backend(frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full) -> (frames_alloc', tiles_alloc')
on the two whole allocations (guard | payload | guard); the GPU test's calls film_debug_yuv_cut, NumpyBackend applies the restatement,
optionally with one of FAULTS planted.
"""
import collections

import numpy as np

import tile_map_ref as T

LAYOUTS = ('i420', 'nv12')
COLOURS = [(m, f) for m in ('bt709', 'bt601') for f in (False, True)]
KR_KB = {'bt709': (0.2126, 0.0722), 'bt601': (0.299, 0.114)}
F = np.float32

Case = collections.namedtuple('Case', 'name B H W block align overlap')
# the geometries of the cut test: small, and together they reach every branch of the kernel (branches() below)
CASES = [
    Case('y1-30x50-b3x2', 2, 30, 50, (3, 2), 8, (0, 0)),       # 10 x 25 patches: an odd column origin, chroma rows at every byte offset mod 4
    Case('y2-30x50-b3x2-ov3x5', 2, 30, 50, (3, 2), 8, (3, 5)),  # odd origins in both axes
    Case('y3-16x16', 1, 16, 16, None, None, (0, 0)),           # untiled, no padding: the pure fast path
    Case('y4-2x2', 1, 2, 2, None, 8, (0, 0)),                  # one chroma sample, the rest padding
    Case('y5-18x44-b1x2', 3, 18, 44, (1, 2), 16, (0, 0)),
    Case('y6-12x22-b1x2-noalign', 1, 12, 22, (1, 2), None, (0, 0)),   # 11-pixel tiles without padding: a tile row of 33 floats (scalar stores)
]


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def constants(matrix):
    """The float32 constants of a matrix: computed in double from (Kr, Kb), rounded once."""
    Kr, Kb = KR_KB[matrix]
    Kg = 1.0 - Kr - Kb
    return {'a_r': F(2.0 * (1.0 - Kr)), 'a_b': F(2.0 * (1.0 - Kb)), 'g_b': F(2.0 * Kb * (1.0 - Kb) / Kg), 'g_r': F(2.0 * Kr * (1.0 - Kr) / Kg),
            'kr': F(Kr), 'kg': F(Kg), 'kb': F(Kb), 's_b': F(0.5 / (1.0 - Kb)), 's_r': F(0.5 / (1.0 - Kr))}


def tables(full):
    """(y[256], c[256]): the luma and chroma value of every byte, IEEE float32 division."""
    v = np.arange(256).astype(F)
    if full:
        return v / F(255), (v - F(128)) / F(255)
    return (v - F(16)) / F(219), (v - F(128)) / F(224)


def _clip01(v):
    return np.minimum(np.maximum(v, F(0)), F(1))


def matrix_to_rgb(y, cb, cr, matrix):
    """float32 luma and chroma values of equal shape -> float32 [..., 3], clipped."""
    k = constants(matrix)
    R = y + k['a_r'] * cr
    B = y + k['a_b'] * cb
    G = (y - k['g_b'] * cb) - k['g_r'] * cr
    out = np.stack([_clip01(R), _clip01(G), _clip01(B)], -1)
    assert out.dtype == F
    return out


def ranges_of(case, geo):
    bh, bw = len(geo['origins_y']), len(geo['origins_x'])
    return T.partitions(case.B * bh * bw, bh * bw)


# the faults every format can plant where the cut gathers its samples (the last: a semi-planar frame read as the planar layout); a format's
# other faults are planted by its rgb_of_samples
GATHER_FAULTS = ('chroma_from_tile_coordinate', 'cb_cr_swapped', 'nv12_as_i420')


class Format:
    """The restatement for one sample format.  What a format decides:
    depth            bits of a code: 8 (a sample is a byte) or 10 (a 16-bit word); gives the dtype, the samples per 32-bit word and the code ranges
    guard            samples of guard band on each side of a frame batch (the payload stays 4-byte aligned)
    layouts          (planar, semi-planar) names
    faults           what NumpyBackend can plant
    sample           'byte' / 'sample': how the kernels' one-at-a-time paths are called in branches() / out_branches()
    tables           full -> (y[codes], c[codes]): the luma and chroma value of every code
    designed_frames  (b, h, w, seed, layout) -> the frames of the cut test
    code, store      (samples, layout) -> codes and back; None: a sample is its code
    rgb_of_samples   (Y, Cb, Cr, layout, matrix, full, fault) -> float32 RGB of gathered samples with an optional planted fault; None: the table
                     look-up, no faults of its own
    """

    def __init__(self, depth, guard, layouts, faults, sample, tables, designed_frames, code=None, store=None, rgb_of_samples=None):
        self.depth, self.guard, self.layouts, self.faults, self.sample = depth, guard, layouts, faults, sample
        self.dtype = np.dtype(np.uint8 if depth == 8 else np.uint16)
        self.per_word = 4 // self.dtype.itemsize
        self.tables, self.designed_frames = tables, designed_frames
        self.code = code or (lambda samples, layout: np.asarray(samples))
        self.store = store or (lambda codes, layout: np.asarray(codes))
        self.rgb_of_samples = rgb_of_samples or (lambda Y, Cb, Cr, layout, matrix, full, fault: self.samples_to_rgb(Y, Cb, Cr, matrix, full))

    # ---- planes ----
    def unpack(self, frame, layout):
        """[H * 3 // 2, W] -> the stored samples (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2]) (views)."""
        h3, W = frame.shape
        H = h3 * 2 // 3
        assert H % 2 == 0 and W % 2 == 0 and H * 3 // 2 == h3 and layout in self.layouts and frame.dtype == self.dtype
        flat = frame.reshape(-1)
        Y, c = flat[:H * W].reshape(H, W), flat[H * W:]
        if layout == self.layouts[0]:
            return Y, c[:H * W // 4].reshape(H // 2, W // 2), c[H * W // 4:].reshape(H // 2, W // 2)
        c = c.reshape(H // 2, W // 2, 2)
        return Y, c[..., 0], c[..., 1]

    def pack(self, Y, Cb, Cr, layout):
        """Stored samples -> one frame."""
        H, W = Y.shape
        c = np.concatenate([Cb.ravel(), Cr.ravel()]) if layout == self.layouts[0] else np.stack([Cb, Cr], -1).ravel()
        return np.concatenate([Y.ravel(), c]).astype(self.dtype).reshape(H * 3 // 2, W)

    def frames_view(self, alloc, case):
        n = case.B * case.H * case.W * 3 // 2
        return alloc[self.guard:self.guard + n].reshape(case.B, case.H * 3 // 2, case.W)

    def new_frames_alloc(self, case, layout, seed):
        """[guard | the frame batch | guard] in whole 32-bit words (the cut reads aligned words), the payload 4-byte aligned when the allocation is."""
        n = case.B * case.H * case.W * 3 // 2
        assert self.guard % self.per_word == 0
        size = -(-(2 * self.guard + n) // self.per_word) * self.per_word
        a = np.random.default_rng(seed).integers(0, 1 << 8 * self.dtype.itemsize, size, dtype=self.dtype)
        a[self.guard:self.guard + n] = self.designed_frames(case.B, case.H, case.W, seed, layout).ravel()
        return a

    # ---- the conversions ----
    def samples_to_rgb(self, Y, Cb, Cr, matrix, full):
        """Codes of equal shape (chroma already replicated) -> float32 [..., 3]."""
        ty, tc = self.tables(full)
        return matrix_to_rgb(ty[Y], tc[Cb], tc[Cr], matrix)

    def yuv_in(self, frame, layout, matrix='bt709', full=False):
        """One 4:2:0 frame -> float32 [H,W,3]: pixel (y, x) takes the chroma sample (y >> 1, x >> 1)."""
        Y, Cb, Cr = (self.code(p, layout) for p in self.unpack(np.ascontiguousarray(frame), layout))
        rep = lambda c: c.repeat(2, 0).repeat(2, 1)       # noqa: E731
        return self.samples_to_rgb(Y, rep(Cb), rep(Cr), matrix, full)

    def quantise(self, v):
        return (np.minimum(np.maximum(v, F(0)), F((1 << self.depth) - 1)) + F(0.5)).astype(self.dtype)

    def out_unquantised(self, rgb, matrix, full):
        """float32 [H,W,3] -> the float32 values right before the quantiser: (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2])."""
        k = constants(matrix)
        x = _clip01(np.asarray(rgb, F))
        R, G, B = x[..., 0], x[..., 1], x[..., 2]
        Yf = (k['kr'] * R + k['kg'] * G) + k['kb'] * B
        cbf = (B - Yf) * k['s_b']
        crf = (R - Yf) * k['s_r']
        box = lambda c: ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * F(0.25)       # noqa: E731
        top, s = (1 << self.depth) - 1, 1 << (self.depth - 8)      # 255 / 1023; the limited ranges are the 8-bit ones times s
        ys, yo, cs = (F(top), F(0), F(top)) if full else (F(219 * s), F(16 * s), F(224 * s))
        vals = Yf * ys + yo, box(cbf) * cs + F(128 * s), box(crf) * cs + F(128 * s)
        assert all(v.dtype == F for v in vals)
        return vals

    def yuv_out(self, rgb, layout, matrix='bt709', full=False):
        """float32 [H,W,3] -> one 4:2:0 frame [H * 3 // 2, W]."""
        return self.pack(*[self.store(self.quantise(v), layout) for v in self.out_unquantised(rgb, matrix, full)], layout)

    # ---- the cut ----
    def cut(self, frames, geo, tile0, ntiles, layout, matrix, full, fault=None):
        """Tiles [tile0, tile0 + ntiles) of the 4:2:0 frame batch [B, H * 3 // 2, W] as float32 RGB [ntiles, TH, TW, 3] with +0.0 padding."""
        B, h3, W = frames.shape
        H = h3 * 2 // 3
        g = T._Geo(geo, (B, H, W))
        out = np.zeros((ntiles, g.TH, g.TW, 3), F)
        for k in range(ntiles):
            b, ty, tx = g.tile(tile0 + k)
            sy, sx = g.ys[ty], g.xs[tx]
            Y, Cb, Cr = self.unpack(np.ascontiguousarray(frames[b]), self.layouts[0] if fault == 'nv12_as_i420' else layout)
            if fault == 'cb_cr_swapped':
                Cb, Cr = Cr, Cb
            yy, xx = sy + np.arange(g.eh), sx + np.arange(g.ew)
            cy, cx = yy >> 1, xx >> 1
            if fault == 'chroma_from_tile_coordinate':      # the pairing counted from the tile's first row / column
                cy, cx = (sy >> 1) + (np.arange(g.eh) >> 1), (sx >> 1) + (np.arange(g.ew) >> 1)
            out[k, g.oy:g.oy + g.eh, g.ox:g.ox + g.ew] = self.rgb_of_samples(Y[yy][:, xx], Cb[cy][:, cx], Cr[cy][:, cx], layout, matrix, full, fault)
        return out

    def cut_via_frames(self, frames, geo, tile0, ntiles, layout, matrix, full):
        """The same through the frame-level conversion (table look-ups) and tile_map_ref's float cut: the two must agree."""
        rgb = np.stack([self.yuv_in(f, layout, matrix, full) for f in frames])
        return T.cut(rgb, geo, tile0, ntiles)

    def NumpyBackend(self, geo_of, fault=None):
        """The restatement as a backend, with at most one of the format's faults planted."""
        assert fault is None or fault in self.faults

        def backend(frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full):
            geo = geo_of(case)
            fr, tl = np.array(frames_alloc), np.array(tiles_alloc)
            T.tiles_view(tl, geo)[:ntiles] = self.cut(self.frames_view(fr, case), geo, tile0, ntiles, layout, matrix, full, fault)
            return fr, tl
        return backend

    def check_cut(self, backend, case, geo, layout, matrix, full, ranges, seed=0, twice=True):
        """Yields a message per finding (as tile_map_ref.check_cut): for every range, on freshly filled allocations, tiles_dev[0 : ntiles]
        equals the restatement on the bits with +0.0 padding, the rest of the tile tensor (one tile more than the longest range), its guards
        and the frame allocation are untouched, and the same call again gives the same bits."""
        cap = max(nt for _, nt in ranges) + 1
        samples = lambda a: np.asarray(a).view(self.dtype)       # noqa: E731
        for i, (tile0, nt) in enumerate(ranges):
            fr0 = self.new_frames_alloc(case, layout, seed + 2 * i)
            tl0 = T.new_tiles_alloc(geo, cap, seed + 2 * i + 1)
            fr0.setflags(write=False); tl0.setflags(write=False)
            fr1, tl1 = backend(fr0, tl0, case, tile0, nt, layout, matrix, full)
            where = f'{case.name} {layout} {matrix}{" full" if full else ""} cut [{tile0}, {tile0 + nt})'
            ref = self.cut(self.frames_view(fr0, case), geo, tile0, nt, layout, matrix, full)
            want = np.array(tl0)
            T.tiles_view(want, geo)[:nt] = ref
            got = T.tiles_view(tl1, geo)[:nt]
            if not T._same(samples(fr1), fr0):
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
                if not (T._same(samples(fr2), samples(fr1)) and T._same(tl2, tl1)):
                    yield f'{where}: the same call again gives other bits'

    # ---- which branches of the kernels a call takes (restates the kernels' own conditions) ----
    def branches(self, case, geo, layout, tile0, ntiles):
        """Names of the instance of frame_yuv_to_tiles_kernel and of the branches the call takes, for a tile tensor whose first float is
        16-byte aligned and a frame batch whose first sample is 4-byte aligned.  Addresses below count samples, pw to a 32-bit word."""
        g = T._Geo(geo, (case.B, case.H, case.W))
        semi, pw = layout == self.layouts[1], self.per_word
        pair_words = semi and pw == 2          # a CbCr pair IS a word: the kernel reads the pair words themselves
        count = ('no', 'one', 'two', 'three')
        y_words = 4 // pw                      # words that hold four aligned Y samples
        out = {f'frame_yuv_to_tiles_kernel<{"true" if g.ovy | g.ovx else "false"}, FILM_PIX_{layout.upper()}>'}
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
                            out.add(f'word path, Y in {count[y_words]} aligned word{"s" if y_words > 1 else ""}' if ya % pw == 0
                                    else f'word path, Y across {count[y_words + 1]} words')
                            out.add('word path, odd column: three chroma samples' if fx & 1 else 'word path, even column: two chroma samples')
                            c0, nc = fx >> 1, ((fx + 3) >> 1) - (fx >> 1) + 1
                            if pair_words:
                                out.add(f'word path, {"three" if nc == 3 else "two"} CbCr pair words')
                            else:
                                ca = b * plane * 3 // 2 + plane + (fy >> 1) * (g.W if semi else g.W // 2) + (2 * c0 if semi else c0)
                                out.add('word path, chroma across two words' if ca % pw + (2 * nc if semi else nc) > pw else 'word path, chroma in one word')
                        else:
                            out.add(f'{self.sample} path')
                    else:
                        out.add('padding group')
                    vec = xp0 * 3 + 12 <= row and (r * row + xp0 * 3) % 4 == 0
                    out.add('vector stores' if vec else 'scalar stores')
        return out

    def out_branches(self, h, w, layout, dst_offset=0):
        """The same for rgb_to_yuv_kernel on an h x w frame whose dst lies dst_offset BYTES (whole samples) behind a 4-byte boundary (src 16-byte aligned)."""
        assert dst_offset % self.dtype.itemsize == 0
        o, pw = dst_offset // self.dtype.itemsize, self.per_word
        out = {f'rgb_to_yuv_kernel<FILM_PIX_{layout.upper()}>'}
        for y0 in range(0, h, 2):
            for x0 in range(0, w, 8):
                n = min(8, w - x0)
                for dy in (0, 1):
                    out.add('vector loads' if n == 8 and (((y0 + dy) * w + x0) * 12) % 16 == 0 else 'scalar loads')
                    out.add('Y word stores' if n == 8 and (o + (y0 + dy) * w + x0) % pw == 0 else f'Y {self.sample} stores')
                if layout == self.layouts[1]:
                    ok = n == 8 and (o + h * w + (y0 >> 1) * w + x0) % pw == 0
                else:
                    a = o + h * w + (y0 >> 1) * (w >> 1) + (x0 >> 1)
                    ok = n == 8 and a % pw == 0 and (a + h * w // 4) % pw == 0
                out.add('chroma word stores' if ok else f'chroma {self.sample} stores')
        return out


# ---- 8-bit samples ------------------------------------------------------------------------------------------------------------------------
FAULTS = GATHER_FAULTS


def designed_frames(b, h, w, seed, layout='i420'):
    """b frames whose planes hold every byte value wherever a plane has 256 samples (a rolled ramp, as tile_map_ref.designed_u8); smaller
    planes of a batch share the ramp out among the frames."""
    rng = np.random.default_rng(seed)
    ramp = np.arange(256, dtype=np.uint8)
    out = []
    for i in range(b):
        planes = []
        for pi, n in enumerate((h * w, h * w // 4, h * w // 4)):
            p = rng.integers(0, 256, n, dtype=np.uint8)
            m = min(n, 256)
            start = min(17 * i + 5, n - m)
            p[start:start + m] = np.roll(ramp, 40 * pi + 7 * i - i * m)[:m]
            planes.append(p)
        out.append(pack(planes[0].reshape(h, w), planes[1].reshape(h // 2, w // 2), planes[2].reshape(h // 2, w // 2), layout))
    return np.stack(out)


_FMT = Format(8, T.GUARD_U8, LAYOUTS, FAULTS, 'byte', tables, designed_frames)
unpack, pack, frames_view, new_frames_alloc = _FMT.unpack, _FMT.pack, _FMT.frames_view, _FMT.new_frames_alloc
samples_to_rgb, yuv_in, out_unquantised, yuv_out = _FMT.samples_to_rgb, _FMT.yuv_in, _FMT.out_unquantised, _FMT.yuv_out
cut, cut_via_frames, NumpyBackend, check_cut = _FMT.cut, _FMT.cut_via_frames, _FMT.NumpyBackend, _FMT.check_cut
branches, out_branches = _FMT.branches, _FMT.out_branches


def convert_layout(frame, src, dst):
    """I420 <-> NV12 of one frame."""
    return pack(*unpack(frame, src), dst)
