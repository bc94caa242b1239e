"""Numpy restatement of the Y'CbCr arithmetic of include/film_hip.h over (depth, SX, SY, matrix) ("The 4:2:0 arithmetic", "The 10-bit 4:2:0
arithmetic", "The 4:2:2 and 4:4:4 arithmetic"): the code of a stored sample, the tables, the conversion in (samples -> float32 RGB, what
frame_yuv_to_tiles_kernel of csrc/frame_kernels.hip fuses into the tile cut), the conversion out (float32 RGB -> samples, rgb_to_yuv_kernel
there), the histogram of a frame, and the cut of a frame batch into tiles over the geometry film_tiling_json reports.  Every operation is
float32 with one rounding (numpy does not fuse), so every comparison against the kernels is on the bits.

Format(depth, SX, SY) states all of it once: depth 8 (a sample is a byte, its own code) or 10 (a 16-bit word; I010 / I210 / I410 keep the code
in bits 0-9, P010 in bits 6-15, the other six bits are ignored on the way in and zero on the way out); (SX, SY) the chroma shifts, (1, 1) 4:2:0,
(1, 0) 4:2:2, (0, 0) 4:4:4.  FORMATS maps every layout name to its Format.  A frame is an array [rows, W] of samples: rows [0, H) are the Y
plane, behind it Cb [H >> SY][W >> SX] then Cr [H >> SY][W >> SX] (planar) or, 4:2:0 only, the CbCr pairs [H/2][W/2][2] (semi-planar: NV12,
P010); rows = H * 3 // 2, 2 * H or 3 * H.

The tile bookkeeping is tests/tile_map_ref.py's.  A "backend" of check_cut is a callable
    backend(frames_alloc, tiles_alloc, case, tile0, ntiles, layout, matrix, full) -> (frames_alloc', tiles_alloc')
on the two whole allocations (guard | payload | guard); the GPU tests' call film_debug_yuv_cut, NumpyBackend applies the restatement,
optionally with one of FAULTS planted.  tests/golden/yuv_ref_digests.json pins what this module computes (tools/make_yuv_ref_golden.py).
"""
import collections

import numpy as np

import tile_map_ref as T

F = np.float32
MATRICES = ('bt709', 'bt601', 'bt2020nc')
KR_KB = {'bt709': (0.2126, 0.0722), 'bt601': (0.299, 0.114), 'bt2020nc': (0.2627, 0.0593)}
OLD_LAYOUTS = ('i420', 'nv12', 'i010', 'p010')
NEW_LAYOUTS = ('i422', 'i444', 'i210', 'i410')
LAYOUTS_OF = {(8, 1, 1): ('i420', 'nv12'), (10, 1, 1): ('i010', 'p010'), (8, 1, 0): ('i422',), (8, 0, 0): ('i444',), (10, 1, 0): ('i210',), (10, 0, 0): ('i410',)}

Case = collections.namedtuple('Case', 'name B H W block align overlap')
# the geometries of the cut tests: small, and together they reach every branch of the kernel (Format.branches)
CASES = [
    Case('y1-30x50-b3x2', 2, 30, 50, (3, 2), 8, (0, 0)),       # 10 x 25 patches: an odd column origin, chroma rows at every byte offset mod 4
    Case('y2-30x50-b3x2-ov3x5', 2, 30, 50, (3, 2), 8, (3, 5)),  # odd origins in both axes
    Case('y3-16x16', 1, 16, 16, None, None, (0, 0)),           # untiled, no padding: the pure fast path
    Case('y4-2x2', 1, 2, 2, None, 8, (0, 0)),                  # one chroma sample, the rest padding
    Case('y5-18x44-b1x2', 3, 18, 44, (1, 2), 16, (0, 0)),
    Case('y6-12x22-b1x2-noalign', 1, 12, 22, (1, 2), None, (0, 0)),   # 11-pixel tiles without padding: a tile row of 33 floats (scalar stores)
]
# ... and beyond them, the smallest shapes at which the 4:2:2 and 4:4:4 paths can go wrong
CASES_422 = [
    Case('s1-1x2', 1, 1, 2, None, 8, (0, 0)),                           # one row, one chroma sample per plane
    Case('s2-33x50-b3x2', 1, 33, 50, (3, 2), 8, (0, 0)),                # odd H; odd row origins 11, 22; an odd column origin
    Case('s3-33x50-b3x2-ov3x5', 2, 33, 50, (3, 2), 8, (3, 5)),
]
CASES_444 = [
    Case('f1-1x1', 1, 1, 1, None, 8, (0, 0)),
    Case('f2-33x51-b3x3', 2, 33, 51, (3, 3), 8, (0, 0)),                # 5049 samples a frame: frame 1 starts off a word boundary
    Case('f3-33x51-b3x3-ov3x5', 2, 33, 51, (3, 3), 8, (3, 5)),
]

# what NumpyBackend can plant.  Where the cut gathers its samples: chroma_from_tile_coordinate (the pairing counted from the tile's first row /
# column), cb_cr_swapped, nv12_as_i420 (a semi-planar frame read as planar), chroma_row_halved (4:2:2 reads chroma row fy >> 1, as 4:2:0 does),
# chroma_col_halved (4:4:4 reads chroma column fx >> 1).  In the value of a gathered sample: p010_as_i010 / i010_as_p010 (the other layout's code
# rule), ignored_bits_not_masked (the whole word as the value - I010: float(w); P010: float(w) / 64), eight_bit_scale_shifted (the divisors
# 219 << 2, 224 << 2, 255 << 2 - right for limited range, 1020 for 1023 in full range), bt709_under_bt2020 (BT.709 constants under the BT.2020
# flag).  On the way out: box_2x2_mean (4:2:0's 2 x 2 mean where 4:2:2 takes the 1 x 2 mean; the chroma rows are then pairwise equal).
FAULTS = ('chroma_from_tile_coordinate', 'cb_cr_swapped', 'nv12_as_i420', 'chroma_row_halved', 'chroma_col_halved', 'p010_as_i010', 'i010_as_p010',
          'ignored_bits_not_masked', 'eight_bit_scale_shifted', 'bt709_under_bt2020', 'box_2x2_mean')
EXTREMES = (0, 1, 3, 4, 63, 64, 65, 511, 512, 513, 939, 940, 941, 959, 960, 961, 1019, 1020, 1022, 1023)      # of the 10-bit ranges


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
def constants(matrix):
    """The float32 constants of a matrix: computed in double from (Kr, Kb), rounded once."""
    Kr, Kb = KR_KB[matrix]
    Kg = 1.0 - Kr - Kb
    return {'a_r': F(2.0 * (1.0 - Kr)), 'a_b': F(2.0 * (1.0 - Kb)), 'g_b': F(2.0 * Kb * (1.0 - Kb) / Kg), 'g_r': F(2.0 * Kr * (1.0 - Kr) / Kg),
            'kr': F(Kr), 'kg': F(Kg), 'kb': F(Kb), 's_b': F(0.5 / (1.0 - Kb)), 's_r': F(0.5 / (1.0 - Kr))}


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


# ---- designed data ----------------------------------------------------------------------------------------------------------------------
# Three generators (Format.designed_frames chooses), because the frames are data that tests and recorded results depend on.
def _designed_420_8(f, b, h, w, seed, layout):
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
        out.append(f.pack(planes[0].reshape(h, w), planes[1].reshape(h // 2, w // 2), planes[2].reshape(h // 2, w // 2), layout))
    return np.stack(out)


def _designed_420_10(f, b, h, w, seed, layout):
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
        fr = f.pack(f.store(planes[0].reshape(h, w), layout), f.store(planes[1].reshape(h // 2, w // 2), layout), f.store(planes[2].reshape(h // 2, w // 2), layout), layout)
        out.append(f.with_junk(fr, layout, seed * 31 + i))
    return np.stack(out)


def _designed_any(f, b, h, w, seed, layout):
    """b frames whose planes hold every code where a plane has room for them (a rolled ramp, strided where it has not), the extremes of
    the 10-bit ranges at the end of a plane, random codes elsewhere; a 10-bit frame carries random junk in the bits the layout ignores."""
    rng = np.random.default_rng(seed)
    codes = 1 << f.depth
    ch, cw = f.chroma_shape(h, w)
    out = []
    for i in range(b):
        planes = []
        for pi, n in enumerate((h * w, ch * cw, ch * cw)):
            p = rng.integers(0, codes, n)
            m = min(n, codes)
            rolled = np.roll(np.arange(codes), (codes // 6) * pi + 7 * i)
            start = min(17 * i + 5, n - m)
            p[start:start + m] = rolled if m == codes else rolled[np.arange(m) * codes // m]
            if f.depth == 10 and n > codes + 64:
                p[n - len(EXTREMES):] = np.roll(EXTREMES, -3 * i - 7 * pi)
            planes.append(p)
        fr = f.pack(f.store(planes[0].reshape(h, w), layout), f.store(planes[1].reshape(ch, cw), layout), f.store(planes[2].reshape(ch, cw), layout), layout)
        out.append(f.with_junk(fr, layout, seed * 31 + i))
    return np.stack(out)


def designed_rgb(h, w, seed):
    """float32 [h,w,3] in [-0.2, 1.2] with exact 0 and 1 and values below 0 and above 1: the source of the film_to_yuv test."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (h, w, 3)).astype(F)
    x[0, 0] = (0, 1, -3)
    x[-1, -1] = (7, 0.5, 1) if h * w > 1 else (7, 0.5, -3)      # (one pixel: above 1 and below 0 in one)
    return x


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
class Format:
    """The restatement for the layouts of one (depth, SX, SY): .layouts, the planar name first, then (4:2:0) the semi-planar one."""

    def __init__(self, depth, sx, sy):
        self.depth, self.sx, self.sy = depth, sx, sy
        self.layouts = LAYOUTS_OF[depth, sx, sy]
        self.dtype = np.dtype(np.uint8 if depth == 8 else np.uint16)
        self.per_word = 4 // self.dtype.itemsize                # samples per 32-bit word
        self.guard = T.GUARD_U8 // self.dtype.itemsize          # samples of guard band on each side of a frame batch (the payload stays 4-byte aligned)
        self.sample = 'byte' if depth == 8 else 'sample'        # how branches() / out_branches() call the kernels' one-at-a-time paths

    # ---- a stored sample and its code ----
    def code(self, samples, layout):
        """The code of every stored sample."""
        if self.depth == 8:
            return np.asarray(samples)
        w = np.asarray(samples).astype(np.uint32) & 0xffff
        return (w >> 6) if layout == 'p010' else (w & 1023)

    def store(self, codes, layout):
        """The sample a code is stored as: the ignored bits are zero."""
        if self.depth == 8:
            return np.asarray(codes)
        c = np.asarray(codes).astype(np.uint16)
        assert int(c.max(initial=0)) <= 1023
        return (c << 6).astype(np.uint16) if layout == 'p010' else c

    def with_junk(self, frame, layout, seed):
        """The same codes with random bits where a 10-bit layout ignores them (an 8-bit frame has no such bits)."""
        if self.depth == 8:
            return frame
        j = np.random.default_rng(seed).integers(0, 64, frame.shape).astype(np.uint16)
        return (self.store(self.code(frame, layout), layout) | (j if layout == 'p010' else (j << 10))).astype(np.uint16)

    def _ranges(self, full, fault=None):
        """float32 (Y offset, Y scale, chroma scale, chroma midpoint): the 8-bit ranges times s, but for the top code, 255 -> 1023."""
        s = 1 << (self.depth - 8)
        top = 255 * s if fault == 'eight_bit_scale_shifted' else (1 << self.depth) - 1
        return (F(0), F(top), F(top), F(128 * s)) if full else (F(16 * s), F(219 * s), F(224 * s), F(128 * s))

    def _values(self, y, cb, cr, full, fault=None):
        """float32 codes -> the luma and chroma values, IEEE float32 division."""
        yo, ys, cs, mid = self._ranges(full, fault)
        return (y - yo) / ys, (cb - mid) / cs, (cr - mid) / cs

    def tables(self, full):
        """(y[codes], c[codes]): the luma and chroma value of every code."""
        v = np.arange(1 << self.depth).astype(F)
        return self._values(v, v, v, full)[:2]

    # ---- planes ----
    def rows(self, H):
        return H * 3 // 2 if self.sy else 2 * H if self.sx else 3 * H

    def height(self, rows):
        return rows * 2 // 3 if self.sy else rows // 2 if self.sx else rows // 3

    def chroma_shape(self, H, W):
        return H >> self.sy, W >> self.sx

    def samples(self, H, W):
        ch, cw = self.chroma_shape(H, W)
        return H * W + 2 * ch * cw

    def unpack(self, frame, layout):
        """[rows, W] -> the stored samples (Y [H,W], Cb, Cr [H >> SY, W >> SX]) (views)."""
        rows, W = frame.shape
        H = self.height(rows)
        assert self.rows(H) == rows and not (W & self.sx) and not (H & self.sy) and layout in self.layouts and frame.dtype == self.dtype
        ch, cw = self.chroma_shape(H, W)
        flat = frame.reshape(-1)
        Y, c = flat[:H * W].reshape(H, W), flat[H * W:]
        if layout == self.layouts[0]:
            return Y, c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)
        c = c.reshape(ch, cw, 2)
        return Y, c[..., 0], c[..., 1]

    def pack(self, Y, Cb, Cr, layout):
        """Stored samples -> one frame."""
        H, W = Y.shape
        assert Cb.shape == Cr.shape == self.chroma_shape(H, W)
        c = np.concatenate([Cb.ravel(), Cr.ravel()]) if layout == self.layouts[0] else np.stack([Cb, Cr], -1).ravel()
        return np.concatenate([Y.ravel(), c]).astype(self.dtype).reshape(self.rows(H), W)

    def frames_view(self, alloc, case):
        n = case.B * self.samples(case.H, case.W)
        return alloc[self.guard:self.guard + n].reshape(case.B, self.rows(case.H), case.W)

    def designed_frames(self, b, h, w, seed, layout=None, general=False):
        """The frames of the tests.  4:2:0 has generators of its own, one per depth; general=True takes the one of the other subsamplings there too."""
        make = _designed_any if general or not self.sy else _designed_420_8 if self.depth == 8 else _designed_420_10
        return make(self, b, h, w, seed, layout or self.layouts[0])

    def new_frames_alloc(self, case, layout, seed, general=False):
        """[guard | the frame batch | guard] in whole 32-bit words (the cut reads aligned words), the payload 4-byte aligned when the allocation is."""
        n = case.B * self.samples(case.H, case.W)
        assert self.guard % self.per_word == 0
        size = -(-(2 * self.guard + n) // self.per_word) * self.per_word
        a = np.random.default_rng(seed).integers(0, 1 << 8 * self.dtype.itemsize, size, dtype=self.dtype)
        a[self.guard:self.guard + n] = self.designed_frames(case.B, case.H, case.W, seed, layout, general).ravel()
        return a

    # ---- the conversion in ----
    def samples_to_rgb(self, Y, Cb, Cr, matrix, full):
        """Codes of equal shape (chroma already replicated) -> float32 [..., 3]: the table look-up."""
        ty, tc = self.tables(full)
        return matrix_to_rgb(ty[Y], tc[Cb], tc[Cr], matrix)

    def yuv_in(self, frame, layout, matrix='bt709', full=False):
        """One frame -> float32 [H,W,3]: pixel (y, x) takes the chroma sample (y >> SY, x >> SX)."""
        Y, Cb, Cr = (self.code(p, layout) for p in self.unpack(np.ascontiguousarray(frame), layout))
        rep = lambda c: c.repeat(1 << self.sy, 0).repeat(1 << self.sx, 1)       # noqa: E731
        return self.samples_to_rgb(Y, rep(Cb), rep(Cr), matrix, full)

    def histogram(self, frame, layout):
        """int64 [3][256]: plane p's samples in bin code >> (depth - 8) (include/film_hip.h, "Scene cuts")."""
        return np.stack([np.bincount((self.code(p, layout).astype(np.int64) >> (self.depth - 8)).ravel(), minlength=256)
                         for p in self.unpack(np.ascontiguousarray(frame), layout)]).astype(np.int64)

    # ---- the conversion out ----
    def mean(self, c, fault=None):
        """The chroma mean of the subsampling, in the kernels' summation order."""
        box = lambda c: ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * F(0.25)       # noqa: E731
        if self.sy:
            return box(c)
        if self.sx:
            return box(c).repeat(2, 0) if fault == 'box_2x2_mean' else (c[:, 0::2] + c[:, 1::2]) * F(0.5)      # (the fault: even H only, both rows of a pair)
        return c

    def out_unquantised(self, rgb, matrix, full, fault=None):
        """float32 [H,W,3] -> the float32 values right before the quantiser: (Y [H,W], Cb, Cr [H >> SY, W >> SX])."""
        k = constants(matrix)
        x = _clip01(np.asarray(rgb, F))
        R, G, B = x[..., 0], x[..., 1], x[..., 2]
        Yf = (k['kr'] * R + k['kg'] * G) + k['kb'] * B
        cbf = (B - Yf) * k['s_b']
        crf = (R - Yf) * k['s_r']
        yo, ys, cs, mid = self._ranges(full)
        vals = Yf * ys + yo, self.mean(cbf, fault) * cs + mid, self.mean(crf, fault) * cs + mid
        assert all(v.dtype == F for v in vals)
        return vals

    def quantise(self, v):
        return (np.minimum(np.maximum(v, F(0)), F((1 << self.depth) - 1)) + F(0.5)).astype(self.dtype)

    def yuv_out(self, rgb, layout, matrix='bt709', full=False, fault=None):
        """float32 [H,W,3] -> one frame [rows, W]."""
        return self.pack(*[self.store(self.quantise(v), layout) for v in self.out_unquantised(rgb, matrix, full, fault)], layout)

    # ---- the cut ----
    def _rgb_of_samples(self, Y, Cb, Cr, layout, matrix, full, fault):
        """float32 RGB of gathered samples from the formulas (not the tables), with the faults that change a sample's value."""
        if fault == 'p010_as_i010' and layout == 'p010':
            layout = 'i010'
        elif fault == 'i010_as_p010' and layout == 'i010':
            layout = 'p010'
        if fault == 'bt709_under_bt2020' and matrix == 'bt2020nc':
            matrix = 'bt709'
        if fault == 'ignored_bits_not_masked':
            v = [p.astype(F) / F(64) if layout == 'p010' else p.astype(F) for p in (Y, Cb, Cr)]
        else:
            v = [self.code(p, layout).astype(F) for p in (Y, Cb, Cr)]
        return matrix_to_rgb(*self._values(*v, full, fault), matrix)

    def cut(self, frames, geo, tile0, ntiles, layout, matrix, full, fault=None):
        """Tiles [tile0, tile0 + ntiles) of the frame batch [B, rows, W] as float32 RGB [ntiles, TH, TW, 3] with +0.0 padding."""
        B, rows, W = frames.shape
        g = T._Geo(geo, (B, self.height(rows), W))
        out = np.zeros((ntiles, g.TH, g.TW, 3), F)
        for k in range(ntiles):
            b, ty, tx = g.tile(tile0 + k)
            sy, sx = g.ys[ty], g.xs[tx]
            Y, Cb, Cr = self.unpack(np.ascontiguousarray(frames[b]), self.layouts[0] if fault == 'nv12_as_i420' else layout)
            if fault == 'cb_cr_swapped':
                Cb, Cr = Cr, Cb
            yy, xx = sy + np.arange(g.eh), sx + np.arange(g.ew)
            cy, cx = yy >> self.sy, xx >> self.sx
            if fault == 'chroma_from_tile_coordinate':
                cy, cx = (sy >> self.sy) + (np.arange(g.eh) >> self.sy), (sx >> self.sx) + (np.arange(g.ew) >> self.sx)
            if fault == 'chroma_row_halved' and not self.sy:
                cy = yy >> 1
            if fault == 'chroma_col_halved' and not self.sx:
                cx = xx >> 1
            out[k, g.oy:g.oy + g.eh, g.ox:g.ox + g.ew] = self._rgb_of_samples(Y[yy][:, xx], Cb[cy][:, cx], Cr[cy][:, cx], layout, matrix, full, fault)
        return out

    def cut_via_frames(self, frames, geo, tile0, ntiles, layout, matrix, full):
        """The same through the frame-level conversion (table look-ups) and tile_map_ref's float cut: the two must agree."""
        rgb = np.stack([self.yuv_in(f, layout, matrix, full) for f in frames])
        return T.cut(rgb, geo, tile0, ntiles)

    def NumpyBackend(self, geo_of, fault=None):
        """The restatement as a backend, with at most one of FAULTS planted."""
        assert fault is None or fault in FAULTS

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
        16-byte aligned and a frame batch whose first sample is 4-byte aligned.  Addresses count samples from the batch's first, pw to a
        32-bit word.  The names grew with the layouts and tests assert on them: 4:2:0 says whether Y's words are aligned and names the words
        of Cb alone; the other subsamplings count the words of Y, Cb and Cr and name what 4:2:0 cannot meet."""
        g = T._Geo(geo, (case.B, case.H, case.W))
        semi, pw, S, plane = layout != self.layouts[0], self.per_word, self.samples(case.H, case.W), case.H * case.W
        ch, cw = self.chroma_shape(case.H, case.W)
        count = ('no', 'one', 'two', 'three')
        words_of = lambda a, n: (a % pw + n + pw - 1) // pw       # noqa: E731  (32-bit words that hold samples [a, a + n))
        plural = lambda n: 's' if n > 1 else ''                   # noqa: E731
        out = {f'frame_yuv_to_tiles_kernel<{"true" if g.ovy | g.ovx else "false"}, FILM_PIX_{layout.upper()}>'}
        row, groups = g.TW * 3, (g.TW + 3) // 4
        for k in range(ntiles):
            b, ty, tx = g.tile(tile0 + k)
            if g.ys[ty] & 1: out.add('odd row origin')
            if g.xs[tx] & 1: out.add('odd column origin')
            if not self.sy and (b * S) % pw: out.add('frame starts off a word boundary')
            for y in range(g.TH):
                r = k * g.TH + y
                sy = y - g.oy
                for q in range(groups):
                    xp0 = q * 4
                    s0 = xp0 - g.ox
                    if 0 <= sy < g.eh and s0 + 4 > 0 and s0 < g.ew:
                        fy, fx = g.ys[ty] + sy, g.xs[tx] + s0
                        if self.sx and not self.sy and fy & 1: out.add('chroma from row fy (an odd row)')
                        if s0 >= 0 and s0 + 4 <= g.ew:
                            ya = b * S + fy * g.W + fx
                            n = words_of(ya, 4)
                            if not self.sy:
                                out.add(f'word path, Y in {count[n]} word{plural(n)}')
                            else:
                                out.add(f'word path, Y in {count[n]} aligned word{plural(n)}' if ya % pw == 0 else f'word path, Y across {count[n]} words')
                            out.add('word path, four chroma samples' if not self.sx else
                                    'word path, odd column: three chroma samples' if fx & 1 else 'word path, even column: two chroma samples')
                            c0 = fx >> self.sx
                            nc = ((fx + 3) >> self.sx) - c0 + 1
                            if semi and pw == 2:      # a CbCr pair IS a word: the kernel reads the pair words themselves
                                out.add(f'word path, {"three" if nc == 3 else "two"} CbCr pair words')
                            else:
                                ca = b * S + plane + ((fy >> self.sy) * cw + c0) * (1 + semi)
                                for a in (ca,) if self.sy else (ca, ca + ch * cw):
                                    n = words_of(a, nc * (1 + semi))
                                    out.add(f'word path, chroma in {count[n]} word{plural(n)}' if not self.sy or n == 1 else 'word path, chroma across two words')
                        else:
                            out.add(f'{self.sample} path')
                    else:
                        out.add('padding group')
                    vec = xp0 * 3 + 12 <= row and (r * row + xp0 * 3) % 4 == 0
                    out.add('vector stores' if vec else 'scalar stores')
        return out

    def out_branches(self, h, w, layout, dst_offset=0):
        """The same for rgb_to_yuv_kernel on an h x w frame whose dst lies dst_offset BYTES (whole samples) behind a 4-byte boundary (src
        16-byte aligned).  A block is two rows by eight pixels; 4:2:0 stores one chroma row per block, the others one per row."""
        assert dst_offset % self.dtype.itemsize == 0
        o, pw = dst_offset // self.dtype.itemsize, self.per_word
        ch, cw = self.chroma_shape(h, w)
        out = {f'rgb_to_yuv_kernel<FILM_PIX_{layout.upper()}>'}
        for y0 in range(0, h, 2):
            rows = min(2, h - y0)
            if not self.sy: out.add('block of two rows' if rows == 2 else 'odd block row: one row')
            for x0 in range(0, w, 8):
                n = min(8, w - x0)
                if n & 1: out.add('odd pixel count per row')
                for dy in range(rows):
                    out.add('vector loads' if n == 8 and (((y0 + dy) * w + x0) * 12) % 16 == 0 else 'scalar loads')
                    out.add('Y word stores' if n == 8 and (o + (y0 + dy) * w + x0) % pw == 0 else f'Y {self.sample} stores')
                    if self.sy and dy:
                        continue
                    if layout != self.layouts[0]:      # semi-planar: one row of CbCr pairs
                        ok = n == 8 and (o + h * w + (y0 >> 1) * w + x0) % pw == 0
                    else:
                        a = o + h * w + ((y0 + dy) >> self.sy) * cw + (x0 >> self.sx)
                        ok = n == 8 and a % pw == 0 and (a + ch * cw) % pw == 0
                    out.add('chroma word stores' if ok else f'chroma {self.sample} stores')
        return out


FORMATS = {layout: fmt for fmt in (Format(*key) for key in LAYOUTS_OF) for layout in fmt.layouts}      # 'i420' ... 'i410' -> its Format
assert set(FORMATS) == set(NEW_LAYOUTS + OLD_LAYOUTS)


def convert_layout(frame, src, dst):
    """One frame in another layout of its format (I420 <-> NV12, I010 <-> P010): the same codes, the ignored bits zero."""
    f = FORMATS[src]
    return f.pack(*[f.store(f.code(p, src), dst) for p in f.unpack(np.ascontiguousarray(frame), src)], dst)


def cases_of(layout):
    """The geometries of the cut test for a 4:2:2 or 4:4:4 layout: CASES (even sizes) and the subsampling's own."""
    return list(CASES) + (CASES_422 if FORMATS[layout].sx else CASES_444)


# ---- what the GPU test of film_to_yuv runs (tests/test_yuv_chroma_cpu.py shows which kernel branches these reach) ----------------------------
OUT_OFFSETS = (0, 1)      # film_to_yuv's dst: on a 4-byte boundary, and this many SAMPLES behind it


def out_sizes(layout):
    """The (h, w) of the film_to_yuv test: even sizes for every layout; an odd H where the layout has no vertical subsampling; an odd W for 4:4:4."""
    f = FORMATS[layout]
    return [(2, 2), (16, 18), (30, 50)] + ([] if f.sy else [(1, 2), (31, 50)]) + ([] if f.sx else [(1, 1), (31, 49)])


def smallest(layout):
    f = FORMATS[layout]
    return (2, 2) if f.sy else (1, 2) if f.sx else (1, 1)
