"""Numpy restatement of the Y'CbCr arithmetic of include/film_hip.h over (depth, SX, SY, matrix): "The 4:2:2 and 4:4:4 arithmetic" for the planar
layouts I422 / I444 (8-bit) and I210 / I410 (10-bit codes in bits 0-9 of 16-bit words), and the BT.2020 non-constant-luminance matrix
('bt2020nc') for every layout, the six older ones included.  SubFormat is tests/yuv_ref.py's Format with what the chroma shifts (SX, SY) decide
overridden: the plane bookkeeping, the replication in, the mean out, the cut, the branches of the kernels; and with constants of its own that
know the third matrix.  (SX, SY) = (1, 1) is 4:2:0 - there it restates what yuv_ref / yuv10_ref state, which tests/test_yuv_chroma_cpu.py
checks - (1, 0) is 4:2:2, (0, 0) is 4:4:4.  Every operation is float32 with one rounding (numpy does not fuse), so every comparison against the
kernels is on the bits.

A frame is an array [rows, W] of samples: rows [0, H) are the Y plane, behind it Cb [H >> SY][W >> SX] and Cr [H >> SY][W >> SX] (or, 4:2:0
semi-planar, the CbCr pairs): rows = H * 3 // 2, 2 * H or 3 * H.

FORMATS maps every layout name to its SubFormat; a "backend" of check_cut is what yuv_ref describes.
"""
import numpy as np

import tile_map_ref as T
import yuv10_ref as R10
import yuv_ref as R8
from yuv_ref import Case, Format, ranges_of      # noqa: F401

F = np.float32
MATRICES = ('bt709', 'bt601', 'bt2020nc')
COLOURS = [(m, f) for m in MATRICES for f in (False, True)]      # the six colour settings
KR_KB = dict(R8.KR_KB, bt2020nc=(0.2627, 0.0593))
NEW_LAYOUTS = ('i422', 'i444', 'i210', 'i410')
OLD_LAYOUTS = ('i420', 'nv12', 'i010', 'p010')

# the faults a SubFormat can plant: in the cut (where it gathers its samples and which constants it takes) and in the mean of the way out
FAULTS = ('chroma_row_halved',                # 4:2:2 reads chroma row fy >> 1, as 4:2:0 does
          'chroma_col_halved',                # 4:4:4 reads chroma column fx >> 1
          'chroma_from_tile_coordinate',      # the pairing counted from the tile's first row / column
          'cb_cr_swapped',
          'bt709_under_bt2020',               # BT.709 constants under the BT.2020 flag
          'box_2x2_mean')                     # out: the 2 x 2 mean of 4:2:0 where 4:2:2 takes the 1 x 2 mean (the chroma rows are then pairwise equal)

# the geometries of the cut test beyond yuv_ref.CASES: the smallest shapes at which the new paths can go wrong
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


def constants(matrix):
    """The float32 constants of a matrix: computed in double from (Kr, Kb), rounded once (yuv_ref.constants with the third matrix)."""
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


def designed_rgb(h, w, seed):
    """float32 [h,w,3] in [-0.2, 1.2] with exact 0 and 1 and values below 0 and above 1: the source of the film_to_yuv test."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (h, w, 3)).astype(F)
    x[0, 0] = (0, 1, -3)
    x[-1, -1] = (7, 0.5, 1) if h * w > 1 else (7, 0.5, -3)      # (one pixel: above 1 and below 0 in one)
    return x


class SubFormat(Format):
    def __init__(self, depth, sx, sy):
        assert (sx, sy) in ((1, 1), (1, 0), (0, 0))
        base = R8 if depth == 8 else R10
        if sy:
            layouts = base.LAYOUTS
        else:
            layouts = ({(8, 1): 'i422', (8, 0): 'i444', (10, 1): 'i210', (10, 0): 'i410'}[depth, sx],)
        self.sx, self.sy = sx, sy
        super().__init__(depth, T.GUARD_U8 if depth == 8 else R10.GUARD_U16, layouts, FAULTS, 'byte' if depth == 8 else 'sample', base.tables,
                         self._designed_frames, *((R10.code, R10.store) if depth == 10 else ()), rgb_of_samples=self._rgb_of_samples)

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
        H, W = Y.shape
        assert Cb.shape == Cr.shape == self.chroma_shape(H, W)
        c = np.concatenate([Cb.ravel(), Cr.ravel()]) if layout == self.layouts[0] else np.stack([Cb, Cr], -1).ravel()
        return np.concatenate([Y.ravel(), c]).astype(self.dtype).reshape(self.rows(H), W)

    def frames_view(self, alloc, case):
        n = case.B * self.samples(case.H, case.W)
        return alloc[self.guard:self.guard + n].reshape(case.B, self.rows(case.H), case.W)

    def new_frames_alloc(self, case, layout, seed):
        n = case.B * self.samples(case.H, case.W)
        assert self.guard % self.per_word == 0
        size = -(-(2 * self.guard + n) // self.per_word) * self.per_word
        a = np.random.default_rng(seed).integers(0, 1 << 8 * self.dtype.itemsize, size, dtype=self.dtype)
        a[self.guard:self.guard + n] = self.designed_frames(case.B, case.H, case.W, seed, layout).ravel()
        return a

    def _designed_frames(self, b, h, w, seed, layout):
        """b frames whose planes hold every code where a plane has room for them (a rolled ramp, strided where it has not), the extremes of
        the 10-bit ranges at the end of a plane, random codes elsewhere; a 10-bit frame carries random junk in the bits the layout ignores."""
        rng = np.random.default_rng(seed)
        codes = 1 << self.depth
        ch, cw = self.chroma_shape(h, w)
        out = []
        for i in range(b):
            planes = []
            for pi, n in enumerate((h * w, ch * cw, ch * cw)):
                p = rng.integers(0, codes, n)
                m = min(n, codes)
                rolled = np.roll(np.arange(codes), (codes // 6) * pi + 7 * i)
                start = min(17 * i + 5, n - m)
                p[start:start + m] = rolled if m == codes else rolled[np.arange(m) * codes // m]
                if self.depth == 10 and n > codes + 64:
                    p[n - len(R10.EXTREMES):] = np.roll(R10.EXTREMES, -3 * i - 7 * pi)
                planes.append(p)
            fr = self.pack(self.store(planes[0].reshape(h, w), layout), self.store(planes[1].reshape(ch, cw), layout), self.store(planes[2].reshape(ch, cw), layout), layout)
            out.append(self.with_junk(fr, layout, seed * 31 + i))
        return np.stack(out)

    def with_junk(self, frame, layout, seed):
        """The same codes with random bits where a 10-bit layout ignores them (an 8-bit frame has no such bits)."""
        if self.depth == 8:
            return frame
        j = np.random.default_rng(seed).integers(0, 64, frame.shape).astype(np.uint16)
        return (self.store(self.code(frame, layout), layout) | (j if layout == 'p010' else (j << 10))).astype(np.uint16)

    def histogram(self, frame, layout):
        """int64 [3][256]: plane p's samples in bin code >> (depth - 8)."""
        return np.stack([np.bincount((self.code(p, layout).astype(np.int64) >> (self.depth - 8)).ravel(), minlength=256)
                         for p in self.unpack(np.ascontiguousarray(frame), layout)]).astype(np.int64)

    # ---- the conversions ----
    def samples_to_rgb(self, Y, Cb, Cr, matrix, full):
        ty, tc = self.tables(full)
        return matrix_to_rgb(ty[Y], tc[Cb], tc[Cr], matrix)

    def _rgb_of_samples(self, Y, Cb, Cr, layout, matrix, full, fault):
        if fault == 'bt709_under_bt2020' and matrix == 'bt2020nc':
            matrix = 'bt709'
        return self.samples_to_rgb(*(self.code(p, layout) for p in (Y, Cb, Cr)), matrix, full)

    def yuv_in(self, frame, layout, matrix='bt709', full=False):
        """One frame -> float32 [H,W,3]: pixel (y, x) takes the chroma sample (y >> SY, x >> SX)."""
        Y, Cb, Cr = (self.code(p, layout) for p in self.unpack(np.ascontiguousarray(frame), layout))
        rep = lambda c: c.repeat(1 << self.sy, 0).repeat(1 << self.sx, 1)       # noqa: E731
        return self.samples_to_rgb(Y, rep(Cb), rep(Cr), matrix, full)

    def mean(self, c, fault=None):
        """The chroma mean of the subsampling, in the kernels' summation order."""
        if self.sy:
            return ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * F(0.25)
        if self.sx:
            if fault == 'box_2x2_mean':      # (even H only) the 2 x 2 mean, written to both rows of the pair
                return (((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * F(0.25)).repeat(2, 0)
            return (c[:, 0::2] + c[:, 1::2]) * F(0.5)
        return c

    def out_unquantised(self, rgb, matrix, full, fault=None):
        k = constants(matrix)
        x = _clip01(np.asarray(rgb, F))
        R, G, B = x[..., 0], x[..., 1], x[..., 2]
        Yf = (k['kr'] * R + k['kg'] * G) + k['kb'] * B
        cbf = (B - Yf) * k['s_b']
        crf = (R - Yf) * k['s_r']
        top, s = (1 << self.depth) - 1, 1 << (self.depth - 8)
        ys, yo, cs = (F(top), F(0), F(top)) if full else (F(219 * s), F(16 * s), F(224 * s))
        vals = Yf * ys + yo, self.mean(cbf, fault) * cs + F(128 * s), self.mean(crf, fault) * cs + F(128 * s)
        assert all(v.dtype == F for v in vals)
        return vals

    def yuv_out(self, rgb, layout, matrix='bt709', full=False, fault=None):
        return self.pack(*[self.store(self.quantise(v), layout) for v in self.out_unquantised(rgb, matrix, full, fault)], layout)

    # ---- the cut ----
    def cut(self, frames, geo, tile0, ntiles, layout, matrix, full, fault=None):
        B, rows, W = frames.shape
        H = self.height(rows)
        g = T._Geo(geo, (B, H, W))
        out = np.zeros((ntiles, g.TH, g.TW, 3), F)
        for k in range(ntiles):
            b, ty, tx = g.tile(tile0 + k)
            sy, sx = g.ys[ty], g.xs[tx]
            Y, Cb, Cr = self.unpack(np.ascontiguousarray(frames[b]), layout)
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
            out[k, g.oy:g.oy + g.eh, g.ox:g.ox + g.ew] = self.rgb_of_samples(Y[yy][:, xx], Cb[cy][:, cx], Cr[cy][:, cx], layout, matrix, full, fault)
        return out

    # ---- which branches of the kernels a call takes (restates the kernels' own conditions) ----
    def branches(self, case, geo, layout, tile0, ntiles):
        """As Format.branches, for any (SX, SY): addresses count samples from the batch's first sample (4-byte aligned), pw to a 32-bit word."""
        if self.sy:
            return super().branches(case, geo, layout, tile0, ntiles)
        g = T._Geo(geo, (case.B, case.H, case.W))
        pw, S, plane = self.per_word, self.samples(case.H, case.W), case.H * case.W
        cplane, cw = (case.H * case.W) >> self.sx, case.W >> self.sx
        count = ('no', 'one', 'two', 'three')
        out = {f'frame_yuv_to_tiles_kernel<{"true" if g.ovy | g.ovx else "false"}, FILM_PIX_{layout.upper()}>'}
        row, groups = g.TW * 3, (g.TW + 3) // 4
        for k in range(ntiles):
            b, ty, tx = g.tile(tile0 + k)
            if g.ys[ty] & 1: out.add('odd row origin')
            if g.xs[tx] & 1: out.add('odd column origin')
            if (b * S) % pw: out.add('frame starts off a word boundary')
            for y in range(g.TH):
                r = k * g.TH + y
                sy = y - g.oy
                for q in range(groups):
                    xp0 = q * 4
                    s0 = xp0 - g.ox
                    if 0 <= sy < g.eh and s0 + 4 > 0 and s0 < g.ew:
                        fy, fx = g.ys[ty] + sy, g.xs[tx] + s0
                        if self.sx and fy & 1: out.add('chroma from row fy (an odd row)')
                        if s0 >= 0 and s0 + 4 <= g.ew:
                            ya = b * S + fy * g.W + fx
                            words = (ya % pw + 4 + pw - 1) // pw
                            out.add(f'word path, Y in {count[words]} word{"s" if words > 1 else ""}')
                            c0 = fx >> self.sx
                            nc = ((fx + 3) >> self.sx) - c0 + 1
                            out.add('word path, four chroma samples' if not self.sx else
                                    'word path, odd column: three chroma samples' if fx & 1 else 'word path, even column: two chroma samples')
                            for name, ca in (('Cb', b * S + plane + fy * cw + c0), ('Cr', b * S + plane + cplane + fy * cw + c0)):
                                words = (ca % pw + nc + pw - 1) // pw
                                out.add(f'word path, chroma in {count[words]} word{"s" if words > 1 else ""}')
                        else:
                            out.add(f'{self.sample} path')
                    else:
                        out.add('padding group')
                    vec = xp0 * 3 + 12 <= row and (r * row + xp0 * 3) % 4 == 0
                    out.add('vector stores' if vec else 'scalar stores')
        return out

    def out_branches(self, h, w, layout, dst_offset=0):
        if self.sy:
            return super().out_branches(h, w, layout, dst_offset)
        assert dst_offset % self.dtype.itemsize == 0
        o, pw = dst_offset // self.dtype.itemsize, self.per_word
        cw, cplane = w >> self.sx, (h * w) >> self.sx
        out = {f'rgb_to_yuv_kernel<FILM_PIX_{layout.upper()}>'}
        for y0 in range(0, h, 2):
            rows = min(2, h - y0)
            out.add('block of two rows' if rows == 2 else 'odd block row: one row')
            for x0 in range(0, w, 8):
                n = min(8, w - x0)
                if n & 1: out.add('odd pixel count per row')
                for dy in range(rows):
                    out.add('vector loads' if n == 8 and (((y0 + dy) * w + x0) * 12) % 16 == 0 else 'scalar loads')
                    out.add('Y word stores' if n == 8 and (o + (y0 + dy) * w + x0) % pw == 0 else f'Y {self.sample} stores')
                    a = o + h * w + (y0 + dy) * cw + (x0 >> self.sx)
                    ok = n == 8 and a % pw == 0 and (a + cplane) % pw == 0
                    out.add('chroma word stores' if ok else f'chroma {self.sample} stores')
        return out


_BY_KEY = {(d, sx, sy): SubFormat(d, sx, sy) for d in (8, 10) for sx, sy in ((1, 1), (1, 0), (0, 0))}
FORMATS = {layout: fmt for fmt in _BY_KEY.values() for layout in fmt.layouts}      # 'i420' ... 'i410' -> its SubFormat
assert set(FORMATS) == set(NEW_LAYOUTS + OLD_LAYOUTS)


def cases_of(layout):
    """The geometries of the cut test for a new layout: yuv_ref.CASES (even sizes) and the layout's own."""
    return list(R8.CASES) + (CASES_422 if FORMATS[layout].sx else CASES_444)


# ---- what the GPU test runs (tests/test_yuv_chroma_cpu.py shows which kernel branches these reach) ----------------------------------------------
OUT_OFFSETS = (0, 1)      # film_to_yuv's dst: on a 4-byte boundary, and this many SAMPLES behind it


def out_sizes(layout):
    """The (h, w) of the film_to_yuv test: even sizes for every layout; an odd H where the layout has no vertical subsampling; an odd W for 4:4:4."""
    f = FORMATS[layout]
    return [(2, 2), (16, 18), (30, 50)] + ([] if f.sy else [(1, 2), (31, 50)]) + ([] if f.sx else [(1, 1), (31, 49)])


def smallest(layout):
    f = FORMATS[layout]
    return (2, 2) if f.sy else (1, 2) if f.sx else (1, 1)
