"""Numpy restatement of the 10-bit Y'CbCr 4:2:0 arithmetic of include/film_hip.h ("The 10-bit 4:2:0 arithmetic"): the code of a stored
word, the conversion in (words -> float32 RGB, what the 10-bit instances of frame_yuv_to_tiles_kernel of csrc/frame_kernels.hip fuse into
the tile cut), the conversion out (float32 RGB -> words, rgb_to_yuv_kernel there), I010 <-> P010, the cut of a 10-bit frame batch into tiles
over the geometry film_tiling_json reports, and the histogram of a 10-bit frame.  This module states what is 10-bit: the code rule, the
tables, the formulas on gathered words with their planted faults, the designed frames.  The plane bookkeeping, the conversions around them,
the cut, its comparison and the kernels' branches are tests/yuv_ref.py's Format, instantiated at the end and exported under the plain
names; the matrix constants, the cases and the tile ranges are that module's too, the tile bookkeeping tests/tile_map_ref.py's.  Every
operation is float32 with one rounding (numpy does not fuse), so every comparison against the kernels is on the bits.

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
from yuv_ref import CASES, COLOURS, Format, constants, matrix_to_rgb, ranges_of      # noqa: F401  (the cases and ranges of the 8-bit cut test, re-exported)

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


def convert_layout(frame, src, dst):
    """I010 <-> P010 of one frame: the same codes, the ignored bits zero."""
    return pack(*[store(code(p, src), dst) for p in unpack(np.ascontiguousarray(frame), src)], dst)


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
    return matrix_to_rgb(y, cb, cr, matrix)


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


# ---- the shared restatement (yuv_ref.Format) on 10-bit codes, under this module's names ---------------------------------------------------
_FMT = Format(10, GUARD_U16, LAYOUTS, FAULTS, 'sample', tables, designed_frames, code, store, _rgb_of_words)
unpack, pack, frames_view, new_frames_alloc = _FMT.unpack, _FMT.pack, _FMT.frames_view, _FMT.new_frames_alloc
samples_to_rgb, yuv_in, out_unquantised, yuv_out = _FMT.samples_to_rgb, _FMT.yuv_in, _FMT.out_unquantised, _FMT.yuv_out
cut, cut_via_frames, NumpyBackend, check_cut = _FMT.cut, _FMT.cut_via_frames, _FMT.NumpyBackend, _FMT.check_cut
branches, out_branches = _FMT.branches, _FMT.out_branches
