"""Numpy restatement of the frame <-> tile kernels (csrc/frame_kernels.hip: frame_to_tiles_kernel<false / true>,
frame_u8_to_tiles_kernel<false / true>, tiles_to_frame_kernel, blend_tiles_kernel) and the comparison that tests/test_tile_map_gpu.py
runs film_debug_tile_map through.  The arithmetic is specified to the bit (include/film_hip.h, "block_overlap_h"; the comment above
blend_tiles_kernel), so every comparison here is on uint32 views.

The geometry comes ONLY from the dict film_tiling_json returns (FilmEngine.tiling) and the shape of the frame batch.

A "backend" is what the comparison drives: a callable
    backend(mode, u8, frames_alloc, tiles_alloc, case, tile0, ntiles) -> (frames_alloc', tiles_alloc')
that takes the two whole allocations (guard | payload | guard, numpy arrays it must not modify) and returns them as they are after ONE
cut (mode 'cut') or join ('join') of tiles [tile0, tile0 + ntiles).  The GPU test's backend uploads both, calls film_debug_tile_map and
downloads both; NumpyBackend applies the restatement - optionally with one of FAULTS planted, which tests/test_tile_map_cpu.py uses to
show that the comparison on the designed data finds each of them.
"""
import collections

import numpy as np

GUARD = 64          # floats of guard band on each side of a float32 payload
GUARD_U8 = 16       # bytes of guard band on each side of an 8-bit frame batch (the payload stays 4-byte aligned)

Case = collections.namedtuple('Case', 'name B H W block align overlap')

# (B, H, W, block, align) x overlaps: the smallest geometries at which each index expression of the kernels can go wrong
_GEOMETRIES = [
    ('g1', 2, 30, 42, (3, 2), 8, [(0, 0), (3, 5), (5, 10), (-1, -1)]),   # 10 x 21 patches, 126-byte rows; (5, 10): 2 o = p on y; -1 -> (3, 1)
    ('g2', 1, 36, 35, (3, 5), 8, [(6, 3)]),                              # nine tiles cover some pixels; 105-byte rows
    ('g3', 1, 40, 63, (4, 3), None, [(5, 10), (0, 0)]),                  # 20 x 41 tiles: a tile row of 123 floats (no multiple of 12, of 4)
    ('g4', 3, 24, 40, (1, 4), 8, [(7, 5)]),                              # one block row: its overlap resolves to 0
    ('g5', 1, 20, 22, (2, 2), 64, [(1, 1)]),                             # 12 x 13 content at (26, 25) of a 64 x 64 tile: mostly padding
    ('g6', 2, 70, 101, None, 64, [(0, 0)]),                              # untiled, offsets (29, 13) in 128 x 128; 303-byte rows
]
CASES = [Case(f'{n}-ov{o[0]}x{o[1]}', b, h, w, blk, al, o) for n, b, h, w, blk, al, ovs in _GEOMETRIES for o in ovs]

# what the issue pins of the resolved geometry (on top of expected_geometry below)
PINNED = {
    'g1-ov-1x-1': {'overlap_h': 3, 'overlap_w': 1},
    'g1-ov0x0': {'tile_h': 10, 'tile_w': 21},
    'g1-ov5x10': {'tile_h': 20, 'origins_y': [0, 5, 10]},
    'g3-ov5x10': {'tile_h': 20, 'tile_w': 41, 'padded_w': 41},
    'g4-ov7x5': {'overlap_h': 0, 'overlap_w': 5},
    'g5-ov1x1': {'tile_h': 12, 'tile_w': 13, 'padded_h': 64, 'padded_w': 64, 'pad_y': 26, 'pad_x': 25},
    'g6-ov0x0': {'padded_h': 128, 'padded_w': 128, 'pad_y': 29, 'pad_x': 13},
}


def blocks(case):
    return tuple(case.block) if case.block else (1, 1)


def axis_geometry(n, nb, o, align):
    """One axis of the definition: content e, padded size, pad offset, resolved overlap, origins."""
    p = n // nb; assert n == p * nb
    pad0 = (align - p % align) % align if align else 0
    if nb == 1: o = 0
    elif o < 0: o = min(pad0 // 2, p // 2)
    assert 0 <= 2 * o <= p
    e = p + 2 * o
    E = e + ((align - e % align) % align if align else 0)
    return e, E, (E - e) // 2, o, [min(max(i * p - o, 0), n - e) for i in range(nb)]


def expected_geometry(case):
    """What film_tiling_json must report for the case (the definition restated, as tests/test_overlap_cpu.py::axis does)."""
    bh, bw = blocks(case)
    eh, EH, py, oh, ys = axis_geometry(case.H, bh, case.overlap[0], case.align)
    ew, EW, px, ow, xs = axis_geometry(case.W, bw, case.overlap[1], case.align)
    return {'overlap_h': oh, 'overlap_w': ow, 'tile_h': eh, 'tile_w': ew, 'padded_h': EH, 'padded_w': EW, 'pad_y': py, 'pad_x': px,
            'origins_y': ys, 'origins_x': xs}


def partitions(total, T):
    """The tile ranges of the issue as {name: [(tile0, ntiles), ...]}: one range, single tiles, ranges of 4, T - 1 tiles then the rest."""
    out = {'one': [(0, total)], 'singles': [(n, 1) for n in range(total)],
           'fours': [(n, min(4, total - n)) for n in range(0, total, 4)]}
    if 1 <= T - 1 < total:
        out['T-1+rest'] = [(0, T - 1), (T - 1, total - (T - 1))]
    return out


# ---- designed data ------------------------------------------------------------------------------------------------------------------
def designed_floats(n, seed):
    """n finite float32 of both signs and two magnitudes (1 and 1e3), no zeros, every float distinct."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    v = np.where(np.abs(v) < 1e-3, np.float32(1e-3) * np.where(v < 0, -1, 1), v).astype(np.float32)
    v = (v * np.where(rng.random(n) < 0.5, np.float32(1), np.float32(1e3))).astype(np.float32)
    while True:
        _, first = np.unique(v.view(np.uint32), return_index=True)
        if first.size == n:
            break
        dup = np.setdiff1d(np.arange(n), first)
        v[dup] = np.nextafter(v[dup], np.float32(np.inf) * np.sign(v[dup]))
    assert np.isfinite(v).all() and (v != 0).all() and (v > 0).any() and (v < 0).any()
    return v


def designed_u8(b, h, w, seed):
    """b uint8 frames that hold every byte value in every channel (a ramp over pixels of each frame, as tests/test_stream_gpu.py::_frames_u8)."""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    ramp = np.arange(256, dtype=np.uint8)
    for i in range(b):
        flat = fr[i].reshape(-1, 3)
        for c in range(3):
            flat[17 * i + 5:17 * i + 5 + 256, c] = np.roll(ramp, 40 * c + i)
    assert all(len(np.unique(fr[i, ..., c])) == 256 for i in range(b) for c in range(3))
    return fr


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
FAULTS = ('origin_not_clamped', 'wy_wx_exchanged', 'normalised_over_both_axes', 'sum_restarts', 'padding_kept', 'oy_ox_exchanged',
          'read_one_pixel_off', 'frame_index_dropped', 'u8_row_one_byte_off', 'fma')


class _Geo:
    def __init__(self, geo, shape, fault=None):
        self.B, self.H, self.W = shape[:3]
        self.ys, self.xs = list(geo['origins_y']), list(geo['origins_x'])
        self.bh, self.bw = len(self.ys), len(self.xs)
        self.T = self.bh * self.bw
        self.ph, self.pw = self.H // self.bh, self.W // self.bw
        self.eh, self.ew, self.TH, self.TW = geo['tile_h'], geo['tile_w'], geo['padded_h'], geo['padded_w']
        self.oy, self.ox, self.ovy, self.ovx = geo['pad_y'], geo['pad_x'], geo['overlap_h'], geo['overlap_w']
        if fault == 'origin_not_clamped':      # s = i p - o for the last tile of an axis too (the first one stays at 0)
            self.ys[-1] = max((self.bh - 1) * self.ph - self.ovy, 0)
            self.xs[-1] = max((self.bw - 1) * self.pw - self.ovx, 0)

    def tile(self, n):
        b, t = divmod(n, self.T)
        return (b,) + divmod(t, self.bw)


def _fade(s, e, n):
    """a_i over the whole axis for the tile at origin s: the distance to the nearest interior edge counted from 1, 0 outside the tile."""
    a = np.zeros(n, np.float32)
    y = np.arange(s, min(s + e, n))
    d = np.full(y.size, 1 << 30, np.int64)
    if s > 0: d = np.minimum(d, y - s + 1)
    if s + e < n: d = np.minimum(d, s + e - y)
    a[y] = d
    return a


def _frame_values(frames):
    if frames.dtype == np.uint8:
        return frames.astype(np.float32) / np.float32(255)
    assert frames.dtype == np.float32
    return frames


def cut(frames, geo, tile0, ntiles, fault=None, into=None):
    """Tiles [tile0, tile0 + ntiles) of the frame batch [B,H,W,3] (float32, or uint8 read as float32(byte) / float32(255)) as
    [ntiles, TH, TW, 3] float32 with zero padding.  (`into`: what the tile buffer held before - read by the 'padding_kept' fault only.)"""
    g = _Geo(geo, frames.shape, fault)
    x = _frame_values(frames)
    if fault == 'u8_row_one_byte_off' and frames.dtype == np.uint8:
        flat = np.concatenate([x.ravel()[1:], x.ravel()[:1]])       # the frame as read one byte further on
    out = np.zeros((ntiles, g.TH, g.TW, 3), np.float32)
    if fault == 'padding_kept':
        out = np.array(into[:ntiles], np.float32)
    for k in range(ntiles):
        b, ty, tx = g.tile(tile0 + k)
        if fault == 'frame_index_dropped':
            b = 0
        sy, sx = g.ys[ty], g.xs[tx]
        eh, ew = min(g.eh, g.H - sy), min(g.ew, g.W - sx)           # (content past the frame: only with 'origin_not_clamped')
        src = x[b, sy:sy + eh, sx:sx + ew]
        if fault == 'u8_row_one_byte_off' and frames.dtype == np.uint8:
            src = np.array(src)
            for r in range(eh):
                start = ((b * g.H + sy + r) * g.W + sx) * 3
                if start % 4:
                    src[r] = flat[start:start + ew * 3].reshape(ew, 3)
        out[k, g.oy:g.oy + g.eh, g.ox:g.ox + g.ew] = 0
        out[k, g.oy:g.oy + eh, g.ox:g.ox + ew] = src
    return out


def covered(shape, geo, tile0, ntiles):
    """bool [B,H,W]: the frame pixels that a tile of [tile0, tile0 + ntiles) covers."""
    g = _Geo(geo, shape)
    m = np.zeros(shape[:3], bool)
    for n in range(tile0, tile0 + ntiles):
        b, ty, tx = g.tile(n)
        m[b, g.ys[ty]:g.ys[ty] + g.eh, g.xs[tx]:g.xs[tx] + g.ew] = True
    return m


def join(frames, tiles, geo, tile0, ntiles, fault=None):
    """The frame batch after joining tiles[0 : ntiles] = tiles [tile0, tile0 + ntiles) of the batch into it (frames is not modified).
    Overlap 0: the patches are pasted.  Else the cross-fade, per covering tile in row-major order: wy = a_i(y) / sum_y, wx = a_j(x) / sum_x,
    w = wy * wx, t = w * v, acc = t for the first covering tile of the WHOLE frame, else acc + t - a range that starts behind a pixel's
    first covering tile goes on from the value in the frame.  One float32 rounding per operation."""
    g = _Geo(geo, frames.shape, fault)
    out = np.array(frames, np.float32)
    flat = np.ascontiguousarray(tiles, np.float32).reshape(-1)
    tile_floats = g.TH * g.TW * 3

    def read(k, eh, ew):       # content [eh, ew, 3] of tile k of the buffer, by flat index as the kernel forms it
        oy, ox = (g.ox, g.oy) if fault == 'oy_ox_exchanged' else (g.oy, g.ox)
        if fault == 'read_one_pixel_off':
            ox += 1
        idx = ((k * g.TH + oy + np.arange(eh)[:, None, None]) * g.TW + ox + np.arange(ew)[None, :, None]) * 3 + np.arange(3)[None, None, :]
        return flat[idx % (ntiles * tile_floats)]

    ay = [_fade(s, g.eh, g.H) for s in g.ys]
    ax = [_fade(s, g.ew, g.W) for s in g.xs]
    sum_y, sum_x = np.sum(ay, 0, dtype=np.float32), np.sum(ax, 0, dtype=np.float32)
    seen = np.zeros(frames.shape[:3], bool)        # covered by an earlier tile of the frame, in this range or not
    for n in range((tile0 // g.T) * g.T, tile0 + ntiles):
        b, ty, tx = g.tile(n)
        sy, sx = g.ys[ty], g.xs[tx]
        eh, ew = min(g.eh, g.H - sy), min(g.ew, g.W - sx)
        sl = (b, slice(sy, sy + eh), slice(sx, sx + ew))
        if n >= tile0:
            k = n - tile0
            if fault == 'frame_index_dropped':
                k = (n % g.T - tile0) % ntiles
            v = read(k, eh, ew)
            if not (g.ovy | g.ovx):
                out[sl] = v
            else:
                a_y, a_x = ay[ty][sl[1], None], ax[tx][None, sl[2]]
                if fault == 'wy_wx_exchanged':      # the weight of relative block row dy taken for relative column dx and the other way round
                    Y, X = np.arange(sy, sy + eh)[:, None], np.arange(sx, sx + ew)[None, :]
                    ry, rx = Y // g.ph + (tx - X // g.pw), X // g.pw + (ty - Y // g.ph)
                    a_y = np.where((ry >= 0) & (ry < g.bh), np.stack(ay)[np.clip(ry, 0, g.bh - 1), Y], np.float32(0))
                    a_x = np.where((rx >= 0) & (rx < g.bw), np.stack(ax)[np.clip(rx, 0, g.bw - 1), X], np.float32(0))
                if fault == 'normalised_over_both_axes':
                    w = (a_y * a_x) / (sum_y[sl[1], None] * sum_x[None, sl[2]])
                else:
                    w = (a_y / sum_y[sl[1], None]) * (a_x / sum_x[None, sl[2]])
                w = w.astype(np.float32)[..., None]
                t = (w * v).astype(np.float32)
                if fault == 'fma':
                    acc = (w.astype(np.float64) * v.astype(np.float64) + out[sl].astype(np.float64)).astype(np.float32)
                else:
                    acc = (out[sl] + t).astype(np.float32)
                first = ~seen[sl]
                if fault == 'sum_restarts':
                    first = first | ~covered(frames.shape, geo, tile0, n - tile0)[sl]      # nothing of THIS range was there yet
                out[sl] = np.where(first[..., None], t, acc)
        seen[sl] = True
    return out


class NumpyBackend:
    """The restatement as a backend, with at most one of FAULTS planted."""

    def __init__(self, geo_of, fault=None):
        assert fault is None or fault in FAULTS
        self.geo_of, self.fault = geo_of, fault

    def __call__(self, mode, u8, frames_alloc, tiles_alloc, case, tile0, ntiles):
        geo = self.geo_of(case)
        fr, tl = np.array(frames_alloc), np.array(tiles_alloc)
        frames, tiles = frames_view(fr, case, u8), tiles_view(tl, geo)
        if mode == 'cut':
            tiles[:ntiles] = cut(frames, geo, tile0, ntiles, self.fault, into=tiles)
        else:
            frames[...] = join(frames, tiles[:ntiles], geo, tile0, ntiles, self.fault)
        return fr, tl


# ---- allocations: guard | payload | guard --------------------------------------------------------------------------------------------
def frames_view(alloc, case, u8):
    n = case.B * case.H * case.W * 3
    g = GUARD_U8 if u8 else GUARD
    return alloc[g:g + n].reshape(case.B, case.H, case.W, 3)


def tiles_view(alloc, geo):
    return alloc[GUARD:alloc.size - GUARD].reshape(-1, geo['padded_h'], geo['padded_w'], 3)


def new_frames_alloc(case, u8, seed):
    n = case.B * case.H * case.W * 3
    if not u8:
        return designed_floats(n + 2 * GUARD, seed)
    size = (GUARD_U8 + n + GUARD_U8 + 3) // 4 * 4          # whole 32-bit words: the 8-bit cut reads aligned words
    a = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    a[GUARD_U8:GUARD_U8 + n] = designed_u8(case.B, case.H, case.W, seed).ravel()
    return a


def new_tiles_alloc(geo, ntiles, seed):
    return designed_floats(ntiles * geo['padded_h'] * geo['padded_w'] * 3 + 2 * GUARD, seed)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_cut(backend, case, geo, u8, ranges, seed=0, twice=True):
    """Yields a message per finding: for every range, on freshly filled allocations, tiles_dev[0 : ntiles] equals the restatement (the
    padding +0.0), the rest of the tile tensor (one more tile than the longest range), its guards and the frame allocation are untouched,
    and the same call again gives the same bits."""
    cap = max(nt for _, nt in ranges) + 1
    for i, (tile0, nt) in enumerate(ranges):
        fr0 = new_frames_alloc(case, u8, seed + 2 * i)
        tl0 = new_tiles_alloc(geo, cap, seed + 2 * i + 1)
        fr0.setflags(write=False); tl0.setflags(write=False)
        fr1, tl1 = backend('cut', u8, fr0, tl0, case, tile0, nt)
        where = f'{case.name} {"u8" if u8 else "f32"} cut [{tile0}, {tile0 + nt})'
        want = np.array(tl0)
        ref = cut(frames_view(fr0, case, u8), geo, tile0, nt)
        tiles_view(want, geo)[:nt] = ref
        got = tiles_view(tl1, geo)[:nt]
        if not _same(fr1, fr0):
            yield f'{where}: the frames (or their guards) were written'
        if not _same(got, ref):
            bad = np.argwhere(bits(got) != bits(ref))
            yield f'{where}: {len(bad)} tile floats differ, first at (tile, y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {ref[tuple(bad[0])]!r}'
        pad = np.ones(ref.shape, bool)
        pad[:, geo['pad_y']:geo['pad_y'] + geo['tile_h'], geo['pad_x']:geo['pad_x'] + geo['tile_w']] = False
        if bits(got)[pad].any():
            yield f'{where}: the padding is not +0.0'
        rest_got, rest_want = np.array(tl1), np.array(want)
        tiles_view(rest_got, geo)[:nt] = 0; tiles_view(rest_want, geo)[:nt] = 0
        if not _same(rest_got, rest_want):
            yield f'{where}: written outside tiles [0, {nt}) of the tile tensor (the later tiles or the guards)'
        if twice:
            fr2, tl2 = backend('cut', u8, fr0, tl0, case, tile0, nt)
            if not (_same(fr2, fr1) and _same(tl2, tl1)):
                yield f'{where}: the same call again gives other bits'


def check_join(backend, case, geo, ranges, seed=0, twice=True):
    """Yields a message per finding: the ranges are joined one after another into a frame batch that starts as background; after every
    call the frame batch equals the restatement applied to the same starting bits, no pixel outside the range's tiles changed (nor the
    guards, nor the tile tensor), and the same call again gives the same bits."""
    cap = max(nt for _, nt in ranges) + 1
    fr0 = new_frames_alloc(case, False, seed)
    for i, (tile0, nt) in enumerate(ranges):
        tl0 = new_tiles_alloc(geo, cap, seed + 1 + i)
        fr0 = np.array(fr0)
        fr0.setflags(write=False); tl0.setflags(write=False)
        fr1, tl1 = backend('join', False, fr0, tl0, case, tile0, nt)
        where = f'{case.name} join [{tile0}, {tile0 + nt})'
        if not _same(tl1, tl0):
            yield f'{where}: the tile tensor (or its guards) was written'
        before = frames_view(fr0, case, False)
        ref = join(before, tiles_view(tl0, geo)[:nt], geo, tile0, nt)
        got = frames_view(fr1, case, False)
        if not _same(got, ref):
            bad = np.argwhere(bits(got) != bits(ref))
            yield f'{where}: {len(bad)} frame floats differ, first at (b, y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {ref[tuple(bad[0])]!r}'
        if geo['overlap_h'] | geo['overlap_w']:
            own = covered(before.shape, geo, tile0, nt)
        else:       # the patches of the range
            own = np.zeros(before.shape[:3], bool)
            bh, bw = len(geo['origins_y']), len(geo['origins_x'])
            ph, pw = case.H // bh, case.W // bw
            for n in range(tile0, tile0 + nt):
                b, t = divmod(n, bh * bw)
                own[b, t // bw * ph:(t // bw + 1) * ph, t % bw * pw:(t % bw + 1) * pw] = True
        outside_got, outside_want = np.array(fr1), np.array(fr0)
        frames_view(outside_got, case, False)[own] = 0; frames_view(outside_want, case, False)[own] = 0
        if not _same(outside_got, outside_want):
            yield f'{where}: a pixel that no tile of the range covers (or a guard) was written'
        if twice:
            fr2, tl2 = backend('join', False, fr0, tl0, case, tile0, nt)
            if not (_same(fr2, fr1) and _same(tl2, tl1)):
                yield f'{where}: the same call again gives other bits'
        fr0 = fr1


def check_case(backend, case, geo, seed=0, twice=True):
    """Every check of the issue for one case: f32 cut, u8 cut and join over the four partitions."""
    bh, bw = len(geo['origins_y']), len(geo['origins_x'])
    for pi, (name, ranges) in enumerate(partitions(case.B * bh * bw, bh * bw).items()):
        s = seed + 1000 * pi
        for msg in check_cut(backend, case, geo, False, ranges, s, twice): yield f'[{name}] {msg}'
        for msg in check_cut(backend, case, geo, True, ranges, s + 300, twice): yield f'[{name}] {msg}'
        for msg in check_join(backend, case, geo, ranges, s + 600, twice): yield f'[{name}] {msg}'


# ---- which branches of the kernels a call takes (for the coverage the GPU test asserts; restates the kernels' own conditions) ---------
def branches(case, geo, mode, u8, tile0, ntiles):
    """Names of the kernel instance and of the branches the call [tile0, tile0 + ntiles) takes, for a tile tensor whose first float is
    16-byte aligned and a frame batch whose first byte is 4-byte aligned."""
    g = _Geo(geo, (case.B, case.H, case.W))
    ov = bool(g.ovy | g.ovx)
    out = set()
    if mode == 'cut' and not u8:
        out.add(f'frame_to_tiles_kernel<{"true" if ov else "false"}>')
    elif mode == 'cut':
        out.add(f'frame_u8_to_tiles_kernel<{"true" if ov else "false"}>')
        row = g.TW * 3
        groups = (row + 11) // 12
        cw3 = g.ew * 3
        for k in range(ntiles):
            b, ty, tx = g.tile(tile0 + k)
            for y in range(g.TH):
                r = k * g.TH + y
                for q in range(groups):
                    xc0 = q * 12
                    s0 = xc0 - g.ox * 3
                    if 0 <= y - g.oy < g.eh and s0 + 12 > 0 and s0 < cw3:
                        if s0 >= 0 and s0 + 12 <= cw3:
                            a = ((b * g.H + g.ys[ty] + y - g.oy) * g.W + g.xs[tx]) * 3 + s0
                            out.add('u8 fast path, aligned words' if a % 4 == 0 else 'u8 fast path, shifted words')
                        else:
                            out.add('u8 byte path')
                    else:
                        out.add('u8 padding group')
                    vec = xc0 + 12 <= row and (r * row + xc0) % 4 == 0
                    out.add('u8 vector stores' if vec else ('u8 scalar stores, partial group' if xc0 + 12 > row else 'u8 scalar stores, unaligned group'))
    elif not ov:
        out.add('tiles_to_frame_kernel')
    else:
        out.add('blend_tiles_kernel')
        last = tile0 + ntiles - 1
        out.add('blend one-frame row window' if tile0 // g.T == last // g.T else 'blend multi-frame launch')
        mine = covered((case.B, case.H, case.W), geo, tile0, ntiles)
        f0, f1 = tile0 // g.T, last // g.T
        if tile0 > f0 * g.T and (mine & covered((case.B, case.H, case.W), geo, f0 * g.T, tile0 - f0 * g.T)).any():
            out.add('blend continues from dst')
        if last + 1 < (f1 + 1) * g.T and (mine & covered((case.B, case.H, case.W), geo, last + 1, (f1 + 1) * g.T - last - 1)).any():
            out.add('blend skips later tiles')
        if tile0 // g.T == last // g.T:
            y0, y1 = g.ys[(tile0 % g.T) // g.bw], g.ys[(last % g.T) // g.bw] + g.eh
            if y0 > 0 or y1 < g.H:
                out.add('blend row window smaller than the frame')
    return out
