"""Numpy restatement of the duplicate-frame statistic and rule of include/film_hip.h ("Duplicate frames"), written over the layout table
film_hip/pixfmt.py: the three planes of full-depth codes of a frame, the 8 x 8 blocks anchored on the plane, out[3][4] = {total, max, over,
blocks} per plane, and the integer rule.  tests/test_frame_diff_gpu.py compares frame_diff_kernel with it, all twelve numbers exact, and
tests/test_dedup_stream_gpu.py the streams; tests/test_frame_diff_cpu.py checks it against known answers and shows that the designed data
below tells it from wrong restatements (`fault`).

Frames are numpy arrays as the streams take them (film_hip.pixfmt.frame_shape): [H,W,3] uint8 / float32, or [rows, W] uint8 / uint16."""
import numpy as np

from film_hip import pixfmt

BLOCK = 8
FAULTS = ('swap_cbcr', 'p010_as_i010', 'i010_as_p010', 'drop_partial', 'ge', 'total32', 'tile_anchor', 'f32_before_quantise')


def quantise(x):
    """film_to_uint8's rule on float32: uint8(clip(x * 255, 0, 255) + 0.5), the same float32 operations in the same order."""
    x = np.asarray(x, np.float32)
    return (np.clip(x * np.float32(255), np.float32(0), np.float32(255)) + np.float32(0.5)).astype(np.uint8)


def scale(pix):
    """m of the rule: 4 for the 10-bit layouts, else 1."""
    return 4 if pixfmt.BY_NAME[pix].depth == 10 else 1


def planes(frame, pix, fault=None):
    """The three planes of a frame as int64 [Hp, Wp] arrays of full-depth codes."""
    lay = pixfmt.BY_NAME[pix]
    frame = np.asarray(frame)
    assert frame.dtype == lay.dtype, (frame.dtype, pix)
    h, w = pixfmt.frame_size(pix, frame.shape)
    if lay.depth is None:
        q = quantise(frame) if pix == 'f32' else frame
        return [q[..., c].astype(np.int64) for c in range(3)]
    assert not (w & lay.sx) and not (h & lay.sy)
    hc, wc = h >> lay.sy, w >> lay.sx
    flat = frame.ravel()
    assert flat.size == h * w + 2 * hc * wc
    y, c = flat[:h * w].reshape(h, w), flat[h * w:]
    if lay.semi_planar:
        c = c.reshape(hc, wc, 2)
        cb, cr = c[..., 0], c[..., 1]
    else:
        cb, cr = c[:hc * wc].reshape(hc, wc), c[hc * wc:].reshape(hc, wc)
    if fault == 'swap_cbcr' and lay.semi_planar:
        cb, cr = cr, cb
    high = pix == 'p010'                      # where the 10-bit code sits: bits 6-15 (P010) or 0-9
    if (fault == 'p010_as_i010' and pix == 'p010') or (fault == 'i010_as_p010' and pix == 'i010'):
        high = not high
    out = []
    for p in (y, cb, cr):
        p = p.astype(np.int64)
        if lay.depth == 10:
            p = (p >> 6) & 1023 if high else p & 1023
        out.append(p)
    return out


def block_sads(d, fault=None):
    """The SADs of the 8 x 8 blocks of one plane of absolute differences d [Hp, Wp], as int64 [ceil(Hp / 8), ceil(Wp / 8)]."""
    hp, wp = d.shape
    top, left = (3, 5) if fault == 'tile_anchor' else (0, 0)      # a grid anchored on a padded tile whose content starts at (3, 5)
    if fault == 'drop_partial':
        d = d[:hp // BLOCK * BLOCK, :wp // BLOCK * BLOCK]
        hp, wp = d.shape
    H8, W8 = -(-(hp + top) // BLOCK), -(-(wp + left) // BLOCK)
    pad = np.zeros((H8 * BLOCK, W8 * BLOCK), np.int64)
    pad[top:top + hp, left:left + wp] = d
    return pad.reshape(H8, BLOCK, W8, BLOCK).sum((1, 3))


def frame_diff(a, b, pix, lo=0, fault=None):
    """out[3][4] as a list of three lists of Python ints: {total, max, over, blocks} of every plane."""
    assert 0 <= lo <= 65535
    if fault == 'f32_before_quantise' and pix == 'f32':
        d3 = quantise(np.abs(np.asarray(a, np.float32) - np.asarray(b, np.float32))).astype(np.int64)
        ds = [d3[..., c] for c in range(3)]
    else:
        ds = [np.abs(x - y) for x, y in zip(planes(a, pix, fault), planes(b, pix, fault))]
    out = []
    for d in ds:
        s = block_sads(d, fault)
        assert s.size == 0 or int(s.max()) <= 64 * 1023
        total = int(s.sum())
        if fault == 'total32':
            total &= 0xffffffff
        over = int((s >= lo).sum()) if fault == 'ge' else int((s > lo).sum())
        out.append([total, int(s.max()) if s.size else 0, over, int(s.size)])
    return out


def rule(stats, m, hi, frac):
    """The rule on out[3][4] whose `over` was counted at lo * m: a duplicate iff for every plane max <= hi * m and 1000 over <= frac * blocks."""
    assert hi >= 0 and 0 <= frac <= 1000
    return all(int(mx) <= hi * m and 1000 * int(over) <= frac * int(blocks) for _, mx, over, blocks in stats)


def is_duplicate(a, b, pix, hi, lo=0, frac=1000):
    m = scale(pix)
    return rule(frame_diff(a, b, pix, lo * m), m, hi, frac)


# ---- designed data ------------------------------------------------------------------------------------------------------------------------------
def random_frame(pix, h, w, seed):
    """Uniform random stored samples: every bit of a 16-bit word is drawn, the ignored ones included; F32: values around [0, 1] with half-way
    values, out-of-range values and exact codes mixed."""
    rng = np.random.default_rng(seed)
    lay = pixfmt.BY_NAME[pix]
    shape = pixfmt.frame_shape(pix, h, w)
    if pix == 'f32':
        n = h * w * 3
        k = np.arange(n)
        x = rng.integers(0, 256, n).astype(np.float32) / np.float32(255)
        x = np.where(k % 4 == 0, ((rng.integers(0, 255, n) + 0.5) / 255).astype(np.float32), x)
        x = np.where(k % 7 == 3, rng.uniform(-0.3, 1.3, n).astype(np.float32), x)
        return np.ascontiguousarray(x.reshape(shape), np.float32)
    return rng.integers(0, 1 << (16 if lay.depth == 10 else 8), shape, dtype=lay.dtype)


def constant_frame(pix, h, w, code):
    """Every sample at full-depth code `code` (P010: stored as code << 6; F32: code / 255.0f)."""
    lay = pixfmt.BY_NAME[pix]
    shape = pixfmt.frame_shape(pix, h, w)
    if pix == 'f32':
        return np.full(shape, np.float32(code) / np.float32(255), np.float32)
    return np.full(shape, code << 6 if pix == 'p010' else code, lay.dtype)


def plane_index(pix, h, w, p, y, x):
    """The flat index, in the frame's array, of sample (y, x) of plane p."""
    lay = pixfmt.BY_NAME[pix]
    if lay.depth is None:
        return (y * w + x) * 3 + p
    if p == 0:
        return y * w + x
    hc, wc = h >> lay.sy, w >> lay.sx
    if lay.semi_planar:
        return h * w + (y * wc + x) * 2 + (p - 1)
    return h * w + (p - 1) * hc * wc + y * wc + x


def plane_shape(pix, h, w, p):
    lay = pixfmt.BY_NAME[pix]
    return (h, w) if p == 0 or lay.depth is None else (h >> lay.sy, w >> lay.sx)


def with_sample(frame, pix, p, y, x, delta):
    """A copy of `frame` whose sample (y, x) of plane p has its full-depth code moved by `delta` (the code stays inside its range; for F32
    the value moves by delta / 255)."""
    h, w = pixfmt.frame_size(pix, frame.shape)
    out = frame.copy()
    flat = out.reshape(-1)
    i = plane_index(pix, h, w, p, y, x)
    if pix == 'f32':
        flat[i] = np.float32(flat[i] + np.float32(delta) / np.float32(255))
    elif pix == 'p010':
        flat[i] = np.uint16(int(flat[i]) + (delta << 6))
    else:
        flat[i] = flat.dtype.type(int(flat[i]) + delta)
    return out


def corner_positions(hp, wp):
    """Where one differing sample tests the block geometry of an hp x wp plane: the four corners of the first block, the corners of the last
    (possibly partial) block, and the last row and column of the plane inside a middle block."""
    ys = sorted({0, min(7, hp - 1), (hp - 1) // 8 * 8, hp - 1})
    xs = sorted({0, min(7, wp - 1), (wp - 1) // 8 * 8, wp - 1})
    return [(y, x) for y in ys for x in xs]


def single_sample_cases(pix, h, w):
    """(name, a, b) pairs that differ in exactly one sample by one code step, over every plane and corner_positions; a is a mid-grey frame."""
    a = constant_frame(pix, h, w, 100)
    for p in range(3):
        hp, wp = plane_shape(pix, h, w, p)
        for y, x in corner_positions(hp, wp):
            yield f'p{p}y{y}x{x}', a, with_sample(a, pix, p, y, x, 1)


def ignored_bits_pair(pix, h, w, seed):
    """Two frames whose samples differ only where the statistic does not look: the ignored six bits of a 10-bit word (P010 low, the others
    high), or F32 values that differ but quantise alike.  Their statistic is zero."""
    rng = np.random.default_rng(seed)
    a = random_frame(pix, h, w, seed)
    if pix == 'f32':
        code = rng.integers(0, 256, a.shape)
        a = (code / 255).astype(np.float32)
        b = ((code + rng.uniform(-0.3, 0.3, a.shape)) / 255).astype(np.float32)
        assert not np.array_equal(a, b)
        return a, b
    assert pixfmt.BY_NAME[pix].depth == 10
    noise = rng.integers(0, 64, a.shape).astype(np.uint16)
    keep = np.uint16(0xffc0 if pix == 'p010' else 0x03ff)
    b = (a & keep) | (noise if pix == 'p010' else noise << 10).astype(np.uint16)
    assert not np.array_equal(a, b)
    return a, b
