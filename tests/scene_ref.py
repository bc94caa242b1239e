"""Numpy restatement of the scene-cut statistic and rule of include/film_hip.h ("Scene cuts"): the per-frame sample histogram, the distance
of two histograms and the integer decision rule.  tests/test_scene_gpu.py compares frame_histogram_kernel and the streams with it, bit for
bit; tests/test_scene_cpu.py checks it against known answers and shows that the comparison finds planted kernel faults.

Frames are numpy arrays as the streams take them: 'u8' uint8 [H,W,3], 'f32' float32 [H,W,3], 'i420' / 'nv12' uint8 [H * 3 // 2, W]."""
import numpy as np

LAYOUTS = ('u8', 'f32', 'i420', 'nv12')
YUV = ('i420', 'nv12')


def quantise(x):
    """film_to_uint8's rule on float32: uint8(clip(x * 255, 0, 255) + 0.5), the same float32 operations in the same order."""
    x = np.asarray(x, np.float32)
    return (np.clip(x * np.float32(255), np.float32(0), np.float32(255)) + np.float32(0.5)).astype(np.uint8)


def planes(frame, pix):
    """The three planes of 8-bit codes of a frame, each as a flat uint8 array."""
    frame = np.asarray(frame)
    if pix in ('u8', 'f32'):
        assert frame.ndim == 3 and frame.shape[2] == 3 and frame.dtype == (np.uint8 if pix == 'u8' else np.float32)
        q = frame if pix == 'u8' else quantise(frame)
        return [q[..., c].ravel() for c in range(3)]
    assert pix in YUV and frame.ndim == 2 and frame.dtype == np.uint8 and frame.shape[0] % 3 == 0
    h, w = frame.shape[0] * 2 // 3, frame.shape[1]
    assert h % 2 == 0 and w % 2 == 0
    flat = frame.ravel()
    y, c = flat[:h * w], flat[h * w:]
    if pix == 'i420':
        return [y, c[:h * w // 4], c[h * w // 4:]]
    return [y, c[0::2], c[1::2]]


def histogram(frame, pix):
    """int64 [3, 256]: hist[p][v] = the number of samples of plane p with code v."""
    return np.stack([np.bincount(p, minlength=256) for p in planes(frame, pix)]).astype(np.int64)


def distance(h0, h1):
    """D = sum |h1 - h0| as a Python int."""
    return int(np.abs(np.asarray(h1, np.int64) - np.asarray(h0, np.int64)).sum())


def samples(h, w, pix):
    """S: the samples of one h x w frame."""
    return 3 * h * w // 2 if pix in YUV else 3 * h * w


def is_cut(D, S, k):
    """The rule, in integers: cut iff 1000 D >= k * 2 S (k in permille, 1 .. 1000)."""
    assert 1 <= k <= 1000
    return 1000 * int(D) >= int(k) * 2 * int(S)


def frame_shape(h, w, pix):
    return (h * 3 // 2, w) if pix in YUV else (h, w, 3)


def to_layout(codes, h, w, pix):
    """A frame of layout `pix` from a flat array of S codes in MEMORY order ('f32': code / 255.0f, which quantises back to the code)."""
    codes = np.asarray(codes, np.uint8).reshape(frame_shape(h, w, pix))
    return (codes.astype(np.float32) / np.float32(255)) if pix == 'f32' else codes


# ---- a numpy model of frame_histogram_kernel's walk (csrc/frame_kernels.hip), for the planted faults of tests/test_scene_cpu.py ---------------
def kernel_model(frame, pix, fault=None, head=0):
    """The kernel's own route to the histogram: the frame's elements in memory order, walked in 16-byte vectors from a 16-byte boundary `head`
    elements in front of the frame, the plane of an element from its index.  fault: None, 'drop_tail' (the last partial vector is not
    counted), 'swap_cbcr' (NV12: Cb and Cr exchanged), 'truncate' (F32: no + 0.5)."""
    frame = np.asarray(frame)
    if pix == 'f32':
        x = frame.ravel().astype(np.float32)
        v = np.clip(x * np.float32(255), np.float32(0), np.float32(255))
        codes = (v if fault == 'truncate' else v + np.float32(0.5)).astype(np.uint8)
        epv = 4
    else:
        codes = frame.ravel()
        epv = 16
    n = codes.size
    idx = np.arange(n)
    if pix in ('u8', 'f32'):
        plane = idx % 3
    else:
        hw = n * 2 // 3
        if pix == 'i420':
            plane = (idx >= hw).astype(np.int64) + (idx >= hw + hw // 4)
        else:
            odd = (idx - hw) & 1
            plane = np.where(idx < hw, 0, 1 + (1 - odd if fault == 'swap_cbcr' else odd))
    keep = np.ones(n, bool)
    if fault == 'drop_tail':
        nvec = (head + n + epv - 1) // epv
        last0 = (nvec - 1) * epv - head
        if last0 + epv > n:        # the last vector is partial
            keep[max(last0, 0):] = False
    hist = np.zeros((3, 256), np.int64)
    np.add.at(hist, (plane[keep], codes[keep].astype(np.int64)), 1)
    return hist


# ---- designed data ------------------------------------------------------------------------------------------------------------------------------
def designed_codes(n, seed):
    """n codes in which every code 0..255 is present (n >= 256) at unequal counts: code v is drawn with weight v + 1."""
    rng = np.random.default_rng(seed)
    c = rng.choice(256, size=n, p=np.arange(1, 257) / np.arange(1, 257).sum()).astype(np.uint8)
    if n >= 256:
        c[rng.permutation(n)[:256]] = np.arange(256, dtype=np.uint8)
    return c


def f32_test_frame(h, w, seed):
    """A float32 [h,w,3] frame for the kernel tests: mostly code / 255.0f of designed codes, with half-way values (v + 0.5) / 255, values
    below 0 and above 1 and plain noise mixed in - its first value is always a half-way value, so a frame of any size has one."""
    rng = np.random.default_rng(seed)
    n = h * w * 3
    x = designed_codes(n, seed).astype(np.float32) / np.float32(255)
    k = np.arange(n)
    half = ((rng.integers(0, 255, n) + 0.5) / 255).astype(np.float32)
    x = np.where(k % 4 == 0, half, x)
    x = np.where(k % 11 == 5, rng.uniform(-0.3, 1.3, n).astype(np.float32), x)
    x = np.where(k % 17 == 3, np.float32(-2.5), x)
    x = np.where(k % 19 == 7, np.float32(3), x)
    return np.ascontiguousarray(x.reshape(h, w, 3), np.float32)


def scene_frames(pix, h=64, w=64, seed=3):
    """The six frames of the stream tests: frames 0-2 are scene A rolled by (2, -2) pixels per frame, codes confined to 16..235; frames 3-5 are
    scene B = A with a designed quarter of its samples set to 255 (RGB: 16 full rows; 4:2:0: 24 full rows of Y), rolled on in the same way.
    255 does not occur in A, so D(frame 2, frame 3) = S / 4 + S / 4 = S / 2 exactly, and D = 0 inside a scene (a roll permutes the samples)."""
    assert (h, w) == (64, 64)
    rng = np.random.default_rng(seed)
    if pix in YUV:
        Y = rng.integers(16, 236, (h, w), dtype=np.uint8)
        Cb = rng.integers(16, 236, (h // 2, w // 2), dtype=np.uint8)
        Cr = rng.integers(16, 236, (h // 2, w // 2), dtype=np.uint8)

        def pack(y, cb, cr):
            if pix == 'i420':
                return np.concatenate([y.ravel(), cb.ravel(), cr.ravel()]).reshape(h * 3 // 2, w)
            return np.concatenate([y.ravel(), np.stack([cb, cr], -1).ravel()]).reshape(h * 3 // 2, w)

        def roll(i, y):
            return pack(np.roll(y, (2 * i, -2 * i), (0, 1)), np.roll(Cb, (i, -i), (0, 1)), np.roll(Cr, (i, -i), (0, 1)))

        YB = Y.copy()
        YB[20:44] = 255          # 24 rows x 64 = 1536 = S / 4 samples
        frames = [roll(i, Y) for i in range(3)] + [roll(i, YB) for i in range(3, 6)]
    else:
        A = rng.integers(16, 236, (h, w, 3), dtype=np.uint8)
        B = A.copy()
        B[24:40] = 255           # 16 rows x 64 x 3 = 3072 = S / 4 samples
        frames = [np.roll(A, (2 * i, -2 * i), (0, 1)) for i in range(3)] + [np.roll(B, (2 * i, -2 * i), (0, 1)) for i in range(3, 6)]
        if pix == 'f32':
            frames = [f.astype(np.float32) / np.float32(255) for f in frames]
    out = np.stack(frames)
    out.setflags(write=False)
    return out
