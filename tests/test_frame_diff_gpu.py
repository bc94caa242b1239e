"""GPU tests of frame_diff_kernel through film_frame_diff, all twelve numbers exact against the numpy restatement tests/frame_diff_ref.py
(include/film_hip.h, "Duplicate frames"): all ten pixel types at the smallest sizes that reach every branch of the kernel - one whole block,
partial blocks both ways, odd sizes whose rows start off a word boundary and whose frame ends inside a word, a frame beyond one pass of the
capped grid - on designed data (tests/test_frame_diff_cpu.py shows which wrong kernels that data finds), random, identical and swapped
frames; `out` is pre-filled with noise between guard words, and a second call gives the same bits."""
import numpy as np
import pytest

import frame_diff_ref as R
from film_hip import pixfmt

pytestmark = pytest.mark.gpu

GUARD = 64          # guard bytes in front of and behind a frame (a multiple of 16: the frame starts where the offset puts it)
OUT_GUARD = 4       # guard uint64 around the twelve counters
# csrc/film_kernels.h: the launcher's grid is at most FILM_DIFF_WG_PER_CU workgroups per compute unit of FILM_DIFF_THREADS lanes, and a lane takes
# one block position of a plane group per step of its grid-stride loop
FILM_DIFF_THREADS, FILM_DIFF_WG_PER_CU = 256, 1
ALL = tuple(lay.name for lay in pixfmt.LAYOUTS)


def test_constants_are_the_launchers():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_kernels.h')).read()
    for name, val in (('FILM_DIFF_THREADS', FILM_DIFF_THREADS), ('FILM_DIFF_WG_PER_CU', FILM_DIFF_WG_PER_CU)):
        assert re.search(rf'^#define {name} {val}$', text, re.M), name


def _upload(frame, offset_words):
    """The frame's bytes inside an allocation of whole words, between guard bytes, `offset_words` words behind a 16-byte boundary."""
    import torch
    raw = np.ascontiguousarray(frame).view(np.uint8).ravel()
    off = 4 * offset_words
    alloc = np.concatenate([np.full(GUARD + off, 0x5a, np.uint8), raw, np.full((-raw.size) % 4 + GUARD, 0x5a, np.uint8)])
    t = torch.from_numpy(alloc).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + GUARD + off, alloc


def _diff(pix, h, w, a, b, lo=0, offset_words=0):
    """film_frame_diff of two host frames -> out[3][4] as lists of ints; checks the guards, the overwrite and the repeat on the way."""
    import torch
    from film_hip.engine import frame_diff_device
    ta, pa, alloc_a = _upload(a, offset_words)
    tb, pb, alloc_b = _upload(b, offset_words)
    noise = np.random.default_rng(5).integers(1, 2 ** 63, 12 + 2 * OUT_GUARD, dtype=np.int64)
    to = torch.from_numpy(noise.copy()).cuda()
    first = None
    for rep in range(2):                                     # `out` holds noise, then the first answer: a call overwrites, never accumulates
        frame_diff_device(pa, pb, h, w, to.data_ptr() + 8 * OUT_GUARD, pix, lo=lo)
        torch.cuda.synchronize()
        got = to.cpu().numpy()
        assert np.array_equal(got[:OUT_GUARD], noise[:OUT_GUARD]) and np.array_equal(got[-OUT_GUARD:], noise[-OUT_GUARD:]), (pix, h, w)
        stats = got[OUT_GUARD:OUT_GUARD + 12].reshape(3, 4).tolist()
        assert first is None or stats == first, (pix, h, w, rep, stats, first)
        first = stats
    assert np.array_equal(ta.cpu().numpy(), alloc_a) and np.array_equal(tb.cpu().numpy(), alloc_b)      # the frames and their guards are unmodified
    return first


def _sizes(pix):
    lay = pixfmt.BY_NAME[pix]
    if lay.sy:
        return [(8, 8), (18, 22), (34, 50)]                  # 4:2:0: even sizes; chroma 17 x 25 - rows start off a word boundary
    if lay.sx:
        return [(8, 8), (18, 22), (33, 50)]                  # 4:2:2: an odd height
    return [(8, 8), (18, 22), (33, 50), (33, 51), (1, 1)]    # RGB and 4:4:4: any size - a frame that ends inside a word


CASES = [(pix, h, w) for pix in ALL for h, w in _sizes(pix)]


@pytest.mark.parametrize('pix,h,w', CASES, ids=lambda v: str(v))
def test_frame_diff(pix, h, w):
    a, b = R.random_frame(pix, h, w, 11 + h), R.random_frame(pix, h, w, 12 + w)
    lo = int(np.median(R.block_sads(np.abs(R.planes(a, pix)[0] - R.planes(b, pix)[0]))))      # a `lo` that splits the blocks of the Y / R plane
    for off in (0, 1):                                       # the frame on a 16-byte boundary and 4 bytes behind one (no 8-byte alignment)
        got = _diff(pix, h, w, a, b, 0, off)
        assert got == R.frame_diff(a, b, pix, 0), (pix, h, w, off, got)
        assert _diff(pix, h, w, b, a, 0, off) == got                          # symmetric
    for at in (lo, max(lo - 1, 0), lo + 1, 65535):
        assert _diff(pix, h, w, a, b, at) == R.frame_diff(a, b, pix, at), (pix, h, w, at)
    same = _diff(pix, h, w, a, a.copy())
    assert same == R.frame_diff(a, a, pix) and [s[:3] for s in same] == [[0, 0, 0]] * 3


@pytest.mark.parametrize('pix', ALL)
def test_one_differing_sample(pix):
    """One sample moved by one code at every corner of the first and the last (partial) block of every plane - the last Y sample and the first
    Cb sample, and Cr-only differences of the semi-planar layouts, among them: exactly one block of exactly one plane answers."""
    for h, w in _sizes(pix)[1:3]:
        for name, a, b in R.single_sample_cases(pix, h, w):
            p = int(name[1])
            got = _diff(pix, h, w, a, b)
            assert got == R.frame_diff(a, b, pix), (pix, h, w, name, got)
            assert [g[:3] for g in got] == [[1, 1, 1] if q == p else [0, 0, 0] for q in range(3)], (pix, h, w, name, got)


@pytest.mark.parametrize('pix', [p for p in ALL if p == 'f32' or pixfmt.BY_NAME[p].depth == 10])
def test_ignored_bits_give_zero(pix):
    """Words that differ only in the six ignored bits (P010: the low six; the others: the high six), F32 values that differ but quantise alike."""
    for h, w in _sizes(pix)[:3]:
        a, b = R.ignored_bits_pair(pix, h, w, 13)
        got = _diff(pix, h, w, a, b)
        assert got == R.frame_diff(a, b, pix) and [g[:3] for g in got] == [[0, 0, 0]] * 3, (pix, h, w, got)


@pytest.mark.parametrize('pix', ALL)
def test_extremes_and_the_threshold(pix):
    lay = pixfmt.BY_NAME[pix]
    h, w = 16, 24
    top = 1023 if lay.depth == 10 else 255
    a, b = R.constant_frame(pix, h, w, 0), R.constant_frame(pix, h, w, top)
    for lo in (64 * top - 1, 64 * top):                      # a whole block at exactly lo is not over, at lo + 1 it is
        got = _diff(pix, h, w, a, b, lo)
        assert got == R.frame_diff(a, b, pix, lo), (pix, lo, got)
        assert got[0] == [h * w * top, 64 * top, 6 if lo == 64 * top - 1 else 0, 6]
    assert lay.depth != 10 or got[0][1] == 65472


@pytest.mark.parametrize('pix', ('u8', 'f32', 'i420', 'nv12', 'i010', 'p010'))
def test_beyond_one_pass_of_the_grid(pix):
    """One frame per kernel instance whose first plane group holds more block positions than one pass of the capped grid takes (a strip one
    or two rows high: blocks are counted by ceil): the grid-stride loops and the reduction across all workgroups."""
    import torch
    one_pass = torch.cuda.get_device_properties(0).multi_processor_count * FILM_DIFF_WG_PER_CU * FILM_DIFF_THREADS
    h, w = (2 if pixfmt.BY_NAME[pix].sy else 1), 8 * (one_pass + one_pass // 8 + 3)
    assert -(-w // 8) > one_pass
    a, b = R.random_frame(pix, h, w, 21), R.random_frame(pix, h, w, 22)
    want = R.frame_diff(a, b, pix, 40)
    assert want[0][3] > one_pass
    assert _diff(pix, h, w, a, b, 40) == want


def test_a_total_past_32_bits():
    """2048 x 2056 i410 frames of code 0 against code 1023: every plane's total is 2048 * 2056 * 1023 > 2^32.  The expectation is the
    reference's answer for one strip of 8 rows times the 256 strips (the blocks are all alike, the sums are linear)."""
    import torch
    from film_hip.torch_io import frame_diff
    h, w = 2048, 2056
    strip = R.frame_diff(R.constant_frame('i410', 8, w, 0), R.constant_frame('i410', 8, w, 1023), 'i410')
    want = [[t * 256, mx, ov * 256, n * 256] for t, mx, ov, n in strip]
    assert want[0] == [h * w * 1023, 65472, 256 * 257, 256 * 257] and want[0][0] > 2 ** 32
    a = torch.zeros((3 * h, w), dtype=torch.int16, device='cuda')
    b = torch.full((3 * h, w), 1023, dtype=torch.int16, device='cuda')
    got = frame_diff(a, b, 'i410')
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 4) and got.is_cuda
    assert got.cpu().tolist() == want


def test_torch_io_frame_diff():
    """The tensor interface on three kinds of frame: [3, 4] int64 on the frames' device, the reference's numbers."""
    import torch
    from film_hip.torch_io import frame_diff
    for pix, h, w in (('u8', 33, 51), ('f32', 18, 22), ('nv12', 18, 22), ('p010', 34, 50)):
        a, b = R.random_frame(pix, h, w, 31), R.random_frame(pix, h, w, 32)
        ta, tb = (torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in (a, b))
        got = frame_diff(ta, tb, pix, lo=100)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 4) and got.device == ta.device
        assert got.cpu().tolist() == R.frame_diff(a, b, pix, 100), pix
