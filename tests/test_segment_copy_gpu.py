"""GPU tests of the segment copy (film_debug_segment_copy; film_kernels.h, SegmentTable): the kernel a grouped stream restores and saves its
carry with.  One launch moves a table of up to 32 segments {source float offset, destination float offset, count}; a destination vector
that lies inside its segment is one 16-byte store, the head and the tail of a segment that starts or ends inside a vector go float by
float.  Every (source offset mod 4, destination offset mod 4) with every count of 0, 1, 3, 4, 5, 7, 1023 and 4099, as tables of 1 and of 32
segments; segments of 3 floats per image packed back to back, as the level-6 image of a 64 x 64 tile is.  The destination is pre-filled with
a pattern, every segment stands between guard bands, and the whole buffer is compared bit for bit with numpy.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 3, 4, 5, 7, 1023, 4099)
GUARD = 9                      # floats between two segments, on either side: more than a vector, and odd
PATTERN = 0x7FC0BEEF           # a quiet NaN with a payload: a copy that went through a float operation could lose it


def _bits(n, seed):
    """n random 32-bit patterns - NaNs, infinities and denormals among them - as uint32."""
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _place(cases):
    """cases: (source offset mod 4, destination offset mod 4, count) -> segments (src, dst, count) laid out one behind the other in both buffers,
    GUARD floats apart at least, each start at the wanted offset mod 4; and the floats either buffer needs."""
    segs, s, d = [], GUARD, GUARD
    for sm, dm, c in cases:
        s += (sm - s) % 4
        d += (dm - d) % 4
        segs.append((s, d, c))
        s += c + GUARD
        d += c + GUARD
    return segs, s, d


def _run(segs, n_src, n_dst, seed, table=32):
    """Copies `segs` in launches of `table` segments; returns (source bits, destination bits before, destination bits after)."""
    import torch
    from film_hip.engine import segment_copy_device
    src = _bits(n_src, seed)
    before = np.full(n_dst, PATTERN, np.uint32) ^ np.arange(n_dst, dtype=np.uint32)
    tsrc = torch.from_numpy(src.view(np.int32)).cuda()
    tdst = torch.from_numpy(before.view(np.int32).copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(0, max(len(segs), 1), table):                                     # (no segments: one launch of an empty table)
        segment_copy_device(segs[i:i + table], tsrc.data_ptr(), tdst.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(tsrc.cpu().numpy().view(np.uint32), src)                  # the source is only read
    return src, before, tdst.cpu().numpy().view(np.uint32)


def _expected(src, before, segs):
    want = before.copy()
    for s, d, c in segs:
        want[d:d + c] = src[s:s + c]
    return want


def _assert_same(got, want, segs):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], [g for g in segs if g[1] - 4 <= bad[0] < g[1] + g[2] + 4])


ALIGNMENTS = [(sm, dm) for sm in range(4) for dm in range(4)]


@pytest.mark.parametrize('table', [1, 32])
def test_every_alignment_and_count(table):
    cases = [(sm, dm, c) for c in COUNTS for sm, dm in ALIGNMENTS]
    assert len(cases) == 128
    segs, n_src, n_dst = _place(cases)
    assert {(s % 4, d % 4) for s, d, _ in segs} == set(ALIGNMENTS)
    src, before, got = _run(segs, n_src + 4, n_dst + 4, seed=table, table=table)
    want = _expected(src, before, segs)
    assert np.count_nonzero(want != before) > sum(c for _, _, c in segs) * 0.99     # (the pattern differs from what is copied)
    _assert_same(got, want, segs)


def test_three_floats_per_image_packed_back_to_back():
    """The level-6 image of a 64 x 64 tile is 1 x 1 x 3 floats: the segments of r = 1, 2 and 3 images start at any offset mod 4 and
    have any length, and in the carry one segment begins in the very vector in which the one before ends - no gap, no guard.  Buffers of
    other sizes stand between them, as the levels of the pyramids do."""
    per_image = (3, 12, 3 * 64, 3, 64, 3)
    segs, s, d = [], 5, 0
    for slot in range(4):
        for r in (1, 2, 3):
            for p in per_image:
                segs.append((s, d, r * p))
                s += 3 * p + 1                                                   # the plan: room for three images, and no common alignment
                d += r * p                                                       # the carry: packed
    assert len(segs) == 72 and {g[2] % 4 for g in segs} == {0, 1, 2, 3} and {g[1] % 4 for g in segs} == {0, 1, 2, 3}
    src, before, got = _run(segs, s + 4, d + GUARD, seed=3)
    want = _expected(src, before, segs)
    assert np.array_equal(want[d:], before[d:])
    _assert_same(got, want, segs)
    # and back: plan <- carry, into a destination with gaps
    back = [(dd, ss, c) for ss, dd, c in segs]
    src2, before2, got2 = _run(back, d + GUARD, s + 4, seed=4)
    _assert_same(got2, _expected(src2, before2, back), back)


def test_empty_segments_and_an_empty_table():
    segs, n_src, n_dst = _place([(1, 2, 0), (0, 0, 0), (3, 1, 6), (2, 2, 0), (0, 3, 1), (1, 1, 0)])
    src, before, got = _run(segs, n_src + 4, n_dst + 4, seed=5)
    _assert_same(got, _expected(src, before, segs), segs)
    src, before, got = _run([], 16, 16, seed=6)
    assert np.array_equal(got, before)
    zeros = [(0, 0, 0)] * 32
    src, before, got = _run(zeros, 16, 16, seed=7)
    assert np.array_equal(got, before)
