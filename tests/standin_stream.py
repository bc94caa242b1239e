"""The stand-in interpolator of the eval/video_cli.py CPU tests (test_stream_select_cpu.py, test_dedup_retime_cpu.py) and of
tools/make_video_cli_golden.py: a mid-frame is the average of its two parents, and the stream records what was asked of it.  No GPU."""
import numpy as np


def avg(a, b):
    return ((a.astype(np.int32) + b) // 2).astype(np.uint8)


def between(a, b, times):
    """{position: frame} of the stand-in's recursion between a and b: a frame is the average of its two parents."""
    at = {0: a, 1 << times: b}
    step = 1 << times
    while step > 1:
        for lo in range(0, 1 << times, step):
            at[lo + step // 2] = avg(at[lo], at[lo + step])
        step //= 2
    return at


class Stream:
    """A recording stream: with dedup in the open arguments a pushed frame equal to the carried one is dropped (nothing runs, nothing changes);
    input frame cut_at starts a new scene; records every select() and, per push that was not dropped, (input index, selection in force)."""

    def __init__(self, times, cut_at, dedup=None):
        self.prev, self.i, self.times, self.cut_at, self.dedup = None, -1, times, cut_at, dedup
        self.was_cut = self.was_dup = 0
        self.selection = tuple(range(1, 1 << times))
        self.selects, self.pushes = [], []

    def __enter__(self): return self
    def __exit__(self, *exc): pass

    def select(self, positions=None):
        self.selection = tuple(range(1, 1 << self.times)) if positions is None else tuple(sorted(set(positions)))
        self.selects.append(self.selection)

    def cut_info(self):
        return -1, 1, self.was_cut

    def dup_info(self):
        assert self.dedup is not None, 'dup_info() of a stream opened without dedup'
        return None, self.was_dup

    def push(self, frame):
        self.i += 1
        self.was_cut = 0
        self.was_dup = int(self.dedup is not None and self.prev is not None and np.array_equal(frame, self.prev))
        if self.was_dup:
            return None
        mid = None
        self.was_cut = int(self.prev is not None and self.i == self.cut_at)
        if self.prev is not None:
            self.pushes.append((self.i, self.selection))
        if self.prev is not None and not self.was_cut and self.selection:
            at = between(self.prev, frame, self.times)
            mid = at[1] if self.times == 1 else np.stack([at[p] for p in self.selection])
        self.prev = frame
        return mid


class It:
    """The interpolator: open_stream takes what eval.interpolator.Interpolator.open_stream takes and keeps the keyword arguments it got."""

    def __init__(self, cut_at=None): self.cut_at, self.kw, self.stream = cut_at, None, None

    def open_stream(self, h, w, pix, matrix, full_range, **kw):
        self.kw = kw
        self.stream = Stream(kw.get('times', 1), self.cut_at if kw.get('scene_cut') else None, kw.get('dedup'))
        return self.stream
