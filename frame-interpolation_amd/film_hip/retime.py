"""Frame-rate conversion by selected mid-frames: which positions of which push make a video of rate c/d out of one of rate a/b.

A "stream_times" = T frame stream can produce, between two consecutive input frames, the frames at the 2^T - 1 instants i / 2^T of the
interval (FilmStream.select picks some of them).  Output frame j of the converted video lies at u_j = j (a d) / (b c) input intervals
from the first input frame; it is SNAPPED to the nearest instant of that grid, g_j = round(u_j 2^T), ties to the even grid index (the
even index is the shallower, cheaper frame of the recursion): g_j >> T is an input frame and g_j & (2^T - 1) the position behind it, 0
the frame itself.  The snap error |g_j / 2^T - u_j| is at most 2^-(T + 1) input intervals, and the g_j are strictly increasing as long as
the output rate is at most 2^T times the input rate, which is what Retime accepts.  Integers only: no rate is ever a float here.

Spans (Retime.span), the one walk over the outputs.  The input frames a stream keeps are k_0 = 0 < k_1 < ... - all of them, k_m = m, unless it
drops duplicate frames (engine option "dup_hi").  Span m = [k_m, k_(m+1)) is n_m input intervals long and is closed by ONE push, whose 2^T grid
is spread over all of it: output j belongs to the span iff k_m <= u_j < k_(m+1), and its grid index is g = round((u_j - k_m) 2^T / n_m), ties to
even - 0 and 2^T are the two kept frames.  A span of one interval writes the frames of the g_j above: g = g_j - k_m 2^T.
"""
from math import gcd
from typing import Iterable, NamedTuple, Tuple


def parse_rate(text: str) -> Tuple[int, int]:
    """'60', '60000:1001' or '60000/1001' -> the reduced fraction (num, den); ValueError for anything else or a rate that is not positive."""
    s = str(text).strip().replace('/', ':')
    parts = s.split(':')
    if not 1 <= len(parts) <= 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f'a frame rate is N, N:D or N/D with positive integers, got {text!r}')
    num, den = int(parts[0]), int(parts[1]) if len(parts) == 2 else 1
    if num < 1 or den < 1:
        raise ValueError(f'a frame rate is N, N:D or N/D with positive integers, got {text!r}')
    g = gcd(num, den)
    return num // g, den // g


def closure(times: int, positions: Iterable[int]) -> Tuple[int, ...]:
    """C: the positions (1 .. 2^times - 1) and all their ancestors in the recursion tree, ascending - the pair runs of a push with that
    selection.  The mid-frame at position i = (2 j + 1) h, h = 2^(times - depth), is a child of the one of i - h, i + h that is an odd
    multiple of 2 h."""
    n = 1 << times
    c = set()
    for i in positions:
        if not 1 <= i < n:
            raise ValueError(f'a position of a times = {times} push is 1 .. {n - 1}, got {i!r}')
        while i not in c:
            c.add(i)
            h = i & -i
            if 2 * h == n:
                break                    # the root: its parents are the two input frames
            i = i - h if (i - h) // (2 * h) & 1 else i + h
    return tuple(sorted(c))


def push_cost(times: int, positions: Iterable[int]) -> Tuple[int, int]:
    """(pair runs, feature extractions) of a primed push with that selection: |C|, and 1 (the pushed frame) + the members of C that have
    a child in C."""
    c = set(closure(times, positions))
    fed = sum(1 for i in c if (i & -i) > 1 and (i - (i & -i) // 2 in c or i + (i & -i) // 2 in c))
    return len(c), 1 + fed


class Span(NamedTuple):
    j: int                        # the index of the first output inside the span (the next span's when `grid` is empty)
    grid: Tuple[int, ...]         # per output, in order: 0 = the kept frame that opens the span, 2^T = the one that closes it, else a position


class Retime:
    """rate_in = (a, b), rate_out = (c, d), times = T: the timing of the conversion on the grid of 2^-T input intervals."""

    def __init__(self, rate_in: Tuple[int, int], rate_out: Tuple[int, int], times: int):
        (a, b), (c, d) = ((int(x) for x in r) for r in (rate_in, rate_out))
        if min(a, b, c, d) < 1:
            raise ValueError(f'frame rates are fractions of positive integers, got {rate_in!r} -> {rate_out!r}')
        if not 1 <= int(times) <= 6:
            raise ValueError(f'times must be 1 .. 6, got {times!r}')
        self.times = int(times)
        p, q = a * d, b * c           # u_j = j p / q
        g = gcd(p, q)
        self.p, self.q = p // g, q // g
        if self.q > self.p << self.times:
            raise ValueError(f'output rate {c}/{d} is more than 2^{self.times} = {1 << self.times} times the input rate {a}/{b}: two '
                             f'outputs would land on one instant of the timing grid - use a deeper grid (times_to_interpolate)')

    def grid(self, j: int) -> int:
        """g_j: u_j 2^T rounded to the nearest integer, ties to even."""
        g, r = divmod(j * self.p << self.times, self.q)
        return g + (2 * r > self.q or (2 * r == self.q and g & 1))

    def error(self, j: int) -> Tuple[int, int]:
        """The snap error g_j / 2^T - u_j of output j in input intervals, as (numerator, denominator > 0)."""
        return self.grid(j) * self.q - (j * self.p << self.times), self.q << self.times

    def span(self, k: int, n: int) -> 'Span':
        """The outputs of a STRETCHED interval: input frames k and k + n (n >= 1) are kept and the n - 1 between them were dropped as duplicates
        of frame k.  Output j belongs to the span iff k <= u_j < k + n (compared exactly, as fractions); its grid index spreads the span over
        the 2^T grid, g = round((u_j - k) 2^T / n), ties to the even index, 0 <= g <= 2^T: g = 0 is frame k verbatim, g = 2^T is frame k + n
        verbatim, anything else is position g of the push of frame k + n, which closes the span.  A long span may give several outputs one g:
        the position is selected once and written once per such output.  Returns Span(j, grid): the index of the span's first output and the
        grid indices of its outputs in order.  n = 1: g = grid(j) - k 2^T (an output that rounds UP to input frame k + 1 closes its span with
        g = 2^T; the shift by k 2^T is even, so the ties fall alike)."""
        if k < 0 or n < 1:
            raise ValueError(f'a span starts at an input frame k >= 0 and is n >= 1 intervals long, got k = {k!r}, n = {n!r}')
        j0 = -(-k * self.q // self.p)                     # the first j with j p / q >= k
        den, grid, j = self.q * n, [], j0
        while j * self.p < (k + n) * self.q:
            g, r = divmod((j * self.p - k * self.q) << self.times, den)
            grid.append(g + (2 * r > den or (2 * r == den and g & 1)))
            j += 1
        return Span(j0, tuple(grid))

    def span_error(self, k: int, n: int, j: int) -> Tuple[int, int]:
        """The snap error k + g n / 2^T - u_j of output j of span(k, n) in INPUT intervals, as (numerator, denominator > 0) with error()'s
        denominator: the instant the written frame stands for against the instant the output is shown at."""
        sp = self.span(k, n)
        g = sp.grid[j - sp.j]
        return (g * n + (k << self.times)) * self.q - (j * self.p << self.times), self.q << self.times

    def outputs(self, frames_in: int) -> int:
        """The frames a video of frames_in input frames converts to: the outputs at or before the last input frame."""
        if frames_in < 1:
            return 0
        last = (frames_in - 1) << self.times
        j = last * self.q // (self.p << self.times)          # u_j <= frames_in - 1 < u_(j + 1); rounding moves at most one output across
        while self.grid(j + 1) <= last:
            j += 1
        while j >= 0 and self.grid(j) > last:
            j -= 1
        return j + 1
