"""Reader and writer of YUV4MPEG2 (.y4m) streams of 8-bit and 10-bit planar Y'CbCr frames - the frames a Y'CbCr frame stream takes (film_stream_open
with FILM_PIX_I420 / FILM_PIX_I010: FilmEngine.open_stream(pix='i420' | 'i010')), so that video goes in and out without PNGs and without ffmpeg.

A stream is one header line, "YUV4MPEG2" and space-separated tokens - W<width> H<height> F<num>:<den> I<interlacing> A<n>:<d>
C<colour space> X<anything> ... - then per frame a line "FRAME[ <parameters>]" and the payload: Y [H][W], Cb [H/2][W/2], Cr [H/2][W/2],
which is the I420 layout.  A frame is handed on as one uint8 array [H * 3 // 2, W] (FilmStream.shape).  C420p10 (what
`ffmpeg -pix_fmt yuv420p10le` pipes) holds the same planes with one little-endian 16-bit word per sample, the 10-bit code in bits 0-9 - the
I010 layout; such a frame is handed on as one uint16 array [H * 3 // 2, W], and only by a reader opened with depths=(8, 10): a caller
written for uint8 arrays never receives uint16 by surprise.

Planar 4:2:2 and 4:4:4 - C422, C444 (8-bit) and C422p10, C444p10 (what `ffmpeg -pix_fmt yuv422p10le` / `yuv444p10le` pipe) - are read only by a
reader opened with chroma=('420', '422', '444') (or a part of it), like the depths: the payload is Y [H][W], then Cb and Cr [H][W/2] each (4:2:2,
W even, frames [2 * H, W]) or [H][W] each (4:4:4, any size, frames [3 * H, W]) - the I422 / I444 / I210 / I410 layouts; the reader's `.chroma`
and `.pix` say which.

Accepted: 8-bit C420, C420jpeg, C420mpeg2, C420paldv (no C token means 420) - the three differ in where the chroma samples sit, which
the engine's box treatment (include/film_hip.h) does not tell apart; Ip, I? or no I token.  Refused, with the token in the message:
mono, alpha (C444alpha), C411, 12-bit and deeper (and 10-bit, 4:2:2, 4:4:4 by a reader that was not asked for them), interlaced material, odd
sizes along a subsampled axis.
XCOLORRANGE=FULL marks full-range samples.
"""
from __future__ import annotations

import math
from typing import BinaryIO, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import pixfmt

MAGIC = b'YUV4MPEG2'
FRAME = b'FRAME'
C420 = ('420', '420jpeg', '420mpeg2', '420paldv')
C420_10 = ('420p10',)      # 10-bit 4:2:0, little-endian 16-bit words
# the planar 4:2:2 / 4:4:4 tokens: token -> (chroma, depth); and the stream layout (FilmEngine.open_stream's pix) of every (chroma, depth)
PIX_NAME = pixfmt.Y4M_PIX
C_OTHER = {c + ('p10' if d == 10 else ''): (c, d) for c, d in PIX_NAME if c != '420'}
CHROMAS = ('420', '422', '444')
_MAX_LINE = 4096


class Y4MError(ValueError):
    pass


def _read_exact(f: BinaryIO, n: int) -> bytes:
    """n bytes, or fewer at the end of the stream (a pipe hands out short reads)."""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return b''.join(parts)


def _read_line(f: BinaryIO) -> bytes:
    """One line without its newline; b'' at the end of the stream."""
    out = bytearray()
    while len(out) <= _MAX_LINE:
        c = f.read(1)
        if not c:
            if out:
                raise Y4MError(f'truncated: the stream ends inside the line {bytes(out[:40])!r}')
            return b''
        if c == b'\n':
            return bytes(out)
        out += c
    raise Y4MError(f'a line of more than {_MAX_LINE} bytes: not a YUV4MPEG2 stream')


def multiply_rate(tokens: Sequence[str], k: int) -> List[str]:
    """The header tokens with the numerator of the F token multiplied by the integer k >= 1 (k times the frames in the same time);
    everything else as it is."""
    if int(k) != k or k < 1:
        raise ValueError(f'the frame rate is multiplied by a positive integer, got {k!r}')
    out = []
    for t in tokens:
        if t[:1] == 'F' and ':' in t:
            num, den = t[1:].split(':', 1)
            t = f'F{int(num) * int(k)}:{den}'
        out.append(t)
    return out


def double_rate(tokens: Sequence[str]) -> List[str]:
    """The header tokens with the numerator of the F token doubled (twice the frames in the same time); everything else as it is."""
    return multiply_rate(tokens, 2)


def set_rate(tokens: Sequence[str], rate: Tuple[int, int]) -> List[str]:
    """The header tokens with the F token naming the frame rate num / den, as the reduced fraction (appended when there is no F token);
    everything else as it is."""
    num, den = int(rate[0]), int(rate[1])
    if num < 1 or den < 1:
        raise ValueError(f'a frame rate is a fraction of positive integers, got {rate!r}')
    g = math.gcd(num, den)
    f = f'F{num // g}:{den // g}'
    out = [f if t[:1] == 'F' and ':' in t else t for t in tokens]
    return out if f in out else out + [f]


def parse_header(line: bytes, depths: Sequence[int] = (8,), chroma: Sequence[str] = ('420',)) -> Tuple[int, int, List[str]]:
    """(width, height, tokens) of a header line; the refusals of this module.  depths: the sample depths the caller takes, 8 and / or 10;
    chroma: the subsamplings it takes, '420', '422' and / or '444'."""
    if not depths or any(d not in (8, 10) for d in depths):
        raise ValueError(f'depths must name 8 and / or 10, got {depths!r}')
    if not chroma or any(c not in CHROMAS for c in chroma):
        raise ValueError(f"chroma must name '420', '422' and / or '444', got {chroma!r}")
    colours = ((C420 if 8 in depths else ()) + (C420_10 if 10 in depths else ())) if '420' in chroma else ()
    colours += tuple(t for t, (c, d) in C_OTHER.items() if c in chroma and d in depths)
    parts = line.decode('ascii', 'replace').split()
    if not parts or parts[0] != MAGIC.decode():
        raise Y4MError(f'not a YUV4MPEG2 stream: it starts with {line[:16]!r}')
    tokens = parts[1:]
    w = h = None
    for t in tokens:
        key, val = t[:1], t[1:]
        if key == 'W' or key == 'H':
            if not val.isdigit() or int(val) < 1:
                raise Y4MError(f'bad size token {t!r}')
            if key == 'W':
                w = int(val)
            else:
                h = int(val)
        elif key == 'C' and val not in colours:
            if tuple(chroma) != ('420',) and (val in C_OTHER or val in C420 + C420_10):
                raise Y4MError(f'colour space token {t!r}: this reader was opened for {" / ".join(str(d) for d in depths)}-bit samples and '
                               f'chroma {" / ".join(chroma)} (depths={tuple(depths)!r}, chroma={tuple(chroma)!r})')
            if val in C420 + C420_10:
                raise Y4MError(f'colour space token {t!r}: this reader was opened for {" / ".join(str(d) for d in depths)}-bit samples '
                               f'(depths={tuple(depths)!r})')
            if 10 in depths:
                raise Y4MError(f'colour space token {t!r}: only 4:2:0 with 8-bit or 10-bit samples ({", ".join("C" + c for c in C420 + C420_10)}) '
                               'is read - no 4:2:2, 4:4:4, mono, 12-bit or deeper')
            raise Y4MError(f'colour space token {t!r}: only 8-bit 4:2:0 ({", ".join("C" + c for c in C420)}) is read - no 4:2:2, 4:4:4, '
                           'mono, 10-bit or deeper')
        elif key == 'I' and val not in ('p', '?'):
            raise Y4MError(f'interlacing token {t!r}: only progressive material (Ip, I? or no I token) is read')
    if w is None or h is None:
        raise Y4MError('the header names no W / H')
    c = chroma_of(tokens)
    if c == '420' and (w | h) & 1:
        raise Y4MError(f'tokens W{w} H{h}: a 4:2:0 frame stream needs even sizes')
    if c == '422' and w & 1:
        raise Y4MError(f'tokens W{w} H{h}: a 4:2:2 frame stream needs an even width')
    return w, h, tokens


def depth_of(tokens: Sequence[str]) -> int:
    """The sample depth the (accepted) tokens of a header name: 10 for C420p10 / C422p10 / C444p10, else 8."""
    return 10 if any(t[:1] == 'C' and (t[1:] in C420_10 or C_OTHER.get(t[1:], ('', 8))[1] == 10) for t in tokens) else 8


def chroma_of(tokens: Sequence[str]) -> str:
    """The subsampling the (accepted) tokens of a header name: '422' or '444' for their four tokens, else '420'."""
    for t in tokens:
        if t[:1] == 'C' and t[1:] in C_OTHER:
            return C_OTHER[t[1:]][0]
    return '420'


def frame_rows(chroma: str, height: int) -> int:
    """Rows of the [rows, W] array a frame is handed on as."""
    return height * 3 // 2 if chroma == '420' else 2 * height if chroma == '422' else 3 * height


class Y4MReader:
    """Iterates over the frames of a YUV4MPEG2 stream (a binary file object) as uint8 arrays [H * 3 // 2, W].  depths=(8, 10) also takes
    C420p10 streams, whose frames are uint16 arrays of that shape (decoded from little-endian bytes); `depth` says which it is.
    chroma=('420', '422', '444') also takes C422 / C444 (and, with depths=(8, 10), C422p10 / C444p10) streams, whose frames are [2 * H, W] /
    [3 * H, W]; `chroma` says which it is and `pix` names the stream layout (PIX_NAME)."""

    def __init__(self, f: BinaryIO, depths: Sequence[int] = (8,), chroma: Sequence[str] = ('420',)):
        self._f = f
        line = _read_line(f)
        if not line:
            raise Y4MError('empty stream: no YUV4MPEG2 header')
        self.width, self.height, self.tokens = parse_header(line, depths, chroma)
        self.depth = depth_of(self.tokens)
        self.chroma = chroma_of(self.tokens)
        self.pix = PIX_NAME[self.chroma, self.depth]
        self.rows = frame_rows(self.chroma, self.height)
        self.frame_bytes = self.width * self.rows * (2 if self.depth == 10 else 1)
        self.frames_read = 0

    @property
    def full_range(self) -> bool:
        return any(t.upper() == 'XCOLORRANGE=FULL' for t in self.tokens)

    @property
    def rate(self) -> Optional[Tuple[int, int]]:
        for t in self.tokens:
            if t[:1] == 'F' and ':' in t:
                num, den = t[1:].split(':', 1)
                return int(num), int(den)
        return None

    def read_frame(self) -> Optional[np.ndarray]:
        """The next frame, or None at the end of the stream; Y4MError when the stream ends inside a frame."""
        line = _read_line(self._f)
        if not line:
            return None
        if line != FRAME and not line.startswith(FRAME + b' '):
            raise Y4MError(f'frame {self.frames_read}: expected a FRAME line, got {line[:40]!r}')
        data = _read_exact(self._f, self.frame_bytes)
        if len(data) != self.frame_bytes:
            raise Y4MError(f'truncated: frame {self.frames_read} has {len(data)} of {self.frame_bytes} bytes')
        self.frames_read += 1
        if self.depth == 10:
            return np.frombuffer(data, '<u2').astype(np.uint16, copy=False).reshape(self.rows, self.width)
        return np.frombuffer(data, np.uint8).reshape(self.rows, self.width)

    def __iter__(self) -> Iterator[np.ndarray]:
        while True:
            fr = self.read_frame()
            if fr is None:
                return
            yield fr


class Y4MWriter:
    """Writes a YUV4MPEG2 stream: the header from `tokens` (as Y4MReader.tokens; W and H among them, checked like a reader's), then
    one frame per write(): uint8 arrays, or uint16 arrays (written as little-endian words) when the tokens say C420p10 / C422p10 / C444p10;
    [H * 3 // 2, W], or [2 * H, W] / [3 * H, W] when they say 4:2:2 / 4:4:4."""

    def __init__(self, f: BinaryIO, tokens: Sequence[str]):
        self._f = f
        self.tokens = list(tokens)
        self.width, self.height, _ = parse_header(' '.join([MAGIC.decode()] + self.tokens).encode('ascii'), (8, 10), CHROMAS)
        self.depth = depth_of(self.tokens)
        self.rows = frame_rows(chroma_of(self.tokens), self.height)
        self.frames_written = 0
        f.write(b' '.join([MAGIC] + [t.encode('ascii') for t in self.tokens]) + b'\n')

    def write(self, frame: np.ndarray) -> None:
        a = np.ascontiguousarray(frame)
        want = np.uint16 if self.depth == 10 else np.uint8
        if a.dtype != want or a.shape != (self.rows, self.width):
            raise ValueError(f'expected a {np.dtype(want).name} array of shape {(self.rows, self.width)}, got {a.dtype} {a.shape}')
        self._f.write(FRAME + b'\n')
        self._f.write(a.astype('<u2', copy=False).tobytes() if self.depth == 10 else a.tobytes())
        self.frames_written += 1


def header_tokens(width: int, height: int, rate: Tuple[int, int] = (30, 1), full_range: bool = False, colour: str = '420jpeg') -> List[str]:
    """Tokens of a progressive stream with square pixels: 8-bit 4:2:0, 10-bit with colour='420p10', or planar 4:2:2 / 4:4:4 with colour='422' |
    '444' | '422p10' | '444p10'."""
    return [f'W{width}', f'H{height}', f'F{rate[0]}:{rate[1]}', 'Ip', 'A1:1', f'C{colour}'] + (['XCOLORRANGE=FULL'] if full_range else [])
