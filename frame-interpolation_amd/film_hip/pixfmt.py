"""The pixel types of a frame stream (include/film_hip.h, FILM_PIX_*), one row each: what engine.py, torch_io.py, y4m.py, eval/video_cli.py and
tools/stream_bench.py know about a layout comes from here.  Imports numpy only (y4m.py stays free of the engine and of torch).
depth: the bits of a code (10-bit codes lie in 16-bit words), None for the two RGB types; (sx, sy): the chroma shifts - (1, 1) 4:2:0, (1, 0) 4:2:2,
(0, 0) 4:4:4; semi_planar: one plane of CbCr pairs behind the Y plane, not a Cb and a Cr plane.  A Y'CbCr frame is one array [rows, W] of samples."""
import collections
from typing import Tuple

import numpy as np

Layout = collections.namedtuple('Layout', 'name code dtype depth sx sy semi_planar')
LAYOUTS = (
    Layout('f32', 0, np.float32, None, 0, 0, False),
    Layout('u8', 1, np.uint8, None, 0, 0, False),
    Layout('i420', 16, np.uint8, 8, 1, 1, False),
    Layout('nv12', 17, np.uint8, 8, 1, 1, True),
    Layout('i010', 32, np.uint16, 10, 1, 1, False),       # the code in bits 0-9 of a word (= yuv420p10le)
    Layout('p010', 33, np.uint16, 10, 1, 1, True),        # the code in bits 6-15
    Layout('i422', 20, np.uint8, 8, 1, 0, False),
    Layout('i444', 24, np.uint8, 8, 0, 0, False),
    Layout('i210', 36, np.uint16, 10, 1, 0, False),
    Layout('i410', 40, np.uint16, 10, 0, 0, False),
)
BY_NAME = {lay.name: lay for lay in LAYOUTS}
CHROMA = {(1, 1): '420', (1, 0): '422', (0, 0): '444'}      # the chroma shifts under the name Y4M and the engine's messages give them
# (chroma, depth) -> the planar layout a YUV4MPEG2 stream of that kind is: ('420', 8) -> 'i420' ... ('444', 10) -> 'i410'
Y4M_PIX = {(CHROMA[lay.sx, lay.sy], lay.depth): lay.name for lay in LAYOUTS if lay.depth and not lay.semi_planar}


def is_yuv(pix: str) -> bool:
    return BY_NAME[pix].depth is not None


def names(chroma: str = None) -> Tuple[str, ...]:
    """The Y'CbCr layouts, all or those of one subsampling ('420' | '422' | '444'), in the table's order."""
    return tuple(lay.name for lay in LAYOUTS if lay.depth and chroma in (None, CHROMA[lay.sx, lay.sy]))


def _rows(lay) -> Tuple[int, int]:
    """Rows of a frame per row of the picture, as a fraction: (3, 2), (2, 1) or (3, 1)."""
    return (3, 2) if lay.sy else (2, 1) if lay.sx else (3, 1)


def frame_shape(pix: str, h: int, w: int) -> Tuple[int, ...]:
    """The array shape of one h x w frame of pixel type `pix`: [H, W, 3] for the RGB types, [H * 3 // 2, W] / [2 * H, W] / [3 * H, W] samples
    for the 4:2:0 / 4:2:2 / 4:4:4 layouts."""
    h, w = int(h), int(w)
    if pix not in BY_NAME or not is_yuv(pix):      # (a name the table lacks has the RGB shape; pix_code is what refuses it)
        return (h, w, 3)
    num, den = _rows(BY_NAME[pix])
    return (h * num // den, w)


def frame_size(pix: str, shape) -> Tuple[int, int]:
    """The inverse of frame_shape: (h, w) of the picture in a frame array of that shape."""
    if not is_yuv(pix):
        assert len(shape) == 3 and shape[-1] == 3
        return int(shape[0]), int(shape[1])
    num, den = _rows(BY_NAME[pix])
    assert len(shape) == 2 and shape[0] % num == 0
    return int(shape[0]) * den // num, int(shape[1])
