"""Device-resident plumbing around the engine: PyTorch-ROCm tensors for memory and streams only.

The hot path is entirely inside libfilm_hip.so (film_interpolate: pad / patch / model / crop / stitch);
torch is used here only to hold frames in HBM and to hand raw pointers + the current stream to the C-ABI.
pad_to_align / image_to_patches / patches_to_image below are torch restatements of the reference's layout
rules, kept for tests and for callers that want the patches themselves.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import pixfmt
from .engine import FilmEngine, frame_diff_device, frame_histogram_device


def pinned_frame(shape) -> 'np.ndarray':
    """A float32 numpy array in page-locked host memory (the tensor that owns it rides along as `.base`): frames handed to
    Interpolator.__call__ / FilmEngine.interpolate_frames in such arrays move at the PCIe rate without the runtime pinning pageable pages per call."""
    return torch.empty(tuple(int(v) for v in shape), dtype=torch.float32, pin_memory=True).numpy()


def pad_to_align(x: torch.Tensor, align: int) -> Tuple[torch.Tensor, Tuple[int, int, int, int]]:
    """[B,H,W,C] -> zero padded to multiples of align, offset pad//2 (eval/interpolator.py:30-63)."""
    b, h, w, c = x.shape
    hp = (align - h % align) if h % align else 0
    wp = (align - w % align) if w % align else 0
    oy, ox = hp // 2, wp // 2
    if hp == 0 and wp == 0:
        return x.contiguous(), (0, 0, h, w)
    out = torch.zeros((b, h + hp, w + wp, c), dtype=x.dtype, device=x.device)
    out[:, oy:oy + h, ox:ox + w, :] = x
    return out, (oy, ox, h, w)


def image_to_patches(image: torch.Tensor, block_shape: List[int]) -> torch.Tensor:
    """[1,H,W,C] -> [bh*bw, H/bh, W/bw, C], row-major blocks (eval/interpolator.py:66-99)."""
    bh, bw = block_shape
    _, h, w, c = image.shape
    ph, pw = h // bh, w // bw
    assert h == ph * bh, 'block_height=%d should evenly divide height=%d.' % (bh, h)
    assert w == pw * bw, 'block_width=%d should evenly divide width=%d.' % (bw, w)
    return image[0].reshape(bh, ph, bw, pw, c).permute(0, 2, 1, 3, 4).reshape(bh * bw, ph, pw, c).contiguous()


def patches_to_image(patches: torch.Tensor, block_shape: List[int]) -> torch.Tensor:
    """inverse of image_to_patches (eval/interpolator.py:102-126)."""
    bh, bw = block_shape
    _, ph, pw, c = patches.shape
    return patches.reshape(bh, bw, ph, pw, c).permute(0, 2, 1, 3, 4).reshape(1, bh * ph, bw * pw, c).contiguous()


def pix_dtypes(pix: str):
    """The torch dtypes a frame of pixel type `pix` may have.  A 10-bit frame is 16-bit words: torch.int16 is taken as a bit pattern, and
    torch.uint16 where the installed torch has it."""
    if pixfmt.BY_NAME[pix].dtype.__name__ == 'uint16':
        return (torch.int16,) + ((torch.uint16,) if hasattr(torch, 'uint16') else ())
    return (torch.float32,) if pix == 'f32' else (torch.uint8,)


def frame_histogram(frame: torch.Tensor, pix: str = 'u8') -> torch.Tensor:
    """film_frame_histogram of one CUDA frame of pixel type `pix` (film_hip/pixfmt.py; shape and dtype as FilmStream describes them: [H,W,3]
    uint8 or float32, or a Y'CbCr frame [H * 3 // 2, W] / [2 * H, W] / [3 * H, W], uint8 or - 10-bit, bin = code >> 2 - int16 / uint16)
    -> int64 [3, 256] on the frame's device: the number of samples of every plane with every 8-bit code (include/film_hip.h, "Scene
    cuts").  Asynchronous on the current torch stream."""
    assert frame.is_cuda and frame.dtype in pix_dtypes(pix)
    frame = frame.contiguous()
    h, w = pixfmt.frame_size(pix, tuple(frame.shape))
    hist = torch.empty((3, 256), dtype=torch.int32, device=frame.device)
    with torch.cuda.device(frame.device):
        frame_histogram_device(frame.data_ptr(), h, w, hist.data_ptr(), pix, stream=torch.cuda.current_stream(frame.device).cuda_stream)
    return hist.to(torch.int64)      # (counts stay below 2^31: H * W < 2^31)


def frame_diff(a: torch.Tensor, b: torch.Tensor, pix: str = 'u8', lo: int = 0) -> torch.Tensor:
    """film_frame_diff of two CUDA frames of pixel type `pix` (shapes and dtypes as frame_histogram takes them, both alike and on one device)
    -> int64 [3, 4] on the frames' device: per plane the total, the maximum, the number above `lo` (strictly; 0 .. 65535, stored-code units)
    and the number of the 8 x 8 block SADs between the two frames, on full-depth codes (include/film_hip.h, "Duplicate frames").
    Asynchronous on the current torch stream."""
    assert a.is_cuda and a.dtype in pix_dtypes(pix) and b.device == a.device and b.dtype == a.dtype and b.shape == a.shape
    a, b = a.contiguous(), b.contiguous()
    h, w = pixfmt.frame_size(pix, tuple(a.shape))
    out = torch.empty((3, 4), dtype=torch.int64, device=a.device)   # (the twelve uint64 stay far below 2^63)
    with torch.cuda.device(a.device):
        frame_diff_device(a.data_ptr(), b.data_ptr(), h, w, out.data_ptr(), pix, lo=lo, stream=torch.cuda.current_stream(a.device).cuda_stream)
    return out


class DeviceStream:
    """A frame stream on frames that already live in HBM (DeviceInterpolator.stream): push(frame) takes a [H,W,3] CUDA tensor, float32
    or uint8 as opened (a 4:2:0 stream: uint8 [H * 3 // 2, W]; a 10-bit one: int16 or uint16 of that shape), and returns the mid-frame between it and the frame pushed before as a new tensor of the same kind - None for
    the first frame after opening or reset(), and for a frame that the engine option "scene_cut" found to start a new scene.  Asynchronous on the
    current torch stream (with "scene_cut" > 0 a push waits for the frame's histogram: include/film_hip.h).
    times > 1: a primed push returns the [2^times - 1, *frame shape] frames of the times_to_interpolate recursion (FilmStream)."""

    def __init__(self, engine: FilmEngine, h: int, w: int, align, block_shape, pix: str, matrix: str = 'bt709', full_range: bool = False,
                 scene_cut: int = 0, times: int = 1, dedup=None):
        self._stream = engine.open_stream(h, w, align=align, block_shape=block_shape, pix=pix, matrix=matrix, full_range=full_range,
                                          scene_cut=scene_cut, times=times, dedup=dedup)
        self._dtypes = pix_dtypes(pix)

    def push(self, frame: torch.Tensor) -> Optional[torch.Tensor]:
        assert frame.is_cuda and frame.dtype in self._dtypes and tuple(frame.shape) == self._stream.shape
        frame = frame.contiguous()
        st = self._stream
        out = torch.empty_like(frame) if st.times == 1 else torch.empty((len(st.selection),) + tuple(frame.shape), dtype=frame.dtype, device=frame.device)
        stream = torch.cuda.current_stream(frame.device).cuda_stream
        return out if st.push_device(frame.data_ptr(), out.data_ptr(), stream) else None

    def select(self, positions=None) -> None:
        """FilmStream.select: a primed push returns only the frames at these 1-based positions, [len(selection), *frame shape] (None: all)."""
        self._stream.select(positions)

    @property
    def selection(self):
        return self._stream.selection

    def reset(self) -> None:
        self._stream.reset()

    def cut_info(self):
        """FilmStream.cut_info: (distance, samples, cut) of the last push (engine option "scene_cut")."""
        return self._stream.cut_info()

    def dup_info(self):
        """FilmStream.dup_info: (stats [3, 4] or None, dup) of the last push (engine option "dup_hi"): a push dropped as a duplicate of the
        carried frame returned None and changed nothing."""
        return self._stream.dup_info()

    def layout(self) -> dict:
        """FilmStream.layout: tiles, tile groups, tiles per group, workspace and carry bytes of the open stream."""
        return self._stream.layout()

    def close(self) -> None:
        self._stream.close()

    def __enter__(self) -> 'DeviceStream':
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class DeviceInterpolator:
    """Interpolator.__call__ semantics (eval/interpolator.py:178-209) on frames that already live
    in HBM: float32 CUDA(=HIP) tensors in, float32 CUDA tensor out, no host round trip.

    Asynchronous on the current torch stream.  block_overlap (an int or (height, width); -1 = what the align padding holds): overlapped,
    cross-faded tiles - an option of the ENGINE (eval.interpolator.Interpolator), so 0 (default) leaves the engine as it is."""

    def __init__(self, engine: FilmEngine, align: Optional[int] = None, block_shape: Optional[List[int]] = None, *, block_overlap=0):
        self._engine = engine
        if block_overlap not in (0, (0, 0), [0, 0]):
            engine.set_block_overlap(block_overlap)
        self._align = align or None
        self._block_shape = block_shape or None

    def _run(self, x0: torch.Tensor, x1: torch.Tensor, block_shape) -> torch.Tensor:
        assert x0.is_cuda and x0.dtype == torch.float32 and x0.shape == x1.shape and x0.shape[-1] == 3
        x0 = x0.contiguous()
        x1 = x1.contiguous()
        b, h, w, _ = x0.shape
        out = torch.empty_like(x0)
        stream = torch.cuda.current_stream(x0.device).cuda_stream
        self._engine.interpolate_frames_device(x0.data_ptr(), x1.data_ptr(), b, h, w, out.data_ptr(),
                                               align=self._align, block_shape=block_shape, stream=stream)
        return out

    def interpolate(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """Interpolator.interpolate (eval/interpolator.py:152-176): pad to align, model, crop - inside
        film_interpolate (HIP kernels read these tensors and write the result tensor directly)."""
        return self._run(x0, x1, None)

    def batch(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """Extension: Interpolator.__call__ applied to every pair of a batch (tiled or not) in one call."""
        bs = self._block_shape
        return self._run(x0, x1, bs if bs is not None and bs[0] * bs[1] > 1 else None)

    def sequence(self, frames: torch.Tensor) -> torch.Tensor:
        """Extension: the mid-frames of every consecutive pair of frames [F,H,W,3] -> [F-1,H,W,3] (film_interpolate_sequence: one feature
        extraction per frame).  Bit-identical to batch(frames[:-1], frames[1:]), tiled by block_shape the same way."""
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 4 and frames.shape[-1] == 3
        frames = frames.contiguous()
        f, h, w, _ = frames.shape
        out = torch.empty((f - 1, h, w, 3), dtype=frames.dtype, device=frames.device)
        bs = self._block_shape
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        self._engine.interpolate_sequence_device(frames.data_ptr(), f, h, w, out.data_ptr(), align=self._align,
                                                 block_shape=bs if bs is not None and bs[0] * bs[1] > 1 else None, stream=stream)
        return out

    def stream(self, h: int, w: int, pix: str = 'f32', matrix: str = 'bt709', full_range: bool = False, scene_cut: int = 0,
               times: int = 1, dedup=None) -> DeviceStream:
        """Extension: a frame stream of h x w frames (film_stream_*), padded / tiled like batch(): push one CUDA tensor at a time, float32
        or ('u8') uint8, and get the mid-frame with the frame before - bit-identical to batch(previous, frame), one extraction per frame.
        A Y'CbCr pix (film_hip/pixfmt.py; FilmStream describes the frames): tensors of the frame's shape, converted inside the cut and the
        quantisation; uint8, or for the 10-bit layouts 16-bit - torch.int16 (taken as a bit pattern) or torch.uint16 where the installed
        torch has it; the mid-frame comes back in the dtype that was pushed.
        matrix: 'bt709' | 'bt601' | 'bt2020nc', for every Y'CbCr layout.
        scene_cut (0 .. 1000 permille): non-zero sets the ENGINE option "scene_cut" before the stream opens, and it stays set (like block_overlap).
        times (1 .. 6): the stream's "stream_times" - a primed push returns [2^times - 1, ...] frames, the times_to_interpolate recursion.
        dedup (None | hi | (hi, lo, frac)): not None sets the ENGINE options "dup_hi" / "dup_lo" / "dup_frac" before the stream opens, and they stay
        set (like scene_cut): a push judged a duplicate of the carried frame returns None and changes nothing (DeviceStream.dup_info)."""
        bs = self._block_shape
        return DeviceStream(self._engine, h, w, self._align, bs if bs is not None and bs[0] * bs[1] > 1 else None, pix, matrix, full_range,
                            scene_cut, times, dedup)

    def __call__(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        if self._block_shape is not None and self._block_shape[0] * self._block_shape[1] > 1:
            if x0.shape[0] != 1:    # the reference's tiled path takes one pair (eval/interpolator.py:96-98); see .batch
                raise ValueError(f'the tiled path takes one frame pair per call, got a batch of {x0.shape[0]}; '
                                 'use DeviceInterpolator.batch for batches of tiled frames')
            return self._run(x0, x1, self._block_shape)
        return self._run(x0, x1, None)
