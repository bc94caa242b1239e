"""Device-resident, breadth-first version of the reference's recursive mid-point driver.

The reference (eval/util.py:62-91, _recursive_generator) subdivides depth first: one Interpolator call with
batch size 1 per generated frame, each returning to numpy.  A mid-frame depends only on its two parents, so
the 2^(d-1) frames of recursion depth d are independent: here they are ONE film_interpolate call on a batch of
2^(d-1) frame pairs (times the tiles of block_shape), parents and children stay in HBM, and the frames come
back in the same temporal order with bit-identical values (tests/test_gpu_parity.py).

Per input pair and T recursions: T engine calls instead of 2^T - 1, no host round trips.
"""
from __future__ import annotations

from typing import Iterable, List

import torch

from .torch_io import DeviceInterpolator


def interpolate_pair_recursively(frame1: torch.Tensor, frame2: torch.Tensor, times_to_interpolate: int,
                                 interpolator: DeviceInterpolator) -> torch.Tensor:
    """frame1, frame2: [H,W,3] float32 CUDA tensors.  Returns [2^T + 1, H, W, 3]: frame1, the 2^T - 1 generated
    frames in temporal order, frame2 (eval/util.py:62-91 yields the same sequence without frame2)."""
    frames = torch.stack([frame1, frame2]).contiguous()
    for _ in range(times_to_interpolate):
        mids = interpolator.batch(frames[:-1].contiguous(), frames[1:].contiguous())
        out = torch.empty((2 * frames.shape[0] - 1,) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
        out[0::2] = frames
        out[1::2] = mids
        frames = out
    return frames


def interpolate_recursively(frames: List[torch.Tensor], times_to_interpolate: int,
                            interpolator: DeviceInterpolator) -> Iterable[torch.Tensor]:
    """Device twin of eval/util.py:125-153 interpolate_recursively_from_memory: yields (n-1)*2^T + 1 frames."""
    n = len(frames)
    for i in range(1, n):
        seq = interpolate_pair_recursively(frames[i - 1], frames[i], times_to_interpolate, interpolator)
        for k in range(seq.shape[0] - 1):
            yield seq[k]
    yield frames[-1]


def interpolate_sequence_recursively(frames: List[torch.Tensor], times_to_interpolate: int,
                                     interpolator: DeviceInterpolator) -> List[torch.Tensor]:
    """The same (n-1)*2^T + 1 frames as interpolate_recursively, breadth first over the WHOLE sequence: depth d is one
    DeviceInterpolator.sequence call on the (n-1)*2^(d-1) + 1 frames of depth d - 1 (one feature extraction per frame, and the
    pairs of different input pairs in one batch), its mid-frames interleaved with them.  Bit-identical to interpolate_recursively."""
    seq = torch.stack(list(frames)).contiguous()
    for _ in range(times_to_interpolate):
        seq = _interleave(seq, interpolator.sequence(seq))
    return list(seq)


def _interleave(frames: torch.Tensor, mids: torch.Tensor) -> torch.Tensor:
    out = torch.empty((2 * frames.shape[0] - 1,) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
    out[0::2] = frames
    out[1::2] = mids
    return out


class Uint8FrameStream:
    """The recursion of ONE input pair as a stream of quantised frames (round 4; replaces "all 2^T + 1 float32 frames in one
    blocking .cpu()" for callers that write files - eval/interpolator_cli.py).

    Breadth first on the device as interpolate_pair_recursively; behind every depth its 2^(d-1) new frames are quantised ON THE
    DEVICE (film_to_uint8: clip(x * 255, 0, 255) + 0.5 truncated, the reference's write_image rounding - eval/util.py:51-52 - on
    the float32 values, so the bytes are the ones the host rounding gives), copied into pinned host memory on a COPY stream
    (1 byte per value over PCIe instead of 4) and handed to `sink(index, uint8 [H,W,3])` from a worker thread while the next
    depth computes.  The float32 frames stay in HBM for the deeper levels, exactly as before.  index = position in the
    2^T + 1 long temporal sequence (0 and 2^T are the inputs and are not emitted)."""

    def __init__(self, interpolator: DeviceInterpolator, engine, workers: int = 2):
        import concurrent.futures
        self._it = interpolator
        self._engine = engine
        self._copy_stream = torch.cuda.Stream(device=torch.device('cuda', engine.device))
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=workers)
        self._pinned = {}          # depth -> pinned uint8 buffer (reused across pairs)

    def run(self, frame1: torch.Tensor, frame2: torch.Tensor, times_to_interpolate: int, sink) -> List:
        """Returns the futures of the hand-offs (wait on them before reusing the sink's targets)."""
        T = times_to_interpolate
        frames = torch.stack([frame1, frame2]).contiguous()
        compute = torch.cuda.current_stream(frames.device)
        futures = []
        for d in range(1, T + 1):
            mids = self._it.batch(frames[:-1].contiguous(), frames[1:].contiguous())
            u8 = torch.empty(mids.shape, dtype=torch.uint8, device=mids.device)
            self._engine.to_uint8_device(mids.data_ptr(), u8.data_ptr(), mids.numel(), stream=compute.cuda_stream)
            ready = torch.cuda.Event()
            ready.record(compute)
            host = self._pinned.get((d, tuple(mids.shape)))
            if host is None:
                host = torch.empty(mids.shape, dtype=torch.uint8, pin_memory=True)
                self._pinned[(d, tuple(mids.shape))] = host
            done = torch.cuda.Event()
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(ready)
                host.copy_(u8, non_blocking=True)
                u8.record_stream(self._copy_stream)
                done.record(self._copy_stream)
            step = 2 ** (T - d)

            def hand_off(done=done, host=host, step=step, count=mids.shape[0]):
                done.synchronize()
                arr = host.numpy()
                for j in range(count):
                    sink((2 * j + 1) * step, arr[j].copy())   # (the pinned buffer is reused by the next pair)
            futures.append(self._pool.submit(hand_off))
            out = torch.empty((2 * frames.shape[0] - 1,) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
            out[0::2] = frames
            out[1::2] = mids
            frames = out
        return futures

    def close(self) -> None:
        self._pool.shutdown(wait=True)


class Uint8SequenceStream:
    """Uint8FrameStream for a WINDOW of consecutive input frames: the recursion of all its pairs breadth first, each depth one
    DeviceInterpolator.sequence call over the window's frames of the previous depth; behind every depth its new frames are quantised
    on the device (film_to_uint8), copied to pinned host memory on a copy stream and handed to `sink(index, uint8 [H,W,3])` from a
    worker thread while the next depth computes.  index = position in the window's (m-1)*2^T + 1 long temporal sequence (the m
    input frames, at multiples of 2^T, are not emitted)."""

    def __init__(self, interpolator: DeviceInterpolator, engine, workers: int = 2):
        import concurrent.futures
        self._it = interpolator
        self._engine = engine
        self._copy_stream = torch.cuda.Stream(device=torch.device('cuda', engine.device))
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=workers)
        self._pinned = {}          # (depth, shape) -> pinned uint8 buffer (reused across windows)

    def run(self, frames: torch.Tensor, times_to_interpolate: int, sink) -> List:
        """frames: [m,H,W,3] float32 on the device, m >= 2.  Returns the futures of the hand-offs."""
        T = times_to_interpolate
        seq = frames.contiguous()
        compute = torch.cuda.current_stream(seq.device)
        futures = []
        for d in range(1, T + 1):
            mids = self._it.sequence(seq)
            u8 = torch.empty(mids.shape, dtype=torch.uint8, device=mids.device)
            self._engine.to_uint8_device(mids.data_ptr(), u8.data_ptr(), mids.numel(), stream=compute.cuda_stream)
            ready = torch.cuda.Event()
            ready.record(compute)
            host = self._pinned.get((d, tuple(mids.shape)))
            if host is None:
                host = torch.empty(mids.shape, dtype=torch.uint8, pin_memory=True)
                self._pinned[(d, tuple(mids.shape))] = host
            done = torch.cuda.Event()
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(ready)
                host.copy_(u8, non_blocking=True)
                u8.record_stream(self._copy_stream)
                done.record(self._copy_stream)
            step = 2 ** (T - d)

            def hand_off(done=done, host=host, step=step, count=mids.shape[0]):
                done.synchronize()
                arr = host.numpy()
                for j in range(count):
                    sink((2 * j + 1) * step, arr[j].copy())   # (the pinned buffer is reused by the next window)
            futures.append(self._pool.submit(hand_off))
            seq = _interleave(seq, mids)
        return futures

    def close(self) -> None:
        self._pool.shutdown(wait=True)
