"""Host-side frame IO and the recursive mid-point driver (mirror of the reference's eval/util.py).

Same function names, arguments and rounding rules as the reference module; TensorFlow's image codecs
(tf.io.decode_image / encode_png / encode_jpeg, reference eval/util.py:38-59) are replaced by PIL.
"""
import os
import shutil
from typing import Generator, Iterable, List, Optional

import numpy as np

from . import interpolator as interpolator_lib

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None

_UINT8_MAX_F = float(np.iinfo(np.uint8).max)
_CONFIG_FFMPEG_NAME_OR_PATH = 'ffmpeg'


def _pil():
    from PIL import Image, PngImagePlugin
    # photos/one.png carries a very large zTXt chunk; PIL refuses it by default.
    PngImagePlugin.MAX_TEXT_CHUNK = max(PngImagePlugin.MAX_TEXT_CHUNK, 256 * 1024 * 1024)
    Image.MAX_IMAGE_PIXELS = None
    return Image


def read_image(filename: str) -> np.ndarray:
    """8-bit sRGB file -> float32 [H,W,3] in [0,1] (uint8 / 255, reference eval/util.py:29-41)."""
    with _pil().open(filename) as im:
        rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    return rgb.astype(np.float32) / _UINT8_MAX_F


def read_image_uint8(filename: str) -> np.ndarray:
    """8-bit sRGB file -> uint8 [H,W,3]: read_image without the conversion to float32 (read_image(f) == read_image_uint8(f) / 255)."""
    with _pil().open(filename) as im:
        return np.asarray(im.convert('RGB'), dtype=np.uint8)


def to_uint8(image: np.ndarray) -> np.ndarray:
    """clip(x*255, 0, 255) + 0.5, truncated to uint8 - the reference's rounding (eval/util.py:51-52)."""
    scaled = np.clip(image * _UINT8_MAX_F, 0.0, _UINT8_MAX_F)
    return (scaled + 0.5).astype(np.uint8)


def write_image(filename: str, image: np.ndarray) -> None:
    """float32 [H,W,3] in [0,1] -> .jpg when the extension says so, PNG otherwise (eval/util.py:44-59)."""
    pixels = to_uint8(image)
    Image = _pil()
    extension = os.path.splitext(filename)[1]
    if extension == '.jpg':
        Image.fromarray(pixels, 'RGB').save(filename, format='JPEG', quality=95)
    else:
        Image.fromarray(pixels, 'RGB').save(filename, format='PNG')


def write_image_uint8(filename: str, pixels: np.ndarray) -> None:
    """write_image for pixels that are already quantised (uint8 [H,W,3]): the same encoder settings, so the same file bytes as
    write_image(filename, x) whenever pixels == to_uint8(x)."""
    Image = _pil()
    if os.path.splitext(filename)[1] == '.jpg':
        Image.fromarray(pixels, 'RGB').save(filename, format='JPEG', quality=95)
    else:
        Image.fromarray(pixels, 'RGB').save(filename, format='PNG')


def interpolate_pairs_to_files(inputs: List[str], first: int, end: int, n_pairs: int, times_to_interpolate: int,
                               interpolator: 'interpolator_lib.Interpolator', frames_dir: str, keep: bool = False,
                               workers: Optional[int] = None):
    """Input pairs [first, end) of `inputs` -> frames_dir/frame_%03d.png with the reference's numbering (frame k of pair p at
    p * 2^T + k; the owner of the last pair also writes the final input frame - eval/interpolator_cli.py:127-149,
    eval/util.py:94-123), as a PIPELINE (round 4): the recursion of a pair runs breadth first on the device
    (film_hip.recursive.Uint8FrameStream), each depth's frames are quantised on the device, cross PCIe as bytes on a copy stream
    and are PNG-encoded by a thread pool while the next depth / the next pair computes; the next input file is decoded meanwhile.
    Byte-identical files to write_image(interpolate_recursively_from_files(...)).  Returns (frames written, [uint8 frames in
    order] if keep else None).  Needs the HIP-backed Interpolator; returns None for any other callable (callers fall back)."""
    engine = getattr(interpolator, 'engine', None)
    if engine is None or engine.device < 0 or os.environ.get('FILM_HOST_RECURSION') == '1':
        return None
    import concurrent.futures
    import torch
    from film_hip.recursive import Uint8FrameStream
    from film_hip.torch_io import DeviceInterpolator
    T = times_to_interpolate
    step = 2 ** T
    dev = torch.device('cuda', engine.device)
    dev_it = DeviceInterpolator(engine, align=interpolator.align, block_shape=interpolator.block_shape)
    nw = workers or max(2, min(32, (os.cpu_count() or 4)))
    kept = {} if keep else None
    written = 0
    with torch.cuda.device(dev), concurrent.futures.ThreadPoolExecutor(max_workers=nw) as enc:
        stream = Uint8FrameStream(dev_it, engine)
        pending = []

        def emit(index: int, pixels: np.ndarray) -> None:
            if kept is not None:
                kept[index] = pixels
            pending.append(enc.submit(write_image_uint8, f'{frames_dir}/frame_{index:03d}.png', pixels))

        reads = {}
        try:
            # decode ahead: the two inputs of the first pair at once, then always one file beyond the pair being interpolated
            reads = {i: enc.submit(read_image, inputs[i]) for i in range(first, min(first + 2, end + 1))} if end > first else {}
            for p in range(first, end):
                f1 = reads.pop(p).result() if p in reads else read_image(inputs[p])
                f2 = reads[p + 1].result()                      # (stays in `reads`: it is the next pair's first frame)
                if p + 2 <= end:
                    reads[p + 2] = enc.submit(read_image, inputs[p + 2])
                emit(p * step, to_uint8(f1))
                written += 1
                if T > 0:
                    a = torch.from_numpy(np.ascontiguousarray(f1, dtype=np.float32)).to(dev, non_blocking=False)
                    b = torch.from_numpy(np.ascontiguousarray(f2, dtype=np.float32)).to(dev, non_blocking=False)
                    futs = stream.run(a, b, T, lambda k, px, base=p * step: emit(base + k, px))
                    for fu in futs:
                        fu.result()
                    written += step - 1
                if p == n_pairs - 1:
                    emit((p + 1) * step, to_uint8(f2))
                    written += 1
            for fu in pending:
                fu.result()
        except BaseException:
            # a failed forward / decode / encode: do not let the queued PNG writes run on (a half-written frames directory that
            # looks finished), do not leak the stream's worker pool (round-4 ADVICE)
            for fu in pending:
                fu.cancel()
            for fu in reads.values():
                fu.cancel()
            raise
        finally:
            stream.close()
            engine.save_tune_cache()
    return written, ([kept[i] for i in sorted(kept)] if kept is not None else None)


def interpolate_stream_to_files(inputs: List[str], first: int, end: int, n_pairs: int, interpolator: 'interpolator_lib.Interpolator',
                                frames_dir: str, keep: bool = False, workers: Optional[int] = None):
    """interpolate_pairs_to_files for times_to_interpolate == 1 through a frame stream (eval/interpolator_cli.py --stream): the input
    frames [first, end] are decoded as bytes (no float32 frame on the host), pushed one by one through an 8-bit stream
    (Interpolator.open_stream(pix='u8'): one byte per value each way, one feature extraction per frame) and the mid-frames come back
    as bytes; decoding and PNG encoding run on a thread pool beside the pushes.  An input frame is written as decoded:
    to_uint8(u8 / 255) == u8 for every byte value.  Same file names and bytes as interpolate_pairs_to_files; same return value; None
    for an Interpolator that is not HIP-backed."""
    engine = getattr(interpolator, 'engine', None)
    if engine is None or engine.device < 0 or os.environ.get('FILM_HOST_RECURSION') == '1':
        return None
    import concurrent.futures
    nw = workers or max(2, min(32, (os.cpu_count() or 4)))
    kept = {} if keep else None
    written = 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=nw) as enc:
        pending = []

        def emit(index: int, pixels: np.ndarray) -> None:
            nonlocal written
            if kept is not None:
                kept[index] = pixels
            pending.append(enc.submit(write_image_uint8, f'{frames_dir}/frame_{index:03d}.png', pixels))
            written += 1

        reads = {}
        stream = None
        try:
            reads = {i: enc.submit(read_image_uint8, inputs[i]) for i in range(first, min(first + 2, end + 1))} if end > first else {}
            for i in range(first, end + 1 if end > first else first):
                px = reads.pop(i).result()
                if i + 2 <= end:
                    reads[i + 2] = enc.submit(read_image_uint8, inputs[i + 2])     # decode ahead of the push
                if stream is None:      # (the first frame of the range primes the stream: it produces nothing)
                    stream = interpolator.open_stream(px.shape[0], px.shape[1], pix='u8')
                mid = stream.push(px)
                if mid is not None:
                    emit(2 * i - 1, mid)
                if i < end or i == n_pairs:     # the owner of the last pair also writes the final input frame
                    emit(2 * i, px)
            for fu in pending:
                fu.result()
        except BaseException:
            for fu in pending:
                fu.cancel()
            for fu in reads.values():
                fu.cancel()
            raise
        finally:
            if stream is not None:
                stream.close()
            engine.save_tune_cache()
    return written, ([kept[i] for i in sorted(kept)] if kept is not None else None)


def interpolate_windows_to_files(inputs: List[str], first: int, end: int, n_pairs: int, times_to_interpolate: int,
                                 interpolator: 'interpolator_lib.Interpolator', frames_dir: str, window: int, keep: bool = False,
                                 workers: Optional[int] = None):
    """interpolate_pairs_to_files in sequence mode (eval/interpolator_cli.py --sequence_window): input pairs [first, end) in windows of
    `window` consecutive input frames (window - 1 pairs; a window's last frame is the next window's first), the recursion of a
    window breadth first on the device with one feature extraction per frame and depth (film_hip.recursive.Uint8SequenceStream).
    Same file names and bytes as interpolate_pairs_to_files; same return value; None for an Interpolator that is not HIP-backed."""
    engine = getattr(interpolator, 'engine', None)
    if engine is None or engine.device < 0 or os.environ.get('FILM_HOST_RECURSION') == '1':
        return None
    if window < 2:
        raise ValueError(f'a sequence window holds at least 2 frames, got {window}')
    import concurrent.futures
    import torch
    from film_hip.recursive import Uint8SequenceStream
    from film_hip.torch_io import DeviceInterpolator
    T = times_to_interpolate
    step = 2 ** T
    dev = torch.device('cuda', engine.device)
    dev_it = DeviceInterpolator(engine, align=interpolator.align, block_shape=interpolator.block_shape)
    nw = workers or max(2, min(32, (os.cpu_count() or 4)))
    kept = {} if keep else None
    written = 0
    with torch.cuda.device(dev), concurrent.futures.ThreadPoolExecutor(max_workers=nw) as enc:
        stream = Uint8SequenceStream(dev_it, engine)
        pending = []

        def emit(index: int, pixels: np.ndarray) -> None:
            if kept is not None:
                kept[index] = pixels
            pending.append(enc.submit(write_image_uint8, f'{frames_dir}/frame_{index:03d}.png', pixels))

        reads = {}
        try:
            a = first
            while a < end:
                b = min(a + window - 1, end)
                for i in range(a, b + 1):
                    if i not in reads:
                        reads[i] = enc.submit(read_image, inputs[i])
                imgs = [reads.pop(i).result() for i in range(a, b)] + [reads[b].result()]   # (frame b stays: the next window's first)
                for i in range(b + 1, min(b + window, end + 1)):   # decode the next window while this one computes
                    reads[i] = enc.submit(read_image, inputs[i])
                for i in range(a, b):
                    emit(i * step, to_uint8(imgs[i - a]))
                written += b - a
                if T > 0:
                    x = torch.from_numpy(np.ascontiguousarray(np.stack(imgs), dtype=np.float32)).to(dev, non_blocking=False)
                    futs = stream.run(x, T, lambda k, px, base=a * step: emit(base + k, px))
                    for fu in futs:
                        fu.result()
                    written += (b - a) * (step - 1)
                if b == n_pairs:
                    emit(b * step, to_uint8(imgs[-1]))
                    written += 1
                a = b
            for fu in pending:
                fu.result()
        except BaseException:
            for fu in pending:
                fu.cancel()
            for fu in reads.values():
                fu.cancel()
            raise
        finally:
            stream.close()
            engine.save_tune_cache()
    return written, ([kept[i] for i in sorted(kept)] if kept is not None else None)


def _recursive_generator(
        frame1: np.ndarray, frame2: np.ndarray, num_recursions: int,
        interpolator: 'interpolator_lib.Interpolator',
        bar=None) -> Generator[np.ndarray, None, None]:
    """Depth-first binary subdivision (reference eval/util.py:62-91).

    Yields frame1, then every generated frame in temporal order, but not frame2.  Each mid-frame is
    one interpolator call with batch size 1 and time 0.5; the raw (un-clipped) float result is what
    deeper recursion levels consume, exactly as upstream.
    """
    if num_recursions == 0:
        yield frame1
        return
    time = np.full(shape=(1,), fill_value=0.5, dtype=np.float32)
    mid_frame = interpolator(frame1[np.newaxis, ...], frame2[np.newaxis, ...], time)[0]
    if bar is not None:
        bar.update(1)
    yield from _recursive_generator(frame1, mid_frame, num_recursions - 1, interpolator, bar)
    yield from _recursive_generator(mid_frame, frame2, num_recursions - 1, interpolator, bar)


def _device_driver(interpolator):
    """The device-resident breadth-first driver (film_hip/recursive.py) for the HIP-backed Interpolator: the two
    input frames go to HBM once, depth d of the recursion is ONE batched film_interpolate call on 2^(d-1) frame
    pairs, and the 2^T - 1 generated frames come back once - instead of the reference's 2^T - 1 numpy round
    trips with batch size 1 (eval/util.py:62-91).  Same frames, same order, same bits (tests/test_gpu_parity.py).
    Any other callable (e.g. the CPU oracle in tests), or FILM_HOST_RECURSION=1, gets the reference-order host
    generator above."""
    engine = getattr(interpolator, 'engine', None)
    if engine is None or engine.device < 0 or os.environ.get('FILM_HOST_RECURSION') == '1':
        return None
    import torch
    from film_hip import recursive
    from film_hip.torch_io import DeviceInterpolator
    dev = torch.device('cuda', engine.device)
    dev_it = DeviceInterpolator(engine, align=interpolator.align, block_shape=interpolator.block_shape)

    def run(frame1: np.ndarray, frame2: np.ndarray, num_recursions: int, bar=None):
        if num_recursions == 0:
            yield frame1
            return
        with torch.cuda.device(dev):
            a = torch.from_numpy(np.ascontiguousarray(frame1, dtype=np.float32)).to(dev)
            b = torch.from_numpy(np.ascontiguousarray(frame2, dtype=np.float32)).to(dev)
            seq = recursive.interpolate_pair_recursively(a, b, num_recursions, dev_it)[:-1].cpu().numpy()
        engine.save_tune_cache()     # no-op unless $FILM_TUNE_CACHE is set and a new shape was measured
        if bar is not None:
            bar.update(seq.shape[0] - 1)
        yield frame1
        for k in range(1, seq.shape[0]):
            yield seq[k]
    return run


def _progress(total: int):
    if tqdm is None:
        return None
    return tqdm(total=total, ncols=100, colour='green')


def interpolate_recursively_from_files(
        frames: List[str], times_to_interpolate: int,
        interpolator: 'interpolator_lib.Interpolator') -> Iterable[np.ndarray]:
    """Streams (n-1)*(2^T-1) generated frames plus the n inputs, reading files lazily
    (reference eval/util.py:94-123)."""
    n = len(frames)
    bar = _progress((n - 1) * (2 ** times_to_interpolate - 1))
    driver = _device_driver(interpolator)
    for i in range(1, n):
        f1, f2 = read_image(frames[i - 1]), read_image(frames[i])
        if driver is not None:
            yield from driver(f1, f2, times_to_interpolate, bar)
        else:
            yield from _recursive_generator(f1, f2, times_to_interpolate, interpolator, bar)
    yield read_image(frames[-1])


def interpolate_recursively_from_memory(
        frames: List[np.ndarray], times_to_interpolate: int,
        interpolator: 'interpolator_lib.Interpolator') -> Iterable[np.ndarray]:
    """Same as interpolate_recursively_from_files for frames already in memory
    (reference eval/util.py:125-153)."""
    n = len(frames)
    bar = _progress((n - 1) * (2 ** times_to_interpolate - 1))
    driver = _device_driver(interpolator)
    for i in range(1, n):
        if driver is not None:
            yield from driver(frames[i - 1], frames[i], times_to_interpolate, bar)
        else:
            yield from _recursive_generator(frames[i - 1], frames[i], times_to_interpolate, interpolator, bar)
    yield frames[-1]


def get_ffmpeg_path() -> str:
    """reference eval/util.py:156-162."""
    path = shutil.which(_CONFIG_FFMPEG_NAME_OR_PATH)
    if not path:
        raise RuntimeError(
            f"Program '{_CONFIG_FFMPEG_NAME_OR_PATH}' is not found;"
            " perhaps install ffmpeg using 'apt-get install ffmpeg'.")
    return path
