r"""Benchmark evaluation of a frame interpolation model over triplet folders - the image-folder twin of the
reference's eval/eval_cli.py (which reads TFRecords from gs://, eval/config/*.gin).

  python -m eval.eval_cli --model_path <saved model dir> --triplet_dir <root> --output_dir <dir> \
      [--metrics l1 l2 ssim psnr] [--max_examples -1] [--output_frames] [--align 64] \
      [--block_height 1 --block_width 1] [--metrics_device cpu|gpu] [--batch_size 1] [--io_workers 4]

`triplet_dir` is searched recursively for folders that hold a triplet: Vimeo-90K style `im1.png im2.png im3.png`
(eval/config/vimeo_90K.gin) or `frame_0 / frame_1(middle) / frame_2` style names; more generally any folder with
exactly three images, in natural order (first, ground-truth middle, last).

Same outputs as the reference loop (eval/eval_cli.py:88-178): `readme.txt`, `results.csv` with a title row
`key, <metric>, ...`, one row per example, a final `mean, ...` row; predictions are clipped to [0,1] before the
metrics (:165); with --output_frames the inputs, ground truth and prediction are written as `<key>_<name>.png`.
"""
import argparse
import collections
import itertools
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import interpolator as interpolator_lib
from . import metrics as metrics_lib
from . import util

_IMAGE_EXT = ('.png', '.jpg', '.jpeg')


def _natural(s: str):
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r'(\d+)', s)]


def find_triplets(root: str) -> List[Tuple[str, Tuple[str, str, str]]]:
    """[(key, (first, middle, last))], key = folder path relative to root with '/' -> '_'."""
    out = []
    for d, _sub, files in sorted(os.walk(root)):
        imgs = sorted((f for f in files if f.lower().endswith(_IMAGE_EXT)), key=_natural)
        if len(imgs) == 3:
            rel = os.path.relpath(d, root)
            key = 'root' if rel == '.' else rel.replace(os.sep, '_')
            out.append((key, tuple(os.path.join(d, f) for f in imgs)))
    return out


def _decoded(triplets, io_workers: int, ahead: int):
    """(key, x0, y, x1) per triplet, in order; with io_workers > 0 a thread pool decodes up to `ahead` triplets in advance, so the
    next batch's images are read while the current one runs."""
    def load(t):
        key, (f0, fy, f1) = t
        return key, util.read_image(f0), util.read_image(fy), util.read_image(f1)
    if io_workers <= 0:
        yield from map(load, triplets)
        return
    with ThreadPoolExecutor(max_workers=io_workers) as pool:
        pending = collections.deque()
        for t in triplets:
            pending.append(pool.submit(load, t))
            if len(pending) > ahead:
                yield pending.popleft().result()
        while pending:
            yield pending.popleft().result()


def _same_size_batches(items, batch_size: int):
    """Consecutive items whose frames have the same shape, at most batch_size per list."""
    batch = []
    for it in items:
        if batch and (len(batch) == batch_size or it[1].shape != batch[0][1].shape):
            yield batch
            batch = []
        batch.append(it)
    if batch:
        yield batch


def _write_frames(output_dir: str, keys, x0, x1, y, image) -> None:
    for k, key in enumerate(keys):
        for name, img in (('x0', x0[k]), ('x1', x1[k]), ('y', y[k]), ('image', image[k])):
            util.write_image(os.path.join(output_dir, f'{key}_{name}.png'), img)


def _cpu_scorer(interpolator, fns, output_dir: str, output_frames: bool):
    """The reference loop's scoring: interpolator on host arrays, np.clip, the numpy metrics per triplet."""
    def score(keys, x0, x1, y):
        image = interpolator(x0, x1, np.full((len(keys),), 0.5, np.float32))
        if output_frames:
            _write_frames(output_dir, keys, x0, x1, y, image)
        image = np.clip(image, 0.0, 1.0)   # eval/eval_cli.py:162-165
        return [[fn(image[k:k + 1], y[k:k + 1]) for _n, fn in fns] for k in range(len(keys))]
    return score


def _gpu_scorer(interpolator, names, output_dir: str, output_frames: bool):
    """x0, x1, y uploaded from pinned staging, the batch interpolated (DeviceInterpolator.batch) and scored where it lies in HBM
    (film_image_metrics, the clip fused); only the per-image scalars come back, and the prediction with output_frames."""
    import torch
    from film_hip.torch_io import DeviceInterpolator
    from . import device_metrics
    engine = getattr(interpolator, 'engine', None)
    if engine is None:
        raise ValueError('metrics_device="gpu" needs an eval.interpolator.Interpolator (it scores on its engine)')
    device = torch.device('cuda', engine.device)
    dev = DeviceInterpolator(engine, interpolator.align, interpolator.block_shape)
    metric_set = device_metrics.DeviceMetricSet(engine, names)
    staging = {}

    def upload(slot: str, a: np.ndarray) -> 'torch.Tensor':
        buf = staging.get((slot, a.shape))
        if buf is None:
            buf = staging[(slot, a.shape)] = torch.empty(a.shape, dtype=torch.float32, pin_memory=True)
        buf.numpy()[...] = a   # the previous copy out of buf has completed: every batch ends with a synchronising metrics call
        return buf.to(device, non_blocking=True)

    def score(keys, x0, x1, y):
        t0, t1, ty = upload('x0', x0), upload('x1', x1), upload('y', y)
        image = dev.batch(t0, t1)
        rows = metric_set.rows(image, ty, clip=True)
        if output_frames:
            _write_frames(output_dir, keys, x0, x1, y, image.cpu().numpy())
        return rows
    return score


def run_evaluation(interpolator, triplets: Sequence[Tuple[str, Tuple[str, str, str]]], output_dir: str,
                   max_examples: int = -1, metrics: Sequence[str] = ('l1', 'l2', 'ssim', 'psnr'),
                   output_frames: bool = False, model_path: str = '', source: str = '',
                   metrics_device: str = 'cpu', batch_size: int = 1, io_workers: int = 4) -> dict:
    """The reference loop (eval/eval_cli.py:88-178).  Extensions: metrics_device 'gpu' scores with the HIP metric kernels
    (eval/device_metrics.py) on the prediction in HBM, for an eval.interpolator.Interpolator; batch_size > 1 interpolates up to that
    many consecutive triplets of the same frame size in one call (rows stay in triplet order, values as with 1); io_workers threads
    decode the next triplets' images meanwhile (0: decode in this thread)."""
    if metrics_device not in ('cpu', 'gpu'):
        raise ValueError(f"metrics_device must be 'cpu' or 'gpu', got {metrics_device!r}")
    if batch_size < 1:
        raise ValueError(f'batch_size must be >= 1, got {batch_size}')
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'readme.txt'), 'w') as f:
        print('Results for:', file=f)
        print(f' model:   {model_path}', file=f)
        print(f' triplets: {source}', file=f)
    fns = metrics_lib.test_losses(list(metrics))
    names = [n for n, _ in fns]
    if metrics_device == 'gpu':
        score = _gpu_scorer(interpolator, names, output_dir, output_frames)
    else:
        score = _cpu_scorer(interpolator, fns, output_dir, output_frames)
    all_losses = {n: [] for n in names}
    if max_examples >= 0:
        triplets = itertools.islice(triplets, max_examples)
    decoded = _decoded(triplets, io_workers, ahead=max(2 * batch_size, io_workers))
    with open(os.path.join(output_dir, 'results.csv'), 'w') as csv_file:
        print(', '.join(['key'] + names), file=csv_file)
        for batch in _same_size_batches(decoded, batch_size):
            keys = [b[0] for b in batch]
            x0, y, x1 = (np.stack([b[j] for b in batch]) for j in (1, 2, 3))
            for key, values in zip(keys, score(keys, x0, x1, y)):
                for n, v in zip(names, values):
                    all_losses[n].append(v)
                print(f'{key}, {str(values)[1:-1]}', file=csv_file)
        totals = {n: float(np.mean(v)) for n, v in all_losses.items() if v}
        if totals:
            print(f'mean, {str([totals[n] for n in names])[1:-1]}', file=csv_file)
    return totals


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--model_path', required=True, help='The path of the saved model to use (SavedModel dir or film_weights.npz dir).')
    ap.add_argument('--triplet_dir', required=True, help='Root folder searched for image triplets.')
    ap.add_argument('--output_dir', required=True, help='Directory to store the results into.')
    ap.add_argument('--metrics', nargs='+', default=['l1', 'l2', 'ssim', 'psnr'], help='evaluation.metrics of the gin config.')
    ap.add_argument('--max_examples', type=int, default=-1, help='Maximum examples to evaluate (-1: all).')
    ap.add_argument('--output_frames', action='store_true', help='If true, saves the inputs, ground-truth and interpolated frames.')
    ap.add_argument('--align', type=int, default=64, help='If >1, pad the input size so it is evenly divisible by this value.')
    ap.add_argument('--block_height', type=int, default=1)
    ap.add_argument('--block_width', type=int, default=1)
    ap.add_argument('--block_overlap_height', type=int, default=0,
                    help='(extension) rows every patch takes from its neighbours, results cross-faded; 0: disjoint patches, -1: what the align padding holds.')
    ap.add_argument('--block_overlap_width', type=int, default=0, help='(extension) the same for columns.')
    ap.add_argument('--device', type=int, default=0, help='HIP device ordinal.')
    ap.add_argument('--precision', type=int, default=0, choices=[0, 1, 2], help='engine precision mode: 0 fp32 MFMA, 1 bf16x6, 2 bf16x3.')
    ap.add_argument('--metrics_device', default='cpu', choices=['cpu', 'gpu'],
                    help='cpu: numpy metrics on the host (the reference loop); gpu: HIP metric kernels on the prediction in HBM.')
    ap.add_argument('--batch_size', type=int, default=1, help='Consecutive triplets of the same frame size interpolated per call.')
    ap.add_argument('--io_workers', type=int, default=4, help='Threads that decode the next triplets while the current batch runs (0: none).')
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    triplets = find_triplets(args.triplet_dir)
    if not triplets:
        print(f'no image triplets under {args.triplet_dir}', file=sys.stderr)
        return 1
    overlap = (args.block_overlap_height, args.block_overlap_width)
    it = interpolator_lib.Interpolator(args.model_path, args.align, [args.block_height, args.block_width], device=args.device, precision=args.precision,
                                       **({'block_overlap': overlap} if any(overlap) else {}))
    totals = run_evaluation(it, triplets, args.output_dir, args.max_examples, args.metrics, args.output_frames,
                            args.model_path, args.triplet_dir, metrics_device=args.metrics_device, batch_size=args.batch_size,
                            io_workers=args.io_workers)
    print('mean,', totals)
    return 0


if __name__ == '__main__':
    sys.exit(main())
