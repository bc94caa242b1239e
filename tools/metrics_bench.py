"""Evaluation metrics on the GPU (film_image_metrics) against eval/metrics.py, and the eval loop with either.

  1. ms per image of film_image_metrics on device tensors (HIP events around warm calls, each call ending in its own stream
     synchronise) at 448x256, 1080p and 4K, all four metrics and ssim alone; the numpy time of eval/metrics.py on the same image
     (one run each); the interpolation time of the same frame size for scale (DeviceInterpolator.batch, B = 8 at 448x256, B = 1 else).
  2. eval_cli.run_evaluation triplets/s on synthetic 448x256 triplets (PNG folders in a temporary directory): --metrics_device cpu
     with --batch_size 1 (the reference loop) against gpu with 8; one warm-up pass of each first, the rows of both runs compared.

Usage:  python tools/metrics_bench.py [--triplets 48] [--out LOG]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'frame-interpolation_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [('448x256', 256, 448, 8), ('1080p', 1080, 1920, 1), ('4K', 2160, 4096, 1)]
ALL = ['l1', 'l2', 'ssim', 'psnr']


def _event_ms(fn, iters):
    fn()
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _numpy_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--triplets', type=int, default=48)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args(argv)
    from eval import eval_cli, metrics as M, util
    from eval.interpolator import Interpolator
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator

    it = Interpolator('', align=64, weights=W.make_synthetic_weights(PUBLISHED, seed=0), device=0)
    eng = it.engine
    dev = DeviceInterpolator(eng, align=64)
    lines = [f'# tools/metrics_bench.py  {FilmEngine.version()}  {torch.cuda.get_device_name(0)}',
             f'# {"size":<8} | {"gpu all4":>9} {"gpu ssim":>9} ms/image | {"numpy l1":>9} {"l2":>8} {"psnr":>8} {"ssim":>9} '
             f'{"all4":>9} ms/image | {"interp":>8} ms/pair (B) | gpu all4 / interp | numpy all4 / gpu all4']
    rng = np.random.default_rng(0)
    for name, h, w, bi in SIZES:
        ref = rng.random((1, h, w, 3), dtype=np.float32)
        pred = np.clip(ref + rng.normal(0, 0.05, ref.shape), -0.1, 1.1).astype(np.float32)
        tp, tr = torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()
        iters = 50 if h < 2000 else 20
        g_all = _event_ms(lambda: eng.image_metrics_device(tp.data_ptr(), tr.data_ptr(), 1, h, w, 3, ALL, clip=True), iters)
        g_ssim = _event_ms(lambda: eng.image_metrics_device(tp.data_ptr(), tr.data_ptr(), 1, h, w, 3, ['ssim'], clip=True), iters)
        pc = np.clip(pred, 0.0, 1.0)
        np_ms = [_numpy_ms(lambda f=f: f(pc, ref)) for f in (M.l1, M.l2, M.psnr, M.ssim)]
        x0 = torch.rand((bi, h, w, 3), device='cuda')
        x1 = torch.rand((bi, h, w, 3), device='cuda')
        interp = _event_ms(lambda: dev.batch(x0, x1), 5 if h < 2000 else 3) / bi
        lines.append(f'  {name:<8} | {g_all:9.3f} {g_ssim:9.3f}          | {np_ms[0]:9.1f} {np_ms[1]:8.1f} {np_ms[2]:8.1f} '
                     f'{np_ms[3]:9.1f} {sum(np_ms):9.1f}          | {interp:8.2f} ({bi})     | {100 * g_all / interp:6.2f} %'
                     f'           | {sum(np_ms) / g_all:8.0f}x')
        print(lines[-1], flush=True)
        del tp, tr, x0, x1

    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'triplets')
        for i in range(args.triplets):
            d = os.path.join(root, f'{i // 8:05d}', f'{i % 8:04d}')
            os.makedirs(d)
            base = rng.random((256, 448, 3), dtype=np.float32)
            for j in (1, 2, 3):
                util.write_image(os.path.join(d, f'im{j}.png'), np.roll(base, (2 * j, -3 * j), axis=(0, 1)))
        trip = eval_cli.find_triplets(root)
        results = {}
        for label, kw in (('cpu B=1', dict(metrics_device='cpu', batch_size=1)), ('gpu B=8', dict(metrics_device='gpu', batch_size=8))):
            out = os.path.join(tmp, label.replace(' ', '_').replace('=', ''))
            eval_cli.run_evaluation(it, trip[:8], out, **kw)                       # warm-up: plans, autotune, pinned buffers
            t = time.perf_counter()
            eval_cli.run_evaluation(it, trip, out, **kw)
            dt = time.perf_counter() - t
            rows = [l.split(', ') for l in open(os.path.join(out, 'results.csv')).read().strip().split('\n')[1:]]
            results[label] = (len(trip) / dt, rows)
            lines.append(f'# eval_cli {label}: {len(trip)} triplets of 448x256 in {dt:.2f} s = {len(trip) / dt:.1f} triplets/s')
            print(lines[-1], flush=True)
        (rc, rows_c), (rg, rows_g) = results['cpu B=1'], results['gpu B=8']
        assert [r[0] for r in rows_c] == [r[0] for r in rows_g]
        dmax = max(abs(float(a) - float(b)) for rc_, rg_ in zip(rows_c, rows_g) for a, b in zip(rc_[1:], rg_[1:]))
        lines.append(f'# eval_cli speed-up gpu B=8 / cpu B=1: {rg / rc:.1f}x; max |gpu - cpu| over every value of results.csv: {dmax:.3e}')
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
