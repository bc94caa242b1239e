"""Milliseconds per step of the tiled path with overlapped, cross-faded tiles (engine options "block_overlap_h" / "block_overlap_w"),
same process, same engine: a device-resident 1080p pair on 2 x 2 tiles and one 4K pair on 4 x 4 tiles at the overlaps
(0, 0), (-1, -1) ("free": what the align padding holds - the plan of overlap 0), (18, 32), (32, 32), (64, 64).

Per case: the resolved overlap, the padded tile and its area against overlap 0's, ms per step (median of `--rounds` blocks of `--steps`
steps, each block behind an untimed warm-up call that brings the case's plan back into the cache), the ratio of times beside the ratio
of areas, and from one call with option `profile` (one stream, an event pair around every op of the plan) the time of that call
minus the sum of its plan ops: what the two tile kernels (cut, and stitch or blend) and the launch gaps around them cost.
Usage:  python tools/overlap_bench.py [--quick] [--out LOG]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'frame-interpolation_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (name, height, width, block_shape)
POINTS = [('1080p 2x2', 1080, 1920, (2, 2)), ('4K 4x4', 2160, 3840, (4, 4))]
OVERLAPS = [(0, 0), (-1, -1), (18, 32), (32, 32), (64, 64)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='the 1080p point only')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    args = ap.parse_args(argv)
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    lines = [f'# tools/overlap_bench.py  {FilmEngine.version()}  {torch.cuda.get_device_name(0)}  rounds={args.rounds} steps={args.steps}',
             f'# {"point":<10} {"asked":>9} {"resolved":>9} {"padded tile":>12} {"area":>6} | {"ms/step":>8} {"time":>6} | '
             f'{"plan ops ms":>11} {"outside ops ms":>15} (profiled call: the call - its plan ops = tile kernels + gaps)']
    print('\n'.join(lines), flush=True)
    results = []
    for name, h, w, block in POINTS:
        if args.quick and not name.startswith('1080p'):
            continue
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.random((1, h, w, 3), dtype=np.float32)).cuda()
        b = torch.roll(a, (2, -3), dims=(1, 2)).contiguous()
        it = DeviceInterpolator(eng, align=64, block_shape=list(block))
        base_ms, base_area = None, None
        for ov in OVERLAPS:
            eng.set_block_overlap(ov)
            geo = eng.tiling(h, w, 64, block)
            area = geo['padded_h'] * geo['padded_w']
            it(a, b)                                   # plan build, autotune
            torch.cuda.synchronize()
            times = []
            for _ in range(args.rounds):
                it(a, b)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    it(a, b)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3 / args.steps)
            ms = statistics.median(times)
            # one profiled call (one stream, an event pair per op of the plan): what the step spends outside the plan's ops is the
            # two cuts, the blend / stitch and launch gaps
            eng.set_option('profile', 1)
            try:
                it(a, b)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                it(a, b)
                torch.cuda.synchronize()
                prof_ms = (time.perf_counter() - t0) * 1e3
                chunks = -(-block[0] * block[1] // max(1, eng.profile()['B']))
                ops_ms = sum(op['ms'] for op in eng.profile()['ops']) * chunks
            finally:
                eng.set_option('profile', 0)
            if base_ms is None:
                base_ms, base_area = ms, area
            row = (f'  {name:<10} {str(ov):>9} {str((geo["overlap_h"], geo["overlap_w"])):>9} {geo["padded_h"]:>5}x{geo["padded_w"]:<6} '
                   f'{area / base_area:>6.3f} | {ms:>8.2f} {ms / base_ms:>6.3f} | {ops_ms:>11.2f} {prof_ms - ops_ms:>15.2f}')
            print(row, flush=True)
            lines.append(row)
            results.append({'point': name, 'asked': ov, 'tiling': geo, 'area_ratio': area / base_area, 'ms_per_step': [round(t, 3) for t in times],
                            'profiled_step_ms': round(prof_ms, 3), 'profiled_plan_ops_ms': round(ops_ms, 3)})
        eng.set_block_overlap(0)
        del a, b
        torch.cuda.empty_cache()
    lines.append('# area / time: against overlap (0, 0) of the same point; a time ratio well above the area ratio = a level left a kernel family\'s sweet spot')
    lines.append(json.dumps(results))
    print(lines[-2] + '\n' + lines[-1])
    eng.close()
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
