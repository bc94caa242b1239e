"""Milliseconds per generated frame: pairwise vs sequence interpolation of the same frames, same process, same engine (A/B on one box).

  pairwise  the CLI's default driver: every input pair's recursion on its own (film_hip/recursive.py interpolate_recursively;
            depth d of a pair = one film_interpolate call on 2^(d-1) pairs)
  batched   the whole sequence breadth first, depth d = ONE film_interpolate call on all its pairs (DeviceInterpolator.batch):
            the batching gain alone, every interior frame still extracted twice
  sequence  the whole sequence breadth first through film_interpolate_sequence (interpolate_sequence_recursively): batching +
            one feature extraction per frame

Each method runs as a block: one untimed warm-up (plan builds, autotune), then `--rounds` timed runs; the three blocks run twice
(ABC ABC, for drift) and the median of a method's timed runs is reported.  Blocks, not a round robin: a handle keeps at most
three device plans, and the methods use different plan shapes (the recursion depths of a T = 3 point alone need three), so
alternating run by run would rebuild workspaces inside the timed region.  Outputs are compared bit for bit.  Usage:  python tools/sequence_bench.py [--quick] [--out LOG]
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

# (name, frames, height, width, block_shape, T)
POINTS = [
    ('1080p 2x2', 8, 1080, 1920, (2, 2), 1),
    ('1080p 2x2', 8, 1080, 1920, (2, 2), 3),
    ('448x256', 16, 256, 448, None, 1),
    ('448x256', 16, 256, 448, None, 3),
    ('4K 4x4', 4, 2160, 3840, (4, 4), 1),
]


def _frames(f, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3), dtype=np.float32)
    return np.stack([np.roll(base, (2 * i, -3 * i), axis=(0, 1)) for i in range(f)]).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='the 448x256 points only')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    args = ap.parse_args(argv)
    from film_hip import recursive, weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    lines = [f'# tools/sequence_bench.py  {FilmEngine.version()}  {torch.cuda.get_device_name(0)}  rounds={args.rounds}',
             f'# {"point":<11} {"F":>3} {"T":>2} {"gen":>4} | {"pairwise":>9} {"batched":>9} {"sequence":>9} ms/frame | '
             f'{"seq vs pairwise":>15} {"seq vs batched":>14} | identical']
    print('\n'.join(lines), flush=True)
    results = []
    for name, F, h, w, block, T in POINTS:
        if args.quick and not name.startswith('448'):
            continue
        it = DeviceInterpolator(eng, align=64, block_shape=list(block) if block else None)
        x = [torch.from_numpy(f).cuda() for f in _frames(F, h, w)]
        gen = (F - 1) * (2 ** T - 1)

        def pairwise():
            return list(recursive.interpolate_recursively(x, T, it))

        def batched():
            seq = torch.stack(x)
            for _ in range(T):
                mids = it.batch(seq[:-1].contiguous(), seq[1:].contiguous())
                seq = recursive._interleave(seq, mids)
            return list(seq)

        def sequence():
            return recursive.interpolate_sequence_recursively(x, T, it)

        methods = {'pairwise': pairwise, 'batched': batched, 'sequence': sequence}
        outs = {k: fn() for k, fn in methods.items()}
        torch.cuda.synchronize()
        same = all(all(torch.equal(a, b) for a, b in zip(outs['pairwise'], outs[k])) for k in ('batched', 'sequence'))
        del outs
        times = {k: [] for k in methods}
        for _ in range(2):
            for k, fn in methods.items():
                fn()                          # warm-up of the block: this method's plans back in the cache
                torch.cuda.synchronize()
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    r = fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3 / gen)
                    del r
        med = {k: statistics.median(v) for k, v in times.items()}
        row = (f'  {name:<11} {F:>3} {T:>2} {gen:>4} | {med["pairwise"]:>9.2f} {med["batched"]:>9.2f} {med["sequence"]:>9.2f} ms/frame | '
               f'{100 * (1 - med["sequence"] / med["pairwise"]):>+14.1f}% {100 * (1 - med["sequence"] / med["batched"]):>+13.1f}% | {same}')
        print(row, flush=True)
        lines.append(row)
        results.append({'point': name, 'F': F, 'H': h, 'W': w, 'block': block, 'T': T, 'generated': gen, 'identical': same,
                        'ms_per_frame': {k: [round(t, 3) for t in v] for k, v in times.items()}})
        del x
        torch.cuda.empty_cache()
    lines.append('# gain = 1 - sequence / other (positive: sequence is faster); raw per-round ms/frame:')
    lines.append(json.dumps(results))
    print(lines[-2] + '\n' + lines[-1])
    eng.close()
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    if not all(r['identical'] for r in results):
        raise SystemExit('outputs differ')


if __name__ == '__main__':
    main()
