"""Milliseconds per steady-state push of a frame stream (film_stream_*) against the per-pair film_interpolate call of a BASELINE checkout
(e.g. the parent commit, built), alternating on one box in one session, and against this tree's film_interpolate_sequence.

  python tools/stream_bench.py --baseline-root <checkout of the commit to compare with, built> [--rounds 3] [--out LOG]

A round = one fresh worker process per tree, baseline first: the baseline worker times `pair` (film_interpolate, device-resident, one
pair per call - what a frame-by-frame caller had before), this tree's worker times `pair` too (the two agree unless the trees differ
in what a pair call runs: their difference over the rounds IS the box's spread), then `push_f32` / `push_u8` (a steady-state push,
device-resident), `push_i420` / `push_nv12` (the same on 8-bit 4:2:0 frames, where the tree has them), `push_i010` / `push_p010` (10-bit
4:2:0 frames, where the tree has them), `sequence`
(film_interpolate_sequence over a long sequence, per generated frame) and, at the first point, the host-buffer calls `host_pair`
(film_interpolate on numpy arrays, as bench.py's host_buffers), `host_push_f32`, `host_push_u8`, `host_push_i420`, `host_push_nv12`,
`host_push_i010`, `host_push_p010`; and, for trees that have the planar 4:2:2 / 4:4:4 layouts, `push_i422`, `push_i444`, `push_i210`, `push_i410` and
their `host_` forms.
The 8-bit 4:2:0 rows are compared with the BASELINE's `push_u8` / `host_push_u8` (what such a caller had before: RGB bytes), the 10-bit rows
with the BASELINE's `push_i420` / `host_push_i420` (what such a caller had before: the frames truncated to 8 bits), whose spread over the
rounds is reported next to them.  --rows / --points restrict a run to some measurements.
--scene_cut adds, at the first point and for `u8` and `i420`, device-resident and host buffers, what option "scene_cut" costs (trees
without the option skip them): `*_sc1000` - the steady-state push with scene_cut = 1000, which never cuts on the bench frames (rolled
copies of one picture: D = 0 for RGB, a fraction of a percent of 2 S for 4:2:0, whose chroma is averaged after the roll) but pays the histogram kernel, the 3 KB download and the wait; `*_cut` - a push that IS a cut (scene_cut = 1,
alternating a frame and its halved codes: extraction only); `*_first` - a first push (reset() + push, scene_cut = 0), what a cut should cost;
and `hist <layout> <size> <data>` - frame_histogram_kernel alone (film_frame_histogram, hip events around 50 calls, microseconds per call)
at 1080p and 4K on random bytes and on a constant frame, beside the frame's bytes over the measured HBM copy rate (6.29 TB/s).
--times T --select "3,6/2,5" is a run of its own about selected mid-frames (FilmStream.select; a frame-rate conversion such as 24 -> 60
takes the positions {3, 6} and {2, 5} of a T = 3 push in turn): at 1080p 2x2, the milliseconds PER PUSH of a device-resident `f32` push
and a host `i420` push that take the selections in turn, beside this tree's full push and - with --baseline-root - the baseline's.
--times T[,T..] is a run of its own about recursive streams (engine option "stream_times"): at 1080p 2x2, for `f32` and `i420`, device-resident
and host pushes, the milliseconds PER GENERATED FRAME of a steady push of a stream opened with times = T (2^T - 1 frames per push) beside
this tree's times = 1 push, beside film_hip.recursive.interpolate_pair_recursively on the same pair (float32, device-resident: 2^T - 1 pair
calls, every fed-back frame extracted twice) and - with --baseline-root - beside the baseline's times = 1 push; the frames of the f32 push are
compared bit for bit with that recursion in the worker.  It also lists the stream plan's workspace for T = 1, 2, 3 and 6.
--dedup is a run of its own about duplicate frames (engine options "dup_hi" / "dup_lo" / "dup_frac"): at 1080p 2x2, for `u8`, `i420` and `i010`,
device-resident and host pushes, (a) this tree's push with dup_hi = -1 beside - with --baseline-root - the baseline's push, whose code path it is;
(b) `*_dd0` - the steady push with dup_hi = 0 on the bench frames, which are never duplicates (rolled copies of one picture), against -1 in the
same process: the price of the copy, the kernel, the 96-byte download and the wait; (c) `*_dup` - a push that IS a duplicate (the carried frame
again); (d) `<layout> <size> <data>` - frame_diff_kernel alone (film_frame_diff, hip events around 50 calls, microseconds per call) at 1080p and
4K on two random frames and on a frame against itself, beside the bytes of both frames over the measured HBM copy rate (6.29 TB/s).
--groups is a run of its own about tile groups (include/film_hip.h, "Tile groups": a frame of more tiles than one invocation takes), this tree
alone, one process: (b) at 1080p 2x2, the device-resident `f32` push of a stream opened with max_batch = 2 (two groups of two tiles) against
max_batch = 0 (one group), T = 1 and T = 3 - what the carry costs per pair run; (c) at the point `4K 4x4` (16 tiles of 576 x 960, two groups
of 8), for `i010` and `f32`, device-resident and host pushes, the ms per push of T = 1 and of T = 3 taking the selections {3, 6} and {2, 5} in
turn (24 -> 60), beside per-pair film_interpolate on the same frames, with the layout's workspace and carry bytes; the first mid-frame of
every stream is compared bit for bit with that call; (d) the segment-copy kernel alone over the restore table of one 4K group (two slots),
hip events around 50 calls, beside hipMemcpyAsync device-to-device over the same segments, and both beside the measured HBM copy rate (6.29 TB/s).
--groups-parts b,c,d restricts the run.
Every measurement: untimed warm-up calls (plan build, autotune, first launches), then --reps timed windows of `n` calls, each
ended by a device synchronise; the window's ms per call is one sample.  Each tree keeps its autotune choices in a file of its own
under --scratch, so that the rounds of a tree run the same tiles.  The report gives mean and range over all samples of a
measurement and, per round, push - baseline pair.  Outputs of push_f32 and the pair call are compared bit for bit in the worker.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, height, width, align, block_shape, calls per timed window, frames of the sequence run)
POINTS = [
    ('1080p 2x2', 1080, 1920, 64, (2, 2), 30, 16),
    ('448x256', 256, 448, 64, None, 200, 32),
    ('256x256', 256, 256, 64, None, 200, 32),
]
# the point of --groups: more tiles than one invocation takes with "stream_times" >= 2 (the default runs take it only when --points names it)
GROUPS_POINT = ('4K 4x4', 2160, 3840, 64, (4, 4), 4, 4)
POINTS.append(GROUPS_POINT)


def _frames(f, h, w, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3), dtype=np.float32)
    return np.clip(np.stack([np.roll(base, (2 * i, -3 * i), axis=(0, 1)) for i in range(f)]), 0, 1).astype(np.float32)


def worker(root, reps, quick, rows=None, points=None, scene_cut=False):
    """Times what the checkout at `root` offers (of `rows` / `points`, when given); prints one JSON line."""
    for p in (root, os.path.join(root, 'frame-interpolation_amd')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from film_hip import weights as W
    from film_hip import engine as engine_mod
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    has_stream = hasattr(eng, 'open_stream')
    PIX = getattr(engine_mod, 'PIX', {})                       # this worker also runs in older trees (--baseline-root): what the tree has, it uses
    has_yuv, has_yuv10 = 'i420' in PIX, 'i010' in PIX
    has_chroma = 'i444' in PIX                                 # planar 4:2:2 / 4:4:4, 8- and 10-bit
    shape_of = getattr(engine_mod, 'frame_shape', lambda pix, h, w: (h * 3 // 2, w))      # (a tree without it has the 4:2:0 layouts alone)
    has_scene = scene_cut and hasattr(engine_mod, 'frame_histogram_device')
    want = lambda key: rows is None or key in rows      # noqa: E731
    out = {'version': FilmEngine.version(), 'device': torch.cuda.get_device_name(0), 'points': {}}

    def timed(call, n, warm=3):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        samples = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) * 1e3 / n)
        return [round(s, 4) for s in samples]

    for pi, (name, h, w, align, block, n, fseq) in enumerate(POINTS):
        if (quick and pi == 0) or (points is not None and name not in points) or (points is None and name == GROUPS_POINT[0]):
            continue
        res = {}
        it = DeviceInterpolator(eng, align=align, block_shape=list(block) if block else None)
        fr = _frames(4, h, w)
        x = [torch.from_numpy(f).cuda() for f in fr]
        x8 = [torch.from_numpy((f * 255 + 0.5).astype(np.uint8)).cuda() for f in fr]
        state = {'i': 0}

        def nxt(m):      # the next frame index, round robin
            state['i'] = (state['i'] + 1) % m
            return state['i']

        def pair():
            i = nxt(3)
            return it.batch(x[i][None], x[i + 1][None])

        if want('pair'):
            res['pair'] = timed(pair, n)
        if has_stream:
            ref = it.batch(x[0][None], x[1][None])[0]
            with it.stream(h, w, 'f32') as st:
                st.push(x[0])
                res['identical'] = bool(torch.equal(st.push(x[1]), ref))
                if want('push_f32'):
                    res['push_f32'] = timed(lambda: st.push(x[nxt(4)]), n)
            if want('push_u8'):
                with it.stream(h, w, 'u8') as st:
                    st.push(x8[0])
                    res['push_u8'] = timed(lambda: st.push(x8[nxt(4)]), n)
            yuv = {}
            if has_yuv and h % 2 == 0 and w % 2 == 0:      # the frames as 4:2:0, converted by the engine itself
                for pix in ('i420', 'nv12') + (('i010', 'p010') if has_yuv10 else ()) + (('i422', 'i444', 'i210', 'i410') if has_chroma else ()):
                    if not (want('push_' + pix) or want('host_push_' + pix) or (pix == 'i420' and has_scene and pi == 0)):
                        continue
                    yuv[pix] = [torch.empty(shape_of(pix, h, w), dtype=torch.int16 if PIX[pix][1] is np.uint16 else torch.uint8, device='cuda') for _ in x]
                    for src, dst in zip(x, yuv[pix]):
                        (eng.to_yuv_device if has_chroma else eng.to_yuv420_device)(src.data_ptr(), dst.data_ptr(), h, w, pix)
                    torch.cuda.synchronize()
                    if want('push_' + pix):
                        with it.stream(h, w, pix) as st:
                            st.push(yuv[pix][0])
                            res['push_' + pix] = timed(lambda: st.push(yuv[pix][nxt(4)]), n)
            if want('sequence'):
                seq = torch.from_numpy(_frames(fseq, h, w)).cuda()
                res['sequence'] = [round(s / (fseq - 1), 4) for s in timed(lambda: it.sequence(seq), max(1, n // (fseq - 1)), warm=2)]
                del seq
            if pi == 0 or quick and pi == 1:
                f8 = [(f * 255 + 0.5).astype(np.uint8) for f in fr]
                hn = max(5, n // 3)
                if want('host_pair'):
                    res['host_pair'] = timed(lambda: eng.interpolate_frames(fr[:1], fr[1:2], align=align, block_shape=block), hn, warm=2)
                for pix, frames in [('f32', fr), ('u8', f8)] + [(p, [t.cpu().numpy().view(np.uint16 if t.dtype == torch.int16 else np.uint8) for t in v])
                                                               for p, v in yuv.items()]:
                    if want('host_push_' + pix):
                        with eng.open_stream(h, w, align=align, block_shape=block, pix=pix) as st:
                            st.push(frames[0])
                            res['host_push_' + pix] = timed(lambda: st.push(frames[nxt(4)]), hn, warm=2)
            if has_scene and pi == 0 and has_yuv:
                res.update(scene_rows(eng, it, timed, nxt, h, w, align, block, n, x8, yuv['i420']))
            del yuv
        out['points'][name] = res
        del x, x8
        torch.cuda.empty_cache()
    if has_scene:
        out['histogram_us'] = histogram_alone()
    eng.save_tune_cache()
    eng.close()
    print('STREAM_BENCH ' + json.dumps(out), flush=True)


def times_worker(root, reps, times_list):
    """--times: the rows of the recursive streams at the first point (see the module text); prints one JSON line."""
    for p in (root, os.path.join(root, 'frame-interpolation_amd')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from film_hip import weights as W
    from film_hip import recursive
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    name, h, w, align, block, n, _ = POINTS[0]
    res = {}
    out = {'version': FilmEngine.version(), 'device': torch.cuda.get_device_name(0), 'points': {name: res}}

    def timed(call, calls, per_call, warm=2):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        samples = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) * 1e3 / (calls * per_call))
        return [round(s, 4) for s in samples]

    til = eng.tiling(h, w, align=align, block_shape=block)
    tiles = block[0] * block[1]
    res['workspace_bytes'] = {str(t): 4 * eng.stream_pair_plan(tiles, til['padded_h'], til['padded_w'], t, 1, 0, True)['arena_floats'] for t in (1, 2, 3, 6)}
    it = DeviceInterpolator(eng, align=align, block_shape=list(block))
    fr = _frames(4, h, w)
    x = [torch.from_numpy(f).cuda() for f in fr]
    y = [torch.empty((h * 3 // 2, w), dtype=torch.uint8, device='cuda') for _ in x]
    for src, dst in zip(x, y):
        eng.to_yuv420_device(src.data_ptr(), dst.data_ptr(), h, w, 'i420')
    torch.cuda.synchronize()
    host = {'f32': list(fr), 'i420': [t.cpu().numpy() for t in y]}
    dev = {'f32': x, 'i420': y}
    state = {'i': 0}

    def nxt(m):
        state['i'] = (state['i'] + 1) % m
        return state['i']

    res['identical'] = True
    for t in [1] + [v for v in times_list if v != 1]:
        per = (1 << t) - 1
        calls = max(3, n // per)
        for pix in ('f32', 'i420'):
            with it.stream(h, w, pix, times=t) as st:
                st.push(dev[pix][0])
                if pix == 'f32' and t > 1:
                    got = st.push(x[1])
                    ref = recursive.interpolate_pair_recursively(x[0], x[1], t, it)[1:-1]
                    res['identical'] = res['identical'] and bool(torch.equal(got, ref))
                res[f'push_{pix}_t{t}'] = timed(lambda: st.push(dev[pix][nxt(4)]), calls, per)
            with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, times=t) as st:
                st.push(host[pix][0])
                res[f'host_push_{pix}_t{t}'] = timed(lambda: st.push(host[pix][nxt(4)]), max(3, calls // 3), per)
        if t > 1:
            def rec():
                i = nxt(3)
                return recursive.interpolate_pair_recursively(x[i], x[i + 1], t, it)
            res[f'recursive_pair_t{t}'] = timed(rec, calls, per)
    eng.save_tune_cache()
    eng.close()
    print('STREAM_BENCH ' + json.dumps(out), flush=True)


def select_worker(root, reps, t, selections):
    """--select: the milliseconds PER PUSH of a times = t stream at the first point, `f32` device-resident and `i420` from host buffers:
    `full_*` - every position (what any tree with "stream_times" offers) - and, where the tree has FilmStream.select, `select_*` - the
    selections taken in turn, push after push, one select() per push.  The selected frames of the f32 push are compared bit for bit
    with those positions of the full push of the same frames.  Prints one JSON line."""
    for p in (root, os.path.join(root, 'frame-interpolation_amd')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from film_hip import weights as W
    from film_hip.engine import FilmEngine, FilmStream
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    name, h, w, align, block, _, _ = POINTS[0]
    res = {}
    out = {'version': FilmEngine.version(), 'device': torch.cuda.get_device_name(0), 'points': {name: res}}
    calls = 2 * len(selections)          # pushes per timed window: every selection as often as every other

    def timed(call, warm=2):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        samples = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) * 1e3 / calls)
        return [round(s, 4) for s in samples]

    it = DeviceInterpolator(eng, align=align, block_shape=list(block))
    fr = _frames(4, h, w)
    x = [torch.from_numpy(f).cuda() for f in fr]
    y = [torch.empty((h * 3 // 2, w), dtype=torch.uint8, device='cuda') for _ in x]
    for src, dst in zip(x, y):
        eng.to_yuv420_device(src.data_ptr(), dst.data_ptr(), h, w, 'i420')
    torch.cuda.synchronize()
    host = [v.cpu().numpy() for v in y]
    state = {'i': 0, 's': 0}

    def nxt(m):
        state['i'] = (state['i'] + 1) % m
        return state['i']

    def turn(st):          # the next selection, in turn
        state['s'] = (state['s'] + 1) % len(selections)
        st.select(selections[state['s']])
        return state['s']

    has_select = hasattr(FilmStream, 'select')
    with it.stream(h, w, 'f32', times=t) as st:
        st.push(x[0])
        res['full_push_f32'] = timed(lambda: st.push(x[nxt(4)]))
        if has_select:
            st.reset()
            st.push(x[0])
            full = st.push(x[1])
            res['identical'] = True
            for sel in selections:
                st.reset()
                st.push(x[0])
                st.select(sel)
                got = st.push(x[1])
                res['identical'] = res['identical'] and bool(torch.equal(got, full[[p - 1 for p in sel]]))
            res['select_push_f32'] = timed(lambda: (turn(st), st.push(x[nxt(4)])))
    with eng.open_stream(h, w, align=align, block_shape=block, pix='i420', times=t) as st:
        st.push(host[0])
        out_full = np.empty(((1 << t) - 1,) + host[0].shape, np.uint8)
        res['full_host_push_i420'] = timed(lambda: st.push(host[nxt(4)], out=out_full))
        if has_select:
            outs = [np.empty((len(sel),) + host[0].shape, np.uint8) for sel in selections]
            res['select_host_push_i420'] = timed(lambda: st.push(host[nxt(4)], out=outs[turn(st)]))
    eng.save_tune_cache()
    eng.close()
    print('STREAM_BENCH ' + json.dumps(out), flush=True)


def select_main(args, t, selections):
    """--select: rounds of (the baseline's full pushes,) this tree's full and selected pushes; the report in ms per push.  Both trees keep
    their autotune choices in ONE file (the first worker fills it): the full pushes are compared on equal tile choices."""
    os.makedirs(args.scratch, exist_ok=True)
    tune = os.path.join(args.scratch, 'stream_bench_tune_select.txt')
    name = POINTS[0][0]
    base, this = [], []
    for r in range(args.rounds):
        if args.baseline_root:
            base.append(_run_worker(os.path.abspath(args.baseline_root), args.reps, False, tune, times=[t], select=args.select))
            print(f'# round {r + 1}/{args.rounds} baseline: done', flush=True)
        this.append(_run_worker(HERE, args.reps, False, tune, times=[t], select=args.select))
        print(f'# round {r + 1}/{args.rounds} this: done', flush=True)
    pts = [r['points'][name] for r in this]
    bpts = [r['points'][name] for r in base]
    lines = [f'# tools/stream_bench.py --times {t} --select "{args.select}"  this = {this[0]["version"]}' +
             (f'  baseline = {base[0]["version"]}' if base else '') + f'  {this[0]["device"]}  rounds={args.rounds} reps={args.reps}',
             f'# ms per PUSH of a times = {t} stream (a full push generates {(1 << t) - 1} frames; the selections {args.select} are taken in turn), '
             'f32 device-resident, i420 from host buffers: mean [min .. max] over rounds x reps windows',
             f'{name}:']
    for pix in ('push_f32', 'host_push_i420'):
        full, sel = 'full_' + pix, 'select_' + pix
        if bpts:
            lines.append(f'  {"baseline " + full:<32} {_stat([s for p in bpts for s in p[full]])}')
        lines.append(f'  {full:<32} {_stat([s for p in pts for s in p[full]])}')
        lines.append(f'  {sel:<32} {_stat([s for p in pts for s in p[sel]])}')
        fm, sm = (statistics.mean(s for p in pts for s in p[k]) for k in (full, sel))
        lines.append(f'  {sel + " / " + full:<48} {sm / fm:.3f}')
        if bpts:
            bw = [s for p in bpts for s in p[full]]
            bm = [statistics.mean(p[full]) for p in bpts]
            d = [statistics.mean(p[full]) - b for p, b in zip(pts, bm)]
            lines.append(f'  {full + " - baseline " + full:<48} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms'
                         f'   (baseline: round means {" ".join(f"{b:.3f}" for b in bm)}, spread of its windows {max(bw) - min(bw):.3f} ms)')
            d = [statistics.mean(p[sel]) - b for p, b in zip(pts, bm)]
            lines.append(f'  {sel + " - baseline " + full:<48} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms'
                         f'   ({sm / statistics.mean(bw):.3f} of the baseline\'s full push)')
    lines.append(f'  selected frames of push_f32 == those positions of the full push, bit for bit: {all(p["identical"] for p in pts)}')
    lines.append('# raw: ' + json.dumps({'baseline': base, 'this': this}))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    if not all(p['identical'] for p in pts):
        raise SystemExit('a selected frame differs from the full push')


def scene_rows(eng, it, timed, nxt, h, w, align, block, n, x8, i420):
    """The --scene_cut rows of one point: see the module text.  x8 / i420: the bench frames as CUDA tensors."""
    res = {}
    hn = max(5, n // 3)
    for pix, dev in (('u8', x8), ('i420', i420)):
        other = dev[0] // 2                         # no histogram in common with the bench frames: every push of the pair is a cut
        host, host_other = [t.cpu().numpy() for t in dev], other.cpu().numpy()
        try:
            with it.stream(h, w, pix, scene_cut=1000) as st:
                st.push(dev[0])
                res[f'push_{pix}_sc1000'] = timed(lambda: st.push(dev[nxt(4)]), n)
                assert st.cut_info()[0] >= 0 and st.cut_info()[2] == 0, (pix, st.cut_info())      # (compared, and no cut: rolled copies of one picture)
            with it.stream(h, w, pix, scene_cut=1) as st:
                st.push(dev[0])
                flip = {'i': 0}

                def cut_push():
                    flip['i'] ^= 1
                    return st.push(other if flip['i'] else dev[0])
                res[f'push_{pix}_cut'] = timed(cut_push, n)
                assert st.cut_info()[2] == 1, (pix, st.cut_info())
            eng.set_option('scene_cut', 0)
            with it.stream(h, w, pix) as st:
                def first_push():
                    st.reset()
                    return st.push(dev[0])
                res[f'push_{pix}_first'] = timed(first_push, n)
            with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, scene_cut=1000) as st:
                st.push(host[0])
                res[f'host_push_{pix}_sc1000'] = timed(lambda: st.push(host[nxt(4)]), hn, warm=2)
            with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, scene_cut=1) as st:
                st.push(host[0])
                flip = {'i': 0}

                def host_cut_push():
                    flip['i'] ^= 1
                    return st.push(host_other if flip['i'] else host[0])
                res[f'host_push_{pix}_cut'] = timed(host_cut_push, hn, warm=2)
            eng.set_option('scene_cut', 0)
            with eng.open_stream(h, w, align=align, block_shape=block, pix=pix) as st:
                def host_first_push():
                    st.reset()
                    return st.push(host[0])
                res[f'host_push_{pix}_first'] = timed(host_first_push, hn, warm=2)
        finally:
            eng.set_option('scene_cut', 0)
    return res


def histogram_alone(calls=50, reps=3):
    """frame_histogram_kernel alone: {"<layout> <size> <data>": [microseconds per call, ...]} from hip events around `calls` calls."""
    import torch
    from film_hip.torch_io import frame_histogram
    import numpy as np
    from film_hip import engine as engine_mod
    from film_hip.engine import PIX, frame_histogram_device
    shape_of = getattr(engine_mod, 'frame_shape', lambda pix, h, w: (h * 3 // 2, w) if pix in ('i420', 'nv12', 'i010', 'p010') else (h, w, 3))
    out = {}
    hist = torch.empty(768, dtype=torch.int32, device='cuda')
    for size, (h, w) in (('1080p', (1080, 1920)), ('4K', (2160, 3840))):
        for pix in ('u8', 'i420', 'nv12', 'f32') + tuple(p for p in ('i010', 'p010', 'i422', 'i444', 'i210', 'i410') if p in PIX):
            shape = shape_of(pix, h, w)
            for data in ('random', 'constant'):
                if pix == 'f32':
                    fr = torch.rand(shape, device='cuda') if data == 'random' else torch.full(shape, 0.5, device='cuda')
                elif PIX[pix][1] is np.uint16:      # 10-bit codes in 16-bit words (int16 as a bit pattern), P010's in bits 6-15
                    fr = torch.randint(0, 1024, shape, dtype=torch.int32, device='cuda') if data == 'random' else torch.full(shape, 64, dtype=torch.int32, device='cuda')
                    fr = (((fr << 6) + 32768) % 65536 - 32768 if pix == 'p010' else fr).to(torch.int16)
                else:
                    fr = torch.randint(0, 256, shape, dtype=torch.uint8, device='cuda') if data == 'random' else torch.full(shape, 16, dtype=torch.uint8, device='cuda')
                assert int(frame_histogram(fr, pix).sum()) == fr.numel()
                s = torch.cuda.current_stream().cuda_stream
                samples = []
                for _ in range(reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        frame_histogram_device(fr.data_ptr(), h, w, hist.data_ptr(), pix, stream=s)
                    e1.record()
                    torch.cuda.synchronize()
                    samples.append(round(e0.elapsed_time(e1) * 1e3 / calls, 2))
                out[f'{pix} {size} {data}'] = samples[1:] + [fr.numel() * fr.element_size()]      # (the first window warms up; last entry: the frame's bytes)
    return out


DEDUP_PIX = ('u8', 'i420', 'i010')


def dedup_worker(root, reps):
    """--dedup: the rows about option "dup_hi" at the first point (see the module text); prints one JSON line."""
    for p in (root, os.path.join(root, 'frame-interpolation_amd')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from film_hip import weights as W
    from film_hip.engine import FilmEngine, PIX, frame_shape
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    name, h, w, align, block, n, _ = POINTS[0]
    res = {}
    out = {'version': FilmEngine.version(), 'device': torch.cuda.get_device_name(0), 'points': {name: res}}

    def timed(call, n, warm=3):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        samples = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) * 1e3 / n)
        return [round(s, 4) for s in samples]

    it = DeviceInterpolator(eng, align=align, block_shape=list(block))
    fr = _frames(4, h, w)
    x = [torch.from_numpy(f).cuda() for f in fr]
    dev = {'u8': [torch.from_numpy((f * 255 + 0.5).astype(np.uint8)).cuda() for f in fr]}
    for pix in ('i420', 'i010'):
        dev[pix] = [torch.empty(frame_shape(pix, h, w), dtype=torch.int16 if PIX[pix][1] is np.uint16 else torch.uint8, device='cuda') for _ in x]
        for src, dst in zip(x, dev[pix]):
            eng.to_yuv_device(src.data_ptr(), dst.data_ptr(), h, w, pix)
    torch.cuda.synchronize()
    del x
    state = {'i': 0}

    def nxt(m):
        state['i'] = (state['i'] + 1) % m
        return state['i']

    hn = max(5, n // 3)
    try:
        for pix in DEDUP_PIX:
            d = dev[pix]
            host = [t.cpu().numpy().view(np.uint16 if t.dtype == torch.int16 else np.uint8) for t in d]
            for dedup, suf in ((None, ''), (0, '_dd0')):      # "dup_hi" = -1, then 0 on frames that are never duplicates (rolled copies)
                eng.set_option('dup_hi', -1)
                with it.stream(h, w, pix, dedup=dedup) as st:
                    st.push(d[0])
                    res[f'push_{pix}{suf}'] = timed(lambda: st.push(d[nxt(4)]), n)
                    assert st.dup_info() == (None, 0) if dedup is None else (st.dup_info()[0] is not None and st.dup_info()[1] == 0), (pix, st.dup_info())
                with eng.open_stream(h, w, align=align, block_shape=block, pix=pix) as st:      # (the option stays set)
                    st.push(host[0])
                    res[f'host_push_{pix}{suf}'] = timed(lambda: st.push(host[nxt(4)]), hn, warm=2)
            with it.stream(h, w, pix, dedup=0) as st:          # a push that IS a duplicate: the carried frame again
                st.push(d[0])
                res[f'push_{pix}_dup'] = timed(lambda: st.push(d[0]), n)
                assert st.dup_info()[1] == 1, (pix, st.dup_info())
            with eng.open_stream(h, w, align=align, block_shape=block, pix=pix) as st:
                st.push(host[0])
                res[f'host_push_{pix}_dup'] = timed(lambda: st.push(host[0]), hn, warm=2)
                assert st.dup_info()[1] == 1, (pix, st.dup_info())
    finally:
        eng.set_option('dup_hi', -1)
    del dev
    torch.cuda.empty_cache()
    out['diff_us'] = diff_alone()
    eng.save_tune_cache()
    eng.close()
    print('STREAM_BENCH ' + json.dumps(out), flush=True)


def diff_alone(calls=50, reps=3):
    """frame_diff_kernel alone: {"<layout> <size> <data>": [microseconds per call, ..., bytes of both frames]} from hip events around `calls` calls
    of film_frame_diff (memset + kernel), on two random frames and on a frame against itself."""
    import numpy as np
    import torch
    from film_hip.engine import PIX, frame_diff_device, frame_shape
    from film_hip.torch_io import frame_diff
    out = {}
    stats = torch.empty(12, dtype=torch.int64, device='cuda')
    for size, (h, w) in (('1080p', (1080, 1920)), ('4K', (2160, 3840))):
        for pix in ('u8', 'i420', 'nv12', 'i010', 'p010', 'f32'):
            shape = frame_shape(pix, h, w)

            def rand():
                if pix == 'f32':
                    return torch.rand(shape, device='cuda')
                if PIX[pix][1] is np.uint16:
                    return torch.randint(-32768, 32768, shape, dtype=torch.int32, device='cuda').to(torch.int16)      # (every bit of the word)
                return torch.randint(0, 256, shape, dtype=torch.uint8, device='cuda')
            a = rand()
            for data, b in (('random', rand()), ('identical', a.clone())):
                blocks = frame_diff(a, b, pix)[:, 3]
                assert (frame_diff(a, b, pix)[:, 0] == 0).all() == (data == 'identical') and int(blocks[0]) == -(-h // 8) * -(-w // 8)
                s = torch.cuda.current_stream().cuda_stream
                samples = []
                for _ in range(reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        frame_diff_device(a.data_ptr(), b.data_ptr(), h, w, stats.data_ptr(), pix, stream=s)
                    e1.record()
                    torch.cuda.synchronize()
                    samples.append(round(e0.elapsed_time(e1) * 1e3 / calls, 2))
                out[f'{pix} {size} {data}'] = samples[1:] + [2 * a.numel() * a.element_size()]      # (the first window warms up; last entry: the bytes of both frames)
    return out


def dedup_main(args):
    """--dedup: rounds of (the baseline's plain pushes,) this tree's rows; (a) - (d) of the module text."""
    os.makedirs(args.scratch, exist_ok=True)
    name = POINTS[0][0]
    plain_rows = [f'{pre}push_{pix}' for pre in ('', 'host_') for pix in DEDUP_PIX]
    base, this = [], []
    for r in range(args.rounds):
        if args.baseline_root:
            base.append(_run_worker(os.path.abspath(args.baseline_root), args.reps, False, os.path.join(args.scratch, 'stream_bench_tune_baseline.txt'),
                                    plain_rows, [name]))
            print(f'# round {r + 1}/{args.rounds} baseline: done', flush=True)
        this.append(_run_worker(HERE, args.reps, False, os.path.join(args.scratch, 'stream_bench_tune_this.txt'), dedup=True))
        print(f'# round {r + 1}/{args.rounds} this: done', flush=True)
    pts = [r['points'][name] for r in this]
    bpts = [r['points'][name] for r in base]
    lines = [f'# tools/stream_bench.py --dedup  this = {this[0]["version"]}' + (f'  baseline = {base[0]["version"]}' if base else '') +
             f'  {this[0]["device"]}  rounds={args.rounds} reps={args.reps}',
             '# ms per push, device-resident unless "host": mean [min .. max] over rounds x reps windows.  "" = dup_hi -1, _dd0 = dup_hi 0 on frames that are',
             '# never duplicates, _dup = a push that is a duplicate',
             f'{name}:']
    for key in plain_rows:
        if bpts:
            lines.append(f'  {"baseline " + key:<26} {_stat([s for p in bpts for s in p[key]])}')
    for key in plain_rows:
        for suf in ('', '_dd0', '_dup'):
            lines.append(f'  {key + suf:<26} {_stat([s for p in pts for s in p[key + suf]])}')
    for key in plain_rows:
        if bpts:      # (a)
            bm = [statistics.mean(p[key]) for p in bpts]
            d = [statistics.mean(p[key]) - b for p, b in zip(pts, bm)]
            lines.append(f'  (a) {key + " - baseline " + key:<40} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms'
                         f'   (baseline round means {" ".join(f"{b:.3f}" for b in bm)}, spread {max(bm) - min(bm):.3f} ms; '
                         f'all windows {max(s for p in bpts for s in p[key]) - min(s for p in bpts for s in p[key]):.3f} ms)')
    for key in plain_rows:      # (b)
        d = [statistics.mean(p[key + '_dd0']) - statistics.mean(p[key]) for p in pts]
        allw = [s for p in pts for s in p[key]]
        lines.append(f'  (b) {key + "_dd0 - " + key:<40} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms'
                     f'   (spread of {key} over all windows of this tree: {max(allw) - min(allw):.3f} ms)')
    for key in plain_rows:      # (c)
        lines.append(f'  (c) {key + "_dup":<40} {_stat([s for p in pts for s in p[key + "_dup"]])} ms')
    lines.append('(d) frame_diff_kernel alone (memset + kernel per call), microseconds per call: mean [min .. max]; the bytes of both frames / 6.29 TB/s beside it')
    for key in this[0]['diff_us']:
        v = [s for r in this for s in r['diff_us'][key][:-1]]
        nbytes = this[0]['diff_us'][key][-1]
        lines.append(f'  {key:<24} {_stat(v)} us   {nbytes / 1e6:7.2f} MB   {nbytes / 6.29e12 * 1e6:6.2f} us at the HBM rate')
    lines.append('# raw: ' + json.dumps({'baseline': base, 'this': this}))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


def groups_worker(root, reps, parts):
    """--groups: see the module text; prints one JSON line."""
    for p in (root, os.path.join(root, 'frame-interpolation_amd')):
        sys.path.insert(0, p)
    import ctypes
    import numpy as np
    import torch
    from film_hip import weights as W
    from film_hip import engine as engine_mod
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    from film_hip.torch_io import DeviceInterpolator
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(W.make_synthetic_weights(PUBLISHED, seed=0))
    out = {'version': FilmEngine.version(), 'device': torch.cuda.get_device_name(0)}
    state = {'i': 0}

    def nxt(m):
        state['i'] = (state['i'] + 1) % m
        return state['i']

    def timed(call, n, warm=2):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        samples = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            torch.cuda.synchronize()
            samples.append(round((time.perf_counter() - t0) * 1e3 / n, 4))
        return samples

    if 'b' in parts:     # the carry's cost alone: two groups against one, one process
        name, h, w, align, block, n, _ = POINTS[0]
        it = DeviceInterpolator(eng, align=align, block_shape=list(block))
        x = [torch.from_numpy(f).cuda() for f in _frames(4, h, w)]
        res = {}
        for t in (1, 3):
            first = {}
            for mb in (0, 2):
                eng.set_option('max_batch', mb)
                try:
                    with it.stream(h, w, 'f32', times=t) as st:
                        eng.set_option('max_batch', 0)
                        lay = st.layout()
                        st.push(x[0])
                        first[mb] = st.push(x[1]).clone()
                        res[f'push_f32_t{t}_mb{mb}'] = timed(lambda: st.push(x[nxt(4)]), max(4, n // ((1 << t) - 1) // 2))
                        res[f'layout_t{t}_mb{mb}'] = {k: lay[k] for k in ('tiles', 'groups', 'group_tiles', 'workspace_bytes', 'carry_bytes')}
                finally:
                    eng.set_option('max_batch', 0)
            res[f'identical_t{t}'] = bool(torch.equal(first[0], first[2]))
        out['b'] = res
        del x, it, first
        torch.cuda.empty_cache()

    lay4k = None
    if 'c' in parts or 'd' in parts:
        name, h, w, align, block, n, _ = GROUPS_POINT
        it = DeviceInterpolator(eng, align=align, block_shape=list(block))
        fr = _frames(4, h, w)
        x = [torch.from_numpy(f).cuda() for f in fr]
        res = {}
        if 'c' in parts:
            res['pair'] = timed(lambda: it.batch(x[nxt(3)][None], x[state['i'] + 1][None]), n, warm=1)
            res['host_pair'] = timed(lambda: eng.interpolate_frames(fr[:1], fr[1:2], align=align, block_shape=block), n, warm=1)
            ref = it.batch(x[0][None], x[1][None])[0]
            y10 = [torch.empty(engine_mod.frame_shape('i010', h, w), dtype=torch.int16, device='cuda') for _ in x]
            for src, dst in zip(x, y10):
                eng.to_yuv_device(src.data_ptr(), dst.data_ptr(), h, w, 'i010')
            torch.cuda.synchronize()
            h10 = [t.cpu().numpy().view(np.uint16) for t in y10]
            # what an i010 stream computes for frames 0 and 1: film_to_yuv of film_interpolate on the frames the cut dequantises
            deq = [torch.empty_like(x[0]) for _ in range(2)]
            for src, dst in zip(y10, deq):
                eng.debug_yuv_cut(src.data_ptr(), dst.data_ptr(), 1, h, w, None, None, 0, 1, pix='i010')
            ref10 = torch.empty_like(y10[0])
            eng.to_yuv_device(it.batch(deq[0][None], deq[1][None])[0].data_ptr(), ref10.data_ptr(), h, w, 'i010')
            torch.cuda.synchronize()
            del deq
            same = {}
            eng.set_option('max_batch', 8)       # T = 1 in two groups of 8, where the whole frame would fit one invocation
            try:
                with it.stream(h, w, 'f32') as st:
                    eng.set_option('max_batch', 0)
                    lay = st.layout()
                    res['layout_t1_mb8'] = {k: lay[k] for k in ('tiles', 'groups', 'group_tiles', 'workspace_bytes', 'carry_bytes')}
                    st.push(x[0])
                    same['f32_t1_mb8'] = bool(torch.equal(st.push(x[1]), ref))
                    res['push_f32_t1_mb8'] = timed(lambda: st.push(x[nxt(4)]), n, warm=2)
            finally:
                eng.set_option('max_batch', 0)
            for pix, dev, host in (('f32', x, fr), ('i010', y10, h10)):
                for t, sels in ((1, [None]), (3, [(3, 6), (2, 5)])):
                    turn = {'k': 0}

                    def select(st):
                        if t > 1:
                            st.select(sels[turn['k'] % len(sels)])
                            turn['k'] += 1

                    def dev_push(st):
                        select(st)
                        return st.push(dev[nxt(4)])

                    def host_push(st):
                        select(st)
                        return st.push(host[nxt(4)])

                    with it.stream(h, w, pix, times=t) as st:
                        lay4k = st.layout()
                        res[f'layout_t{t}'] = {k: lay4k[k] for k in ('tiles', 'groups', 'group_tiles', 'workspace_bytes', 'carry_bytes')}
                        st.push(dev[0])
                        if t > 1:
                            st.select([4])                      # position 4 of 7 is the mid-frame of the pair
                        mid = st.push(dev[1])
                        want = ref if pix == 'f32' else ref10
                        same[f'{pix}_t{t}'] = bool(torch.equal(mid.reshape(want.shape), want))
                        res[f'push_{pix}_t{t}'] = timed(lambda: dev_push(st), n, warm=2)
                    with eng.open_stream(h, w, align=align, block_shape=block, pix=pix, times=t) as st:
                        st.push(host[0])
                        res[f'host_push_{pix}_t{t}'] = timed(lambda: host_push(st), n, warm=2)
            res['identical'] = all(same.values())
            res['identical_each'] = same
            del y10, h10
        if lay4k is None:
            with it.stream(h, w, 'f32') as st:
                lay4k = st.layout()
        out['c'] = res
        del x, it
        torch.cuda.empty_cache()

    if 'd' in parts and lay4k and lay4k['groups'] > 1:
        # the restore table of group 0: both slots, carry -> plan, at the offsets' own alignments, in buffers of their own
        segs, s_end, d_end = [], 0, 0
        for stt in lay4k['states']:
            if stt['group'] != 0 or stt['slot'] > 1:
                continue
            for g in stt['segments']:
                s_off = (s_end + 63) // 64 * 64 + g['carry_off'] % 64
                d_off = (d_end + 63) // 64 * 64 + g['plan_off'] % 64
                segs.append((s_off, d_off, g['floats']))
                s_end, d_end = s_off + g['floats'], d_off + g['floats']
        src = torch.rand(s_end + 64, device='cuda')
        dst = torch.zeros(d_end + 64, device='cuda')
        stream = torch.cuda.current_stream().cuda_stream
        hip = ctypes.CDLL(engine_mod.hip_runtime_info()[0])
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

        def kernel():
            engine_mod.segment_copy_device(segs, src.data_ptr(), dst.data_ptr(), stream)

        def memcpy():
            for so, do, c in segs:
                assert hip.hipMemcpyAsync(dst.data_ptr() + 4 * do, src.data_ptr() + 4 * so, 4 * c, 3, stream) == 0

        def events(call, calls=50):
            call()
            torch.cuda.synchronize()
            samples = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                samples.append(round(e0.elapsed_time(e1) * 1e3 / calls, 2))
            return samples

        kernel()
        torch.cuda.synchronize()
        ok = all(bool(torch.equal(dst[do:do + c], src[so:so + c])) for so, do, c in segs)
        out['d'] = {'segments': len(segs), 'bytes': 4 * sum(c for _, _, c in segs), 'copied': ok, 'kernel_us': events(kernel), 'memcpy_us': events(memcpy)}
    eng.save_tune_cache()
    eng.close()
    print('STREAM_BENCH ' + json.dumps(out), flush=True)


def groups_main(args):
    os.makedirs(args.scratch, exist_ok=True)
    runs = [_run_worker(HERE, args.reps, False, os.path.join(args.scratch, 'stream_bench_tune_this.txt'), groups=args.groups_parts) for _ in range(args.rounds)]
    r0 = runs[0]
    lines = [f'# tools/stream_bench.py --groups  this = {r0["version"]}  {r0["device"]}  rounds={args.rounds} reps={args.reps}',
             '# ms per PUSH, device-resident unless "host": mean [min .. max] over rounds x reps windows']
    gib = lambda b: f'{b / 2 ** 30:.2f} GiB'      # noqa: E731
    if 'b' in r0:
        lines.append(f'{POINTS[0][0]}: the carry alone - max_batch 2 (two groups of two tiles) against max_batch 0 (one group), one process')
        for t in (1, 3):
            for mb in (0, 2):
                lay = r0['b'][f'layout_t{t}_mb{mb}']
                lines.append(f'  {f"push_f32_t{t}_mb{mb}":<22} {_stat([s for r in runs for s in r["b"][f"push_f32_t{t}_mb{mb}"]])}   {lay["groups"]} x {lay["group_tiles"]} tiles, '
                             f'workspace {gib(lay["workspace_bytes"])}, carry {gib(lay["carry_bytes"])}')
            d = [statistics.mean(r['b'][f'push_f32_t{t}_mb2']) - statistics.mean(r['b'][f'push_f32_t{t}_mb0']) for r in runs]
            lines.append(f'  {f"t{t}: mb2 - mb0":<22} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms per push, '
                         f'{statistics.mean(d) / ((1 << t) - 1):+.3f} ms per pair run ({(1 << t) - 1} per push)')
            lines.append(f'  t{t}: the grouped push == the one-group push, bit for bit: {all(r["b"][f"identical_t{t}"] for r in runs)}')
    if 'c' in r0 and 'pair' in r0['c']:
        c0 = r0['c']
        lines.append(f'{GROUPS_POINT[0]}: T = 1 full pushes; T = 3 pushes taking the selections (3, 6) and (2, 5) in turn (24 -> 60: 2.5 frames per input interval)')
        for t in (1, 3):
            lay = c0[f'layout_t{t}']
            lines.append(f'  layout T = {t}: {lay["tiles"]} tiles in {lay["groups"]} groups of {lay["group_tiles"]}, workspace {lay["workspace_bytes"]} bytes '
                         f'({gib(lay["workspace_bytes"])}), carry {lay["carry_bytes"]} bytes ({gib(lay["carry_bytes"])})')
        lay = c0['layout_t1_mb8']
        lines.append(f'  layout T = 1, max_batch 8: {lay["tiles"]} tiles in {lay["groups"]} groups of {lay["group_tiles"]}, workspace {lay["workspace_bytes"]} bytes '
                     f'({gib(lay["workspace_bytes"])}), carry {lay["carry_bytes"]} bytes ({gib(lay["carry_bytes"])})')
        for key in ('pair', 'host_pair', 'push_f32_t1_mb8') + tuple(f'{pre}push_{pix}_t{t}' for t in (1, 3) for pix in ('f32', 'i010') for pre in ('', 'host_')):
            lines.append(f'  {key:<22} {_stat([s for r in runs for s in r["c"][key]])}' +
                         ('   (per-pair film_interpolate, one frame per call)' if key.endswith('pair') else ''))
        for pre, pair in (('', 'pair'), ('host_', 'host_pair')):
            pm = statistics.mean(s for r in runs for s in r['c'][pair])
            for pix in ('f32', 'i010'):
                p1 = statistics.mean(s for r in runs for s in r['c'][f'{pre}push_{pix}_t1'])
                p3 = statistics.mean(s for r in runs for s in r['c'][f'{pre}push_{pix}_t3'])
                lines.append(f'  {pre}push_{pix}: T = 1 {p1:.1f} ms per frame = {1e3 / p1:.2f} frames/s against {pm:.1f} ms = {1e3 / pm:.2f} frames/s of the pair call; '
                             f'T = 3 selected {p3 / 2:.1f} ms per frame (2 per push) against {pm * 4 / 2:.1f} ms of 4 pair calls per 2 frames')
        lines.append(f'  the first mid-frame of every stream == film_interpolate (i010: film_to_yuv of it on the dequantised frames), bit for bit: '
                     f'{all(r["c"]["identical"] for r in runs)}  {json.dumps(c0["identical_each"])}')
    if 'd' in r0:
        d0 = r0['d']
        lines.append(f'segment copy alone: the restore table of one {GROUPS_POINT[0]} group, {d0["segments"]} segments, {d0["bytes"]} bytes ({d0["bytes"] / 1e9:.2f} GB read and as much written); '
                     f'{2 * d0["bytes"] / 6.29e12 * 1e6:.0f} us at the 6.29 TB/s copy rate (bytes read + bytes written); copied bit for bit: {all(r["d"]["copied"] for r in runs)}')
        for key in ('kernel_us', 'memcpy_us'):
            v = [s for r in runs for s in r['d'][key]]
            lines.append(f'  {key:<22} {_stat(v)} us per call   {2 * d0["bytes"] / statistics.mean(v) / 1e6:.2f} TB/s read + written')
    lines.append('# raw: ' + json.dumps(runs))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    ok = all(r.get('b', {}).get(f'identical_t{t}', True) for r in runs for t in (1, 3)) and all(r.get('c', {}).get('identical', True) for r in runs) and \
        all(r.get('d', {}).get('copied', True) for r in runs)
    if not ok:
        raise SystemExit('a grouped push differs from its reference')


def _run_worker(root, reps, quick, tune_file, rows=None, points=None, scene_cut=False, times=None, select=None, dedup=False, groups=None):
    env = dict(os.environ, FILM_TUNE_CACHE=tune_file)
    cmd = [sys.executable, os.path.abspath(__file__), '--worker', root, '--reps', str(reps)] + (['--quick'] if quick else [])
    cmd += (['--rows', ','.join(rows)] if rows else []) + (['--points', ','.join(points)] if points else []) + (['--scene_cut'] if scene_cut else [])
    cmd += ['--dedup'] if dedup else []
    cmd += ['--groups', '--groups-parts', groups] if groups else []
    cmd += ['--times', ','.join(str(t) for t in times)] if times else []
    cmd += ['--select', select] if select else []
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100 if groups else 900)   # (a hung worker ends the run: nothing is started behind it)
    for line in p.stdout.splitlines():
        if line.startswith('STREAM_BENCH '):
            return json.loads(line[len('STREAM_BENCH '):])
    raise SystemExit(f'worker for {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}')


def _stat(v):
    return f'{statistics.mean(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]'


def times_main(args, times):
    """--times: rounds of (baseline's times = 1 pushes,) this tree's rows; the report in ms per generated frame."""
    os.makedirs(args.scratch, exist_ok=True)
    name = POINTS[0][0]
    t1_rows = ['push_f32', 'push_i420', 'host_push_f32', 'host_push_i420']
    base, this = [], []
    for r in range(args.rounds):
        if args.baseline_root:
            base.append(_run_worker(os.path.abspath(args.baseline_root), args.reps, False, os.path.join(args.scratch, 'stream_bench_tune_baseline.txt'),
                                    t1_rows, [name]))
            print(f'# round {r + 1}/{args.rounds} baseline: done', flush=True)
        this.append(_run_worker(HERE, args.reps, False, os.path.join(args.scratch, 'stream_bench_tune_this.txt'), times=times))
        print(f'# round {r + 1}/{args.rounds} this: done', flush=True)
    pts = [r['points'][name] for r in this]
    lines = [f'# tools/stream_bench.py --times {",".join(map(str, times))}  this = {this[0]["version"]}' +
             (f'  baseline = {base[0]["version"]}' if base else '') + f'  {this[0]["device"]}  rounds={args.rounds} reps={args.reps}',
             '# ms per GENERATED FRAME (a times = T push generates 2^T - 1), device-resident unless "host": mean [min .. max] over rounds x reps windows',
             f'{name}:']
    for key in t1_rows:
        if base:
            lines.append(f'  {"baseline " + key:<26} {_stat([s for r in base for s in r["points"][name][key]])}')
    for key in sorted(k for k in pts[0] if k not in ('identical', 'workspace_bytes')):
        lines.append(f'  {key:<26} {_stat([s for p in pts for s in p[key]])}')
    for pre in ('push_f32', 'push_i420', 'host_push_f32', 'host_push_i420'):
        one = [statistics.mean(p[pre + '_t1']) for p in pts]
        for t in times:
            if t == 1:
                continue
            d = [statistics.mean(p[f'{pre}_t{t}']) - o for p, o in zip(pts, one)]
            lines.append(f'  {f"{pre}_t{t} - {pre}_t1":<40} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms per frame'
                         f'   (spread of {pre}_t1 over all windows: {max(s for p in pts for s in p[pre + "_t1"]) - min(s for p in pts for s in p[pre + "_t1"]):.3f} ms)')
    lines.append(f'  times > 1 push_f32 == interpolate_pair_recursively, bit for bit: {all(p["identical"] for p in pts)}')
    lines.append('  stream plan workspace, bytes: ' + '  '.join(f'T={t}: {b} ({b / 2**30:.2f} GiB)' for t, b in pts[0]['workspace_bytes'].items()))
    lines.append('# raw: ' + json.dumps({'baseline': base, 'this': this}))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    if not all(p['identical'] for p in pts):
        raise SystemExit('a times > 1 push differs from the pairwise recursion')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline-root', default=None, help='a built checkout of the commit to compare with (its film_interpolate is the baseline)')
    ap.add_argument('--rounds', type=int, default=3, help='alternations baseline / this tree (fresh processes)')
    ap.add_argument('--reps', type=int, default=3, help='timed windows per measurement and round')
    ap.add_argument('--quick', action='store_true', help='without the 1080p point')
    ap.add_argument('--scratch', default=os.path.join(HERE, 'tools', 'scratch'), help='where the per-tree autotune caches go')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    ap.add_argument('--rows', default=None, help='comma-separated measurements to take (default: all), e.g. push_u8,push_i420,host_push_u8')
    ap.add_argument('--points', default=None, help='comma-separated points to run (default: all), e.g. "1080p 2x2"')
    ap.add_argument('--scene_cut', action='store_true', help='add the cost of option "scene_cut" and of its histogram kernel alone (see above)')
    ap.add_argument('--times', default=None, help='comma-separated "stream_times" values, e.g. 2,3: the recursive-stream report instead (see above)')
    ap.add_argument('--select', default=None, metavar='"3,6/2,5"',
                    help='with --times T (one value): the selected-push report instead - the selections (1-based positions, comma-separated; '
                         '"/" between selections) are taken in turn, push after push (FilmStream.select), beside the full push of this tree and of the baseline')
    ap.add_argument('--dedup', action='store_true', help='the report about option "dup_hi" and its block-SAD kernel alone instead (see above)')
    ap.add_argument('--groups', action='store_true', help='the report about tile groups instead (see above): the carry alone, 4K 4x4 pushes, the copy kernel alone')
    ap.add_argument('--groups-parts', default='b,c,d', help='with --groups: the parts to run, of b (1080p carry cost), c (4K pushes), d (copy kernel alone)')
    ap.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    rows = args.rows.split(',') if args.rows else None
    points = args.points.split(',') if args.points else None
    times = [int(t) for t in args.times.split(',')] if args.times else None
    if args.select:
        if not times or len(times) != 1:
            raise SystemExit('--select needs --times T with one value')
        selections = [tuple(int(p) for p in part.split(',') if p.strip()) for part in args.select.split('/')]
        if args.worker:
            return select_worker(args.worker, args.reps, times[0], selections)
        return select_main(args, times[0], selections)
    if args.groups:
        return groups_worker(args.worker, args.reps, args.groups_parts.split(',')) if args.worker else groups_main(args)
    if args.dedup:
        return dedup_worker(args.worker, args.reps) if args.worker else dedup_main(args)
    if times and args.worker:
        return times_worker(args.worker, args.reps, times)
    if times:
        return times_main(args, times)
    if args.worker:
        return worker(args.worker, args.reps, args.quick, rows, points, args.scene_cut)
    os.makedirs(args.scratch, exist_ok=True)
    trees = ([('baseline', os.path.abspath(args.baseline_root))] if args.baseline_root else []) + [('this', HERE)]
    runs = {k: [] for k, _ in trees}
    for r in range(args.rounds):
        for k, root in trees:
            runs[k].append(_run_worker(root, args.reps, args.quick, os.path.join(args.scratch, f'stream_bench_tune_{k}.txt'), rows, points, args.scene_cut))
            print(f'# round {r + 1}/{args.rounds} {k}: done', flush=True)
    this = runs['this']
    lines = [f'# tools/stream_bench.py  this = {this[0]["version"]}' + (f'  baseline = {runs["baseline"][0]["version"]}' if args.baseline_root else '') +
             f'  {this[0]["device"]}  rounds={args.rounds} reps={args.reps}',
             '# ms per call, device-resident unless "host": mean [min .. max] over rounds x reps windows']
    for name, *_ in POINTS:
        if name not in this[0]['points']:
            continue
        lines.append(f'{name}:')
        pts = [r['points'][name] for r in this]
        base = [r['points'][name] for r in runs.get('baseline', [])]
        for key in ('pair', 'push_u8', 'push_i420', 'push_i010', 'host_push_u8', 'host_push_i420', 'host_push_i010'):
            if base and key in base[0]:
                lines.append(f'  {"baseline " + key:<22} {_stat([s for p in base for s in p[key]])}')
        for key in ('pair', 'push_f32', 'push_u8', 'push_i420', 'push_nv12', 'push_i010', 'push_p010', 'push_i422', 'push_i444', 'push_i210', 'push_i410',
                    'sequence', 'host_pair', 'host_push_f32', 'host_push_u8', 'host_push_i420', 'host_push_nv12', 'host_push_i010', 'host_push_p010',
                    'host_push_i422', 'host_push_i444', 'host_push_i210', 'host_push_i410'):
            if key in pts[0]:
                lines.append(f'  {key:<22} {_stat([s for p in pts for s in p[key]])}' + ('   (per generated frame)' if key == 'sequence' else ''))
        lines.append(f'  push_f32 == pair, bit for bit: {all(p.get("identical", True) for p in pts)}')
        if base and 'pair' in base[0]:
            bm = [statistics.mean(p['pair']) for p in base]
            spread = max(bm) - min(bm)
            for key in ('pair', 'push_f32', 'push_u8'):
                if key in pts[0]:
                    d = [statistics.mean(p[key]) - b for p, b in zip(pts, bm)]
                    lines.append(f'  {key + " - baseline pair":<36} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms')
            lines.append(f'  spread of the baseline pair call over the rounds (max - min of the round means): {spread:.3f} ms')
        # the 4:2:0 pushes against what the baseline offers such a caller: its 8-bit RGB push
        # ... and the 10-bit pushes against its 8-bit 4:2:0 push (such a caller had to truncate to 8 bits); this tree's own 8-bit pushes
        # against the baseline's show that the 8-bit paths are unchanged
        for mine, theirs in [(f'{pre}push_{pix}', f'{pre}push_u8') for pre in ('', 'host_') for pix in ('i420', 'nv12')] + \
                            [(f'{pre}push_{pix}', f'{pre}push_i420') for pre in ('', 'host_') for pix in ('i010', 'p010')] + \
                            ([(f'{pre}push_{pix}', f'{pre}push_{pix}') for pre in ('', 'host_') for pix in ('u8', 'i420')] if 'push_i010' in pts[0] or 'host_push_i010' in pts[0] else []) + \
                            ([(f'{pre}push_{pix}', f'{pre}push_{pix}') for pre in ('', 'host_') for pix in ('i010', 'p010')] +      # the planar 4:2:2 / 4:4:4 pushes against the
                             [(f'{pre}push_{pix}', f'{pre}push_u8') for pre in ('', 'host_') for pix in ('i422', 'i444', 'i210', 'i410')]      # baseline's 8-bit RGB push
                             if any(k in pts[0] for k in ('push_i444', 'host_push_i444', 'push_i410', 'host_push_i410')) else []):
            if base and theirs in base[0] and mine in pts[0]:
                bm = [statistics.mean(p[theirs]) for p in base]
                d = [statistics.mean(p[mine]) - b for p, b in zip(pts, bm)]
                lines.append(f'  {mine + " - baseline " + theirs:<36} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms'
                             f'   (baseline {theirs}: round means {" ".join(f"{b:.3f}" for b in bm)}, spread {max(bm) - min(bm):.3f} ms)')
        # option "scene_cut": what the histogram and its wait add to a steady push, a push that is a cut beside a first push
        for pre in ('', 'host_'):
            for pix in ('u8', 'i420'):
                plain, sc, cut, first = (f'{pre}push_{pix}{suf}' for suf in ('', '_sc1000', '_cut', '_first'))
                if sc not in pts[0]:
                    continue
                for key in (sc, cut, first):
                    lines.append(f'  {key:<22} {_stat([s for p in pts for s in p[key]])}')
                if plain in pts[0]:
                    d = [statistics.mean(p[sc]) - statistics.mean(p[plain]) for p in pts]
                    lines.append(f'  {sc + " - " + plain:<36} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms   (scene_cut = 1000 against 0, this tree)')
                    if base and plain in base[0]:
                        bm = [statistics.mean(p[plain]) for p in base]
                        d0 = [statistics.mean(p[plain]) - b for p, b in zip(pts, bm)]
                        lines.append(f'  {plain + " - baseline " + plain:<36} per round: {" ".join(f"{v:+.3f}" for v in d0)}   mean {statistics.mean(d0):+.3f} ms'
                                     f'   (scene_cut = 0; baseline round means {" ".join(f"{b:.3f}" for b in bm)}, spread {max(bm) - min(bm):.3f} ms)')
                d = [statistics.mean(p[cut]) - statistics.mean(p[first]) for p in pts]
                lines.append(f'  {cut + " - " + first:<36} per round: {" ".join(f"{v:+.3f}" for v in d)}   mean {statistics.mean(d):+.3f} ms')
    if 'histogram_us' in this[0]:
        lines.append('frame_histogram_kernel alone (memset + kernel per call), microseconds per call: mean [min .. max]; the frame\'s bytes / 6.29 TB/s beside it')
        for key in this[0]['histogram_us']:
            v = [s for r in this for s in r['histogram_us'][key][:-1]]
            nbytes = this[0]['histogram_us'][key][-1]
            lines.append(f'  {key:<22} {_stat(v)} us   {nbytes / 1e6:7.2f} MB   {nbytes / 6.29e12 * 1e6:6.2f} us at the HBM rate')
    lines.append('# raw: ' + json.dumps(runs))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    if not all(p.get('identical', True) for r in this for p in r['points'].values()):
        raise SystemExit('a push differs from the pair call')


if __name__ == '__main__':
    main()
