#!/usr/bin/env python
"""Digest of the planner's output over a grid of configurations, shapes and options: the comparison tool for a change to
csrc/film_planner.cpp that must leave every plan as it is.  Plan-only handles (device = -1): runs without a GPU.  A tool, not a test: it
pins nothing - run it on the library before and after the change and `diff` the two outputs.

  FILM_HIP_LIB=<libfilm_hip*.so> python tools/plan_digest.py            one line per record: "<config> <options> <call> <sha1>", the sha1
                                                                          of the JSON text film_plan_json / film_sequence_plan_json /
                                                                          film_stream_plan_json / film_stream_pair_plan_json /
                                                                          film_stream_schedule_json returned,
                                                                          or of "error <code>: <message>" for a refused call or option value;
                                                                          then "records <n>" and "digest <sha1 over all lines>"
  FILM_HIP_LIB=... python tools/plan_digest.py --splitk                  instead: the conv ops with ksplit > 1 of the default plans of the
                                                                          shapes the GPU suite runs, by kernel family

The library comes from FILM_HIP_LIB like for every other tool (film_hip/engine.py); a host-only build is enough and fastest:
  tools/sanitize/build_host.sh none [outdir]                             (FILM_EXTRA_FAMILIES=1: the flavour that can select the opt-in
                                                                          families - most of the family rules only show there)
Option grid: every film_set_option key that drops the cached plans (kOptions in csrc/film_engine.cpp), one at a time over its whole
range - for the two pixel thresholds, both sides of every level size the planner can compare them with in these shapes - plus the
combinations the rules couple.  Per setting also the stream plans (STREAM_SHAPES): both orientations of the two-slot plan, every pair run
(left, right, extract) the schedules of "stream_times" = 1 .. 3 list, the schedules themselves and one refused argument set.  About
42 000 records (48 000 with the opt-in families), a few minutes on a host-only build."""
import ctypes
import hashlib
import itertools
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, 'frame-interpolation_amd')]
os.environ.setdefault('FILM_NO_TORCH', '1')     # plan-only handles: no need to load PyTorch's HIP runtime first

PAIR_SHAPES = {
    'PUBLISHED': [(1, 64, 64), (2, 64, 128), (1, 128, 192), (3, 128, 192), (1, 256, 256), (1, 256, 448), (8, 256, 448), (1, 768, 1024),
                  (4, 576, 960),        # the 2x2 tiles of a 1080p frame
                  (1, 1088, 1920),
                  (1, 2176, 3840),      # an untiled 4K frame: the 4 GiB rule
                  (1, 96, 64)],         # refused: H is not a multiple of 64
    'TINY': [(1, 32, 32), (2, 32, 48), (1, 64, 40), (1, 64, 64), (2, 64, 96), (1, 256, 256), (1, 36, 32)],   # (the last: refused)
}
SEQUENCE_SHAPES = [(3, 1, 256, 448), (2, 4, 576, 960)]      # (pairs, tiles, H, W)
STREAM_SHAPES = {'PUBLISHED': [(1, 256, 256), (4, 576, 960)], 'TINY': [(1, 32, 48), (2, 32, 48), (1, 64, 96), (2, 64, 96)]}   # (tiles, H, W)
STREAM_TIMES = (1, 2, 3)

# pixels per image of the pyramid levels of the shapes above that lie near the defaults (256 / 1536): "px >= option" flips between t and t + 1
LEVEL_PX = [64, 192, 256, 448, 540, 768, 1024, 1536, 1792, 2160, 4096]
W2D_PX = sorted({v for t in LEVEL_PX for v in (t, t + 1)} | {1535, 255, 8640, 8641, 1 << 30})
SINGLE = {
    'splitk': range(2), 'fuse': range(32), 'fold2x2': range(3), 'planar': range(2), 'winograd': range(4), 'halo_all': range(2),
    'lanes': range(4), 'wino2d': range(3), 'w2d_splitk': range(17), 'w2d_shape': range(-1, 6), 'fold4_shape': range(-1, 2),
    'w43_shape': range(-1, 32), 'precision': range(3),
    'w2d_small_px': [0, 1] + W2D_PX, 'w2d_min_px': [1] + W2D_PX,
}
COUPLED = [
    {'precision': range(3), 'winograd': range(4), 'halo_all': range(2)},
    {'wino2d': range(3), 'winograd': range(4)},
    {'splitk': range(2), 'w2d_splitk': range(17)},
    {'fold2x2': range(3), 'precision': range(3)},
    {'lanes': range(4), 'planar': range(2)},
    {'wino2d': range(3), 'precision': range(3)},
    {'w2d_min_px': [1, 1536, 1 << 30], 'w2d_small_px': [0, 256, 1 << 30], 'winograd': [1, 3]},
]


def settings():
    """Every option setting of the grid once: {} (the defaults), each single value, each coupled combination."""
    seen, out = set(), []
    combos = [{}] + [{k: v} for k, vals in SINGLE.items() for v in vals]
    for group in COUPLED:
        combos += [dict(zip(group, vs)) for vs in itertools.product(*group.values())]
    for s in combos:
        key = tuple(sorted(s.items()))
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


def call_text(eng, fn, *args):
    """The text a film_*_json call returns, byte for byte, or "error <code>: <message>"."""
    need = ctypes.c_int64()
    rc = fn(eng._h, *args, None, 0, ctypes.byref(need))
    if rc == 0:
        buf = ctypes.create_string_buffer(need.value)
        rc = fn(eng._h, *args, buf, need.value, ctypes.byref(need))
        if rc == 0:
            return buf.value
    return b'error %d: ' % rc + (eng._lib.film_last_error(eng._h) or b'')


def engine_with(opt, setting):
    """(plan-only engine with the options set, None) or (None, the refusal of the first option value the library does not take)."""
    from film_hip.engine import FilmEngine, FilmError
    eng = FilmEngine(opt, device=-1)
    for k, v in setting.items():
        try:
            eng.set_option(k, v)
        except FilmError as e:
            eng.close()
            return None, ('error %d: %s' % (e.code, e.msg)).encode()
    return eng, None


def stream_records(eng, head):
    """The stream plans of one engine: see the module text."""
    lib = eng._lib
    runs = {}       # times -> the (left, right, extract) of every pair run its two schedules list, in their order
    for times in STREAM_TIMES:
        for slot in (0, 1):
            text = call_text(eng, lib.film_stream_schedule_json, times, slot)
            yield f'{head} stream_schedule({times},{slot})', text
            for step in json.loads(text)['steps']:
                runs.setdefault(times, {})[(step['left'], step['right'], step['extract'])] = None
    for t, h, w in STREAM_SHAPES[head.split()[0]]:
        for slot in (0, 1):
            yield f'{head} stream_plan({t},{h},{w},{slot})', call_text(eng, lib.film_stream_plan_json, t, h, w, slot)
        for times in STREAM_TIMES:
            for left, right, extract in runs[times]:
                yield (f'{head} stream_pair_plan({t},{h},{w},{times},{left},{right},{extract})',
                       call_text(eng, lib.film_stream_pair_plan_json, t, h, w, times, left, right, extract))
    t, h, w = STREAM_SHAPES[head.split()[0]][0]
    yield f'{head} stream_pair_plan({t},{h},{w},1,1,1,1)', call_text(eng, lib.film_stream_pair_plan_json, t, h, w, 1, 1, 1, 1)   # (refused: left == right)


def records():
    from film_hip import options as O
    for cfg in ('PUBLISHED', 'TINY'):
        for setting in settings():
            name = ','.join(f'{k}={v}' for k, v in setting.items()) or 'defaults'
            eng, refusal = engine_with(getattr(O, cfg), setting)
            if eng is None:
                yield f'{cfg} {name} set_option', refusal
                continue
            for b, h, w in PAIR_SHAPES[cfg]:
                yield f'{cfg} {name} plan({b},{h},{w})', call_text(eng, eng._lib.film_plan_json, b, h, w)
            for n, t, h, w in SEQUENCE_SHAPES if cfg == 'PUBLISHED' else [(2, 1, 64, 40), (2, 2, 32, 48)]:
                yield f'{cfg} {name} sequence_plan({n},{t},{h},{w})', call_text(eng, eng._lib.film_sequence_plan_json, n, t, h, w)
            yield from stream_records(eng, f'{cfg} {name}')
            eng.close()


def splitk_table():
    """Which kernel families carry split-K in the default plans of the shapes the GPU suite runs: wino 3 = conv_wino43_kernel, wino 4 =
    conv_wino2d_kernel, fold 3 = conv_fold4_kernel, neither = conv_buf_kernel."""
    from film_hip import options as O
    eng, _ = engine_with(O.PUBLISHED, {})
    for b, h, w in ((1, 64, 64), (1, 256, 256), (1, 256, 448), (4, 576, 960)):
        plan = json.loads(call_text(eng, eng._lib.film_plan_json, b, h, w))
        for op in plan['ops']:
            if op['kind'] == 'conv_mfma' and op['ksplit'] > 1:
                fam = {3: 'wino43', 4: 'wino2d'}.get(op['wino'], 'fold4' if op['fold'] == 3 else 'buf')
                print(f"{b}x{h}x{w} {fam:7s} ksplit={op['ksplit']} level={op['H']}x{op['W']} K={op['Ctot']} {op['tag']}")


def main():
    if '--splitk' in sys.argv[1:]:
        return splitk_table()
    total, n = hashlib.sha1(), 0
    for what, text in records():
        line = f'{what} {hashlib.sha1(text).hexdigest()}'
        print(line)
        total.update(line.encode() + b'\n')
        n += 1
    print('records', n)
    print('digest', total.hexdigest())


if __name__ == '__main__':
    main()
