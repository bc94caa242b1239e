"""Regenerates tests/golden/video_cli_digests.json: what eval/video_cli.py writes and asks of its stream, per mode and case, on the stand-in
interpolator of the CPU tests (tests/standin_stream.py).

    python tools/make_video_cli_golden.py

Per case: the SHA-256 of the output bytes, the return value, `cuts`, the keyword arguments open_stream got, the select() calls, the (input
index, selection) of every push that ran and every `stats` value (floats as float.hex()).  The cases, all on 4 x 6 I420 frames: plain
--times_to_interpolate 1, 2, 3; --fps over RATES at every depth of 1, 3, 4 the timing accepts; no scene_cut, and 250 with the cut at input 1
and at input 2; the patterns 'ABCDE' and 'A' (equal letters are equal frames), with --dedup 0 also the ones with repeats; a header whose rate
is not reduced (F48:2) and, for the plain mode, one without an F token; and a video whose last output is rounded down to its last frame.

The file was first written from the commit that still had one frame loop per mode (double_frame_rate, convert_frame_rate,
convert_frame_rate_dedup: `run` calls the third where convert_frame_rate takes no dedup), and tests/test_dedup_retime_cpu.py compares the one
loop with it: a change that moves one byte, one select() or one statistic of one mode shows there.  Needs no built library."""
import hashlib
import inspect
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'video_cli_digests.json')
for _p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'frame-interpolation_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RATES = [((24, 1), (60, 1)), ((24, 1), (48, 1)), ((24, 1), (30, 1)), ((24, 1), (96, 1)), ((24000, 1001), (60000, 1001)), ((30, 1), (24, 1))]
SCENES = [(0, None), (250, 1), (250, 2)]                      # (scene_cut, the input frame that starts a new scene)
PATTERNS = ['ABCDE', 'A']
REPEATS = ['AABCD', 'AAABBCCCDD', 'ABCCC', 'AAAA']            # (with dedup only: without it a repeated frame is a frame like any other)
DEDUP = (0, 0, 1000)
UNREDUCED, UNRATED = ['W6', 'H4', 'F48:2', 'C420jpeg'], ['W6', 'H4', 'C420jpeg']


def video(pattern, tokens):
    """The bytes of a 4 x 6 I420 video whose frame i is picture pattern[i]."""
    from film_hip import y4m
    rng = np.random.default_rng(5)
    pics = {c: rng.integers(0, 256, (6, 6), dtype=np.uint8) for c in sorted(set(pattern))}
    data = io.BytesIO()
    wr = y4m.Y4MWriter(data, tokens)
    for c in pattern:
        wr.write(pics[c])
    return data.getvalue()


def cases():
    """{name: (pattern, header tokens, rate_out or None, times, scene_cut, cut_at, dedup or None)}"""
    from film_hip import retime, y4m
    out = {}
    for scene_cut, cut_at in SCENES:
        cut = f'cut {scene_cut}@{cut_at}'
        for times in (1, 2, 3):
            for pattern in PATTERNS:
                for tag, tokens in (('F24:1', y4m.header_tokens(6, 4, (24, 1))), ('F48:2', UNREDUCED), ('no F', UNRATED)):
                    out[f'plain {tag} T{times} {cut} {pattern}'] = (pattern, tokens, None, times, scene_cut, cut_at, None)
        for rate_in, rate_out in RATES:
            for times in (1, 3, 4):
                try:
                    retime.Retime(rate_in, rate_out, times)
                except ValueError:
                    continue
                headers = [('', y4m.header_tokens(6, 4, rate_in))] + ([(' F48:2', UNREDUCED)] if rate_in == (24, 1) else [])
                for tag, tokens in headers:
                    name = f'fps {rate_in[0]}:{rate_in[1]}{tag} -> {rate_out[0]}:{rate_out[1]} T{times} {cut}'
                    for pattern in PATTERNS:
                        out[f'{name} {pattern}'] = (pattern, tokens, rate_out, times, scene_cut, cut_at, None)
                    for pattern in PATTERNS + REPEATS:
                        out[f'{name} {pattern} dedup'] = (pattern, tokens, rate_out, times, scene_cut, cut_at, DEDUP)
    for dedup in (None, DEDUP):          # 24 -> 30 on the grid of halves: output 4 lies at 3.2 intervals and is rounded DOWN to the last input frame
        out['fps 24:1 -> 30:1 T1 cut 0@None ABCD' + (' dedup' if dedup else '')] = ('ABCD', y4m.header_tokens(6, 4, (24, 1)), (30, 1), 1, 0, None, dedup)
    return out


def run(pattern, tokens, rate_out, times, scene_cut, cut_at, dedup):
    """One case through the module's functions, as eval.video_cli.main calls them."""
    from eval import video_cli as cli
    from film_hip import y4m
    import standin_stream
    it, out, cuts, stats = standin_stream.It(cut_at), io.BytesIO(), [], {}
    rd = y4m.Y4MReader(io.BytesIO(video(pattern, tokens)))
    if rate_out is None:
        n = cli.double_frame_rate(it, rd, out, 'bt709', None, scene_cut, cuts, times)
    elif dedup is not None and 'dedup' not in inspect.signature(cli.convert_frame_rate).parameters:
        n = cli.convert_frame_rate_dedup(it, rd, out, rate_out, dedup, 'bt709', None, scene_cut, cuts, times, stats)
    else:
        n = cli.convert_frame_rate(it, rd, out, rate_out, 'bt709', None, scene_cut, cuts, times, stats, **({'dedup': dedup} if dedup is not None else {}))
    return {'sha256': hashlib.sha256(out.getvalue()).hexdigest(), 'frames': n, 'cuts': cuts, 'open_stream': {k: list(v) if isinstance(v, tuple) else v for k, v in it.kw.items()},
            'selects': [list(s) for s in it.stream.selects], 'pushes': [[i, list(s)] for i, s in it.stream.pushes],
            'stats': {k: v.hex() if isinstance(v, float) else v for k, v in stats.items()}}


def records():
    return {name: run(*case) for name, case in cases().items()}


if __name__ == '__main__':
    new = '{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(records().items())) + '\n}\n'       # a case per line
    with open(PATH, 'w') as fo:
        fo.write(new)
    print(f'wrote {PATH}: {len(json.loads(new))} cases, {len(new)} bytes')
