"""Test-only: the case lists of the per-op isolation run (tests/test_ops_gpu.py) and ONE definition of "covered", usable without a GPU.

The planner picks the kernel family and the split-K factor of a layer from the level size, so the plan of a small frame does not hold
what the plan of a 1080p tile holds.  signature(op) is everything that selects a kernel, a template instantiation or a code path inside
it - everything but NB, H, W and the buffer offsets.  An op of a real workload (workload_plans) is covered when some listed case plans an
op with the same signature AND a tile candidate list ("cands" of the plan JSON: conv_candidates, film_tune.cpp) that is a superset of
its own: conv_wino2d_kernel's 16 x 16 arrangements are candidates only where they pad the level no more than the 8 x 32 ones, so a level
that lacks them does not stand for one that has them.  uncovered(cases) lists what no case covers; tests/test_op_coverage_cpu.py holds
it empty on plan-only handles, tests/test_ops_gpu.py requires every workload signature among the ops it actually ran.

A new planner rule or kernel family is therefore done when a SMALL case plans the variant: add it to NEW_CASES (a few seconds on the GPU:
test_workload_variants_in_isolation runs only the ops of a case that no earlier case covers)."""
from __future__ import annotations

import functools
from typing import Dict, FrozenSet, List, Tuple

import op_harness as OH


def _config(name):
    from film_hip.options import Options, PUBLISHED, TINY
    # the fine levels of a 1080p tile at 64 .. 256 channels, on frames of any multiple of 4
    wide = Options(pyramid_levels=3, fusion_pyramid_levels=3, specialized_levels=2, sub_levels=3, flow_convs=(3, 3, 3),
                   flow_filters=(64, 128, 128), filters=64)
    # the published channel counts on four levels, on frames of any multiple of 8: its coarsest level holds the 960-channel features
    deep = Options(pyramid_levels=4, fusion_pyramid_levels=4, specialized_levels=3, sub_levels=4, flow_convs=(3, 3, 3, 3),
                   flow_filters=(32, 64, 128, 256), filters=64)
    return {'published': PUBLISHED, 'tiny': TINY, 'wide': wide, 'deep': deep}[name]


_DEFAULT_PLANS = [('published', (1, 64, 64)), ('published', (2, 128, 64)), ('published', (1, 128, 320)),
                  ('wide', (1, 36, 60)), ('wide', (1, 20, 44)), ('wide', (2, 68, 100)), ('wide', (1, 12, 132)),
                  ('tiny', (3, 64, 24)), ('tiny', (2, 64, 32, 1))]       # (the last: a sequence plan of two pairs of one tile)
_OPTION_SETS = [{'wino2d': 2}, {'winograd': 3}, {'winograd': 0, 'wino2d': 0}, {'winograd': 3, 'wino2d': 0}, {'fold2x2': 0}, {'fold2x2': 2},
                {'planar': 0}, {'fuse': 0}, {'splitk': 0}, {'w2d_splitk': 0}, {'w2d_splitk': 16}]
_EXTRA_OPTION_SETS = [{'precision': 1}, {'precision': 2}, {'halo_all': 1}, {'winograd': 2}, {'winograd': 2, 'wino2d': 0},
                      {'halo_all': 1, 'winograd': 0, 'wino2d': 0}, {'precision': 1, 'halo_all': 1}, {'precision': 2, 'halo_all': 1},
                      {'precision': 2, 'winograd': 2}]
_OPTION_PLANS = [('published', (1, 64, 64)), ('wide', (1, 36, 60))]


def _case_id(cfg, key, options):
    return f'{cfg}-{"x".join(map(str, key))}' + ''.join(f'-{k}{v}' for k, v in options.items())


CASES = [(cfg, key, {}) for cfg, key in _DEFAULT_PLANS] + [(cfg, key, o) for o in _OPTION_SETS for cfg, key in _OPTION_PLANS]
EXTRA_CASES = [(cfg, key, o) for o in _EXTRA_OPTION_SETS for cfg, key in _OPTION_PLANS]
# What the plans of the real workloads hold and no case above plans (tests/test_op_coverage_cpu.py names each):
NEW_CASES = [
    # the four deep layers (K = 9 x 1920 / 896 / 2448 / 1168) on conv_wino2d_kernel UNSPLIT, on 16 x 16 and 8 x 8 levels: every W2D candidate
    ('published', (1, 64, 64), {'wino2d': 2, 'w2d_splitk': 0}),
    # the 9 x 15 coarsest level of a 576 x 960 tile with 960-channel features: conv_buf_kernel, K = 9 x 1920, ksplit = 8, a batch-remapped segment
    ('deep', (1, 72, 120), {}),
    # a published sequence plan of two pairs of one tile: the per-direction warps (warp_d0) at the published channel counts
    ('published', (2, 64, 64, 1), {}),
    ('published', (2, 64, 64, 1), {'fuse': 0}),
]


# ----------------------------------------------------------------------------------------------
# signatures
# ----------------------------------------------------------------------------------------------
def signature(op: dict) -> tuple:
    """What selects the kernel, the template instantiation and the code path of an op.  NB, H, W and buffer offsets are left out."""
    conv = op['kind'] == 'conv_mfma'
    segs = tuple((sg['v']['C'], sg['up'] != 0, sg['bmod'] != 0) for sg in op.get('segs', [])) if conv else ()
    views = () if conv else tuple((n, v['C']) for n, v, *_ in OH.in_views(op) + OH.out_views(op))
    return (op['kind'], OH.family(op), op['Ctot'], op['Cout'], op['ksize'], op['leaky'], op.get('fold', 0), op.get('ksplit', 1), segs, views,
            OH._has(op, 'out2'), OH._has(op, 'pw_out'), OH._has(op, 'img_out'), OH._has(op, 'in3'),
            op.get('misc_nb', 0) > 0, op.get('src_brot', 0) != 0, op.get('flow_brot', 0) != 0, op.get('fscale', 0))


SIGNATURE_FIELDS = ('kind', 'family', 'Ctot', 'Cout', 'ksize', 'leaky', 'fold', 'ksplit', 'segs (C, up, bmod)', 'views (name, C)',
                    'out2', 'pw_out', 'img_out', 'in3', 'misc_nb', 'src_brot', 'flow_brot', 'fscale')


def candidates(op: dict) -> FrozenSet[int]:
    """The tile codes film_debug_run_op and the autotuner try for the op ([] for an op that is no convolution)."""
    return frozenset(op['cands'])


def describe(sig: tuple) -> str:
    return ', '.join(f'{k} {v}' for k, v in zip(SIGNATURE_FIELDS, sig) if v not in ((), False, 0, 0.0) or k in ('Ctot', 'ksplit'))


class Covered:
    """signature -> the candidate sets of the ops that carry it; covers(op): one of them holds every candidate of op."""

    def __init__(self):
        self.sets: Dict[tuple, List[FrozenSet[int]]] = {}

    def add(self, sig: tuple, cands) -> None:
        have = self.sets.setdefault(sig, [])
        cands = frozenset(cands)
        if not any(c >= cands for c in have):
            have.append(cands)

    def add_plan(self, plan: dict) -> None:
        for op in plan['ops']:
            self.add(signature(op), candidates(op))

    def covers(self, op: dict) -> bool:
        own = candidates(op)
        return any(c >= own for c in self.sets.get(signature(op), ()))


# ----------------------------------------------------------------------------------------------
# plans on plan-only handles (no GPU)
# ----------------------------------------------------------------------------------------------
def _freeze(options: dict) -> tuple:
    return tuple(options.items())


@functools.lru_cache(maxsize=None)
def _case_plan(cfg: str, key: tuple, options: tuple) -> dict:
    from film_hip.engine import FilmEngine
    eng = FilmEngine(_config(cfg), device=-1)
    try:
        for k, v in options:
            eng.set_option(k, v)
        return eng.sequence_plan(key[0] // key[3], key[3], key[1], key[2]) if len(key) > 3 else eng.plan(*key)
    finally:
        eng.close()


def case_plan(cfg, key, options) -> dict:
    """The plan of a case as a plan-only handle states it (the options a case sets change no plan with the device)."""
    return _case_plan(cfg, tuple(key), _freeze(options))


PAIR_WORKLOADS = [(4, 576, 960), (1, 576, 960), (8, 576, 960), (1, 256, 256), (1, 768, 1024), (8, 256, 448), (1, 256, 448)]
STREAM_WORKLOADS = [(4, 576, 960), (1, 256, 448)]       # (tiles, H, W)
STREAM_TIMES = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def workload_plans() -> Tuple[Tuple[str, dict], ...]:
    """(label, plan) of what the published network runs on real frames: the pair plans of the benchmark and of BASELINE.json (the 2 x 2
    tiles of 1080p frames at batch 1, 4 and 8, photos, Vimeo batches), the stream plans of both slots, every pair run the stream
    schedules of times = 1 .. 3 list, and a sequence plan - all of the published configuration with default options."""
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    eng = FilmEngine(PUBLISHED, device=-1)
    out = []
    try:
        for b, h, w in PAIR_WORKLOADS:
            out.append((f'plan({b},{h},{w})', eng.plan(b, h, w)))
        for t, h, w in STREAM_WORKLOADS:
            for slot in (0, 1):
                out.append((f'stream_plan({t},{h},{w},{slot})', eng.stream_plan(t, h, w, slot)))
        t, h, w = STREAM_WORKLOADS[0]
        for times in STREAM_TIMES:
            runs = {}       # (insertion-ordered) the pair runs of both schedules
            for slot in (0, 1):
                for step in eng.stream_schedule(times, slot)['steps']:
                    runs[(step['left'], step['right'], bool(step['extract']))] = None
            for left, right, extract in runs:
                out.append((f'stream_pair_plan({t},{h},{w},{times},{left},{right},{int(extract)})',
                            eng.stream_pair_plan(t, h, w, times, left, right, extract)))
        out.append(('sequence_plan(3,4,576,960)', eng.sequence_plan(3, 4, 576, 960)))
    finally:
        eng.close()
    return tuple(out)


def workload_ops():
    """(label, op) of every op of every workload plan."""
    for label, plan in workload_plans():
        for op in plan['ops']:
            yield label, op


def uncovered(cases) -> Dict[tuple, Tuple[str, str, str]]:
    """{signature: (workload, tag, level size) of the first workload op with it} for every workload op no case of `cases` covers."""
    have = Covered()
    for cfg, key, options in cases:
        have.add_plan(case_plan(cfg, key, options))
    out = {}
    for label, op in workload_ops():
        if not have.covers(op):
            out.setdefault(signature(op), (label, op['tag'], f'{op["H"]}x{op["W"]}'))
    return out


def format_uncovered(missing: Dict[tuple, Tuple[str, str, str]]) -> str:
    return '\n'.join(f'  {describe(sig)}\n      e.g. {label}: {tag} on a {size} level' for sig, (label, tag, size) in missing.items())


def ops_no_earlier_case_covers(cases, index: int) -> List[int]:
    """Indices into the plan of cases[index] of the ops whose signature (with candidates) no case in front of it covers."""
    have = Covered()
    for cfg, key, options in cases[:index]:
        have.add_plan(case_plan(cfg, key, options))
    return [i for i, op in enumerate(case_plan(*cases[index])['ops']) if not have.covers(op)]
