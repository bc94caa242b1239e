"""Regenerates tests/golden/yuv_ref_digests.json: what tests/yuv_ref.py computes, as one 16-hex-digit sha256 prefix per function, layout and
case (or size) - the designed frames and allocations, yuv_in / yuv_out over the colour settings, the histogram, the cut over every range
of every partition and all colours, the cut once per planted fault, the branch names of both kernels.

    python tools/make_yuv_ref_golden.py

The file was first written from the three reference modules this one replaced, and tests/test_yuv_chroma_cpu.py compares the module with it:
a change to the restatement that moves one bit or one branch name shows there.  The 4:2:0 layouts are entered twice: under '420' with
their own designed frames, four colour settings and the faults of their depth (what tests/test_yuv*_{cpu,gpu}.py and test_yuv10_* use),
and under 'any' with the general generator, six colour settings and the faults of the subsampled layouts (tests/test_yuv_chroma_*).
Needs the built library (the tile geometries come from a plan-only handle)."""
import collections
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'yuv_ref_digests.json')
for _p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'frame-interpolation_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# fmt: what holds frames_view / yuv_in / yuv_out / cut / branches / out_branches; designed(b, h, w, seed) and alloc(case, seed) are bound to the layout
Source = collections.namedtuple('Source', 'tag layout fmt designed alloc histogram colours faults cases out_sizes subsampling')
FOUR = [(m, f) for m in ('bt709', 'bt601') for f in (False, True)]
SIX = FOUR + [('bt2020nc', False), ('bt2020nc', True)]
FAULTS_420 = {8: ('chroma_from_tile_coordinate', 'cb_cr_swapped', 'nv12_as_i420'),
              10: ('p010_as_i010', 'i010_as_p010', 'ignored_bits_not_masked', 'eight_bit_scale_shifted', 'cb_cr_swapped', 'chroma_from_tile_coordinate')}
FAULTS_ANY = ('chroma_row_halved', 'chroma_col_halved', 'chroma_from_tile_coordinate', 'cb_cr_swapped', 'bt709_under_bt2020', 'box_2x2_mean')
DESIGNED = {      # (b, h, w, seed) of designed_frames calls the tests make, by what the subsampling allows
    'even': [(2, 30, 50, 9), (3, 30, 50, 2), (5, 4, 6, 1), (2, 4, 6, 1), (1, 16, 18, 5), (1, 64, 64, 128), (1, 64, 64, 11), (1, 64, 64, 9), (1, 2, 2, 4), (1, 30, 50, 80)],
    'odd_h': [(5, 3, 6, 1), (3, 31, 50, 2), (1, 1, 2, 3), (1, 33, 50, 83), (1, 99, 250, 349)],
    'odd_w': [(3, 31, 49, 2), (1, 1, 1, 2), (1, 33, 51, 84), (1, 33, 63, 5), (1, 99, 249, 348)],
}


def sources():
    import yuv_ref as R

    def src(tag, layout, general):
        f = R.FORMATS[layout]
        return Source(tag, layout, f, lambda b, h, w, s: f.designed_frames(b, h, w, s, layout, general), lambda c, s: f.new_frames_alloc(c, layout, s, general),
                      f.histogram if general or f.depth == 10 else None, SIX if general else FOUR, FAULTS_ANY if general else FAULTS_420[f.depth],
                      R.CASES if f.sy else R.cases_of(layout), R.out_sizes(layout), (f.sx, f.sy))
    return [src('420', lay, False) for lay in R.OLD_LAYOUTS] + [src('any', lay, True) for lay in R.OLD_LAYOUTS + R.NEW_LAYOUTS]


def geometries(cases):
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    import tile_map_ref as T
    eng = FilmEngine(TINY, device=-1)
    geos = {}
    for c in cases:
        eng.set_block_overlap(c.overlap)
        geo = eng.tiling(c.H, c.W, c.align, c.block)
        geos[c.name] = geo, T.partitions(c.B * len(geo['origins_y']) * len(geo['origins_x']), len(geo['origins_y']) * len(geo['origins_x']))
    eng.close()
    return geos


def digest(values):
    """16 hex digits over arrays (dtype, shape, bytes) and sets of strings (sorted), in the order given."""
    h = hashlib.sha256()
    for v in values:
        if isinstance(v, (set, frozenset)):
            h.update(('|'.join(sorted(v)) + '\n').encode())
        else:
            a = np.ascontiguousarray(v)
            h.update(f'{a.dtype.str}{a.shape}'.encode() + a.tobytes())
    return h.hexdigest()[:16]


def digests(srcs=None):
    srcs = srcs or sources()
    geos = geometries({c.name: c for s in srcs for c in s.cases}.values())
    out = {}
    for s in srcs:
        f, lay, (sx, sy) = s.fmt, s.layout, s.subsampling
        key = lambda fn, what: f'{s.tag}/{lay}/{fn}/{what}'       # noqa: E731
        item = s.designed(1, 2, 2, 0).dtype.itemsize
        for b, h, w, seed in DESIGNED['even'] + (DESIGNED['odd_h'] if not sy else []) + (DESIGNED['odd_w'] if not sx else []):
            out[key('designed_frames', f'{b}x{h}x{w}@{seed}')] = digest([s.designed(b, h, w, seed)])
        for c in s.cases:
            geo, parts = geos[c.name]
            ranges = [r for name in sorted(parts) for r in parts[name]]      # every range of every partition
            out[key('designed_frames', c.name)] = digest(s.designed(c.B, c.H, c.W, seed) for seed in (4, 5))
            out[key('new_frames_alloc', c.name)] = digest(s.alloc(c, seed) for seed in (0, 1, 17))
            frames = s.designed(c.B, c.H, c.W, 5)
            out[key('yuv_in', c.name)] = digest(f.yuv_in(fr, lay, matrix, full) for matrix, full in s.colours for fr in frames)
            if s.histogram:
                out[key('histogram', c.name)] = digest(s.histogram(fr, lay) for fr in frames)
            view = f.frames_view(s.alloc(c, 1), c)
            out[key('cut', c.name)] = digest(f.cut(view, geo, tile0, nt, lay, matrix, full) for tile0, nt in ranges for matrix, full in s.colours)
            out[key('branches', c.name)] = digest(f.branches(c, geo, lay, tile0, nt) for tile0, nt in ranges)
        for fault in s.faults:
            if fault != 'box_2x2_mean':      # (a fault of the way out: among the yuv_out entries of 4:2:2)
                out[key('cut_fault', fault)] = digest(
                    f.cut(f.frames_view(s.alloc(c, 17), c), geos[c.name][0], tile0, nt, lay, matrix, full, fault)
                    for c in s.cases for tile0, nt in geos[c.name][1]['one'] for matrix, full in (('bt709', True), (s.colours[-1][0], False)))
        for h, w in s.out_sizes:
            rgb = np.random.default_rng(h + w).uniform(-0.2, 1.2, (h, w, 3)).astype(np.float32)      # (values below 0 and above 1 among them)
            faults = (None, 'box_2x2_mean') if 'box_2x2_mean' in s.faults and (sx, sy) == (1, 0) and h % 2 == 0 else (None,)
            out[key('yuv_out', f'{h}x{w}')] = digest(f.yuv_out(rgb, lay, matrix, full, *([ft] if ft else [])) for matrix, full in s.colours for ft in faults)
            out[key('out_branches', f'{h}x{w}')] = digest(f.out_branches(h, w, lay, offset) for offset in (0, item, 32))
    return out


if __name__ == '__main__':
    new = json.dumps(digests(), indent=0, sort_keys=True) + '\n'
    with open(PATH, 'w') as fo:
        fo.write(new)
    print(f'wrote {PATH}: {len(json.loads(new))} entries, {len(new)} bytes')
