"""CPU tests of the frame-sequence entry points (film_interpolate_sequence / film_sequence_plan_json) WITHOUT a GPU.

A sequence plan extracts the features of every frame once and runs the flow estimator and the decoder per pair; its op list is
executed by the numpy interpreter (tests/plan_interp.py, unchanged) against the oracle, its work is compared with the pair plan
of the same pair-tiles, and its buffers, views and two-lane ordering are checked here from the plan JSON.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import oracle_options

SEQ_SHAPES = [(1, 1), (3, 1), (2, 2)]   # (n_pairs, tiles per frame)


def _tiny_engine(weights, fuse=None):
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    eng.set_weights(weights)
    eng.set_option('pack_groups', 4)     # every layout copy, so that the interpreter can check all of them
    if fuse is not None:
        eng.set_option('fuse', fuse)
    return eng


@pytest.mark.parametrize('fuse', [None, 0])
@pytest.mark.parametrize('n_pairs,tiles', SEQ_SHAPES)
def test_sequence_plan_interpreter_matches_oracle(tiny_weights, n_pairs, tiles, fuse):
    """Every pair-tile's output equals the oracle's forward of its two images; the feature taps hold every image once."""
    from film_hip.options import TINY
    from oracle import film_oracle as fo
    import plan_interp as pi
    h, w = 32, 48
    eng = _tiny_engine(tiny_weights, fuse)
    plan = eng.sequence_plan(n_pairs, tiles, h, w)
    assert plan['kind'] == 'sequence' and plan['n_pairs'] == n_pairs and plan['tiles'] == tiles
    P = n_pairs * tiles
    assert plan['B'] == P
    if fuse == 0:
        assert any(op['kind'] == 'flow_up' for op in plan['ops'])
    # image-tiles frame-major: image f * tiles + t; pair-tile p = j * tiles + t reads images p and p + tiles
    rng = np.random.default_rng(100 * n_pairs + tiles)
    images = rng.random(((n_pairs + 1) * tiles, h, w, 3), dtype=np.float32)
    k = images.shape[0] // 2
    arena = pi.run_plan(plan, eng.export_layouts(), images[:k], images[k:])   # (loaded back to back into img0)
    x0, x1 = images[:P], images[tiles:]
    want, aux = fo.film_forward(x0, x1, tiny_weights, oracle_options(TINY), return_aux=True)
    for l in range(TINY.pyramid_levels):
        f = pi.tap(plan, arena, f'feat{l}')
        assert f.shape[0] == (n_pairs + 1) * tiles
        assert np.abs(f[:P] - aux['feature_pyramids'][0][l]).max() < 1e-5
        assert np.abs(f[tiles:] - aux['feature_pyramids'][1][l]).max() < 1e-5
        r = pi.tap(plan, arena, f'res{l}')
        assert np.abs(r[:P] - aux['forward_residual_flow_pyramid'][l]).max() < 1e-5
        assert np.abs(r[P:] - aux['backward_residual_flow_pyramid'][l]).max() < 1e-5
    out = pi.tap(plan, arena, 'out')
    assert out.shape[0] == P
    assert np.abs(out - want).max() < 1e-5
    eng.close()


def _family(op):
    """What decides a convolution's summation order: kernel family, split-K, fold form, fused epilogues, and its tile set."""
    return (op['c3'], op['wino'], op['halo'], op['split'], op['fold'], op['ksplit'], op['tile'] >> 5, op['Cout'], op['Ctot'],
            op['H'], op['W'], bool(op['out2']['buf']), bool(op['pw_out']['buf']), op['w_off'])


def _layer_tag(tag):
    return re.sub(r':d[01]', '', tag)


@pytest.mark.parametrize('opt_name,n_pairs,tiles,h,w', [('TINY', 3, 1, 32, 48), ('TINY', 2, 2, 64, 96),
                                                       ('PUBLISHED', 3, 1, 256, 256), ('PUBLISHED', 2, 2, 576, 960)])
def test_sequence_plan_work_and_kernel_families(opt_name, n_pairs, tiles, h, w):
    """The extractor (feat_*) runs on (n_pairs + 1) * tiles images - (n_pairs + 1) / (2 n_pairs) of the pair plan's work for the same
    pair-tiles - and every convolution runs the kernel family, split-K factor and tile set of the same layer and level in the pair plan."""
    from film_hip import options
    from film_hip.engine import FilmEngine
    opt = getattr(options, opt_name)
    eng = FilmEngine(opt, device=-1)
    P = n_pairs * tiles
    seq = eng.sequence_plan(n_pairs, tiles, h, w)
    pair = eng.plan(P, h, w)
    sf = [op for op in seq['ops'] if op['tag'].startswith('feat_')]
    pf = [op for op in pair['ops'] if op['tag'].startswith('feat_')]
    assert sf and [op['tag'] for op in sf] == [op['tag'] for op in pf]
    assert all(op['NB'] == (n_pairs + 1) * tiles for op in sf)
    assert all(op['NB'] == 2 * P for op in pf)
    s_fl, p_fl = sum(op['flops'] for op in sf), sum(op['flops'] for op in pf)
    assert s_fl == pytest.approx(p_fl * (n_pairs + 1) / (2 * n_pairs), rel=1e-5)   # (the JSON prints 6 significant digits)
    pair_conv = {}
    for op in pair['ops']:
        if op['kind'] == 'conv_mfma':
            pair_conv.setdefault(op['tag'], _family(op))
    n_conv = 0
    for op in seq['ops']:
        if op['kind'] != 'conv_mfma':
            continue
        n_conv += 1
        tag = _layer_tag(op['tag'])
        assert tag in pair_conv, op['tag']
        assert _family(op) == pair_conv[tag], op['tag']
    assert n_conv == sum(1 for op in pair['ops'] if op['kind'] == 'conv_mfma') + opt.pyramid_levels   # conv_0 of every flow level: per direction
    # the fused misc16 warp of the pair plan is not used (image 1 is not at +B): the unfused warp_img + pack_flow form
    assert not any(op['img_out']['buf'] for op in seq['ops'])
    assert sum(op['kind'] == 'pack_flow' for op in seq['ops']) == opt.fusion_pyramid_levels
    assert not any(op['src_brot'] or op['flow_brot'] or op['misc_nb'] for op in seq['ops'])
    assert not any(sg['bmod'] for op in seq['ops'] for sg in op.get('segs', []))
    eng.close()


def _view_pixels(op):
    """{view key: pixels the kernel touches through that view} (the semantics of tests/plan_interp.py)."""
    k, nb, h, w = op['kind'], op['NB'], op['H'], op['W']
    out = {}
    if k == 'conv_mfma':
        for i, sg in enumerate(op['segs']):
            hs, ws = (h // 2, w // 2) if sg['up'] else (h, w)
            out[f'seg{i}'] = (sg['bmod'] or nb) * hs * ws
        oh, ow = (2 * h, 2 * w) if op['fold'] else (h, w)
        out['out'] = nb * oh * ow
        out['out2'] = nb * (h // 2) * (w // 2)
        out['pw_out'] = nb * h * w
    elif k in ('flow_head', 'conv_pw', 'pack_flow'):
        for key in ('in', 'in2', 'out', 'out2'):
            out[key] = op['n']
    elif k == 'flow_add':
        for key in ('in', 'in2', 'out'):
            out[key] = op['n'] // 2
    elif k == 'pool':
        out['in'], out['out'] = nb * h * w, nb * (h // 2) * (w // 2)
    elif k == 'flow_up':
        out['in'], out['out'] = nb * h * w, nb * 4 * h * w
    elif k == 'warp':
        for key in ('in', 'in2', 'out', 'out2'):
            out[key] = nb * h * w
        out['in3'] = nb * (h // 2) * (w // 2)
        mb = op['misc_nb'] or nb
        out['img_in'] = 2 * mb
        for key in ('img_out', 'pack_b', 'pack_f'):
            out[key] = mb * h * w
    return out


def _check_bounds(plan):
    bufs = {b['name']: b for b in plan['buffers']}
    for b in plan['buffers']:
        assert 0 <= b['off'] and b['off'] + b['floats'] <= plan['arena_floats'], b['name']
    checked = 0
    for op in plan['ops']:
        for key, px in _view_pixels(op).items():
            v = op['segs'][int(key[3:])]['v'] if key.startswith('seg') else op.get(key)
            if not v or not v.get('buf') or px <= 0:
                continue
            b = bufs[v['buf']]
            end = v['off'] + (px - 1) * v['stride'] + v['C']
            assert b['off'] <= v['off'] and end <= b['off'] + b['floats'], (op['tag'], key, v, b)
            checked += 1
    return checked


def _check_lanes(plan):
    """Every two ops on different lanes that touch overlapping channels of one buffer (RAW / WAR / WAW) are ordered through the
    xdeps edges and per-lane program order (the check of test_plan_cpu.py::test_lane_analysis_orders_every_conflict)."""
    bufs = {b['name']: b for b in plan['buffers']}
    ops = plan['ops']

    def acc(v):
        if v is None or not v.get('buf'):
            return None
        b = bufs[v['buf']]
        if b['C'] == 0 or v['stride'] != b['C']:
            return (v['buf'], 0, 1 << 30)
        c0 = (v['off'] - b['off']) % b['C']
        return (v['buf'], c0, c0 + v['C'])

    def rw(op):
        rd = [acc(sg['v']) for sg in op.get('segs', [])] if op['kind'] == 'conv_mfma' else [acc(op.get('in')), acc(op.get('in2'))]
        rd += [acc(op.get('in3')), acc(op.get('img_in')), acc(op.get('pack_b')), acc(op.get('pack_f'))]
        wr = [acc(op.get('out')) if not (op.get('pw_out') or {}).get('buf') else None, acc(op.get('pw_out')), acc(op.get('out2')),
              acc(op.get('img_out'))]
        return [a for a in rd if a], [a for a in wr if a]

    def hit(a, b):
        return a[0] == b[0] and a[1] < b[2] and b[1] < a[2]

    n = len(ops)
    assert {o['lane'] for o in ops} == {0, 1}
    before = [set() for _ in range(n)]
    last = {0: None, 1: None}
    for j, o in enumerate(ops):
        preds = list(o['xdeps'])
        if last[o['lane']] is not None:
            preds.append(last[o['lane']])
        for p in preds:
            assert p < j
            before[j] |= before[p] | {p}
        last[o['lane']] = j
    acc_rw = [rw(o) for o in ops]
    conflicts = 0
    for j in range(n):
        rj, wj = acc_rw[j]
        for i in range(j):
            if ops[i]['lane'] == ops[j]['lane']:
                continue
            ri, wi = acc_rw[i]
            if any(hit(a, b) for a in wi for b in rj + wj) or any(hit(a, b) for a in ri for b in wj):
                conflicts += 1
                assert i in before[j], (ops[i]['tag'], ops[j]['tag'])
    return conflicts


@pytest.mark.parametrize('opt_name,n_pairs,tiles,h,w,lanes', [('TINY', 3, 1, 64, 96, 1), ('TINY', 2, 2, 32, 48, 1),
                                                             ('PUBLISHED', 3, 1, 128, 192, 1), ('PUBLISHED', 2, 2, 576, 960, 1),
                                                             ('PUBLISHED', 2, 2, 576, 960, 2)])
def test_sequence_plan_integrity(opt_name, n_pairs, tiles, h, w, lanes):
    """Every buffer lies inside the arena, every view of every op inside its buffer, and every two-lane conflict is ordered."""
    from film_hip import options
    from film_hip.engine import FilmEngine
    eng = FilmEngine(getattr(options, opt_name), device=-1)
    eng.set_option('lanes', lanes)
    plan = eng.sequence_plan(n_pairs, tiles, h, w)
    img0 = next(b for b in plan['buffers'] if b['name'] == 'img0')
    assert img0['N'] == (n_pairs + 1) * tiles
    assert _check_bounds(plan) > 100
    assert _check_lanes(plan) > 0
    # the per-direction ops reach the other image by an offset of `tiles` images into the feature buffers
    feat = {b['name']: b for b in plan['buffers'] if b['name'].startswith('feat')}
    offs = {(op['tag'], sg['v']['off'] - feat[sg['v']['buf']]['off']) for op in plan['ops'] if op['kind'] == 'conv_mfma'
            for sg in op['segs'] if sg['v']['buf'] in feat and ':d' in op['tag']}
    assert any(o > 0 for _, o in offs)
    # offset32_buffer_bytes bounds what every 32-bit-addressed kernel sees from the start of its view
    assert plan['offset32_buffer_bytes'] < 0xFFF00000
    eng.close()


def test_pair_plan_checks_hold_too(tiny_weights):
    """The bounds checker above accepts the pair plans it was written after (guards the checker itself)."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    assert _check_bounds(eng.plan(2, 32, 48)) > 100
    eng.close()


def test_sequence_plan_cache_is_separate_from_pair_plans():
    """A sequence plan never stands in for the pair plan of the same B (and back): both kinds describe themselves after each other."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    a = eng.plan(2, 32, 48)
    s = eng.sequence_plan(2, 1, 32, 48)
    b = eng.plan(2, 32, 48)
    s2 = eng.sequence_plan(1, 2, 32, 48)
    assert a == b and 'kind' not in a
    assert s['kind'] == 'sequence' and s['B'] == 2 and s['tiles'] == 1
    assert s2['tiles'] == 2 and s2['n_pairs'] == 1
    assert next(x for x in s['buffers'] if x['name'] == 'img0')['N'] == 3
    assert next(x for x in s2['buffers'] if x['name'] == 'img0')['N'] == 4
    assert next(x for x in a['buffers'] if x['name'] == 'img0')['N'] == 4
    eng.close()


def test_sequence_argument_handling(tiny_weights):
    """F < 2, NULL pointers, bad block shapes: FILM_ERR_INVALID with the reference's messages; valid arguments on a plan-only
    handle: FILM_ERR_NO_DEVICE (no CPU fallback)."""
    from film_hip.engine import FilmError, FILM_ERR_INVALID, FILM_ERR_NO_DEVICE
    eng = _tiny_engine(tiny_weights)
    lib, hnd = eng._lib, eng._h
    frames = np.zeros((3, 32, 48, 3), np.float32)
    out = np.zeros((2, 32, 48, 3), np.float32)

    def call(fr, f, h, w, bh, bw, o, mem=0):
        return lib.film_interpolate_sequence(hnd, fr, f, h, w, 0, bh, bw, o, mem, None)

    fp, op = frames.ctypes.data, out.ctypes.data
    for f in (1, 0, -1):
        assert call(fp, f, 32, 48, 1, 1, op) == FILM_ERR_INVALID
        assert 'at least 2 frames' in lib.film_last_error(hnd).decode()
    assert call(None, 3, 32, 48, 1, 1, op) == FILM_ERR_INVALID
    assert lib.film_last_error(hnd).decode() == 'NULL argument'
    assert call(fp, 3, 32, 48, 1, 1, None) == FILM_ERR_INVALID
    assert call(fp, 3, 32, 48, 3, 1, op) == FILM_ERR_INVALID
    assert lib.film_last_error(hnd).decode() == 'block_height=3 should evenly divide height=32.'
    assert call(fp, 3, 32, 48, 1, 5, op) == FILM_ERR_INVALID
    assert lib.film_last_error(hnd).decode() == 'block_width=5 should evenly divide width=48.'
    assert call(fp, 3, 32, 48, 1, 1, op, mem=7) == FILM_ERR_INVALID
    assert call(fp, 3, 32, 48, 2, 2, op) == FILM_ERR_NO_DEVICE
    assert lib.film_interpolate_sequence(None, fp, 3, 32, 48, 0, 1, 1, op, 0, None) == FILM_ERR_INVALID
    # the Python layer
    with pytest.raises(FilmError) as e:
        eng.interpolate_sequence(frames[:1])
    assert e.value.code == FILM_ERR_INVALID
    with pytest.raises(FilmError) as e:
        eng.interpolate_sequence(frames, block_shape=(3, 1))
    assert e.value.code == FILM_ERR_INVALID and 'block_height=3 should evenly divide height=32.' in str(e.value)
    with pytest.raises(FilmError) as e:
        eng.interpolate_sequence(frames)
    assert e.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        eng.interpolate_sequence(frames[..., :2])
    # the plan description
    need = ctypes.c_int64()
    assert lib.film_sequence_plan_json(hnd, 0, 1, 32, 48, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert lib.film_sequence_plan_json(hnd, 1, 0, 32, 48, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert lib.film_sequence_plan_json(hnd, 1, 1, 30, 48, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID   # not divisible by 8
    eng.close()


def test_sequence_window_flag_parses():
    """--sequence_window: default 0 (today's path), K >= 2 windows; 1 or negative is refused."""
    from eval import interpolator_cli as cli
    assert cli.build_parser().parse_args(['--pattern', 'x']).sequence_window == 0
    assert cli.build_parser().parse_args(['--pattern', 'x', '--sequence_window', '5']).sequence_window == 5
    with pytest.raises(SystemExit):
        cli.main(['--pattern', '/nonexistent/*', '--sequence_window', '1'])
