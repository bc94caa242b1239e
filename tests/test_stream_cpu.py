"""CPU tests of the frame streams (film_stream_* / film_stream_plan_json) WITHOUT a GPU.

A stream plan is the plan of one pair of `tiles` tiles over two frame slots that take turns: the pushed frame's image pyramid and
features are computed into half `slot`, the other half still holds what the push before left there.  Its two orientations are
described by the plan JSON; here they are compared with each other and with the pair plan, checked for bounds and lane ordering,
and executed by the numpy interpreter (tests/plan_interp.py, unchanged) over ONE persistent arena, frame after frame.
"""
import ctypes

import numpy as np
import pytest

from conftest import oracle_options
from test_sequence_cpu import _check_bounds, _check_lanes, _family, _layer_tag, _tiny_engine, _view_pixels

H, W = 32, 48
WRITE_KEYS = ('out', 'out2', 'pw_out', 'img_out')


def _per_image(name):
    return name.startswith('feat') or name.startswith('img')


def _writes(op):
    """[(view, pixels)] of everything the op writes (a conv with a fused 1x1 head does not write `out`)."""
    px = _view_pixels(op)
    res = []
    for key in WRITE_KEYS:
        v = op.get(key)
        if not v or not v.get('buf') or px.get(key, 0) <= 0:
            continue
        if key == 'out' and (op.get('pw_out') or {}).get('buf'):
            continue
        res.append((v, px[key]))
    return res


@pytest.mark.parametrize('tiles', [1, 2])
def test_stream_orientations_agree(tiny_weights, tiles):
    """Both orientations list identical buffers; the first n_extract ops run on `tiles` images and write only into the `slot` half of
    their buffers; nothing behind them writes a feature or image-pyramid buffer."""
    eng = _tiny_engine(tiny_weights)
    plans = [eng.stream_plan(tiles, H, W, s) for s in (0, 1)]
    assert plans[0]['buffers'] == plans[1]['buffers']
    assert plans[0]['arena_floats'] == plans[1]['arena_floats'] and plans[0]['n_extract'] == plans[1]['n_extract']
    assert [op['tag'] for op in plans[0]['ops']] == [op['tag'] for op in plans[1]['ops']]
    for s, plan in enumerate(plans):
        assert plan['kind'] == 'stream' and plan['tiles'] == tiles and plan['slot'] == s and plan['B'] == tiles
        bufs = {b['name']: b for b in plan['buffers']}
        assert bufs['img0']['N'] == 2 * tiles and bufs['feat0']['N'] == 2 * tiles
        ne = plan['n_extract']
        assert 0 < ne < len(plan['ops'])
        checked = 0
        for op in plan['ops'][:ne]:
            assert op['NB'] == tiles, op['tag']
            assert op['tag'].startswith(('image_pyramid', 'feat_')), op['tag']
            for v, px in _writes(op):
                b = bufs[v['buf']]
                half = b['floats'] // 2
                lo = b['off'] + s * half
                end = v['off'] + (px - 1) * v['stride'] + v['C']
                assert lo <= v['off'] and end <= lo + half, (op['tag'], v, b, s)
                checked += 1
        assert checked >= ne
        assert not any(op['tag'].startswith(('image_pyramid', 'feat_')) for op in plan['ops'][ne:])
        for op in plan['ops'][ne:]:
            for v, _ in _writes(op):
                assert not _per_image(v['buf']), (op['tag'], v['buf'])
    eng.close()


@pytest.mark.parametrize('fuse', [None, 0])
@pytest.mark.parametrize('tiles', [1, 2])
def test_stream_carry_in_the_interpreter(tiny_weights, tiles, fuse):
    """Frames A, B, C, D through one persistent arena: A runs the first n_extract ops only, every later frame the whole list of the
    alternating orientation.  out == the oracle's forward of (previous, current) within the bound test_sequence_cpu.py uses for the
    same interpreter, and the half of every feat* buffer a push does not fill keeps its bits."""
    from film_hip.options import TINY
    from oracle import film_oracle as fo
    import plan_interp as pi
    eng = _tiny_engine(tiny_weights, fuse)
    plans = [eng.stream_plan(tiles, H, W, s) for s in (0, 1)]
    packed = eng.export_layouts()
    key = pi.blob_key(packed)
    bufs = {b['name']: b for b in plans[0]['buffers']}
    arena = np.zeros(plans[0]['arena_floats'], np.float32)
    rng = np.random.default_rng(7 + tiles)
    frames = [rng.random((tiles, H, W, 3), dtype=np.float32) for _ in range(4)]
    feats = [b for b in plans[0]['buffers'] if b['name'].startswith('feat')]
    slot = 0
    for i, fr in enumerate(frames):
        plan = plans[slot]
        img0 = bufs['img0']
        arena[img0['off'] + slot * fr.size:img0['off'] + (slot + 1) * fr.size] = fr.ravel()
        before = {b['name']: arena[b['off']:b['off'] + b['floats']].reshape(2, -1)[1 - slot].copy() for b in feats}
        ops = plan['ops'][:plan['n_extract']] if i == 0 else plan['ops']
        for op in ops:
            pi.run_op(op, arena, packed, bufs, verify_key=key)
        for b in feats:
            assert np.array_equal(arena[b['off']:b['off'] + b['floats']].reshape(2, -1)[1 - slot], before[b['name']]), b['name']
        if i > 0:
            want = fo.film_forward(frames[i - 1], fr, tiny_weights, oracle_options(TINY))
            out = pi.tap(plan, arena, 'out')
            assert out.shape == want.shape
            assert np.abs(out - want).max() < 1e-5, i
        slot = 1 - slot
    eng.close()


@pytest.mark.parametrize('opt_name,tiles,h,w', [('TINY', 1, 32, 48), ('TINY', 2, 32, 48), ('PUBLISHED', 1, 256, 256),
                                                ('PUBLISHED', 4, 576, 960)])
def test_stream_plan_work_and_kernel_families(opt_name, tiles, h, w):
    """A push extracts ONE frame - half the pair plan's feat_* work for the same tiles - and every convolution runs the kernel family,
    split-K factor, tile set and weights of the same layer and level in the pair plan."""
    from film_hip import options
    from film_hip.engine import FilmEngine
    opt = getattr(options, opt_name)
    eng = FilmEngine(opt, device=-1)
    pair = eng.plan(tiles, h, w)
    pf = [op for op in pair['ops'] if op['tag'].startswith('feat_')]
    pair_conv = {}
    for op in pair['ops']:
        if op['kind'] == 'conv_mfma':
            pair_conv.setdefault(op['tag'], _family(op))
    for slot in (0, 1):
        st = eng.stream_plan(tiles, h, w, slot)
        sf = [op for op in st['ops'] if op['tag'].startswith('feat_')]
        assert sf and [op['tag'] for op in sf] == [op['tag'] for op in pf]
        assert all(op['NB'] == tiles for op in sf) and all(op['NB'] == 2 * tiles for op in pf)
        assert sum(op['flops'] for op in sf) == pytest.approx(sum(op['flops'] for op in pf) / 2, rel=1e-5)
        n_conv = 0
        for op in st['ops']:
            if op['kind'] != 'conv_mfma':
                continue
            n_conv += 1
            tag = _layer_tag(op['tag'])
            assert tag in pair_conv, op['tag']
            assert _family(op) == pair_conv[tag], op['tag']
        assert n_conv == sum(1 for op in pair['ops'] if op['kind'] == 'conv_mfma') + opt.pyramid_levels
    eng.close()


@pytest.mark.parametrize('opt_name,tiles,h,w,lanes', [('TINY', 1, 32, 48, 1), ('TINY', 2, 64, 96, 1), ('PUBLISHED', 1, 128, 192, 1),
                                                      ('PUBLISHED', 4, 576, 960, 1), ('PUBLISHED', 4, 576, 960, 2)])
def test_stream_plan_integrity(opt_name, tiles, h, w, lanes):
    """Per orientation: buffers inside the arena, views inside their buffers, every two-lane conflict ordered, 32-bit offsets in range."""
    from film_hip import options
    from film_hip.engine import FilmEngine
    eng = FilmEngine(getattr(options, opt_name), device=-1)
    eng.set_option('lanes', lanes)
    for slot in (0, 1):
        plan = eng.stream_plan(tiles, h, w, slot)
        assert _check_bounds(plan) > 100
        assert _check_lanes(plan) > 0
        assert plan['offset32_buffer_bytes'] < 0xFFF00000
        # image 0 of the pair (the earlier frame) is read at (1 - slot) * tiles images into the feature buffers
        feat = {b['name']: b for b in plan['buffers'] if b['name'].startswith('feat')}
        for op in plan['ops']:
            if op['kind'] == 'conv_mfma' and op['tag'].endswith('conv_0') and ':d0:' in op['tag']:
                b = feat[op['segs'][0]['v']['buf']]
                assert op['segs'][0]['v']['off'] - b['off'] == (1 - slot) * (b['floats'] // 2), op['tag']
    eng.close()


def test_stream_plan_cache_is_separate():
    """A stream plan, the pair plan of B = tiles and the sequence plan (1, tiles) each describe themselves, in any order of asking."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    asked = {'pair': lambda: eng.plan(2, H, W), 'seq': lambda: eng.sequence_plan(1, 2, H, W),
             'st0': lambda: eng.stream_plan(2, H, W, 0), 'st1': lambda: eng.stream_plan(2, H, W, 1)}
    first = {}
    for order in (('st0', 'pair', 'seq', 'st1'), ('seq', 'st1', 'pair', 'st0'), ('pair', 'st0', 'st1', 'seq')):
        for k in order:
            got = asked[k]()
            assert first.setdefault(k, got) == got
    assert 'kind' not in first['pair'] and first['seq']['kind'] == 'sequence' and first['st0']['kind'] == 'stream'
    assert (first['st0']['slot'], first['st1']['slot']) == (0, 1)
    assert 'n_extract' not in first['seq'] and 'slot' not in first['seq']
    assert first['st0']['ops'] != first['st1']['ops'] and first['st1']['ops'] != first['seq']['ops']
    for k in ('pair', 'seq', 'st0'):
        assert next(b for b in first[k]['buffers'] if b['name'] == 'img0')['N'] == 4
    eng.close()


def test_stream_argument_handling(tiny_weights):
    """NULL handle, calls without an open stream, bad pix / slot, the reference's block messages, overlap beyond half a patch;
    valid arguments on a plan-only handle: FILM_ERR_NO_DEVICE (no CPU fallback).  (A second open, a bad mem_kind on an open stream:
    tests/test_stream_gpu.py - a plan-only handle cannot open one.)"""
    from film_hip.engine import FilmError, FILM_ERR_INVALID, FILM_ERR_NO_DEVICE, FILM_ERR_STATE
    eng = _tiny_engine(tiny_weights)
    lib, hnd = eng._lib, eng._h
    err = lambda: lib.film_last_error(hnd).decode()   # noqa: E731
    frame = np.zeros((H, W, 3), np.float32)
    produced = ctypes.c_int(5)
    need = ctypes.c_int64()
    assert lib.film_stream_open(None, H, W, 0, 1, 1, 0) == FILM_ERR_INVALID
    assert lib.film_stream_push(None, frame.ctypes.data, frame.ctypes.data, ctypes.byref(produced), 0, None) == FILM_ERR_INVALID
    assert lib.film_stream_reset(None) == FILM_ERR_INVALID and lib.film_stream_close(None) == FILM_ERR_INVALID
    assert lib.film_stream_plan_json(None, 1, H, W, 0, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert lib.film_stream_push(hnd, frame.ctypes.data, frame.ctypes.data, ctypes.byref(produced), 0, None) == FILM_ERR_STATE
    assert 'no open stream' in err()
    assert lib.film_stream_push(hnd, frame.ctypes.data, frame.ctypes.data, ctypes.byref(produced), 7, None) == FILM_ERR_STATE
    assert lib.film_stream_reset(hnd) == FILM_ERR_STATE and lib.film_stream_close(hnd) == FILM_ERR_STATE
    for pix in (-1, 2):
        assert lib.film_stream_open(hnd, H, W, 0, 1, 1, pix) == FILM_ERR_INVALID
        assert 'pix' in err()
    assert lib.film_stream_open(hnd, 0, W, 0, 1, 1, 0) == FILM_ERR_INVALID
    assert lib.film_stream_open(hnd, H, W, 0, 3, 1, 0) == FILM_ERR_INVALID
    assert err() == 'block_height=3 should evenly divide height=32.'
    assert lib.film_stream_open(hnd, H, W, 0, 1, 5, 1) == FILM_ERR_INVALID
    assert err() == 'block_width=5 should evenly divide width=48.'
    eng.set_option('block_overlap_h', 9)     # patch height 16: 2 * 9 > 16
    assert lib.film_stream_open(hnd, H, W, 0, 2, 2, 0) == FILM_ERR_INVALID
    assert 'block_overlap_h' in err() and 'must not exceed the patch size 16' in err()
    eng.set_option('block_overlap_h', 0)
    assert lib.film_stream_open(hnd, H, W, 0, 2, 2, 0) == FILM_ERR_NO_DEVICE
    assert lib.film_stream_open(hnd, H, W, 0, 1, 1, 1) == FILM_ERR_NO_DEVICE
    # the plan description
    for slot in (-1, 2):
        assert lib.film_stream_plan_json(hnd, 1, H, W, slot, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
        assert 'slot must be 0 or 1' in err()
    assert lib.film_stream_plan_json(hnd, 0, H, W, 0, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID
    assert lib.film_stream_plan_json(hnd, 1, 30, W, 0, None, 0, ctypes.byref(need)) == FILM_ERR_INVALID   # not divisible by 8
    # the Python layer
    with pytest.raises(FilmError) as e:
        eng.open_stream(H, W)
    assert e.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(FilmError) as e:
        eng.open_stream(H, W, block_shape=(3, 1))
    assert e.value.code == FILM_ERR_INVALID and 'block_height=3 should evenly divide height=32.' in str(e.value)
    with pytest.raises(ValueError):
        eng.open_stream(H, W, pix='u16')
    # before film_finalize: FILM_ERR_STATE on a handle with a device is covered on the GPU; plan-only reports the missing device first
    eng.close()


def test_stream_flag_parses():
    """--stream: off by default; refused with any times_to_interpolate but 1 and together with --sequence_window."""
    from eval import interpolator_cli as cli
    assert cli.build_parser().parse_args(['--pattern', 'x']).stream is False
    assert cli.build_parser().parse_args(['--pattern', 'x', '--stream', '--times_to_interpolate', '1']).stream is True
    with pytest.raises(SystemExit) as e:
        cli.main(['--pattern', '/nonexistent/*', '--stream', '--times_to_interpolate', '2'])
    assert 'times_to_interpolate 1' in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(['--pattern', '/nonexistent/*', '--stream', '--times_to_interpolate', '1', '--sequence_window', '4'])
    assert 'sequence_window' in str(e.value)
