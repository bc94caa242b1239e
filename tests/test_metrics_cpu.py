"""Evaluation metrics on the GPU (film_image_metrics, eval/device_metrics.py) and the batched eval loop (eval/eval_cli.py): the parts
that need no GPU - the C-ABI declaration, argument checks on a plan-only handle, the composition of per-image sums into the values
of eval/metrics.py, and run_evaluation's batching / decoding pipeline with a stand-in interpolator."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ['l1', 'l2', 'ssim', 'psnr']


def test_entry_point_is_declared_and_exported():
    from film_hip import engine
    header = open(os.path.join(ROOT, 'include', 'film_hip.h')).read()
    assert re.search(r'^int film_image_metrics\(film_t\* h, const float\* pred, const float\* ref, int B, int H, int W, int C, '
                     r'int flags, double max_val,\s+double\* out, int mem_kind, void\* stream\);', header, re.M)
    for name, value in (('L1', 1), ('L2', 2), ('PSNR', 4), ('SSIM', 8), ('CLIP', 16)):
        assert re.search(rf'^#define FILM_METRIC_{name} {value}\b', header, re.M), name
        assert getattr(engine, f'FILM_METRIC_{name}') == value
    mapfile = open(os.path.join(ROOT, 'frame-interpolation_amd', 'csrc', 'film_hip.map')).read()
    assert re.search(r'\bfilm_image_metrics;', mapfile)
    assert 'film_image_metrics' in engine.EXPORTED_SYMBOLS
    assert engine.load_library().film_image_metrics is not None


def _per_image_sums(pred, ref, clip):
    """What film_image_metrics returns per image, computed with eval/metrics.py."""
    from eval import metrics as M
    if clip:
        pred = np.clip(pred, 0.0, 1.0)
    rows = []
    for k in range(pred.shape[0]):
        p, r = pred[k:k + 1], ref[k:k + 1]
        n = p.size
        rows.append([M.l1(p, r) * n, M.l2(p, r) * n, M.psnr(p, r), M.ssim(p, r)])
    return np.array(rows, np.float64)


@pytest.mark.parametrize('b,h,w,c', [(1, 11, 11, 3), (3, 13, 17, 1), (4, 20, 24, 3), (2, 33, 12, 1)])
def test_compose_reproduces_the_numpy_metrics(b, h, w, c):
    from eval import device_metrics as DM, metrics as M
    rng = np.random.default_rng(b * 100 + h)
    pred = rng.uniform(-0.2, 1.2, (b, h, w, c)).astype(np.float32)
    ref = rng.random((b, h, w, c), dtype=np.float32)
    for clip in (False, True):
        per = _per_image_sums(pred, ref, clip)
        got = DM.compose(per, h * w * c, ALL)
        p = np.clip(pred, 0.0, 1.0) if clip else pred
        want = [M.l1(p, ref), M.l2(p, ref), M.ssim(p, ref), M.psnr(p, ref)]
        assert got[0] == pytest.approx(want[0], rel=1e-12) and got[1] == pytest.approx(want[1], rel=1e-12)
        assert got[2] == pytest.approx(want[2], abs=1e-12) and got[3] == pytest.approx(want[3], abs=1e-10)
        # one image: the row of the eval loop
        assert DM.compose(per[1 % b:1 % b + 1], h * w * c, ['psnr', 'l1']) == pytest.approx(
            [M.psnr(p[1 % b:1 % b + 1], ref[1 % b:1 % b + 1]), M.l1(p[1 % b:1 % b + 1], ref[1 % b:1 % b + 1])], rel=1e-12)


def test_compose_of_identical_images():
    from eval import device_metrics as DM
    got = DM.compose(np.array([[0.0, 0.0, np.inf, 1.0]] * 2), 12, ALL)
    assert got[:2] == [0.0, 0.0] and got[2] == 1.0 and np.isinf(got[3])


def test_device_metric_set_names_and_refusals():
    from eval import device_metrics as DM
    assert DM.DeviceMetricSet(None, ['psnr', 'l1']).names == ['psnr', 'l1']
    for bad in (['vgg'], ['l1', 'style']):
        with pytest.raises(ValueError, match='Invalid loss name'):
            DM.DeviceMetricSet(None, bad)


def test_argument_errors_come_before_the_device_check(tiny_plan_engine):
    """Every refusal of include/film_hip.h is FILM_ERR_INVALID with a message; a valid call on a plan-only handle is FILM_ERR_NO_DEVICE."""
    from film_hip.engine import FILM_ERR_INVALID, FILM_ERR_NO_DEVICE, FILM_MEM_HOST, FilmError
    eng = tiny_plan_engine
    lib, h = eng._lib, eng._h
    a = np.zeros((2, 16, 16, 3), np.float32)
    out = np.zeros((2, 4), np.float64)
    p, o = a.ctypes.data, out.ctypes.data

    def call(pred=p, ref=p, b=2, hh=16, ww=16, c=3, flags=15, max_val=1.0, dst=o, mem=FILM_MEM_HOST):
        return lib.film_image_metrics(h, pred, ref, b, hh, ww, c, flags, max_val, dst, mem, None)
    cases = [dict(b=0), dict(b=-1), dict(c=2), dict(c=4), dict(pred=None), dict(ref=None), dict(dst=None), dict(max_val=0.0),
             dict(max_val=-1.0), dict(max_val=float('nan')), dict(hh=10), dict(ww=10), dict(flags=32), dict(mem=7), dict(hh=0)]
    for kw in cases:
        assert call(**kw) == FILM_ERR_INVALID, kw
        assert lib.film_last_error(h), kw
    assert call(hh=10, ww=10, flags=7) == FILM_ERR_NO_DEVICE        # < 11 x 11 is fine without ssim
    assert lib.film_image_metrics(None, p, p, 2, 16, 16, 3, 15, 1.0, o, FILM_MEM_HOST, None) == FILM_ERR_INVALID
    with pytest.raises(FilmError) as ei:
        eng.image_metrics(a, a)
    assert ei.value.code == FILM_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        eng.image_metrics(a, a, names=['vgg'])


@pytest.fixture
def tiny_plan_engine():
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    eng = FilmEngine(TINY, device=-1)
    yield eng
    eng.close()


def _triplet_tree(root, sizes, seed=3):
    from eval import util
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(sizes):
        d = root / f'seq{i:02d}'
        os.makedirs(d)
        for j in (1, 2, 3):
            util.write_image(str(d / f'im{j}.png'), rng.random((h, w, 3), dtype=np.float32))


class _Blend:
    """Stand-in interpolator: the average of the inputs, out of range to exercise the clip; records the batch of every call."""
    def __init__(self):
        self.calls = []

    def __call__(self, x0, x1, dt):
        assert x0.shape == x1.shape and dt.shape == (x0.shape[0],)
        self.calls.append(x0.shape)
        return 0.5 * (x0 + x1) + 0.3


def test_batched_loop_writes_the_same_results(tmp_path):
    from eval import eval_cli
    sizes = [(16, 20)] * 4 + [(24, 16)] * 2 + [(16, 20)] + [(12, 14)] * 3
    _triplet_tree(tmp_path / 'data', sizes)
    trip = eval_cli.find_triplets(str(tmp_path / 'data'))
    assert len(trip) == len(sizes)
    files = {}
    for name, kw in (('b1', dict()), ('b3', dict(batch_size=3)), ('b3_serial', dict(batch_size=3, io_workers=0)),
                     ('b8_max', dict(batch_size=8, max_examples=5))):
        blend = _Blend()
        out = tmp_path / name
        totals = eval_cli.run_evaluation(blend, trip, str(out), metrics=ALL, output_frames=name == 'b3', **kw)
        files[name] = open(out / 'results.csv', 'rb').read()
        assert set(totals) == set(ALL)
        if name == 'b1':
            assert [s[0] for s in blend.calls] == [1] * len(sizes)
        elif name.startswith('b3'):
            # same-size runs of 4, 2, 1, 3 triplets in at most 3 per call
            assert blend.calls == [(3, 16, 20, 3), (1, 16, 20, 3), (2, 24, 16, 3), (1, 16, 20, 3), (3, 12, 14, 3)]
        else:
            assert blend.calls == [(4, 16, 20, 3), (1, 24, 16, 3)]
    assert files['b3'] == files['b1'] == files['b3_serial']
    lines = files['b8_max'].decode().strip().split('\n')
    assert lines[1:6] == files['b1'].decode().split('\n')[1:6] and lines[6].startswith('mean, ')
    assert os.path.isfile(tmp_path / 'b3' / 'seq09_image.png')


def test_default_loop_matches_the_reference_loop(tmp_path):
    """Defaults: results.csv byte-identical to the loop before batching (one triplet per call, metrics on image and y[None])."""
    from eval import eval_cli, metrics as M, util
    _triplet_tree(tmp_path / 'data', [(16, 20), (20, 16), (16, 20)], seed=5)
    trip = eval_cli.find_triplets(str(tmp_path / 'data'))
    blend = _Blend()
    eval_cli.run_evaluation(blend, trip, str(tmp_path / 'out'), metrics=['psnr', 'l1'])
    fns = M.test_losses(['psnr', 'l1'])
    want = ['key, psnr, l1']
    losses = {n: [] for n, _ in fns}
    for key, (f0, fy, f1) in trip:
        x0, y, x1 = util.read_image(f0), util.read_image(fy), util.read_image(f1)
        image = np.clip(_Blend()(x0[None], x1[None], np.full((1,), 0.5, np.float32)), 0.0, 1.0)
        values = [fn(image, y[None]) for _n, fn in fns]
        for (n, _), v in zip(fns, values):
            losses[n].append(v)
        want.append(f'{key}, {str(values)[1:-1]}')
    want.append(f'mean, {str([float(np.mean(losses[n])) for n, _ in fns])[1:-1]}')
    assert open(tmp_path / 'out' / 'results.csv').read() == '\n'.join(want) + '\n'


def test_new_flags_parse():
    from eval import eval_cli
    base = ['--model_path', 'm', '--triplet_dir', 't', '--output_dir', 'o']
    a = eval_cli.build_parser().parse_args(base)
    assert (a.metrics_device, a.batch_size, a.io_workers) == ('cpu', 1, 4)
    a = eval_cli.build_parser().parse_args(base + ['--metrics_device', 'gpu', '--batch_size', '8', '--io_workers', '2'])
    assert (a.metrics_device, a.batch_size, a.io_workers) == ('gpu', 8, 2)
    with pytest.raises(SystemExit):
        eval_cli.build_parser().parse_args(base + ['--metrics_device', 'tpu'])


def test_loop_argument_checks(tmp_path):
    from eval import eval_cli
    with pytest.raises(ValueError):
        eval_cli.run_evaluation(_Blend(), [], str(tmp_path), batch_size=0)
    with pytest.raises(ValueError):
        eval_cli.run_evaluation(_Blend(), [], str(tmp_path), metrics_device='tpu')
    with pytest.raises(ValueError, match='Interpolator'):
        eval_cli.run_evaluation(_Blend(), [], str(tmp_path), metrics_device='gpu')
