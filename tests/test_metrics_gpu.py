"""film_image_metrics on the MI355X (metrics_kernels.hip) against eval/metrics.py on the same arrays: shapes from the smallest SSIM
input to 4K, C = 1 / 3, batches, the clip, known answers, determinism (runs, batch position, memory kinds, stream order), argument
errors, and eval_cli --metrics_device gpu --batch_size 2 against the cpu run."""
import filecmp
import os

import numpy as np
import pytest

import inputs as TI

pytestmark = pytest.mark.gpu

ALL = ['l1', 'l2', 'ssim', 'psnr']


@pytest.fixture(scope='module')
def eng():
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    e = FilmEngine(PUBLISHED, device=0)     # no weights: the metrics need none
    yield e
    e.close()


def _want(pred, ref, clip):
    """Per image: sum |d|, sum d*d, mse, psnr, ssim (ssim None below 11 x 11) with eval/metrics.py."""
    from eval import metrics as M
    if clip:
        pred = np.clip(pred, 0.0, 1.0)
    rows = []
    for k in range(pred.shape[0]):
        p, r = pred[k:k + 1], ref[k:k + 1]
        d = p.astype(np.float64) - r.astype(np.float64)
        ssim = M.ssim(p, r) if min(p.shape[1:3]) >= 11 else None
        rows.append((M.l1(p, r) * p.size, M.l2(p, r) * p.size, float(np.mean(d * d)), M.psnr(p, r), ssim))
    return rows


def _check(got, want):
    for g, (s1, s2, _mse, psnr, ssim) in zip(got, want):
        assert g[0] == pytest.approx(s1, rel=1e-9, abs=0) and g[1] == pytest.approx(s2, rel=1e-9, abs=0)
        if np.isinf(psnr):
            assert np.isinf(g[2]) and g[2] > 0
        else:
            assert abs(g[2] - psnr) < 1e-8
        if ssim is not None:
            assert abs(g[3] - ssim) < 1e-9, (g[3], ssim)


def _pair(rng, b, h, w, c, spread=0.2):
    ref = rng.random((b, h, w, c), dtype=np.float32)
    pred = (ref + rng.normal(0, 0.05, ref.shape) + rng.uniform(-spread, spread, (b, 1, 1, c))).astype(np.float32)
    pred[:, 0, 0, 0], pred[:, -1, -1, -1] = -0.3, 1.4     # values outside [0,1] in every image, for the clip
    return pred, ref


@pytest.mark.parametrize('b,h,w,c', [(1, 11, 11, 3), (2, 13, 17, 1), (3, 13, 17, 3), (1, 257, 449, 3), (4, 256, 448, 3),
                                     (2, 256, 448, 1), (1, 1080, 1920, 3)])
def test_against_numpy(eng, b, h, w, c):
    rng = np.random.default_rng(h * 7 + w + c)
    pred, ref = _pair(rng, b, h, w, c)
    assert pred.min() < 0 and pred.max() > 1
    for clip in (False, True):
        got = eng.image_metrics(pred, ref, ALL, clip=clip)
        _check(got, _want(pred, ref, clip))


def test_4k_image_and_batch_composition(eng):
    from eval import device_metrics as DM, metrics as M
    rng = np.random.default_rng(4)
    pred, ref = _pair(rng, 1, 2160, 4096, 3)
    got = eng.image_metrics(pred, ref, ALL, clip=True)
    _check(got, _want(pred, ref, True))
    p = np.clip(pred, 0.0, 1.0)
    vals = DM.compose(got, p[0].size, ALL)
    want = [M.l1(p, ref), M.l2(p, ref), M.ssim(p, ref), M.psnr(p, ref)]
    assert vals[0] == pytest.approx(want[0], rel=1e-9) and vals[1] == pytest.approx(want[1], rel=1e-9)
    assert abs(vals[2] - want[2]) < 1e-9 and abs(vals[3] - want[3]) < 1e-8


def test_subsets_and_nan_for_what_was_not_asked(eng):
    rng = np.random.default_rng(5)
    pred, ref = _pair(rng, 2, 40, 52, 3)
    full = eng.image_metrics(pred, ref, ALL)
    for names, cols in ((['ssim'], [3]), (['l1', 'psnr'], [0, 2]), (['l2'], [1])):
        got = eng.image_metrics(pred, ref, names)
        for j in range(4):
            if j in cols:
                assert np.array_equal(got[:, j], full[:, j])
            else:
                assert np.isnan(got[:, j]).all()
    small = eng.image_metrics(pred[:, :8, :9], ref[:, :8, :9], ['l1', 'l2', 'psnr'])     # no ssim: any size
    _check(small, _want(pred[:, :8, :9], ref[:, :8, :9], False))


def test_identical_and_constant_images(eng):
    from eval import metrics as M
    rng = np.random.default_rng(6)
    a = rng.random((2, 30, 41, 3), dtype=np.float32)
    got = eng.image_metrics(a, a, ALL)
    assert (got[:, 0] == 0).all() and (got[:, 1] == 0).all() and np.isinf(got[:, 2]).all() and (got[:, 2] > 0).all()
    assert np.abs(got[:, 3] - 1.0).max() < 1e-12
    for va, vb in ((0.3, 0.7), (0.5, 0.5), (0.0, 1.0)):
        x = np.full((1, 24, 19, 1), va, np.float32)
        y = np.full((1, 24, 19, 1), vb, np.float32)
        g = eng.image_metrics(x, y, ALL)
        _check(g, _want(x, y, False))
        assert abs(g[0, 3] - M.ssim(x, y)) < 1e-12


def test_deterministic_across_runs_batch_positions_and_memory_kinds(eng):
    import torch
    rng = np.random.default_rng(7)
    pred, ref = _pair(rng, 4, 97, 131, 3)
    a = eng.image_metrics(pred, ref, ALL, clip=True)
    b = eng.image_metrics(pred, ref, ALL, clip=True)
    assert a.tobytes() == b.tobytes()
    for k in range(4):
        assert eng.image_metrics(pred[k:k + 1], ref[k:k + 1], ALL, clip=True).tobytes() == a[k:k + 1].tobytes()
    assert eng.image_metrics(pred[1:3], ref[1:3], ALL, clip=True).tobytes() == a[1:3].tobytes()
    tp, tr = torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()
    torch.cuda.synchronize()
    d = eng.image_metrics_device(tp.data_ptr(), tr.data_ptr(), 4, 97, 131, 3, ALL, clip=True)
    assert d.tobytes() == a.tobytes()
    # an image whose start is not 16-byte aligned (odd H*W*C): the same bits as at an aligned address
    n = pred[0].size
    assert n % 4 != 0
    flat_p, flat_r = tp.reshape(-1), tr.reshape(-1)
    d1 = eng.image_metrics_device(flat_p[n:].data_ptr(), flat_r[n:].data_ptr(), 1, 97, 131, 3, ALL, clip=True)
    assert d1.tobytes() == a[1:2].tobytes()


def test_ordered_after_the_torch_work_that_wrote_the_inputs(eng):
    import torch
    from eval import device_metrics as DM
    rng = np.random.default_rng(8)
    pred, ref = _pair(rng, 2, 256, 448, 3)
    want = eng.image_metrics(pred, ref, ALL)
    src_p, src_r = torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device='cuda')
    with torch.cuda.stream(side):
        dst_p = torch.zeros_like(src_p)
        dst_r = torch.zeros_like(src_r)
        for _ in range(8):          # keep the stream busy so that an unordered read would see the zeros
            big = big @ big
            big = big / big.abs().max()
        dst_p.copy_(src_p)
        dst_r.copy_(src_r)
        got = DM.DeviceMetricSet(eng, ALL).per_image(dst_p, dst_r)
    assert got.tobytes() == want.tobytes()
    torch.cuda.synchronize()


def test_device_metric_set_matches_the_numpy_metric_set(eng):
    import torch
    from eval import device_metrics as DM, metrics as M
    rng = np.random.default_rng(9)
    pred, ref = _pair(rng, 3, 64, 80, 3)
    names = ['psnr', 'ssim', 'l1']
    ms = DM.DeviceMetricSet(eng, names)
    tp, tr = torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()
    p = np.clip(pred, 0.0, 1.0)
    got = ms(tp, tr, clip=True)
    want = [fn(p, ref) for _n, fn in M.test_losses(names)]
    assert abs(got[0] - want[0]) < 1e-8 and abs(got[1] - want[1]) < 1e-9 and got[2] == pytest.approx(want[2], rel=1e-9)
    rows = ms.rows(tp, tr, clip=True)
    for k in range(3):
        wk = [fn(p[k:k + 1], ref[k:k + 1]) for _n, fn in M.test_losses(names)]
        assert abs(rows[k][0] - wk[0]) < 1e-8 and abs(rows[k][1] - wk[1]) < 1e-9 and rows[k][2] == pytest.approx(wk[2], rel=1e-9)


def test_argument_errors(eng):
    from film_hip.engine import FILM_ERR_INVALID, FILM_MEM_DEVICE, FILM_MEM_HOST
    lib, h = eng._lib, eng._h
    a = np.zeros((2, 16, 16, 3), np.float32)
    out = np.zeros((2, 4), np.float64)
    p, o = a.ctypes.data, out.ctypes.data

    def call(pred=p, ref=p, b=2, hh=16, ww=16, c=3, flags=15, max_val=1.0, dst=o, mem=FILM_MEM_HOST):
        return lib.film_image_metrics(h, pred, ref, b, hh, ww, c, flags, max_val, dst, mem, None)
    assert call() == 0
    for kw in (dict(b=0), dict(b=-3), dict(c=2), dict(c=0), dict(pred=None), dict(ref=None), dict(dst=None), dict(max_val=0.0),
               dict(max_val=-2.0), dict(hh=10), dict(ww=10), dict(hh=10, ww=10, mem=FILM_MEM_DEVICE), dict(flags=64)):
        assert call(**kw) == FILM_ERR_INVALID, kw
        assert lib.film_last_error(h).decode()
    assert call(hh=10, ww=10, flags=7) == 0


def test_eval_cli_gpu_metrics_match_the_cpu_run(tmp_path):
    """eval_cli --metrics_device gpu --batch_size 2 --output_frames on the two Vimeo-sized triplets of
    test_gpu_configs.py::test_eval_cli_on_vimeo_sized_triplets: same keys, values within 1e-9 of the cpu run, byte-identical PNGs."""
    from eval import eval_cli, util
    from film_hip import weights as W
    from film_hip.options import PUBLISHED
    w = W.make_synthetic_weights(PUBLISHED, seed=0)
    model_dir = tmp_path / 'model'
    W.save_weights(str(model_dir), w)
    root = tmp_path / 'vimeo'
    for k, seq in enumerate(('00001/0001', '00001/0002')):
        x0, x1 = TI.frame_pair(1, 256, 448, seed=20 + k, shift=(4, -6), fg_shift=(-3, 5))
        mid, _ = TI.frame_pair(1, 256, 448, seed=20 + k, shift=(2, -3), fg_shift=(-2, 3))
        d = root / seq
        os.makedirs(d)
        for name, img in (('im1.png', x0[0]), ('im2.png', mid[0]), ('im3.png', x1[0])):
            util.write_image(str(d / name), img)
    base = ['--model_path', str(model_dir), '--triplet_dir', str(root), '--output_frames']
    assert eval_cli.main(base + ['--output_dir', str(tmp_path / 'cpu')]) == 0
    assert eval_cli.main(base + ['--output_dir', str(tmp_path / 'gpu'), '--metrics_device', 'gpu', '--batch_size', '2']) == 0
    rows = {}
    for run in ('cpu', 'gpu'):
        rows[run] = [l.strip().split(', ') for l in open(tmp_path / run / 'results.csv')]
    assert rows['gpu'][0] == rows['cpu'][0] == ['key'] + ALL
    assert [r[0] for r in rows['gpu']] == [r[0] for r in rows['cpu']] == ['key', '00001_0001', '00001_0002', 'mean']
    for rg, rc in zip(rows['gpu'][1:], rows['cpu'][1:]):
        g, c = np.array(rg[1:], float), np.array(rc[1:], float)
        print(rg[0], 'gpu', g, 'cpu', c)
        assert np.abs(g - c).max() < 1e-9
    pngs = sorted(f for f in os.listdir(tmp_path / 'cpu') if f.endswith('.png'))
    assert len(pngs) == 8 and pngs == sorted(f for f in os.listdir(tmp_path / 'gpu') if f.endswith('.png'))
    for f in pngs:
        assert filecmp.cmp(tmp_path / 'cpu' / f, tmp_path / 'gpu' / f, shallow=False), f
