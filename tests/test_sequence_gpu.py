"""GPU tests of the frame-sequence entry points: film_interpolate_sequence against film_interpolate on the same pairs (bit for bit),
against the CPU oracle, the sequence recursion driver and the CLI's --sequence_window mode.

(No in-process "graph" = 1 cases: profiles/r06_hipgraph_crash_diagnosis.md.)
"""
import filecmp
import os

import numpy as np
import pytest

from conftest import oracle_options

pytestmark = pytest.mark.gpu

IMAGE_TOL = 1e-3     # north_star: |delta| < 1e-3 fp32 per pixel


def _frames(f, h, w, seed):
    """f frames of a scene moving by (2, -3) px per frame (+ noise), float32 [f, h, w, 3] in [0, 1)."""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3), dtype=np.float32)
    out = [np.roll(base, (2 * i, -3 * i), axis=(0, 1)) + rng.normal(0, 0.01, base.shape).astype(np.float32) for i in range(f)]
    return np.stack(out).astype(np.float32)


@pytest.fixture(scope='module')
def published():
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import PUBLISHED
    w = W.make_synthetic_weights(PUBLISHED, seed=0)
    eng = FilmEngine(PUBLISHED, device=0)
    eng.set_weights(w)
    yield PUBLISHED, w, eng
    eng.close()


# (h, w, F, align, block_shape, memory, graph, max_batch, profile)
CASES = [
    (256, 256, 2, None, None, 'host', 2, 0, 0),
    (256, 256, 3, None, None, 'host', 2, 0, 0),
    (256, 256, 6, None, None, 'host', 2, 0, 0),
    (256, 256, 6, None, None, 'device', 2, 0, 0),
    (256, 256, 3, None, None, 'host', 0, 0, 0),
    (256, 256, 3, None, None, 'device', 0, 0, 1),
    (270, 480, 3, 64, None, 'host', 2, 0, 0),
    (1080, 1920, 4, 64, (2, 2), 'host', 2, 0, 0),
    (1080, 1920, 4, 64, (2, 2), 'device', 2, 0, 0),
    (256, 256, 5, 64, (2, 2), 'host', 2, 3, 0),      # max_batch 3 pair-tiles, 4 tiles: chunks of 2 pairs x 1 tile
    (256, 256, 5, 64, (2, 2), 'device', 0, 2, 0),    # ... 2 pairs x 1 tile, one stream
]


@pytest.mark.parametrize('h,w,F,align,block,mem,graph,max_batch,profile', CASES)
def test_sequence_is_bit_identical_to_pairs(published, h, w, F, align, block, mem, graph, max_batch, profile):
    import torch
    from film_hip.torch_io import DeviceInterpolator
    opt, weights, eng = published
    frames = _frames(F, h, w, seed=F * 31 + h)
    eng.set_option('graph', graph)
    eng.set_option('max_batch', max_batch)
    eng.set_option('profile', profile)
    try:
        if mem == 'host':
            got = eng.interpolate_sequence(frames, align=align, block_shape=block)
            want = eng.interpolate_frames(frames[:-1], frames[1:], align=align, block_shape=block)
        else:
            it = DeviceInterpolator(eng, align=align, block_shape=list(block) if block else None)
            x = torch.from_numpy(frames).cuda()
            got = it.sequence(x).cpu().numpy()
            want = it.batch(x[:-1].contiguous(), x[1:].contiguous()).cpu().numpy()
            torch.cuda.synchronize()
    finally:
        eng.set_option('graph', 2)
        eng.set_option('max_batch', 0)
        eng.set_option('profile', 0)
    assert got.shape == (F - 1, h, w, 3) and np.isfinite(got).all()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    if profile:
        assert eng.profile()['ops']


def test_sequence_matches_the_oracle(published):
    """Every pair of a 256x256 sequence within the north-star bound of the CPU oracle; the feature tap holds every frame once."""
    from oracle import film_oracle as fo
    opt, weights, eng = published
    frames = _frames(4, 256, 256, seed=5)
    got = eng.interpolate_sequence(frames)
    feat0 = eng.tap('feat0')
    assert feat0.shape[0] == 4
    want = fo.film_forward(frames[:-1], frames[1:], weights, oracle_options(opt))
    err = np.abs(got - want).reshape(3, -1).max(axis=1)
    print('sequence vs oracle per pair:', err)
    assert (err < IMAGE_TOL).all()


def test_sequence_recursion_equals_pairwise_recursion(published):
    import torch
    from film_hip import recursive
    from film_hip.torch_io import DeviceInterpolator
    opt, weights, eng = published
    frames = [torch.from_numpy(f).cuda() for f in _frames(4, 128, 192, seed=9)]
    it = DeviceInterpolator(eng)
    want = list(recursive.interpolate_recursively(frames, 3, it))
    got = recursive.interpolate_sequence_recursively(frames, 3, it)
    assert len(got) == len(want) == 3 * 8 + 1
    for i, (g, wnt) in enumerate(zip(got, want)):
        assert torch.equal(g, wnt), i


def test_cli_sequence_window_writes_the_same_files(published, tmp_path, monkeypatch):
    """--sequence_window 3 on five input frames, T = 2: the same frame_*.png files, byte for byte, as the default path."""
    from eval import interpolator as interpolator_lib
    from eval import interpolator_cli as cli
    from eval import util
    opt, weights, eng = published
    real = interpolator_lib.Interpolator

    def interp(model_path, align, block_shape, precision=0):
        it = real.__new__(real)
        it._options, it._engine = eng.options, eng
        it._align, it._block_shape = align or None, block_shape or None
        return it

    frames = np.clip(_frames(5, 96, 160, seed=3), 0, 1)
    dirs = {}
    for name in ('pairs', 'sequence'):
        d = tmp_path / name / 'clip'
        d.mkdir(parents=True)
        for i, f in enumerate(frames):
            util.write_image(str(d / f'f_{i}.png'), f)
        dirs[name] = d
    monkeypatch.setattr(interpolator_lib, 'Interpolator', interp)
    try:
        cli.main(['--pattern', str(tmp_path / 'pairs' / '*'), '--times_to_interpolate', '2'])
        cli.main(['--pattern', str(tmp_path / 'sequence' / '*'), '--times_to_interpolate', '2', '--sequence_window', '3'])
    finally:
        monkeypatch.setattr(interpolator_lib, 'Interpolator', real)
    a = sorted(os.listdir(dirs['pairs'] / 'interpolated_frames'))
    b = sorted(os.listdir(dirs['sequence'] / 'interpolated_frames'))
    assert a == b == [f'frame_{i:03d}.png' for i in range(4 * 4 + 1)]
    for f in a:
        assert filecmp.cmp(dirs['pairs'] / 'interpolated_frames' / f, dirs['sequence'] / 'interpolated_frames' / f, shallow=False), f


def test_interpolator_sequence_equals_calls_per_pair(published):
    """Interpolator.interpolate_sequence (tiled) = Interpolator.__call__ on every pair, bit for bit."""
    from eval import interpolator as interpolator_lib
    opt, weights, eng = published
    it = interpolator_lib.Interpolator.__new__(interpolator_lib.Interpolator)
    it._options, it._engine = eng.options, eng
    it._align, it._block_shape = 64, [1, 2]
    frames = _frames(3, 200, 320, seed=4)
    got = it.interpolate_sequence(frames)
    dt = np.full((1,), 0.5, np.float32)
    for j in range(2):
        assert np.array_equal(got[j], it(frames[j:j + 1], frames[j + 1:j + 2], dt)[0]), j
