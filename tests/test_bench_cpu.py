"""bench.py's options that need no GPU: what `--dump-outputs` writes (dump_outputs on host tensors) and the argument checks."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope='module')
def bench():
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_writes_every_array_in_float32(bench, tmp_path):
    a = torch.arange(2 * 4 * 6 * 3, dtype=torch.float32).reshape(2, 4, 6, 3) / 7
    b = torch.linspace(-1, 1, 10, dtype=torch.float64)
    report = bench.dump_outputs(str(tmp_path), {'interpolated': a, 'other': b})
    assert sorted(os.listdir(tmp_path)) == ['interpolated.npy', 'other.npy']
    got_a, got_b = np.load(tmp_path / 'interpolated.npy'), np.load(tmp_path / 'other.npy')
    assert got_a.dtype == np.float32 and np.array_equal(got_a, a.numpy())
    assert got_b.dtype == np.float32 and np.array_equal(got_b, b.float().numpy())
    assert report == {'interpolated': {'shape': [2, 4, 6, 3], 'sampled_elements': None},
                      'other': {'shape': [10], 'sampled_elements': None}}


def test_dump_outputs_samples_beyond_the_limit_at_fixed_positions(bench, tmp_path, monkeypatch):
    """Outputs larger than the limit in all: every array is cut to its share of the limit, at positions drawn with the fixed
    seed - the same file for the same shapes in every run, whatever the values."""
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 4 * 1000)
    big = torch.arange(3000, dtype=torch.float32)
    small = torch.arange(1000, dtype=torch.float32) + 0.5
    report = bench.dump_outputs(str(tmp_path / 'one'), {'frames': big, 'other': small})
    assert report['frames']['sampled_elements'] == 750 and report['other']['sampled_elements'] == 250
    got = np.load(tmp_path / 'one' / 'frames.npy')
    assert got.dtype == np.float32 and got.size == 750
    idx = got.astype(np.int64)                                      # big[i] == i: the values are the positions
    assert np.array_equal(got, idx) and np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < 3000
    assert sum(os.path.getsize(tmp_path / 'one' / f) for f in os.listdir(tmp_path / 'one')) <= 4 * 1000 + 2 * 128
    bench.dump_outputs(str(tmp_path / 'two'), {'frames': big * 2, 'other': small})
    assert np.array_equal(np.load(tmp_path / 'two' / 'frames.npy'), got * 2)


def test_profile_out_needs_full(tmp_path):
    """The per-op profile is taken from the profiled forward of a --full run; a plain run refuses the option before any work."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--profile-out', str(tmp_path / 'profile.json')],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and '--full' in out.stderr, out.stderr[-2000:]
    assert not os.listdir(tmp_path)
