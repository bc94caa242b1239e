"""GPU tests of the kernels that move pixels between frames and tiles (csrc/frame_kernels.hip: frame_to_tiles_kernel<false / true>,
frame_u8_to_tiles_kernel<false / true>, tiles_to_frame_kernel, blend_tiles_kernel), each launched ALONE
through film_debug_tile_map on designed data: torch device tensors with guard bands, distinct finite floats of both signs and two
magnitudes (every byte value in every channel for the 8-bit frames), against the numpy restatement tests/tile_map_ref.py.  Every
comparison is on the bits: the cuts and the plain join are copies, the 8-bit cut a table lookup, the blend a fixed sequence of float32
operations.  What is checked per call (value, +0.0 padding, nothing else written, the same bits again) is tile_map_ref.check_cut /
check_join; tests/test_tile_map_cpu.py shows that this comparison finds each of ten planted faults, and which kernel instance and branch
every case reaches (test_the_cases_reach_every_instance_and_branch).

No network runs here, except in the last test: two frame sizes whose tiles pad to the same size through ONE engine.
"""
import numpy as np
import pytest

import tile_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    """A handle with a device and NO weights: film_debug_tile_map needs none."""
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    e = FilmEngine(TINY, device=0)
    yield e
    e.close()


class GpuBackend:
    """film_debug_tile_map as a backend of the comparison: both allocations go up as torch tensors (guard | payload | guard in ONE
    allocation each), the entry point gets the payloads' addresses, both come back."""

    def __init__(self, eng):
        self.eng = eng

    def __call__(self, mode, u8, frames_alloc, tiles_alloc, case, tile0, ntiles):
        import torch
        ft, tt = torch.from_numpy(np.array(frames_alloc)).cuda(), torch.from_numpy(np.array(tiles_alloc)).cuda()
        fp = ft.data_ptr() + (R.GUARD_U8 if u8 else 4 * R.GUARD)
        tp = tt.data_ptr() + 4 * R.GUARD
        assert fp % 4 == 0 and tp % 16 == 0 and ft.numel() * ft.element_size() % 4 == 0
        self.eng.debug_tile_map(mode, fp, tp, case.B, case.H, case.W, case.align, case.block, tile0, ntiles, u8=u8)
        torch.cuda.synchronize()
        return ft.cpu().numpy(), tt.cpu().numpy()


@pytest.fixture(params=R.CASES, ids=lambda c: c.name)
def setup(request, eng):
    case = request.param
    eng.set_block_overlap(case.overlap)
    try:
        geo = eng.tiling(case.H, case.W, case.align, case.block)
        assert geo == R.expected_geometry(case), (geo, R.expected_geometry(case))
        for k, v in R.PINNED.get(case.name, {}).items():
            assert geo[k] == v, (k, geo[k], v)
        backend = GpuBackend(eng)
        yield case, geo, backend
    finally:
        eng.set_block_overlap(0)


def _ranges(case, geo):
    bh, bw = len(geo['origins_y']), len(geo['origins_x'])
    return R.partitions(case.B * bh * bw, bh * bw)


def _report(findings):
    findings = list(findings)
    assert not findings, f'{len(findings)} findings:\n' + '\n'.join(findings[:12])


@pytest.mark.parametrize('pix', ['f32', 'u8'])
def test_cut(setup, pix):
    """Every range of every partition: tiles_dev[0 : ntiles] == the restatement on the bits, the padding +0.0, the rest of the tile
    tensor, its guards and the frames untouched, the same bits from the same call again."""
    case, geo, backend = setup
    _report(f'[{name}] {m}' for name, ranges in _ranges(case, geo).items()
            for m in R.check_cut(backend, case, geo, pix == 'u8', ranges, seed=17))


def test_join(setup):
    """The ranges of a partition one after another on a frame batch that starts as background: after every call the batch == the
    restatement applied to the same starting bits; pixels no tile of the range covers, the guards and the tile tensor untouched."""
    case, geo, backend = setup
    _report(f'[{name}] {m}' for name, ranges in _ranges(case, geo).items() for m in R.check_join(backend, case, geo, ranges, seed=41))


# ---- one plan, two frame sizes: the plan's img0 is reused with other pad offsets ------------------------------------------------------
def test_one_plan_serves_two_frame_sizes_with_other_pad_offsets():
    """100 x 250 and then 120 x 200, both 2 x 2 with align 64: 50 x 125 patches at (7, 1) and 60 x 100 patches at (2, 14) of the same
    64 x 128 tiles, so the second call replays the first one's plan on an img0 whose padding lay elsewhere.  Its result == the bits a
    fresh engine gives."""
    import inputs as TI
    from film_hip import weights as W
    from film_hip.engine import FilmEngine
    from film_hip.options import TINY
    w = W.make_synthetic_weights(TINY, seed=0)
    a0, a1 = TI.frame_pair(1, 100, 250, seed=3)
    b0, b1 = TI.frame_pair(1, 120, 200, seed=4)
    both, fresh = FilmEngine(TINY, device=0), FilmEngine(TINY, device=0)
    try:
        for e in (both, fresh):
            e.set_weights(w)
        ga, gb = both.tiling(100, 250, 64, (2, 2)), both.tiling(120, 200, 64, (2, 2))
        assert (ga['padded_h'], ga['padded_w']) == (gb['padded_h'], gb['padded_w']) == (64, 128)
        assert (ga['pad_y'], ga['pad_x'], gb['pad_y'], gb['pad_x']) == (7, 1, 2, 14)
        first = both.interpolate_frames(a0, a1, align=64, block_shape=(2, 2))
        second = both.interpolate_frames(b0, b1, align=64, block_shape=(2, 2))
        want = fresh.interpolate_frames(b0, b1, align=64, block_shape=(2, 2))
        assert np.isfinite(first).all() and np.isfinite(second).all()
        assert np.array_equal(second.view(np.uint32), want.view(np.uint32)), float(np.abs(second - want).max())
        # and back, on the chunked path this time (run_chunk's cuts and joins instead of the host pipeline's own): the first size on
        # the plan the second one used, then the second again
        both.set_option('host_overlap', 0)
        again = both.interpolate_frames(a0, a1, align=64, block_shape=(2, 2))
        assert np.array_equal(again.view(np.uint32), first.view(np.uint32))
        again = both.interpolate_frames(b0, b1, align=64, block_shape=(2, 2))
        assert np.array_equal(again.view(np.uint32), want.view(np.uint32))
    finally:
        both.close(); fresh.close()
