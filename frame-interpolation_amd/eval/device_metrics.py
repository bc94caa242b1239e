"""The evaluation metrics of eval/metrics.py (the reference's losses/losses.py:72-113) computed on the GPU by the HIP kernels behind
film_image_metrics (include/film_hip.h), on float32 torch CUDA tensors, on the current torch stream.

The kernels return per-image sums; compose() turns them into the values the metrics.* functions return for the same batch: l1 and
l2 are means over every element of the batch, psnr and ssim means of the per-image values.  eval/metrics.py stays the oracle.
"""
from typing import List, Sequence

import numpy as np

from . import metrics as metrics_lib

# column of each metric in a per-image row of FilmEngine.image_metrics: sum |d|, sum d*d, psnr dB, ssim
_COLUMN = {'l1': 0, 'l2': 1, 'psnr': 2, 'ssim': 3}


def compose(per_image: np.ndarray, n_per_image: int, names: Sequence[str]) -> List[float]:
    """per_image: float64 [B,4] rows of FilmEngine.image_metrics for B images of n_per_image values (H*W*C) each -> the values
    metrics.<name>(pred, ref) returns for the whole batch, in the order of `names`."""
    per_image = np.asarray(per_image, np.float64).reshape(-1, 4)
    out = []
    for n in names:
        v = per_image[:, _COLUMN[n]]
        if n in ('l1', 'l2'):
            out.append(float(np.sum(v) / (v.shape[0] * n_per_image)))
        else:
            out.append(float(np.mean(v)))
    return out


class DeviceMetricSet:
    """metrics.test_losses(names) on the device: the same names in the same order, the same refusal of vgg / style.

    pred, ref: float32 CUDA tensors [B,H,W,C] (C = 1 or 3) on the engine's device.  Each call runs on the current torch stream, after
    the work queued there before, and returns once the per-image scalars are on the host (only they cross PCIe)."""

    def __init__(self, engine, names: Sequence[str], max_val: float = 1.0):
        self.names = [n for n, _ in metrics_lib.test_losses(list(names))]
        self._engine = engine
        self._max_val = float(max_val)

    def per_image(self, pred, ref, clip: bool = False) -> np.ndarray:
        """float64 [B,4] per image (FilmEngine.image_metrics); clip: pred clipped to [0,1] first, inside the kernels."""
        import torch
        if not (pred.is_cuda and ref.is_cuda and pred.dtype == torch.float32 and ref.dtype == torch.float32):
            raise ValueError('pred and ref must be float32 CUDA tensors')
        if pred.dim() != 4 or pred.shape != ref.shape:
            raise ValueError(f'expected two [B,H,W,C] tensors of equal shape, got {tuple(pred.shape)} and {tuple(ref.shape)}')
        pred, ref = pred.contiguous(), ref.contiguous()
        b, h, w, c = pred.shape
        stream = torch.cuda.current_stream(pred.device).cuda_stream
        return self._engine.image_metrics_device(pred.data_ptr(), ref.data_ptr(), b, h, w, c, names=self.names, clip=clip,
                                                 max_val=self._max_val, stream=stream)

    def rows(self, pred, ref, clip: bool = False) -> List[List[float]]:
        """Per image k: [metrics.<name>(pred[k:k+1], ref[k:k+1]) for name in names]."""
        per = self.per_image(pred, ref, clip)
        n = int(np.prod(pred.shape[1:]))
        return [compose(per[k:k + 1], n, self.names) for k in range(per.shape[0])]

    def __call__(self, pred, ref, clip: bool = False) -> List[float]:
        """[metrics.<name>(pred, ref) for name in names] for the whole batch."""
        return compose(self.per_image(pred, ref, clip), int(np.prod(pred.shape[1:])), self.names)
