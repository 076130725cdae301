"""Spectral distortion index D-lambda (API parity: reference ``functional/image/d_lambda.py:22-130``).

GPU path (the gate of ``uqi._native_uqi_ok`` with UQI's default window): ``tmx::uqi_band_pair_sums`` (``csrc/uqi.hip``) scores
every band pair (i < j) of a tensor in ONE launch that reads the bands in place -- no gathered pair copies, no UQI maps.
Otherwise all band pairs of preds and of target are scored with one batched UQI call each (pairs folded into the batch)
instead of a Python loop over bands."""
from typing import Tuple

import torch
from torch import Tensor
from typing_extensions import Literal

from torchmetrics_forked_amd.functional.image.uqi import _native_uqi_ok, _uqi_windows, universal_image_quality_index
from torchmetrics_forked_amd.ops.image import uqi_band_pair_sums as _uqi_band_pair_sums
from torchmetrics_forked_amd.utilities.distributed import reduce


def _spectral_distortion_index_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    if preds.dtype != target.dtype:
        raise TypeError(
            "Expected `ms` and `fused` to have the same data type."
            f" Got ms: {preds.dtype} and fused: {target.dtype}."
        )
    if len(preds.shape) != 4:
        raise ValueError(
            f"Expected `preds` and `target` to have BxCxHxW shape. Got preds: {preds.shape} and target: {target.shape}."
        )
    if preds.shape[:2] != target.shape[:2]:
        raise ValueError(
            "Expected `preds` and `target` to have same batch and channel sizes."
            f"Got preds: {preds.shape} and target: {target.shape}."
        )
    return preds, target


_UQI_KERNEL_SIZE, _UQI_SIGMA = (11, 11), (1.5, 1.5)  # the defaults of universal_image_quality_index


def _band_uqi_matrix(x: Tensor) -> Tensor:
    """Symmetric ``[L, L]`` matrix of mean UQI between every pair of bands (zero diagonal)."""
    b, length = x.shape[:2]
    m = torch.zeros((length, length), device=x.device)
    if length < 2:
        return m
    i, j = torch.triu_indices(length, length, offset=1, device=x.device)
    if _native_uqi_ok(x, x, _UQI_KERNEL_SIZE, "elementwise_mean"):
        wy, wx = _uqi_windows(_UQI_KERNEL_SIZE, _UQI_SIGMA, x.device)
        sums = _uqi_band_pair_sums(x, wy, wx, torch.finfo(x.dtype).eps)
        valid = (x.shape[2] - _UQI_KERNEL_SIZE[0] + 1) * (x.shape[3] - _UQI_KERNEL_SIZE[1] + 1)
        m[i, j] = (sums.sum(1) / (b * valid)).to(m.dtype)
        return m + m.T
    a = x[:, i].transpose(0, 1).reshape(-1, 1, *x.shape[2:])
    c = x[:, j].transpose(0, 1).reshape(-1, 1, *x.shape[2:])
    uqi = universal_image_quality_index(a, c, reduction="none").reshape(len(i), -1).mean(1)
    m[i, j] = uqi.to(m.dtype)
    return m + m.T


def _spectral_distortion_index_compute(
    preds: Tensor, target: Tensor, p: int = 1, reduction: Literal["elementwise_mean", "sum", "none"] = "elementwise_mean"
) -> Tensor:
    length = preds.shape[1]
    diff = torch.pow(torch.abs(_band_uqi_matrix(target) - _band_uqi_matrix(preds)), p)
    if length == 1:
        out = torch.pow(diff, 1.0 / p)
    else:
        out = torch.pow(1.0 / (length * (length - 1)) * torch.sum(diff), 1.0 / p)
    return reduce(out, reduction)


def spectral_distortion_index(
    preds: Tensor, target: Tensor, p: int = 1, reduction: Literal["elementwise_mean", "sum", "none"] = "elementwise_mean"
) -> Tensor:
    if not isinstance(p, int) or p <= 0:
        raise ValueError(f"Expected `p` to be a positive integer. Got p: {p}.")
    preds, target = _spectral_distortion_index_update(preds, target)
    return _spectral_distortion_index_compute(preds, target, p, reduction)
