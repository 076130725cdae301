"""Cosine similarity (API parity: reference ``functional/regression/cosine_similarity.py:22-96``)."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from torchmetrics_forked_amd.ops import text as _native
from torchmetrics_forked_amd.utilities.checks import _check_same_shape


def _cosine_similarity_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    _check_same_shape(preds, target)
    return preds.float(), target.float()


def _cosine_similarity_compute(preds: Tensor, target: Tensor, reduction: Optional[str] = "sum") -> Tensor:
    if _native.row_pair_native(preds, target):
        # dot and both squared norms in one fused pass per row pair (``tmx::row_pair_measure``); fp64, CPU and autograd inputs compose
        d = preds.shape[-1]
        sim = _native.row_pair_measure(preds.reshape(-1, d), target.reshape(-1, d), _native.KIND_COSINE).reshape(preds.shape[:-1]).to(preds.dtype)
    else:
        dot = (preds * target).sum(dim=-1)
        sim = dot / (preds.norm(dim=-1) * target.norm(dim=-1))
    reductions = {"sum": torch.sum, "mean": torch.mean, "none": lambda x: x, None: lambda x: x}
    return reductions[reduction](sim)


def cosine_similarity(preds: Tensor, target: Tensor, reduction: Optional[str] = "sum") -> Tensor:
    return _cosine_similarity_compute(*_cosine_similarity_update(preds, target), reduction)
