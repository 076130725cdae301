"""The native route of the nominal association metrics (``csrc/nominal.hip`` through ``ops/nominal.py``).

A ``*_matrix`` call on a GPU matrix runs three kernels with no per-pair host loop: ``nominal_labels`` (uint8 column plane, one presence
mask per column), ``nominal_pair_tables`` (all ``V (V - 1) / 2`` contingency tables at once) and ``nominal_scores`` (one wave per table,
fp64 from the exact counts).  The call reads the host once, at its end: the presence masks and the two flag words in one pinned copy.

The existing loop sizes every pair's table by the pair's number of distinct values and silently skips labels at or above it.  The native
result is used only where no label can be skipped: every label in ``[0, 64)`` and, for every pair, the union of the two presence masks
dense from 0.  Otherwise the call returns ``None`` and the caller runs the loop as before.  Also kept on the composition: fp64 and other
dtypes, the CPU, empty inputs, a single column, ``TMX_NOMINAL_NATIVE=0`` (the A/B knob of ``tools/nominal_bench.py``, read once per process).

The table extent handed to ``nominal_pair_tables`` is always 64: taking it from the masks would need a host read ahead of the pair kernel
and a second one for the warning flag, and the kernel already counts a pair with few categories in a small replicated table chosen on the
device from the two masks (``profiles/nominal_bench.json`` has both timings).
"""
import os
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.functional.nominal.utils import _unable_to_use_bias_correction_warning
from torchmetrics_forked_amd.ops import nominal as nominal_ops

_NOMINAL_NATIVE = os.environ.get("TMX_NOMINAL_NATIVE", "1") != "0"
_NATIVE_DTYPES = (torch.int64, torch.int32, torch.float32)
_LABEL_CAP = 64
_WORD = (1 << 64) - 1


def _native_nominal_ok(matrix: Tensor) -> bool:
    """The gate of the ``*_matrix`` route: a non-empty 2-D GPU matrix of int64, int32 or fp32 with at least two columns and fewer than
    ``2**31`` rows, the knob not switched off, and the native library in use."""
    if not (isinstance(matrix, Tensor) and matrix.is_cuda and matrix.ndim == 2 and matrix.dtype in _NATIVE_DTYPES and matrix.numel() > 0):
        return False
    if matrix.shape[1] < 2 or matrix.shape[0] >= 2**31:
        return False
    return _NOMINAL_NATIVE and ops.use_native(matrix)


def _native_pair_ok(preds: Tensor, target: Tensor) -> bool:
    """Two 1-D GPU tensors of one supported dtype and one length; 2-D inputs (the argmax path) and mixed dtypes keep the composition."""
    if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda and target.is_cuda):
        return False
    if preds.ndim != 1 or target.ndim != 1 or preds.shape != target.shape or preds.dtype != target.dtype or preds.device != target.device:
        return False
    return preds.dtype in _NATIVE_DTYPES and 0 < preds.numel() < 2**31 and _NOMINAL_NATIVE and ops.use_native(preds, target)


def _native_scores_ok(confmat: Tensor) -> bool:
    """The gate of the modules' ``compute()``: a square GPU state of at most 64 categories."""
    if not (isinstance(confmat, Tensor) and confmat.is_cuda and confmat.ndim == 2 and confmat.dtype in _NATIVE_DTYPES):
        return False
    if confmat.shape[0] != confmat.shape[1] or not 0 < confmat.shape[0] <= _LABEL_CAP:
        return False
    return _NOMINAL_NATIVE and ops.use_native(confmat)


def _masks_dense(masks: Sequence[int]) -> bool:
    """True when for every pair of columns the union of the presence masks is dense from 0: ``m_i | m_j == (1 << popcount) - 1``."""
    words = [int(m) & _WORD for m in masks]
    for i, a in enumerate(words):
        for b in words[i + 1:]:
            union = a | b
            if union != (1 << bin(union).count("1")) - 1:
                return False
    return True


def _read_words(words: Tensor) -> List[int]:
    """The call's one host read: int64 device words through a pinned buffer."""
    host = torch.empty(words.shape, dtype=words.dtype, pin_memory=True)
    host.copy_(words)
    return host.tolist()


def _native_matrix(matrix: Tensor, kind: int, bias_correction: bool, nan_strategy: str, nan_replace_value: Optional[float],
                   metric_name: str) -> Optional[Tensor]:
    """The ``[V, V]`` fp32 association matrix (diagonal 1) of a matrix that passed ``_native_nominal_ok``, or ``None`` where the loop has to run."""
    v = matrix.shape[1]
    drop = nan_strategy == "drop"
    labels, masks, label_flags = nominal_ops.nominal_labels(matrix, drop, 0.0 if drop or nan_replace_value is None else nan_replace_value)
    tables = nominal_ops.nominal_pair_tables(labels, masks, _LABEL_CAP)
    rows, cols = torch.triu_indices(v, v, 1, device=matrix.device)
    upper = tables.view(v * v, _LABEL_CAP, _LABEL_CAP).index_select(0, rows * v + cols)
    scores, score_flags = nominal_ops.nominal_scores(upper, kind, bias_correction)
    # Theil's U is not symmetric: out[j, i] scores the transposed table, read in place
    mirrored = nominal_ops.nominal_scores(upper.transpose(1, 2), kind, bias_correction)[0] if kind == nominal_ops.KIND_THEILS else scores
    out = torch.ones(v, v, device=matrix.device)
    out[rows, cols] = scores
    out[cols, rows] = mirrored
    words = _read_words(torch.cat([masks, label_flags.long(), score_flags.long()]))
    if words[v] & nominal_ops.FLAG_OUT_OF_RANGE or not _masks_dense(words[:v]):
        return None
    if words[v + 1] & nominal_ops.FLAG_NO_BIAS_CORRECTION:
        _unable_to_use_bias_correction_warning(metric_name=metric_name)
    return out


def _native_state_score(confmat: Tensor, kind: int, bias_correction: bool, metric_name: str) -> Tensor:
    """The score of one accumulated table that passed ``_native_scores_ok``.  Only the bias-corrected metrics read their flag word."""
    scores, flags = nominal_ops.nominal_scores(confmat.unsqueeze(0), kind, bias_correction)
    if bias_correction and kind in (nominal_ops.KIND_CRAMERS, nominal_ops.KIND_TSCHUPROWS):
        if _read_words(flags.long())[0] & nominal_ops.FLAG_NO_BIAS_CORRECTION:
            _unable_to_use_bias_correction_warning(metric_name=metric_name)
    return scores[0]


def _matrix_route(matrix: Tensor, kind: int, bias_correction: bool, nan_strategy: str, nan_replace_value: Optional[float],
                  metric_name: str) -> Optional[Tensor]:
    """The native ``[V, V]`` matrix, or ``None`` where the gate is closed or the loop has to run."""
    if not _native_nominal_ok(matrix):
        return None
    return _native_matrix(matrix, kind, bias_correction, nan_strategy, nan_replace_value, metric_name)


def _pair_route(preds: Tensor, target: Tensor, kind: int, bias_correction: bool, nan_strategy: str, nan_replace_value: Optional[float],
                metric_name: str) -> Optional[Tensor]:
    """The native score of a pair call, entry (0, 1) of the two-column matrix with ``preds`` as column 0, or ``None`` where the gate is
    closed or the composition has to run."""
    if not _native_pair_ok(preds, target):
        return None
    out = _native_matrix(torch.stack([preds, target], dim=1), kind, bias_correction, nan_strategy, nan_replace_value, metric_name)
    return None if out is None else out[0, 1]
