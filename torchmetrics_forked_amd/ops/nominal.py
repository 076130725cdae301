"""Thin wrappers of the nominal-association ops of ``csrc/nominal.hip``: column labels, all-pairs contingency tables and the four
scores (Cramer's V, Tschuprow's T, Pearson's contingency coefficient, Theil's U)."""
from typing import Dict, NamedTuple, Tuple

import torch
from torch import Tensor

KIND_CRAMERS, KIND_TSCHUPROWS, KIND_PEARSON, KIND_THEILS = 0, 1, 2, 3

FLAG_OUT_OF_RANGE = 1  # bit 0 of ``nominal_labels``' flag word: a kept label outside ``[0, label_cap)``
FLAG_NO_BIAS_CORRECTION = 2  # bit 1 of ``nominal_scores``' flag word: ``min(rows_c, cols_c) == 1`` for some table


class NominalTile(NamedTuple):
    """``rows_per_chunk``: rows a workgroup of the pair kernel counts; ``threads``: per workgroup; ``pairs_per_tile[K]``: column pairs a
    workgroup owns at table extent ``K``; ``label_cap``: labels are ``0 .. label_cap - 1``."""

    rows_per_chunk: int
    threads: int
    pairs_per_tile: Dict[int, int]
    label_cap: int


def nominal_labels(matrix: Tensor, drop_nan: bool, nan_replace: float) -> Tuple[Tensor, Tensor, Tensor]:
    """``tmx::nominal_labels``: ``matrix`` ``[N, V]`` (int64 / int32 / fp32, read in place with its strides) to ``(labels, masks, flags)``:
    ``labels`` uint8 ``[V, N]`` (column-major plane; every column starts 16-byte aligned and is padded to a multiple of 16 rows with the
    drop byte 255), ``masks`` int64 ``[V]`` (bit ``l`` set when column ``v`` holds the label ``l``) and ``flags`` int32 ``[1]``.  Per element: NaN becomes
    ``nan_replace``, or under ``drop_nan`` the byte 255; the value is truncated toward zero as ``.long()`` does.  Bit 0 of ``flags`` is set
    when a kept label lies outside ``[0, 64)``.  No host read."""
    labels, masks, flags = torch.ops.tmx.nominal_labels(matrix, bool(drop_nan), float(nan_replace))
    return labels, masks, flags


def nominal_pair_tables(labels: Tensor, masks: Tensor, k: int) -> Tensor:
    """``tmx::nominal_pair_tables``: int32 ``[V, V, k, k]`` with ``tables[i, j, a, b]`` the number of rows with ``col_j == a`` and ``col_i == b`` for
    ``i < j`` (the layout of ``_contingency(preds=col_i, target=col_j)``); the diagonal and ``i > j`` stay zero.  A row where either label is
    the drop byte, or not below ``k``, is skipped for that pair only.  ``k`` in 2, 4, 8, 16, 32, 64.  Exact integer counts through LDS and
    global integer atomics: two runs are bit-equal.  No host read."""
    return torch.ops.tmx.nominal_pair_tables(labels, masks, int(k))


def nominal_scores(tables: Tensor, kind: int, bias_correction: bool) -> Tuple[Tensor, Tensor]:
    """``tmx::nominal_scores``: ``tables`` ``[P, K, K]`` (int32 / int64 / fp32 counts, any strides, ``K <= 64``; rows = target category, columns =
    preds category) to ``(scores fp32 [P], flags int32 [1])``.  ``kind``: ``KIND_CRAMERS``, ``KIND_TSCHUPROWS``, ``KIND_PEARSON`` or ``KIND_THEILS``;
    ``bias_correction`` applies to the first two.  fp64 from the exact counts, rounded once.  Where the bias correction cannot be applied
    (``min(rows_c, cols_c) == 1``) the score is NaN and bit 1 of ``flags`` is set.  No host read."""
    scores, flags = torch.ops.tmx.nominal_scores(tables, int(kind), bool(bias_correction))
    return scores, flags


def nominal_tile() -> NominalTile:
    """The geometry of the kernels (see ``NominalTile``)."""
    v = [int(x) for x in torch.ops.tmx.nominal_tile()]
    return NominalTile(v[0], v[1], dict(zip((2, 4, 8, 16, 32, 64), v[2:8])), v[8])
