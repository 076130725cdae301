"""CPU oracles of the neighbour-difference metrics, dense torch written from the definitions: PSNR with blocked effect, total
variation and image gradients.

Every function takes the working dtype: ``torch.float64`` as the oracle, ``torch.float32`` as the ``comp32`` of ``vif_oracle.value_rule`` (what an
fp32 evaluation of the same formula itself loses).  The boundary and non-boundary pair lists of PSNR-B are built explicitly, pair by
pair, as the reference builds its index lists, and not by the strided masks of the package's composition.
"""
import math
from typing import List, Tuple

import torch
from torch import Tensor


def pair_lists(n: int, block_size: int) -> Tuple[List[int], List[int]]:
    """The neighbour pairs ``(j, j + 1)``, ``j = 0 .. n − 2``, of an axis of length ``n``, by their first index: ``(boundary, others)``.  A pair
    crosses a block boundary when its second element starts a block: ``(j + 1) % block_size == 0``."""
    boundary, others = [], []
    for j in range(n - 1):
        (boundary if (j + 1) % block_size == 0 else others).append(j)
    return boundary, others


def _pair_sum(x: Tensor, dim: int, first: List[int]) -> Tensor:
    """Sum over the listed pairs of the squared difference along ``dim``; an empty list gives 0."""
    if not first:
        return torch.zeros((), dtype=x.dtype)
    idx = torch.tensor(first, dtype=torch.long)
    return (x.index_select(dim, idx) - x.index_select(dim, idx + 1)).pow(2).sum()


def psnrb_sums(p: Tensor, t: Tensor, block_size: int, dtype: torch.dtype = torch.float64) -> Tensor:
    """``[5]`` in ``dtype``: ``Σ(p − t)²``, ``D_B``, ``D_BC``, ``min t``, ``max t`` of ``p`` / ``t`` ``[B, 1, H, W]`` (what ``tmx::psnrb_sums`` returns)."""
    p, t = p.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    assert p.dim() == 4 and p.shape[1] == 1 and p.shape == t.shape
    hb, hbc = pair_lists(p.shape[3], block_size)
    vb, vbc = pair_lists(p.shape[2], block_size)
    d_b = _pair_sum(p, 3, hb) + _pair_sum(p, 2, vb)
    d_bc = _pair_sum(p, 3, hbc) + _pair_sum(p, 2, vbc)
    return torch.stack([(p - t).pow(2).sum(), d_b, d_bc, t.min(), t.max()])


def bef(sums: Tensor, height: int, width: int, block_size: int) -> Tensor:
    """Blocking-effect factor from ``psnrb_sums`` (in its dtype), with the pair counts of the reference's formula."""
    n_hb = height * (width / block_size) - 1
    n_hbc = height * (width - 1) - n_hb
    n_vb = width * (height / block_size) - 1
    n_vbc = width * (height - 1) - n_vb
    d_b = sums[1] / (n_hb + n_vb)
    d_bc = sums[2] / (n_hbc + n_vbc)
    t = math.log2(block_size) / math.log2(min(height, width)) if bool(d_b > d_bc) else 0
    return t * (d_b - d_bc)


def blocky(sums: Tensor, height: int, width: int, block_size: int) -> Tuple[bool, float]:
    """``(d_b > d_bc, |d_b − d_bc| / max(d_b, d_bc))``: which branch ``bef`` takes and by what margin."""
    n_hb = height * (width / block_size) - 1
    n_vb = width * (height / block_size) - 1
    d_b = float(sums[1]) / (n_hb + n_vb)
    d_bc = float(sums[2]) / (height * (width - 1) - n_hb + width * (height - 1) - n_vb)
    return d_b > d_bc, abs(d_b - d_bc) / max(d_b, d_bc)


def psnrb_from_sums(sums: Tensor, num_obs: int, height: int, width: int, block_size: int) -> Tensor:
    data_range = sums[4] - sums[3]
    mse = sums[0] / num_obs + bef(sums, height, width, block_size)
    if bool(data_range > 2):
        return 10 * torch.log10(data_range**2 / mse)
    return 10 * torch.log10(1.0 / mse)


def psnrb(p: Tensor, t: Tensor, block_size: int, dtype: torch.dtype = torch.float64) -> Tensor:
    """PSNR-B of one ``[B, 1, H, W]`` batch, 0-dim in ``dtype``."""
    return psnrb_from_sums(psnrb_sums(p, t, block_size, dtype), p.numel(), p.shape[2], p.shape[3], block_size)


def tv(img: Tensor, dtype: torch.dtype = torch.float64) -> Tensor:
    """``[B]`` in ``dtype``: per image the sum of ``|x[i + 1][j] − x[i][j]|`` and ``|x[i][j + 1] − x[i][j]|`` over ``C, H, W``."""
    x = img.detach().cpu().to(dtype)
    _, _, h, w = x.shape
    out = torch.zeros(x.shape[0], dtype=dtype)
    if h > 1:
        out = out + (x[:, :, 1:, :] - x[:, :, : h - 1, :]).abs().flatten(1).sum(1)
    if w > 1:
        out = out + (x[:, :, :, 1:] - x[:, :, :, : w - 1]).abs().flatten(1).sum(1)
    return out


def gradients(img: Tensor) -> Tuple[Tensor, Tensor]:
    """``(dy, dx)`` in the dtype of ``img``: zeros, then the differences written into all rows but the last and all columns but the last."""
    x = img.detach().cpu()
    dy, dx = torch.zeros_like(x), torch.zeros_like(x)
    dy[:, :, :-1, :] = x[:, :, 1:, :] - x[:, :, :-1, :]
    dx[:, :, :, :-1] = x[:, :, :, 1:] - x[:, :, :, :-1]
    return dy, dx


def planted_pair(shape: Tuple[int, ...], seed: int, scale: float, kind: str, block_size: int = 8) -> Tuple[Tensor, Tensor]:
    """``vif_oracle.noisy_pair`` with a planted answer to ``d_b > d_bc``.  ``"blocky"``: ``preds`` is the target plus one constant per
    ``block_size`` x ``block_size`` block (a fifth of the scale in amplitude), so the boundary pairs differ far more than the others.
    ``"unblocky"``: the second element of every boundary pair of ``preds`` is a copy of the first (columns, then rows), so ``D_B`` is 0."""
    from tests.helpers.vif_oracle import noisy_pair

    p, t = noisy_pair(shape, seed, scale)
    b, c, h, w = shape
    if kind == "blocky":
        g = torch.Generator().manual_seed(seed + 1)
        steps = torch.rand(b, c, -(-h // block_size), -(-w // block_size), generator=g) * 0.2 * scale
        p = t + steps.repeat_interleave(block_size, 2).repeat_interleave(block_size, 3)[:, :, :h, :w]
    elif kind == "unblocky":
        p = p.clone()
        for j in pair_lists(w, block_size)[0]:
            p[:, :, :, j + 1] = p[:, :, :, j]
        for i in pair_lists(h, block_size)[0]:
            p[:, :, i + 1, :] = p[:, :, i, :]
    else:
        raise ValueError(kind)
    return p, t
