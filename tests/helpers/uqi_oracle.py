"""CPU oracle of the universal image quality index, written from the definition with the dense 2-D window.

``uqi_sums`` returns what ``tmx::uqi_sums`` returns (per plane pair the sum of the index over all valid windows):
``oracle64`` with everything in fp64, the window included, and ``comp32`` with the same arithmetic in fp32 and the per-window
values added in fp64 -- the measure of what fp32 window arithmetic itself loses.  ``band_pair_sums`` is the same on explicitly
gathered band pairs, in the layout of ``tmx::uqi_band_pair_sums``.  The bound every native result is held to is
``tests.helpers.vif_oracle.value_rule``.
"""
from typing import Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor


def window_1d(kernel_size: int, sigma: float, dtype: torch.dtype) -> Tensor:
    """Normalised 1-D Gaussian ``[kernel_size]``."""
    d = torch.arange(kernel_size, dtype=dtype) - (kernel_size - 1) / 2
    g = torch.exp(-((d / sigma) ** 2) / 2)
    return g / g.sum()


def uqi_sums(a: Tensor, b: Tensor, kernel_size: Sequence[int], sigma: Sequence[float], eps: float,
             dtype: torch.dtype = torch.float64) -> Tensor:
    """``a`` / ``b`` ``[P, H, W]`` -> fp64 ``[P]``: the sum over the valid windows of
    ``(2 m0 m1) · 2 (m4 − m0 m1) / ((m0² + m1²) · ((m2 − m0²) + (m3 − m1²) + eps))`` computed in ``dtype``; ``kernel_size[0]`` /
    ``sigma[0]`` weigh the H axis."""
    a, b = a.detach().cpu().to(dtype)[:, None], b.detach().cpu().to(dtype)[:, None]
    k = torch.outer(window_1d(kernel_size[0], sigma[0], dtype), window_1d(kernel_size[1], sigma[1], dtype))[None, None]
    m0, m1, m2, m3, m4 = (F.conv2d(x, k) for x in (a, b, a * a, b * b, a * b))
    upper = 2 * (m4 - m0 * m1)
    lower = (m2 - m0 * m0) + (m3 - m1 * m1) + torch.tensor(eps, dtype=dtype)
    uqi = (2 * m0 * m1) * upper / ((m0 * m0 + m1 * m1) * lower)
    return uqi.double().sum((1, 2, 3))


def gather_band_pairs(x: Tensor) -> Tuple[Tensor, Tensor]:
    """``x`` ``[B, L, H, W]`` -> the two planes of every (band pair, image), ``[L (L − 1) / 2 · B, H, W]`` each, pair-major, pairs
    ``(i < j)`` in row-major order of the strict upper triangle."""
    bsz, length = x.shape[:2]
    first, second = [], []
    for i in range(length):
        for j in range(i + 1, length):
            for n in range(bsz):
                first.append(x[n, i])
                second.append(x[n, j])
    return torch.stack(first), torch.stack(second)


def band_pair_sums(x: Tensor, kernel_size: Sequence[int], sigma: Sequence[float], eps: float,
                   dtype: torch.dtype = torch.float64) -> Tensor:
    """``x`` ``[B, L, H, W]`` (``L >= 2``) -> fp64 ``[L (L − 1) / 2, B]``."""
    a, b = gather_band_pairs(x.detach().cpu())
    return uqi_sums(a, b, kernel_size, sigma, eps, dtype).reshape(-1, x.shape[0])


def band_matrix(pair_sums: Tensor, length: int, count: int) -> Tensor:
    """``[npairs, B]`` sums -> the symmetric fp64 ``[L, L]`` matrix of mean UQI (zero diagonal); ``count`` = ``B · Hv · Wv``."""
    m = torch.zeros(length, length, dtype=torch.float64)
    i, j = torch.triu_indices(length, length, offset=1)
    m[i, j] = pair_sums.double().sum(1) / count
    return m + m.T


def d_lambda(m_preds: Tensor, m_target: Tensor, p: int) -> Tensor:
    """The spectral distortion index of two band matrices."""
    length = m_preds.shape[0]
    return ((m_target - m_preds).abs() ** p).sum().div(length * (length - 1)) ** (1.0 / p)
