"""CPU oracle of the sliding-window RMSE and the relative average spectral error, written from the definition and independent
of ``_uniform_filter``: ``numpy.pad(mode="symmetric")`` by ``(ws // 2, (ws − 1) // 2)`` on both image axes, the dense ``ws x ws`` box as
``ws²`` shifted adds, one division by ``ws²``, the square root, the batch sum.

``box_outputs`` returns what ``tmx::box_rmse_maps`` returns plus the RASE scalar of the same call, in fp64 as the oracle or in fp32
as the measure of what fp32 arithmetic itself loses (``comp32`` of ``vif_oracle.value_rule``).  In the fp32 variant every step up to
the per-image value is fp32; ``crop_sums`` adds those fp32 values in fp64, as the kernel is specified to.
"""
from typing import Tuple

import numpy as np
import torch
from torch import Tensor


def crop_of(ws: int) -> int:
    """Python's ``round(ws / 2)``: banker's rounding, so 3 -> 2, 5 -> 2, 7 -> 4, 9 -> 4."""
    return round(ws / 2)


def box_sum(x: np.ndarray, ws: int) -> np.ndarray:
    """``[..., H, W]`` -> the sum over the ``ws x ws`` window of every pixel on the symmetric padding, in ``x``'s dtype."""
    front, back = ws // 2, (ws - 1) // 2
    pad = [(0, 0)] * (x.ndim - 2) + [(front, back), (front, back)]
    xp = np.pad(x, pad, mode="symmetric")
    h, w = x.shape[-2:]
    out = np.zeros_like(x)
    for dy in range(ws):
        for dx in range(ws):
            out = out + xp[..., dy:dy + h, dx:dx + w]
    return out


def rase_from_maps(rmse_map: np.ndarray, target_sum: np.ndarray, n: float, ws: int) -> np.ndarray:
    """``_rase_compute`` on ``[C, H, W]`` maps in the maps' dtype."""
    crop = crop_of(ws)
    dt = rmse_map.dtype.type
    mean_t = (target_sum / dt(n)).mean(0)
    rase_map = dt(100) / mean_t * np.sqrt(((rmse_map / dt(n)) ** 2).mean(0))
    return rase_map[crop:-crop, crop:-crop].mean()


def box_outputs(preds: Tensor, target: Tensor, ws: int, dtype: torch.dtype = torch.float64) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``preds`` / ``target`` ``[B, C, H, W]`` -> ``(rmse_map [C, H, W], crop_sums [C] fp64, target_mean [C, H, W], rase scalar)``."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    p = preds.detach().cpu().double().numpy().astype(np_dtype)
    t = target.detach().cpu().double().numpy().astype(np_dtype)
    area = np_dtype(ws * ws)
    d = t - p
    r = np.sqrt(box_sum(d * d, ws) / area)  # [B, C, H, W]
    m = box_sum(t, ws) / area / area
    rmse_map, target_mean = r[0].copy(), m[0].copy()
    for b in range(1, r.shape[0]):  # sequential batch sum in the working dtype
        rmse_map = rmse_map + r[b]
        target_mean = target_mean + m[b]
    crop = crop_of(ws)
    crop_sums = r.astype(np.float64)[:, :, crop:-crop, crop:-crop].sum((0, 2, 3))
    rase = rase_from_maps(rmse_map, target_mean, r.shape[0], ws)
    return torch.from_numpy(rmse_map), torch.from_numpy(crop_sums), torch.from_numpy(target_mean), torch.tensor(rase)
