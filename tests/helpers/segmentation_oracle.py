"""Independent oracle of the segmentation metrics: class-overlap counts by a per-pixel comparison loop over classes, and the three
scores evaluated from those counts in a given dtype (fp64 as the oracle).  Imports nothing from the package under test.

Definitions (per sample ``b``, class ``c``): ``I`` pixels in ``c`` on both sides, ``P`` in preds, ``T`` in target; ``sdiv(a, b) = a / b``
where ``b != 0`` else 0; ``include_background=False`` drops class 0.
"""
from typing import Optional, Sequence

import torch
from torch import Tensor

BOUND_REL, BOUND_ABS = 2.0**-24, 1e-12  # one fp32 rounding of an fp64 value, plus fp64 summation-order noise


def counts(preds: Tensor, target: Tensor, num_classes: int, input_format: str = "index") -> Tensor:
    """int64 ``[B, C, 3]`` on the CPU.  Index form: a pixel is in class ``c`` iff its label equals ``c``; one-hot: iff the mask is nonzero."""
    # widened first: a uint8 map compared with the Python integer 256 would wrap the integer, not widen the map
    p, t = preds.detach().cpu().to(torch.int64), target.detach().cpu().to(torch.int64)
    B = p.shape[0]
    out = torch.zeros(B, num_classes, 3, dtype=torch.int64)
    for c in range(num_classes):
        if input_format == "index":
            pm, tm = (p == c).reshape(B, -1), (t == c).reshape(B, -1)
        else:
            pm, tm = (p[:, c] != 0).reshape(B, -1), (t[:, c] != 0).reshape(B, -1)
        out[:, c, 0] = torch.logical_and(pm, tm).to(torch.int64).sum(1)
        out[:, c, 1] = pm.to(torch.int64).sum(1)
        out[:, c, 2] = tm.to(torch.int64).sum(1)
    return out


def _sdiv(a: Tensor, b: Tensor) -> Tensor:
    out = torch.zeros_like(a)
    nz = b != 0
    out[nz] = a[nz] / b[nz]
    return out


def _ipt(k: Tensor, include_background: bool, dtype: torch.dtype):
    k = k.cpu()[:, (0 if include_background else 1):].to(dtype)
    return k[..., 0], k[..., 1], k[..., 2]


def mean_iou(k: Tensor, include_background: bool = True, per_class: bool = False, dtype: torch.dtype = torch.float64) -> Tensor:
    i, p, t = _ipt(k, include_background, dtype)
    iou = _sdiv(i, p + t - i)
    return iou if per_class else iou.sum(1) / iou.shape[1]


def dice(k: Tensor, include_background: bool = True, average: Optional[str] = "micro", dtype: torch.dtype = torch.float64) -> Tensor:
    i, p, t = _ipt(k, include_background, dtype)
    d = _sdiv(2 * i, p + t)
    if average == "micro":
        return _sdiv((2 * i).sum(1), (p + t).sum(1))
    if average == "macro":
        return d.sum(1) / d.shape[1]
    if average == "weighted":
        return (_sdiv(t, t.sum(1, keepdim=True).expand_as(t).contiguous()) * d).sum(1)
    assert average in ("none", None), average
    return d


def generalized_dice(k: Tensor, include_background: bool = True, per_class: bool = False, weight_type: str = "square",
                     dtype: torch.dtype = torch.float64) -> Tensor:
    i, p, t = _ipt(k, include_background, dtype)
    if weight_type == "linear":
        w = torch.ones_like(t)
    else:
        w = 1.0 / (t * t if weight_type == "square" else t)  # inf where T == 0
        assert weight_type in ("square", "simple"), weight_type
        for b in range(w.shape[0]):  # a sample's replacement weight comes from its own classes alone
            fin = torch.isfinite(w[b])
            w[b][~fin] = w[b][fin].max() if bool(fin.any()) else 0.0
    if per_class:
        return _sdiv(2 * i * w, (p + t) * w)
    return _sdiv((2 * i * w).sum(1), ((p + t) * w).sum(1))


def within_bound(got: Tensor, want: Tensor, what: str = "") -> float:
    """Largest ``|got - want| / (2^-24 |want| + 1e-12)`` (<= 1 passes); prints one ratio line."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if got.numel() == 0:
        print(f"[segmentation] {what}: empty")
        return 0.0
    ratio = float(((got - want).abs() / (BOUND_REL * want.abs() + BOUND_ABS)).max())
    print(f"[segmentation] {what}: error / bound = {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------------------------------------------------ labels
def random_labels(shape: Sequence[int], num_classes: int, seed: int, dtype: torch.dtype = torch.int64) -> Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, num_classes, tuple(shape), generator=g).to(dtype)


def blocky_labels(shape: Sequence[int], num_classes: int, block: int, seed: int, dtype: torch.dtype = torch.int64) -> Tensor:
    """``[B, H, W]`` maps constant on ``block x block`` squares (the last row / column of squares may be cut)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, num_classes, (B, (H + block - 1) // block, (W + block - 1) // block), generator=g)
    return coarse.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :H, :W].contiguous().to(dtype)


def constant_labels(shape: Sequence[int], value: int, dtype: torch.dtype = torch.int64) -> Tensor:
    return torch.full(tuple(shape), value, dtype=dtype)


def plant(labels: Tensor, values: Sequence[int], seed: int, fraction: float = 0.1) -> Tensor:
    """A copy with about ``fraction`` of the pixels replaced by each of ``values`` in turn (out-of-range labels: -1, C, 255, the int64 limits)."""
    g = torch.Generator().manual_seed(seed)
    out = labels.clone()
    for v in values:
        out[torch.rand(out.shape, generator=g) < fraction] = v
    return out


def to_onehot(labels: Tensor, num_classes: int, dtype: torch.dtype = torch.bool) -> Tensor:
    """``[B, C, *spatial]`` masks of a label map by comparison: an out-of-range label is in no plane."""
    classes = torch.arange(num_classes).view(1, num_classes, *([1] * (labels.ndim - 1)))
    return (labels.unsqueeze(1).to(torch.int64) == classes).to(dtype)
