"""Autograd wrapper of the fused SSIM window kernel: ``tmx::ssim_sums`` forward, ``tmx::ssim_sums_backward`` backward.

The forward is the unchanged native op (value, and the fused-PSNR squared-error row where requested, are exactly what
a call without grad returns).  The backward runs the two gfx950 kernels of ``csrc/ssim_grad.hip``.  A second
derivative is not native: when grad mode is on inside ``backward`` (``create_graph=True``) the first-order gradients
are recomputed through the differentiable grouped-conv composition, so double backward keeps working.
"""
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor


def _composition_sums(p: Tensor, t: Tensor, w: Tensor, consts: Tensor) -> Tuple[Tensor, Tensor]:
    """Per-plane sums of SSIM and contrast sensitivity over the valid windows, as differentiable torch ops.

    ``p`` / ``t`` ``[P, H, W]``, ``w`` the 1-D window (``wy == wx``), ``consts`` ``(c1, c2, ...)`` on the device.  The valid
    (unpadded) convolution visits exactly the windows the reference keeps after cropping its reflect-padded output."""
    dtype = p.dtype if p.dtype in (torch.float32, torch.float64) else torch.float32
    p, t = p.to(dtype).unsqueeze(1), t.to(dtype).unsqueeze(1)
    w = w.to(dtype)
    c1, c2 = consts[0].to(dtype), consts[1].to(dtype)
    kernel = torch.outer(w, w)[None, None]
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel)
    mu_p, mu_t, e_pp, e_tt, e_pt = out.split(p.shape[0])
    mu_pp, mu_tt, mu_pt = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    upper = 2 * (e_pt - mu_pt) + c2
    lower = (e_pp - mu_pp) + (e_tt - mu_tt) + c2
    sim = ((2 * mu_pt + c1) * upper) / ((mu_pp + mu_tt + c1) * lower)
    return sim.double().sum((1, 2, 3)), (upper / lower).double().sum((1, 2, 3))


class SsimSums(torch.autograd.Function):
    """``SsimSums.apply(preds[P,H,W], target[P,H,W], w[KS], consts, with_sse) -> fp64 [2 | 3, P]`` (``tmx::ssim_sums``)."""

    @staticmethod
    def forward(ctx, preds: Tensor, target: Tensor, w: Tensor, consts: Tensor, with_sse: bool) -> Tensor:  # noqa: D102
        ctx.save_for_backward(preds, target, w, consts)
        return torch.ops.tmx.ssim_sums(preds, target, w, w, consts, with_sse)

    @staticmethod
    def backward(ctx, grad_sums: Tensor) -> Tuple[Optional[Tensor], ...]:  # noqa: D102
        preds, target, w, consts = ctx.saved_tensors
        need_p, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_p or need_t):
            return None, None, None, None, None
        # (a squared-error row, if any, is a by-product for the fused PSNR: it carries no gradient)
        g_sim, g_cs = grad_sums[0], grad_sums[1]
        if torch.is_grad_enabled():  # create_graph=True: first-order gradients with a graph, through the composition
            with torch.enable_grad():
                sim, cs = _composition_sums(preds, target, w, consts)
                wrt = [x for x, need in ((preds, need_p), (target, need_t)) if need]
                grads = list(torch.autograd.grad([sim, cs], wrt, [g_sim.to(sim.dtype), g_cs.to(cs.dtype)], create_graph=True))
            gp = grads.pop(0) if need_p else None
            gt = grads.pop(0) if need_t else None
            return gp, gt, None, None, None
        gp, gt = torch.ops.tmx.ssim_sums_backward(preds, target, w, w, consts, g_sim, g_cs, need_p, need_t)
        return (gp if need_p else None), (gt if need_t else None), None, None, None


def ssim_sums(preds: Tensor, target: Tensor, w: Tensor, consts: Tensor, with_sse: bool = False) -> Tensor:
    """Differentiable per-plane SSIM / contrast-sensitivity sums of the native kernel."""
    return SsimSums.apply(preds, target, w, consts, with_sse)


def ssim_tile() -> Tuple[int, int, int, int, int, int]:
    """Geometry of the three 2-D SSIM kernels: ``(output rows per block of the generic kernel, output rows per block of the packed-fp32
    kernel, output columns per block of both, rows and columns of an output tile of the matrix-core kernel, output columns per
    workgroup of that kernel, output rows per strip of that kernel)``."""
    rows, rows_v2, cols, tile, group_cols, strip = torch.ops.tmx.ssim_tile()
    return int(rows), int(rows_v2), int(cols), int(tile), int(group_cols), int(strip)


def ssim3d_sums(preds: Tensor, target: Tensor, wd: Tensor, wh: Tensor, ww: Tensor, consts: Tensor) -> Tensor:
    """``tmx::ssim3d_sums`` (``csrc/ssim3d.hip``): fp64 ``[2, P]`` per-volume sums of SSIM and contrast sensitivity over all
    valid windows of ``preds`` / ``target`` ``[P, D, H, W]``; ``wd`` / ``wh`` / ``ww`` the 1-D windows of the three axes, ``consts``
    ``(c1, c2)`` on the device.  No autograd: differentiable 5-D calls keep the composition."""
    return torch.ops.tmx.ssim3d_sums(preds, target, wd, wh, ww, consts)


def ssim3d_tile() -> Tuple[int, int, int]:
    """``(rows, columns)`` of the output footprint one workgroup of the 3-D SSIM kernel owns, and the smallest strip of
    output slices ``TMX_SSIM3D_STRIP`` can ask for."""
    th, tw, min_strip = torch.ops.tmx.ssim3d_tile()
    return int(th), int(tw), int(min_strip)


def vif_sums(preds: Tensor, target: Tensor, sigma_n_sq: float) -> Tensor:
    """``tmx::vif_sums`` (``csrc/vif.hip``): fp64 ``[4, 2, P]``, per scale and per plane of ``preds`` / ``target`` ``[P, H, W]`` the sums
    over all valid windows of the VIF-p numerator ``log10(1 + g² σt² / (σv² + σn²))`` and denominator ``log10(1 + σt² / σn²)``.
    fp32 / bf16 / fp16 planes of at least 41 x 41, ``sigma_n_sq > 0``.  No autograd: differentiable calls keep the composition."""
    return torch.ops.tmx.vif_sums(preds, target, float(sigma_n_sq))


def vif_tile() -> Tuple[int, int]:
    """``(rows, columns)`` of the output footprint one workgroup of the VIF scale kernel owns."""
    th, tw = torch.ops.tmx.vif_tile()
    return int(th), int(tw)


def uqi_sums(preds: Tensor, target: Tensor, wy: Tensor, wx: Tensor, eps: float) -> Tensor:
    """``tmx::uqi_sums`` (``csrc/uqi.hip``): fp64 ``[P]``, per plane of ``preds`` / ``target`` ``[P, H, W]`` the sum of the universal
    image quality index over all valid windows; ``wy`` / ``wx`` the fp32 1-D windows of the H / W axis (one odd size in 3 .. 15),
    ``eps`` the constant added to the variance term.  fp32 / bf16 / fp16.  No autograd: differentiable calls keep the composition."""
    return torch.ops.tmx.uqi_sums(preds, target, wy, wx, float(eps))


def uqi_band_pair_sums(x: Tensor, wy: Tensor, wx: Tensor, eps: float) -> Tensor:
    """``tmx::uqi_band_pair_sums`` (``csrc/uqi.hip``): fp64 ``[L (L − 1) / 2, B]``, for every band pair ``(i < j)`` of ``x`` ``[B, L, H, W]`` in
    ``torch.triu_indices(L, L, 1)`` order and every image the sum of the UQI between the two bands over all valid windows.  The
    bands are read in place (no gathered copies); ``L < 2`` gives an empty result.  No autograd."""
    return torch.ops.tmx.uqi_band_pair_sums(x, wy, wx, float(eps))


def uqi_tile() -> Tuple[int, int]:
    """``(output rows per strip, output columns per workgroup)`` of the UQI kernel."""
    rows, cols = torch.ops.tmx.uqi_tile()
    return int(rows), int(cols)


def box_rmse_maps(
    preds: Tensor, target: Tensor, window_size: int, crop: int, with_target_mean: bool = False
) -> Tuple[Tensor, Tensor, Tensor]:
    """``tmx::box_rmse_maps`` (``csrc/box_window.hip``): one fused kernel over ``preds`` / ``target`` ``[B, C, H, W]`` (fp32 / bf16 /
    fp16, read in place) with a ``window_size x window_size`` box window (2 .. 16, even or odd) on SciPy's edge-including symmetric
    padding.  Returns ``(rmse_map, crop_sums, target_mean)``: fp32 ``[C, H, W]`` the batch sum of ``sqrt(box mean of (t − p)²)``; fp64
    ``[C]`` the sum of the same per-image values over the pixels at least ``crop`` away from every edge; fp32 ``[C, H, W]`` the batch sum of
    ``(box mean of t) / window_size²`` when ``with_target_mean``, else an empty tensor.  ``crop`` is the caller's ``round(window_size / 2)``
    (banker's rounding); ``H`` and ``W`` must exceed ``2 crop``.  Deterministic, no host read.  No autograd."""
    return torch.ops.tmx.box_rmse_maps(preds, target, int(window_size), int(crop), bool(with_target_mean))


def rase_fold(rmse_map: Tensor, target_sum: Tensor, total_images: Tensor, crop: int) -> Tensor:
    """``tmx::rase_fold`` (``csrc/box_window.hip``): the relative average spectral error of the accumulated ``[C, H, W]`` maps as an fp64
    device scalar: the mean over the pixels at least ``crop`` away from every edge of
    ``100 / mean_c(target_sum / n) · sqrt(mean_c((rmse_map / n)²))`` with ``n = total_images`` (a one-element device tensor, read in the
    kernel), in fp64 arithmetic."""
    return torch.ops.tmx.rase_fold(rmse_map, target_sum, total_images, int(crop))


def box_tile() -> Tuple[int, int]:
    """``(output rows per strip, output columns per workgroup)`` of the box-window kernel."""
    rows, cols = torch.ops.tmx.box_tile()
    return int(rows), int(cols)


def box_batch_chunks(b: int, c: int, h: int, w: int) -> int:
    """How many batch chunks ``box_rmse_maps`` puts on the grid for a ``[b, c, h, w]`` call (a function of the shape alone).  Chunk
    ``k`` holds the images ``k · ceil(b / chunks) ..``; each chunk adds its images in order and the chunks are added in order."""
    return int(torch.ops.tmx.box_batch_chunks(int(b), int(c), int(h), int(w)))


def sam_map(preds: Tensor, target: Tensor) -> Tensor:
    """``tmx::sam_map`` (``csrc/spectral.hip``): fp32 ``[B, H, W]``, per pixel of ``preds`` / ``target`` ``[B, C, H, W]`` (``C >= 2``; fp32 / bf16 /
    fp16, read in place, once) the spectral angle ``acos(clamp(<p,t> / (|p| |t|), -1, 1))`` of the two band vectors.  The three sums run
    over the bands in band order in fp64 and the cosine is formed in fp64, so bit-identical non-zero vectors give exactly 0; a zero
    vector gives NaN in its pixel.  16-bit inputs give the bits of their fp32 up-cast.  No autograd."""
    return torch.ops.tmx.sam_map(preds, target)


def sam_sums(preds: Tensor, target: Tensor) -> Tensor:
    """``tmx::sam_sums`` (``csrc/spectral.hip``): fp64 ``[B]``, per image the sum of the fp32 angles ``sam_map`` would store, without
    writing the map: one fp64 partial per workgroup, added per image in a fixed order (no atomics: two runs are bit-equal).  A NaN
    angle stays in its image's sum.  No host read.  No autograd."""
    return torch.ops.tmx.sam_sums(preds, target)


def ergas_scores(preds: Tensor, target: Tensor, ratio: float) -> Tensor:
    """``tmx::ergas_scores`` (``csrc/spectral.hip``): fp64 ``[B]``, per image of ``preds`` / ``target`` ``[B, C, H, W]`` (fp32 / bf16 / fp16, read
    in place, once) ``100 · ratio · sqrt(mean_c((SSE_bc / HW) / mean_t_bc²))`` with ``SSE`` the plane sum of ``(p − t)²`` and ``mean_t`` the plane
    mean of ``target``.  Short fp32 vector sums added in fp64; the planes are split into ``ergas_chunks`` chunks on the grid and the
    partials added in chunk order (deterministic).  A band whose target mean is 0 gives inf or NaN.  No host read.  No autograd."""
    return torch.ops.tmx.ergas_scores(preds, target, float(ratio))


def ergas_chunks(b: int, c: int, h: int, w: int) -> int:
    """How many chunks ``ergas_scores`` splits every plane of a ``[b, c, h, w]`` call into (a function of the shape alone).  Only the
    last chunk of a plane may be short."""
    return int(torch.ops.tmx.ergas_chunks(int(b), int(c), int(h), int(w)))


def spectral_tile() -> Tuple[int, int]:
    """``(fp32 pixels per workgroup of the SAM kernels, least elements per ERGAS chunk)``; 16-bit inputs take twice the pixels."""
    pixels, elements = torch.ops.tmx.spectral_tile()
    return int(pixels), int(elements)


def psnrb_sums(preds: Tensor, target: Tensor, block_size: int) -> Tensor:
    """``tmx::psnrb_sums`` (``csrc/neighbour_diff.hip``): fp64 ``[5]`` = ``Σ(p − t)²``, ``D_B``, ``D_BC``, ``min target``, ``max target`` over the whole
    ``[B, 1, H, W]`` batch (fp32 / bf16 / fp16, each input read in place, once).  ``D_B`` is the sum of the squared differences of ``preds``
    over the horizontal pairs ``(j, j + 1)`` with ``(j + 1) % block_size == 0`` and the vertical pairs ``(i, i + 1)`` with ``(i + 1) % block_size == 0``,
    ``D_BC`` the same over every other pair; an empty set adds 0.  The differences are fp32, their squares are added in fp64: one
    partial per workgroup, added in a fixed order (no atomics: two runs are bit-equal).  Minimum and maximum give NaN where
    ``target`` holds one.  16-bit inputs give the bits of their fp32 up-cast.  No host read.  No autograd."""
    return torch.ops.tmx.psnrb_sums(preds, target, int(block_size))


def tv_sums(img: Tensor) -> Tensor:
    """``tmx::tv_sums`` (``csrc/neighbour_diff.hip``): fp64 ``[B]``, per image of ``img`` ``[B, C, H, W]`` (fp32 / bf16 / fp16, read in place, once)
    ``Σ|x[i + 1][j] − x[i][j]| + Σ|x[i][j + 1] − x[i][j]|`` over ``C, H, W``: fp32 differences, their absolute values added in fp64, one partial per
    workgroup, an image's partials added in a fixed order (deterministic).  No host read.  No autograd."""
    return torch.ops.tmx.tv_sums(img)


def image_gradients(img: Tensor) -> Tuple[Tensor, Tensor]:
    """``tmx::image_gradients`` (``csrc/neighbour_diff.hip``): ``(dy, dx)`` in the dtype and shape of ``img`` ``[B, C, H, W]`` (fp32 / bf16 / fp16, read in
    place, once): ``dy[i][j] = x[i + 1][j] − x[i][j]`` and ``dx[i][j] = x[i][j + 1] − x[i][j]``, one fp32 subtraction rounded once to the dtype (the bits of
    the composition); the last row of ``dy`` and the last column of ``dx`` are stored as zeros by the same kernel.  No autograd."""
    dy, dx = torch.ops.tmx.image_gradients(img)
    return dy, dx


def gradient_tile() -> Tuple[int, int]:
    """``(fp32 columns per workgroup of the neighbour-difference kernels, rows per strip)``; 16-bit inputs take twice the columns."""
    columns, rows = torch.ops.tmx.gradient_tile()
    return int(columns), int(rows)
