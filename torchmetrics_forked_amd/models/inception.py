"""Inception-v3 feature extractor in the FID ("inception-v3-compat") layout used by FID / KID / IS / MiFID.

Input: uint8 images ``[N, 3, H, W]`` in [0, 255]; resized bilinearly to 299×299, scaled to [-1, 1).  Returns the
requested taps (``'64'``, ``'192'``, ``'768'``, ``'2048'``, ``'logits_unbiased'``, ``'logits'``).  Random init by
default; pass ``weights_path`` to load a compatible state dict (loaded with ``weights_only=True``).

On the GPU, with fp32 weights and no autograd graph, the 89 stride-1 convolutions run as ``tmx::conv_bn_relu`` (split-f16 matrix-core
products with the batch norm folded into the packed weights, ``csrc/conv_taps.hip``) on channels_last maps, and the branches of a Mixed
block write into one block tensor; the five stride-2 convolutions, the pools and every other call keep ``nn.Conv2d``.  The images
are always resized and scaled in fp32; a trunk moved to another precision gets them cast to it after that step."""
import os
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops import image as image_ops

# The trunk's stride-1 convolutions on the split-f16 matrix-core kernels (csrc/conv_taps.hip) instead of MIOpen's fp32 ones;
# TMX_INCEPTION_TRUNK_NATIVE=0 keeps MIOpen.  Per-layer figures: profiles/inception_trunk_bench.json (tools/inception_trunk_bench.py)
_TRUNK_NATIVE = os.environ.get("TMX_INCEPTION_TRUNK_NATIVE", "1") != "0"


class BasicConv2d(nn.Module):
    def __init__(self, c_in: int, c_out: int, **kwargs) -> None:  # noqa: ANN003
        super().__init__()
        self.conv = nn.Conv2d(c_in, c_out, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(c_out, eps=0.001)

    def forward(self, x: Tensor) -> Tensor:
        return F.relu(self.bn(self.conv(x)), inplace=True)


class InceptionA(nn.Module):
    def __init__(self, c_in: int, pool_features: int) -> None:
        super().__init__()
        self.branch1x1 = BasicConv2d(c_in, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(c_in, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(c_in, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(c_in, pool_features, kernel_size=1)

    def forward(self, x: Tensor) -> Tensor:
        b1 = self.branch1x1(x)
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False))
        return torch.cat([b1, b5, b3, bp], 1)


class InceptionB(nn.Module):
    def __init__(self, c_in: int) -> None:
        super().__init__()
        self.branch3x3 = BasicConv2d(c_in, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(c_in, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x: Tensor) -> Tensor:
        b3 = self.branch3x3(x)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, c_in: int, c7: int) -> None:
        super().__init__()
        self.branch1x1 = BasicConv2d(c_in, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(c_in, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(c_in, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(c_in, 192, kernel_size=1)

    def forward(self, x: Tensor) -> Tensor:
        b1 = self.branch1x1(x)
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = x
        for m in (self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            bd = m(bd)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False))
        return torch.cat([b1, b7, bd, bp], 1)


class InceptionD(nn.Module):
    def __init__(self, c_in: int) -> None:
        super().__init__()
        self.branch3x3_1 = BasicConv2d(c_in, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(c_in, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x: Tensor) -> Tensor:
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, c_in: int, pool: str) -> None:
        super().__init__()
        self.pool = pool
        self.branch1x1 = BasicConv2d(c_in, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(c_in, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(c_in, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(c_in, 192, kernel_size=1)

    def forward(self, x: Tensor) -> Tensor:
        b1 = self.branch1x1(x)
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        if self.pool == "avg":
            bp = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)
        else:
            bp = F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
        return torch.cat([b1, b3, bd, self.branch_pool(bp)], 1)


_NATIVE_TAPS = {(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1)}


def _native_layer(conv: nn.Conv2d, h: int, w: int) -> bool:
    """Whether a layer of the native trunk runs ``tmx::conv_bn_relu``: what the kernels serve (stride 1, their tap shapes, padding none
    or same, channel counts in multiples of 16).  A class of (taps, C_in, C_out, plane ``h`` x ``w``) that measures slower than MIOpen
    is sent back to ``nn.Conv2d`` here (``profiles/inception_trunk_bench.json``; none so far)."""
    kh, kw = conv.kernel_size
    return (
        conv.stride == (1, 1)
        and conv.dilation == (1, 1)
        and conv.groups == 1
        and conv.bias is None
        and (kh, kw) in _NATIVE_TAPS
        and conv.padding in ((0, 0), ((kh - 1) // 2, (kw - 1) // 2))
        and conv.in_channels % 16 == 0
        and conv.out_channels % 16 == 0
    )


def _branches(m: nn.Module) -> List[Tuple[Optional[str], List[BasicConv2d], List[BasicConv2d]]]:
    """The branches of a Mixed block in the order of its ``torch.cat``: ``(pool of the block input or None, chain of layers, layers
    that each read the chain's result and write the next channels of the block)``."""
    if isinstance(m, InceptionA):
        return [(None, [], [m.branch1x1]), (None, [m.branch5x5_1], [m.branch5x5_2]),
                (None, [m.branch3x3dbl_1, m.branch3x3dbl_2], [m.branch3x3dbl_3]), ("avg", [], [m.branch_pool])]
    if isinstance(m, InceptionB):
        return [(None, [], [m.branch3x3]), (None, [m.branch3x3dbl_1, m.branch3x3dbl_2], [m.branch3x3dbl_3])]
    if isinstance(m, InceptionC):
        return [(None, [], [m.branch1x1]), (None, [m.branch7x7_1, m.branch7x7_2], [m.branch7x7_3]),
                (None, [m.branch7x7dbl_1, m.branch7x7dbl_2, m.branch7x7dbl_3, m.branch7x7dbl_4], [m.branch7x7dbl_5]),
                ("avg", [], [m.branch_pool])]
    if isinstance(m, InceptionD):
        return [(None, [m.branch3x3_1], [m.branch3x3_2]),
                (None, [m.branch7x7x3_1, m.branch7x7x3_2, m.branch7x7x3_3], [m.branch7x7x3_4])]
    return [(None, [], [m.branch1x1]), (None, [m.branch3x3_1], [m.branch3x3_2a, m.branch3x3_2b]),
            (None, [m.branch3x3dbl_1, m.branch3x3dbl_2], [m.branch3x3dbl_3a, m.branch3x3dbl_3b]), (m.pool, [], [m.branch_pool])]


class FeatureExtractorInceptionV3(nn.Module):
    INPUT_IMAGE_SIZE = 299
    FEATURES = ("64", "192", "768", "2048", "logits_unbiased", "logits")

    def __init__(self, features_list: Sequence[str] = ("2048",), weights_path: Optional[str] = None, num_classes: int = 1008) -> None:
        super().__init__()
        for f in features_list:
            if f not in self.FEATURES:
                raise ValueError(f"Unknown feature tap {f}; expected one of {self.FEATURES}")
        self.features_list = [str(f) for f in features_list]
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.MaxPool_1 = nn.MaxPool2d(kernel_size=3, stride=2)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.MaxPool_2 = nn.MaxPool2d(kernel_size=3, stride=2)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, c7=128)
        self.Mixed_6c = InceptionC(768, c7=160)
        self.Mixed_6d = InceptionC(768, c7=160)
        self.Mixed_6e = InceptionC(768, c7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, pool="avg")
        self.Mixed_7c = InceptionE(2048, pool="max")
        self.AvgPool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, num_classes)
        if weights_path is not None:
            self.load_state_dict(torch.load(weights_path, map_location="cpu", weights_only=True))
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)

    def train(self, mode: bool = True) -> "FeatureExtractorInceptionV3":
        return super().train(False)

    def _native_trunk_ok(self, x: Tensor) -> bool:
        """The trunk on ``tmx::conv_bn_relu``: a GPU input, fp32 weights on its device, no autograd graph being recorded."""
        w = self.Conv2d_1a_3x3.conv.weight
        if not (_TRUNK_NATIVE and x.is_cuda and x.numel() and w.dtype == torch.float32 and w.device == x.device):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return ops.use_native(x)

    def _conv_native(self, m: BasicConv2d, x: Tensor, ax: Optional[Tensor], out: Optional[Tensor] = None,
                     omax: Optional[Tensor] = None, c_off: int = 0) -> Tuple[Tensor, Tensor]:
        """``relu(bn(conv(x)))`` of one layer into channels ``[c_off, ...)`` of ``out`` (its own tensor when ``None``); ``ax`` / ``omax`` are
        the per-image maxima of ``x`` / ``out`` (``ax`` ``None``: not known, reduced here).  Returns ``(out, omax)``.  Stride-2 layers and
        the classes ``_native_layer`` sends back keep ``nn.Conv2d``; the packed planes are cached per layer under the
        ``(data_ptr, _version)`` of the conv weight and the four batch-norm tensors."""
        conv, bn = m.conv, m.bn
        if not _native_layer(conv, x.shape[2], x.shape[3]):
            y = m(x)
            ymax = torch.ops.tmx.conv3x3_absmax(y)
            if out is None:
                return y, ymax
            out[:, c_off : c_off + y.shape[1]] = y
            torch.maximum(omax, ymax, out=omax)
            return out, omax
        tensors = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        entry = m.__dict__.get("_planes")  # (kept on the layer itself, so a copied trunk replaces what it copied)
        if entry is None or entry[0] != key:
            entry = m.__dict__["_planes"] = (key, *image_ops.pack_conv_bn_weights(*tensors, bn.eps))
        return image_ops.conv_bn_relu(x, entry[1], entry[2], entry[3], conv.kernel_size, conv.padding, ax, out, omax, c_off)

    def _mixed_native(self, m: nn.Module, x: Tensor, ax: Tensor) -> Tuple[Tensor, Tensor]:
        """One Mixed block: its output block is allocated once and every branch's last layer writes its own channel range of it, each
        launch folding its per-image maximum into the block's one buffer (a pool cannot raise a maximum, so a pooled input keeps
        ``ax``).  The reducing blocks (6a, 7a) copy their max-pool branch into the last channels."""
        reducing = isinstance(m, (InceptionB, InceptionD))
        branches = _branches(m)
        h, w = ((x.shape[2] - 3) // 2 + 1, (x.shape[3] - 3) // 2 + 1) if reducing else x.shape[2:]
        width = sum(t.conv.out_channels for _, _, tails in branches for t in tails) + (x.shape[1] if reducing else 0)
        out = torch.empty((x.shape[0], width, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        omax = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
        off = 0
        for pool, chain, tails in branches:
            y, ay = x, ax
            if pool is not None:
                y = (F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) if pool == "avg" else F.max_pool2d(x, 3, 1, 1))
            for layer in chain:
                y, ay = self._conv_native(layer, y, ay)
            for layer in tails:
                self._conv_native(layer, y, ay, out, omax, off)
                off += layer.conv.out_channels
        if reducing:
            out[:, off:] = F.max_pool2d(x, kernel_size=3, stride=2)
            torch.maximum(omax, ax, out=omax)
        return out, omax

    def _taps_native(self, x: Tensor) -> Tuple[Tensor, ...]:
        """``_taps`` with every stride-1 convolution run by ``tmx::conv_bn_relu`` (``csrc/conv_taps.hip``) on channels_last fp32 maps:
        batch norm folded into the packed weights, the Mixed blocks written in place of ``torch.cat``, the pooled taps as means over
        H and W.  The five stride-2 convolutions and the pools stay ATen calls on the same channels_last tensors."""
        want = set(self.features_list)
        out = {}
        x = F.interpolate(x.float(), size=(self.INPUT_IMAGE_SIZE, self.INPUT_IMAGE_SIZE), mode="bilinear", align_corners=False)
        x = ((x - 128) / 128).contiguous(memory_format=torch.channels_last)
        x, ax = self._conv_native(self.Conv2d_1a_3x3, x, None)
        x, ax = self._conv_native(self.Conv2d_2a_3x3, x, ax)
        x, ax = self._conv_native(self.Conv2d_2b_3x3, x, ax)
        x = self.MaxPool_1(x)
        if "64" in want:
            out["64"] = x.mean((2, 3))
        x, ax = self._conv_native(self.Conv2d_3b_1x1, x, ax)
        x, ax = self._conv_native(self.Conv2d_4a_3x3, x, ax)
        x = self.MaxPool_2(x)
        if "192" in want:
            out["192"] = x.mean((2, 3))
        for m in (self.Mixed_5b, self.Mixed_5c, self.Mixed_5d, self.Mixed_6a, self.Mixed_6b, self.Mixed_6c, self.Mixed_6d,
                  self.Mixed_6e):
            x, ax = self._mixed_native(m, x, ax)
        if "768" in want:
            out["768"] = x.mean((2, 3))
        for m in (self.Mixed_7a, self.Mixed_7b, self.Mixed_7c):
            x, ax = self._mixed_native(m, x, ax)
        out["2048"] = x = x.mean((2, 3))
        if "logits_unbiased" in want or "logits" in want:
            lu = x.mm(self.fc.weight.T)
            out["logits_unbiased"] = lu
            out["logits"] = lu + self.fc.bias.unsqueeze(0)
        return tuple(out[f] for f in self.features_list)

    def _taps(self, x: Tensor) -> Tuple[Tensor, ...]:
        if self._native_trunk_ok(x):
            return self._taps_native(x)
        want = set(self.features_list)
        out = {}
        x = x.float()
        x = F.interpolate(x, size=(self.INPUT_IMAGE_SIZE, self.INPUT_IMAGE_SIZE), mode="bilinear", align_corners=False)
        x = ((x - 128) / 128).to(self.Conv2d_1a_3x3.conv.weight.dtype)  # (fp32 unless the module was moved to another precision)
        x = self.MaxPool_1(self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x))))
        if "64" in want:
            out["64"] = F.adaptive_avg_pool2d(x, 1).flatten(1)
        x = self.MaxPool_2(self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x)))
        if "192" in want:
            out["192"] = F.adaptive_avg_pool2d(x, 1).flatten(1)
        for m in (self.Mixed_5b, self.Mixed_5c, self.Mixed_5d, self.Mixed_6a, self.Mixed_6b, self.Mixed_6c, self.Mixed_6d,
                  self.Mixed_6e):
            x = m(x)
        if "768" in want:
            out["768"] = F.adaptive_avg_pool2d(x, 1).flatten(1)
        x = torch.flatten(self.AvgPool(self.Mixed_7c(self.Mixed_7b(self.Mixed_7a(x)))), 1)
        out["2048"] = x
        if "logits_unbiased" in want or "logits" in want:
            lu = x.mm(self.fc.weight.T)
            out["logits_unbiased"] = lu
            out["logits"] = lu + self.fc.bias.unsqueeze(0)
        return tuple(out[f] for f in self.features_list)

    def forward(self, x: Tensor) -> Tensor:
        if x.dtype != torch.uint8:
            raise ValueError("Expecting image as torch.Tensor with dtype=torch.uint8")
        return self._taps(x)[0].reshape(x.shape[0], -1)
