"""``tmx::conv_bn_relu`` (split-f16 matrix-core convolutions with folded batch norm, ``csrc/conv_taps.hip``) and the Inception-v3 trunk of
FID / KID built on it, against plain fp64 torch.

Value rule: ``max|native - oracle| <= 4 err_comp32 + 1e-6 max|oracle|``, ``err_comp32`` the error of the fp32 composition every call took
before (``conv2d`` + ``batch_norm`` + ``relu`` on the GPU) against the same fp64 oracle.  The end-to-end test needs the kernels and the
gate and fails without them.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.image import FrechetInceptionDistance, KernelInceptionDistance
from torchmetrics_forked_amd.models.inception import FeatureExtractorInceptionV3
from torchmetrics_forked_amd.ops import image as image_ops

pytestmark = pytest.mark.gpu
CL = torch.channels_last
EPS = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _within(native, comp32, oracle):
    err, err32 = (native.double() - oracle).abs().max().item(), (comp32.double() - oracle).abs().max().item()
    bound = 4 * err32 + 1e-6 * oracle.abs().max().item()
    print(f"err_native {err:.3e} err_comp32 {err32:.3e} bound {bound:.3e}")
    assert err <= bound, (err, err32, bound)


def _layer(kh, kw, c_in, c_out, b, h, w, scale=1.0):
    """Input, weight and non-trivial batch-norm vectors (gamma, beta, mean, var) of one layer."""
    g = torch.Generator().manual_seed(kh + 3 * kw + c_in + 7 * h)
    x = (torch.randn(b, c_in, h, w, generator=g) * scale).cuda().contiguous(memory_format=CL)
    wt = (torch.randn(c_out, c_in, kh, kw, generator=g) / (kh * kw * c_in) ** 0.5).cuda()
    bn = [(torch.rand(c_out, generator=g) + 0.5).cuda(), (torch.randn(c_out, generator=g) * 0.5).cuda(),
          (torch.randn(c_out, generator=g) * 0.5 * scale).cuda(), ((torch.rand(c_out, generator=g) * 1.5 + 0.5) * scale * scale).cuda()]
    return x, wt, bn


CASES = [
    # taps, same padding, C_in, C_out, B, H, W
    ((1, 1), False, 64, 80, 3, 5, 7),  # an M tile spans images; C_out no multiple of 64
    ((1, 1), False, 80, 192, 1, 1, 1),  # padded last slice
    ((1, 1), False, 2048, 320, 2, 8, 8),  # deep K
    ((3, 3), False, 32, 32, 1, 9, 17),
    ((3, 3), True, 96, 96, 2, 17, 17),
    ((5, 5), True, 48, 64, 2, 9, 17),  # padded slice plus the widest halo
    ((1, 7), True, 160, 160, 1, 17, 17),
    ((7, 1), True, 128, 192, 1, 17, 17),
    ((1, 3), True, 384, 384, 1, 8, 8),  # the 64-slot patch
    ((3, 1), True, 384, 384, 1, 8, 8),
    ((3, 3), True, 448, 384, 2, 8, 8),
    ((3, 3), True, 64, 128, 5, 35, 35),  # the 128-channel tile (more than 512 workgroups), several patches per plane
    # planes smaller than the window along an axis
    ((3, 3), True, 16, 16, 2, 1, 2),
    ((5, 5), True, 16, 16, 1, 3, 2),
    ((1, 7), True, 16, 32, 2, 2, 3),
    ((7, 1), True, 16, 16, 1, 3, 2),
    ((1, 3), True, 32, 16, 1, 2, 1),
    ((3, 1), True, 16, 16, 1, 2, 2),
]


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("taps, same, c_in, c_out, b, h, w", CASES)
def test_op_against_fp64(taps, same, c_in, c_out, b, h, w, scale):
    pad = ((taps[0] - 1) // 2, (taps[1] - 1) // 2) if same else (0, 0)
    x, wt, bn = _layer(*taps, c_in, c_out, b, h, w, scale)
    gamma, beta, mean, var = (t.double().reshape(1, -1, 1, 1) for t in bn)
    oracle = F.relu((F.conv2d(x.double(), wt.double(), padding=pad) - mean) * gamma / (var + EPS).sqrt() + beta)
    comp32 = F.relu(F.batch_norm(F.conv2d(x, wt, padding=pad), bn[2], bn[3], bn[0], bn[1], False, 0.0, EPS))
    y, ymax = image_ops.conv_bn_relu(x, *image_ops.pack_conv_bn_weights(wt, *bn, EPS), taps, pad)
    assert y.shape == oracle.shape and y.is_contiguous(memory_format=CL)
    _within(y, comp32, oracle)
    assert torch.equal(ymax, y.amax((1, 2, 3)))  # the maximum the next layer scales by


def test_channel_offset_into_a_shared_block():
    sentinel = -7.0
    block = torch.full((2, 176, 9, 17), sentinel).cuda().contiguous(memory_format=CL)
    bmax = torch.zeros(2).cuda()
    for taps, c_out, off in (((1, 1), 96, 16), ((3, 3), 48, 112)):
        pad = ((taps[0] - 1) // 2, (taps[1] - 1) // 2)
        x, wt, bn = _layer(*taps, 64, c_out, 2, 9, 17)
        gamma, beta, mean, var = (t.double().reshape(1, -1, 1, 1) for t in bn)
        oracle = F.relu((F.conv2d(x.double(), wt.double(), padding=pad) - mean) * gamma / (var + EPS).sqrt() + beta)
        comp32 = F.relu(F.batch_norm(F.conv2d(x, wt, padding=pad), bn[2], bn[3], bn[0], bn[1], False, 0.0, EPS))
        image_ops.conv_bn_relu(x, *image_ops.pack_conv_bn_weights(wt, *bn, EPS), taps, pad, None, block, bmax, off)
        _within(block[:, off : off + c_out], comp32, oracle)
    assert (block[:, :16] == sentinel).all() and (block[:, 160:] == sentinel).all()
    assert torch.equal(bmax, block[:, 16:160].amax((1, 2, 3)))


def test_pointwise_scale_is_per_row():
    x, wt, bn = _layer(1, 1, 64, 80, 2, 5, 7)  # 70 pixels: one M tile holds both images
    x[0] *= 1e-3
    x[1] *= 1e3
    packed = image_ops.pack_conv_bn_weights(wt, *bn, EPS)
    y, ymax = image_ops.conv_bn_relu(x, *packed, (1, 1))
    for i in range(2):
        assert torch.equal(y[i : i + 1], image_ops.conv_bn_relu(x[i : i + 1].contiguous(memory_format=CL), *packed, (1, 1))[0])
    x[0, 5, 3, 4] = float("nan")
    z, zmax = image_ops.conv_bn_relu(x, *packed, (1, 1))
    assert torch.equal(z[1], y[1]) and z[0].isnan().any() and zmax[0].isnan() and zmax[1] == ymax[1]


def _trunk(net, seed=11):
    """Seeded batch-norm statistics that keep the activations of a randomly initialised trunk near one through all layers."""
    torch.manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.uniform_(0.1, 0.3)
            m.running_mean.normal_(0, 0.1)
            m.weight.data.uniform_(0.8, 1.2)
            m.bias.data.normal_(0, 0.1)
    return net


def _composition(net, imgs):
    """The 2048 tap as the chain of ``nn.Conv2d`` + ``BatchNorm2d`` + ``relu`` modules in the trunk's own precision, on the images as
    every route prepares them (resized and scaled in fp32)."""
    x = F.interpolate(imgs.float(), size=(299, 299), mode="bilinear", align_corners=False)
    x = ((x - 128) / 128).to(net.fc.weight.dtype)
    for name, m in net.named_children():  # definition order is forward order; the classifier head follows the last block
        if name == "AvgPool":
            break
        x = m(x)
    return torch.flatten(net.AvgPool(x), 1)


def test_end_to_end_fid_and_kid():
    g = torch.Generator().manual_seed(3)
    batches = [torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8).cuda() for n in (2, 3)]
    torch.manual_seed(11)
    fid = FrechetInceptionDistance(feature=2048).cuda()
    kid = KernelInceptionDistance(feature=2048, subset_size=2, subsets=2).cuda()
    net = _trunk(fid.inception)
    oracle_net = copy.deepcopy(net).double()
    with torch.no_grad():
        for imgs in batches:
            _within(net(imgs), _composition(net, imgs), _composition(oracle_net, imgs))
    for metric in (fid, kid):
        names = kernels_run(lambda: [metric.update(imgs, real=k == 0) for k, imgs in enumerate(batches)])
        assert_route(names, present=["conv_pointwise_kernel", "conv_taps_kernel"])
    assert torch.isfinite(fid.compute()) and torch.isfinite(kid.compute()[0])


@pytest.mark.parametrize("arm", ["cpu", "graph", "fp64"])
def test_arms_that_keep_the_composition(arm, monkeypatch):
    """Reached by argument: a CPU module, weights that record a graph, a trunk moved to fp64."""
    imgs = torch.randint(0, 256, (1, 3, 32, 32), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    net = _trunk(FeatureExtractorInceptionV3(["2048"]), 7)
    if arm != "cpu":
        net, imgs = net.cuda(), imgs.cuda()
    if arm == "fp64":
        net = net.double()
    for p in net.parameters():
        p.requires_grad_(arm == "graph")
    calls = count_calls(monkeypatch, torch.ops.tmx, "conv_bn_relu")
    with torch.set_grad_enabled(arm == "graph"):
        got, want = net._taps(imgs)[0], _composition(net, imgs)
    assert not calls and got.requires_grad == (arm == "graph") and got.dtype == net.fc.weight.dtype
    if arm == "graph":  # (fp32 MIOpen under autograd: rtol for its algorithm choice, as in the LPIPS trunk's test)
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-7)
    else:
        assert torch.equal(got, want)
