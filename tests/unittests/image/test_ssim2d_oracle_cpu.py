"""The dense valid-window SSIM oracle of ``tests/helpers/ssim_oracle.py`` against this package's CPU composition in fp64 (which
``test_image.py`` pins to the reference): the oracle the GPU file holds the kernels to is the operation the functional computes."""
import pytest
import torch

from tests.helpers import ssim_oracle as so
from torchmetrics_forked_amd.functional.image import structural_similarity_index_measure as ssim
from torchmetrics_forked_amd.functional.image.helper import _gaussian


def _window(kw):
    if kw.get("gaussian_kernel", True):
        ks = int(3.5 * kw["sigma"] + 0.5) * 2 + 1
        return _gaussian(ks, kw["sigma"], torch.float64, torch.device("cpu")).reshape(-1)
    return torch.full((kw["kernel_size"],), 1.0 / kw["kernel_size"], dtype=torch.float64)


@pytest.mark.parametrize("kind", ["unit", "255", "negative", "shifted", "shifted_low"])
@pytest.mark.parametrize("kw", [{"sigma": 1.5}, {"sigma": 0.8}, {"gaussian_kernel": False, "kernel_size": 5}], ids=["g11", "g7", "u5"])
def test_oracle_matches_the_composition_in_fp64(kw, kind):
    window = _window(kw)  # the composition's own fp64 window: only the order of evaluation differs
    ks = window.numel()
    p, t, data_range = so.planes((3, 2, 23, 30), 17 + ks, kind)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    sums = so.valid_window_sums(p.reshape(6, 23, 30), t.reshape(6, 23, 30), window, window, c1, c2)
    n = 2 * (23 - ks + 1) * (30 - ks + 1)
    want, want_cs = ssim(p.double(), t.double(), data_range=data_range, reduction="none", return_contrast_sensitivity=True, **kw)
    # two fp64 evaluations of one formula (unfold and matmul against a reflect-padded conv2d and a crop): 1e-15-class differences;
    # 1e-10 is five orders above that and far below what a wrong window, crop or constant gives
    assert float((sums[0].reshape(3, 2).sum(1) / n - want).abs().max()) <= 1e-10
    assert float((sums[1].reshape(3, 2).sum(1) / n - want_cs).abs().max()) <= 1e-10
    sse = ((p.double() - t.double()) ** 2).reshape(6, -1).sum(1)
    assert float(((sums[2] - sse).abs() / sse).max()) <= 1e-12


def test_builders():
    assert so.gaussian(11, 1.5).dtype == torch.float32 and so.uniform(7).dtype == torch.float32
    assert torch.equal(so.gaussian(11, 1.5), _gaussian(11, 1.5, torch.float64, torch.device("cpu")).reshape(-1).float())
    assert abs(float(so.gaussian(15, 2.0).double().sum()) - 1) < 1e-6 and float(so.uniform(7)[0]) == float(torch.tensor(1 / 7, dtype=torch.float32))


def test_fp32_variant_adds_in_fp64_and_differs_from_the_oracle():
    p, t, _ = so.planes((7, 40, 45), 3)
    w = so.gaussian(11, 1.5)
    o64, c32 = so.valid_window_sums(p, t, w, w, 1e-4, 9e-4), so.valid_window_sums(p, t, w, w, 1e-4, 9e-4, torch.float32)
    assert o64.dtype == c32.dtype == torch.float64 and o64.shape == c32.shape == (3, 7)
    rel = (c32 - o64).abs() / o64.abs()
    assert 0 < float(rel.max()) < 1e-5
