"""LPIPS default heads: ``pretrained=True`` uses the published LPIPS v0.1 linear heads, the same values the reference
loads from its ``lpips_models/{net}.pth`` (read here with ``weights_only=True``).  The reference's LPIPS itself needs
torchvision trunks (absent offline), so the network output is compared against our own model with the reference's
.pth given explicitly as ``model_path`` — identical heads, identical random trunk."""
import os

import pytest
import torch

from torchmetrics_forked_amd.functional.image.lpips import _LPIPS

# the reference's three head files (5 to 7 [1, C, 1, 1] weight tensors each), stored as test vectors
REF = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "golden", "lpips_models")


@pytest.mark.parametrize("net", ["alex", "vgg", "squeeze"])
def test_default_heads_equal_reference_pth(net):
    ref = torch.load(os.path.join(REF, f"{net}.pth"), map_location="cpu", weights_only=True)
    ours = _LPIPS(pretrained=True, net=net)
    for key, val in ref.items():
        got = ours.state_dict()[key]
        assert torch.equal(got, val), key
    torch.manual_seed(0)
    a = _LPIPS(pretrained=True, net=net)
    torch.manual_seed(0)
    b = _LPIPS(pretrained=True, net=net, model_path=os.path.join(REF, f"{net}.pth"))
    x, y = torch.rand(2, 3, 64, 64) * 2 - 1, torch.rand(2, 3, 64, 64) * 2 - 1
    with torch.no_grad():
        assert torch.equal(a(x, y), b(x, y))


def test_random_heads_when_not_pretrained():
    m = _LPIPS(pretrained=False, net="alex")
    packaged = _LPIPS(pretrained=True, net="alex")
    assert not torch.equal(m.lin0.model[-1].weight, packaged.lin0.model[-1].weight)
