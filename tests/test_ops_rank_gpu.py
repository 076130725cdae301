"""gfx950 rank kernels (csrc/rank.hip) vs the eager CPU path: Spearman's tie-averaged ranks and Kendall's
inversion count, on tie-heavy and tie-free data (exact: ranks are half-integers, counts are integers); below, planted
edges (tile sizes, infinities, signed zeros, runs at row ends, a count above 2^31) against O(n^2) oracles."""
import pytest
import torch

import torchmetrics_forked_amd as tm
import torchmetrics_forked_amd.functional as F
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


@pytest.mark.parametrize("n", [1, 2, 7, 1000, 1024, 1025, 100_000])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rank_average_vs_cpu(n, ties, dtype):
    from torchmetrics_forked_amd.functional.regression.spearman import _rank_data

    g = torch.Generator().manual_seed(n)
    x = (torch.randint(0, max(2, n // 10), (n,), generator=g).to(dtype) if ties else torch.randn(n, generator=g, dtype=dtype))
    assert torch.equal(_rank_data(x.cuda()).cpu(), _rank_data(x))


@pytest.mark.parametrize("n", [2, 3, 1023, 1024, 1025, 4096, 70_001])
@pytest.mark.parametrize("ties", [False, True])
def test_count_inversions_vs_cpu(n, ties):
    from torchmetrics_forked_amd.functional.regression import kendall as K

    g = torch.Generator().manual_seed(n + ties)
    y = torch.randint(0, 50, (n,), generator=g).double() if ties else torch.randn(n, generator=g, dtype=torch.float64)
    got = int(torch.ops.tmx.count_inversions(y.cuda()))
    assert got == int(K._count_inversions(y))
    if n <= 2000:  # brute force
        assert got == int((y[:, None] > y[None, :]).triu(1).sum())


@pytest.mark.parametrize("variant", ["a", "b", "c"])
@pytest.mark.parametrize("outputs", [1, 3])
def test_kendall_spearman_gpu_vs_cpu(variant, outputs):
    g = torch.Generator().manual_seed(outputs)
    shape = (5000, outputs) if outputs > 1 else (5000,)
    p = torch.randint(0, 30, shape, generator=g).float()
    t = p + torch.randn(shape, generator=g)
    cpu = F.kendall_rank_corrcoef(p, t, variant=variant)
    gpu = F.kendall_rank_corrcoef(p.cuda(), t.cuda(), variant=variant).cpu()
    torch.testing.assert_close(gpu, cpu, rtol=1e-6, atol=1e-7)
    cpu = F.spearman_corrcoef(p, t)
    gpu = F.spearman_corrcoef(p.cuda(), t.cuda()).cpu()
    torch.testing.assert_close(gpu, cpu, rtol=1e-6, atol=1e-7)
    m = tm.SpearmanCorrCoef(num_outputs=outputs).cuda()
    m.update(p.cuda(), t.cuda())
    torch.testing.assert_close(m.compute().cpu(), cpu, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------------
# Planted edges against the O(n^2) oracles of tests/helpers/rowwise_oracle.py (IEEE comparisons, exact results).
import math  # noqa: E402

from tests.helpers import rowwise_oracle as RO  # noqa: E402


def _inversion_inputs(n):
    g = torch.Generator().manual_seed(n)
    inf = math.inf
    y = torch.randn(n, generator=g, dtype=torch.float64)
    y[torch.randperm(n, generator=g)[: max(1, n // 7)]] = inf  # the kernel pads its last tile with +inf as well
    y[torch.randperm(n, generator=g)[: max(1, n // 9)]] = -inf
    zeros = torch.where(torch.rand(n, generator=g) < 0.5, 0.0, -0.0).double()
    zeros[:: 5] = 1.0
    zeros[3 :: 7] = -1.0
    return {
        "all-equal": (torch.full((n,), 2.5, dtype=torch.float64), 0),
        "descending": (torch.arange(n, 0, -1, dtype=torch.float64), n * (n - 1) // 2),
        "+-inf": (y, None),
        "signed-zeros": (zeros, None),
    }


@pytest.mark.parametrize("n", [2, 1024, 1025, 2047, 2048, 2049])
def test_count_inversions_planted_vs_oracle(n):
    """Around the 1024-element LDS tile and the first merge level: equal values, the worst case, infinities inside ``y``
    (next to the +inf padding of the last tile) and -0.0 == +0.0, which is no inversion in either order."""
    for name, (y, closed) in _inversion_inputs(n).items():
        want = RO.inversions_oracle(y)
        assert closed is None or want == closed
        got = int(torch.ops.tmx.count_inversions(y.cuda()))
        assert got == want, (name, n, got, want)
    y = torch.tensor([0.0, -0.0] * (n // 2), dtype=torch.float64)
    assert int(torch.ops.tmx.count_inversions(y.cuda())) == 0


def test_count_inversions_above_2_pow_31():
    """Strictly descending n = 70 001: n (n - 1) / 2 = 2 450 035 000 > 2^31, the closed form checks the 64-bit count."""
    n = 70_001
    y = torch.arange(n, 0, -1, dtype=torch.float64).cuda()
    assert n * (n - 1) // 2 == 2_450_035_000 > 2**31
    assert int(torch.ops.tmx.count_inversions(y)) == 2_450_035_000


def _rank_rows(D, dtype):
    inf = math.inf
    rows = {
        "one run over the whole row": [[4.0] * 9] * D,
        "runs touching both ends": [[1.0, 1.0, 1.0, 2.0, 3.0, 3.5, 7.0, 7.0, 7.0]] * D,
        # row d ends with the value row d + 1 starts with: a run never crosses rows
        "equal across the row boundary": [[float(d), d + 1.0, d + 1.0, d + 2.0, d + 2.0, d + 2.0, d + 3.0, d + 3.0, d + 3.0] for d in range(D)],
        "infinities": [[-inf, -inf, -1.0, 0.0, 0.0, 5.0, inf, inf, inf]] * D,
        "single-element runs": [[float(i) for i in range(9)]] * D,
    }
    return {k: torch.tensor(v, dtype=dtype) for k, v in rows.items()}


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rank_average_direct_vs_oracle(D, dtype):
    """``rank_average`` on sorted rows and a permutation, called directly; also one value per row (n = 1)."""
    g = torch.Generator().manual_seed(D)
    cases_ = _rank_rows(D, dtype)
    cases_["n = 1"] = torch.tensor([[3.0]] * D, dtype=dtype)
    for name, srt in cases_.items():
        n = srt.shape[1]
        assert torch.equal(srt, srt.sort(1).values)
        idx = torch.stack([torch.randperm(n, generator=g) for _ in range(D)])
        x = torch.empty_like(srt).scatter_(1, idx, srt)  # x[d, idx[d, i]] = srt[d, i]
        got = torch.ops.tmx.rank_average(srt.cuda(), idx.cuda()).cpu()
        want = RO.average_ranks_oracle(x)
        assert got.dtype == dtype and torch.equal(got, want), (name, got, want)
