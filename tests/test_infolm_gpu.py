"""The native InfoLM route on the GPU (``csrc/infolm.hip``): sentence distributions and the row-pair measures (nine information measures,
KL divergence, cosine similarity) against inline fp64 numpy oracles under the project's value rule, at every tile, split and alignment
edge, with planted special values; which route ran."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

import torchmetrics_forked_amd.ops.text as T
from tests.helpers.routes import assert_route, kernels_run
from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.functional.regression.cosine_similarity import _cosine_similarity_compute, cosine_similarity
from torchmetrics_forked_amd.functional.regression.kl_divergence import kl_divergence
from torchmetrics_forked_amd.functional.text.infolm import _batch_distribution, _InformationMeasure
from torchmetrics_forked_amd.regression import CosineSimilarity, KLDivergence

pytestmark = pytest.mark.gpu

ACC_TILE, WAVE_LIMIT, BLOCK_TILE = 2048, 1024, 2048
FLT_MAX = float(np.finfo(np.float32).max)
_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def test_tile_geometry(device):
    ops.require()
    assert T.infolm_tile() == (ACC_TILE, 256, 16, WAVE_LIMIT, BLOCK_TILE)


def _rule(label, native, oracle, comp32):
    """max|native - oracle| <= 4 max|comp32 - oracle| + 1e-6 max|oracle| over the finite entries of the oracle; NaN / inf in the same places."""
    native, comp32 = (np.asarray(x.detach().double().cpu()) for x in (native, comp32))
    fin = np.isfinite(oracle)
    assert np.array_equal(native[~fin], oracle[~fin], equal_nan=True), label
    assert fin.sum() >= 7 or oracle.size < 7, label
    with np.errstate(invalid="ignore"):
        err, ref = np.abs(native - oracle)[fin].max(initial=0), np.abs(comp32 - oracle)[fin].max(initial=0)
    bound = 4 * ref + 1e-6 * np.abs(oracle[fin]).max(initial=0)
    print(f"infolm_err {label}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
    assert err <= bound, (label, err, bound)


def _softmax64(x):
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------- distribution
_OWNER = [0, 1, 1, 3, 3, 3, 3, 3, 4]  # runs of 1, 2 and 5 rows, sentence 2 without any, sentence 4 for the NaN row


@pytest.mark.parametrize("temperature", [0.25, 1.0])
@pytest.mark.parametrize("dtype", _DTYPES)
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("v", [1, 3, ACC_TILE - 1, ACC_TILE, ACC_TILE + 1, 2 * ACC_TILE + 5])
def test_accumulate(device, v, view, dtype, temperature):
    g = torch.Generator().manual_seed(v)
    r, s, b = len(_OWNER), 3, 5
    buf = (torch.randn(r, s + 1, v + 3, generator=g) * 3 + 80).to(dtype)  # +80: exp overflows without the max subtraction
    if v > 1:
        buf[2, :, 1] = float("-inf")
    buf[8, :, v] = float("nan")
    buf = buf.to(device)
    logits = buf[:, 1:, 1 : v + 1] if view else buf[:, 1:, 1 : v + 1].contiguous()  # the view: misaligned rows, strided
    pos = (torch.arange(r) % s).to(device)
    owner = torch.tensor(_OWNER, device=device)
    w = (torch.rand(r, generator=g) + 0.5).to(device)
    acc0 = torch.full((b, v), 0.5, device=device)  # non-zero: the op adds

    def run(parts):
        acc = acc0.clone()
        for lo, hi in parts:
            T.infolm_accumulate(logits[lo:hi], pos[lo:hi], owner[lo:hi], w[lo:hi], temperature, acc)
        return acc

    sel = logits[torch.arange(r, device=device), pos].float()
    comp = acc0.clone().index_add_(0, owner, F.softmax(sel / temperature, dim=-1) * w[:, None])
    oracle = np.full((b, v), 0.5)
    np.add.at(oracle, _OWNER, _softmax64(sel.double().cpu().numpy() / temperature) * w.double().cpu().numpy()[:, None])
    one = run([(0, r)])
    _rule("one call", one, oracle, comp)
    _rule("run split over two calls", run([(0, 5), (5, r)]), oracle, comp)
    assert torch.equal(one[2], acc0[2])  # no active row: untouched
    assert torch.equal(one.view(torch.int32), run([(0, r)]).view(torch.int32))  # no atomics: bit-equal


class _Stub:
    """A masked-LM stand-in: logits that depend on every token of the row, from a fixed table of multiples of 1/8 (every sum is exact)."""

    def __init__(self, table):
        self.table = table

    def __call__(self, ids, mask):
        e = self.table.to(ids.device)[ids]
        return SimpleNamespace(logits=e + e.sum(1, keepdim=True) * 0.125 * mask[:, :, None])


@pytest.mark.parametrize("idf", [False, True])
def test_batch_distribution(device, idf):
    g = torch.Generator().manual_seed(3)
    special = {"mask_token_id": 1, "pad_token_id": 0, "sep_token_id": 2, "cls_token_id": 3}
    ids = torch.tensor([[3, 7, 8, 9, 2, 0], [3, 5, 2, 0, 0, 0], [3, 4, 6, 7, 5, 2]])
    mask = (ids != 0).long()
    model = _Stub((torch.randn(10, ACC_TILE + 7, generator=g) * 16).round() / 8 + 80)
    idf_w = torch.rand(ids.shape, generator=g) + 0.5 if idf else None
    args = (0.25, special, 4)  # four rows per pass: runs are split over passes
    names = kernels_run(lambda: _batch_distribution(model, ids.to(device), mask.to(device), None if idf_w is None else idf_w.to(device), *args))
    assert_route(names, present=["infolm_row_stats_kernel", "infolm_accumulate_kernel"])
    got = _batch_distribution(model, ids.to(device), mask.to(device), None if idf_w is None else idf_w.to(device), *args)
    comp = _batch_distribution(model, ids, mask, idf_w, *args)
    oracle = np.zeros(comp.shape)
    for i in range(ids.shape[0]):
        wsum = 0.0
        for j in range(ids.shape[1]):
            if int(ids[i, j]) in (0, 2, 3):
                continue
            row = ids[i : i + 1].clone()
            row[0, j] = 1
            wj = float(idf_w[i, j]) if idf else 1.0
            oracle[i] += wj * _softmax64(model(row, mask[i : i + 1]).logits[0, j].double().numpy() / 0.25)
            wsum += wj
        oracle[i] /= wsum
    _rule("batch distribution", got, oracle, comp)


# ----------------------------------------------------------------------------------------------------------------------- measures
def _measure64(kind, p, t, a, b):
    with np.errstate(all="ignore"):
        if kind == "kl_divergence":
            r = (t * np.log(p / t)).sum(-1)
        elif kind == "alpha_divergence":
            r = (1 - (t**a * p ** (1 - a)).sum(-1)) / (a * (a - 1))
        elif kind in ("ab_divergence", "beta_divergence"):
            a = 1.0 if kind == "beta_divergence" else a
            r = np.log((t ** (b + a)).sum(-1)) / (b * (b + a)) + np.log((p ** (b + a)).sum(-1)) / (a * (b + a)) - np.log((t**a * p**b).sum(-1)) / (a * b)
        elif kind == "renyi_divergence":
            r = np.log((t**a * p ** (1 - a)).sum(-1)) / (a - 1)
        elif kind == "l1_distance":
            r = np.abs(t - p).sum(-1)
        elif kind == "l2_distance":
            r = np.sqrt(((t - p) ** 2).sum(-1))
        elif kind == "l_infinity_distance":
            r = np.abs(t - p).max(-1)
        else:
            s = np.sqrt(p * t).sum(-1)
            r = 2 * np.arccos(np.where(np.isnan(s), s, np.clip(s, 0, 1)))
    return np.nan_to_num(r, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)


_MEASURES = [("kl_divergence", None, None), ("beta_divergence", None, 0.7), ("l1_distance", None, None), ("l2_distance", None, None),
             ("l_infinity_distance", None, None), ("fisher_rao_distance", None, None)]
_MEASURES += [(k, a, b) for a in (0.5, -0.5) for k, b in (("alpha_divergence", None), ("ab_divergence", 0.7), ("renyi_divergence", None))]


def _distributions(n, v, seed, device):
    x = torch.rand(n, v, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) ** 2 + 1e-4
    return (x / x.sum(-1, keepdim=True)).float().to(device)


@pytest.mark.parametrize("v", [1, 63, 64, 65, WAVE_LIMIT, WAVE_LIMIT + 1, BLOCK_TILE + 3])
@pytest.mark.parametrize("kind,alpha,beta", _MEASURES)
def test_measures(device, kind, alpha, beta, v):
    p, t = _distributions(12, v, v, device), _distributions(12, v, v + 1, device)
    if kind == "fisher_rao_distance":
        t = t * 0.8  # sum sqrt(p t) <= sqrt(0.8) < 0.9 at every V (acos is ill-conditioned at 1)
    c = v // 2
    t[8, c] = 0  # a zero in t, a zero in p, both zero at one index, a NaN
    p[9, c] = 0
    p[10, c] = t[10, c] = 0
    p[11, c] = float("nan")
    im = _InformationMeasure(kind, alpha, beta)
    native = im(p, t)
    comp = torch.nan_to_num(getattr(im, f"_calculate_{kind}")(p, t))
    oracle = _measure64(kind, p.double().cpu().numpy(), t.double().cpu().numpy(), alpha, beta)
    special = ((comp == 0) | (comp.abs() == FLT_MAX)).cpu().numpy()
    assert torch.equal(native.cpu()[special], comp.cpu()[special]), (native, comp)
    oracle[special] = np.asarray(comp.double().cpu())[special]
    _rule(f"{kind} a={alpha} V={v}", native, oracle, comp)


@pytest.mark.parametrize("v", [1, 65, WAVE_LIMIT + 1])
def test_fisher_rao_of_equal_rows(device, v):
    p = _distributions(8, v, 5, device)
    r = _InformationMeasure("fisher_rao_distance")(p, p).double()
    assert bool(torch.isfinite(r).all() and (r >= 0).all() and (r <= 2 * np.arccos(1 - v * 2.0**-24)).all()), r


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("v", [10, 65, WAVE_LIMIT + 1, BLOCK_TILE + 3])
def test_16bit_rows_are_upcast(device, v, dtype):
    p, t = _distributions(9, v, 1, device).to(dtype), _distributions(9, v, 2, device).to(dtype)
    for kind in (T.KIND_KL, T.KIND_KL_PROB, T.KIND_COSINE):
        assert torch.equal(T.row_pair_measure(p, t, kind), T.row_pair_measure(p.float(), t.float(), kind))


# ------------------------------------------------------------------------------------------------------------------ KL and cosine
def _kl_cos64(mode, p, q):
    with np.errstate(all="ignore"):
        if mode == "cosine":
            return (p * q).sum(-1) / (np.sqrt((p * p).sum(-1)) * np.sqrt((q * q).sum(-1)))
        if mode == "kl_log":
            return (np.exp(p) * (p - q)).sum(-1)
        p, q = p / p.sum(-1, keepdims=True), q / q.sum(-1, keepdims=True)
        return np.where(p == 0, 0.0, p * np.log(p / q)).sum(-1)


@pytest.mark.parametrize("v", [1, 2, 10, 1000, WAVE_LIMIT + 1])
@pytest.mark.parametrize("mode", ["kl_prob", "kl_log", "cosine"])
def test_kl_and_cosine(device, mode, v):
    kl = mode != "cosine"
    fn = (lambda p, q, **kw: kl_divergence(p, q, log_prob=mode == "kl_log", **kw)) if kl else cosine_similarity
    module = (lambda **kw: KLDivergence(log_prob=mode == "kl_log", **kw)) if kl else CosineSimilarity
    got, want, comp = [], [], []
    for n in (1, 3, 257):
        g = torch.Generator().manual_seed(n + v)
        if mode == "kl_log":
            p, q = (torch.log_softmax(torch.randn(n, v, generator=g), -1) for _ in range(2))
        else:
            p, q = (torch.rand(n, v, generator=g) + 0.1 for _ in range(2))
            p[0, 0] = 0  # a zero in p; a zero in q under a positive p
            if kl and n > 1 and v > 1:
                q[1, 1] = 0
        pd, qd = p.to(device), q.to(device)
        none = fn(pd, qd, reduction="none")
        got.append(none), want.append(_kl_cos64(mode, p.double().numpy(), q.double().numpy())), comp.append(fn(p, q, reduction="none"))
        if mode == "kl_prob" and n > 1 and v > 1:
            assert float(none[1]) == float("inf")
        for red, ref in (("sum", none.sum()), ("mean", none.mean()), (None, none)):
            res = fn(pd, qd, reduction=red)
            torch.testing.assert_close(res, ref, rtol=1e-6, atol=0, equal_nan=True)
            m = module(reduction=red).to(device)
            m.update(pd, qd)
            torch.testing.assert_close(m.compute().reshape(res.shape), res, rtol=1e-6, atol=0, equal_nan=True)
    _rule(f"{mode} V={v}", torch.cat(got), np.concatenate(want), torch.cat(comp))


# ------------------------------------------------------------------------------------------------------------------------- routes
_ENTRY = {
    "measure": lambda p, t: _InformationMeasure("ab_divergence", 0.5, 0.7)(p, t),
    "kl": lambda p, t: kl_divergence(p, t, reduction="none"),
    "cosine": lambda p, t: _cosine_similarity_compute(p, t, "none"),  # (the functional's update casts fp64 to fp32 first)
}


@pytest.mark.parametrize("entry", sorted(_ENTRY))
@pytest.mark.parametrize("v,kernel", [(10, "row_pair_wave_kernel"), (WAVE_LIMIT + 1, "row_pair_block_kernel")])
def test_routes(device, entry, v, kernel):
    p, t = _distributions(5, v, 1, device), _distributions(5, v, 2, device)
    assert_route(kernels_run(lambda: _ENTRY[entry](p, t)), present=[kernel])
    assert_route(kernels_run(lambda: _ENTRY[entry](p.double(), t.double())), absent=["row_pair"])
    pg = p.clone().requires_grad_()
    assert_route(kernels_run(lambda: _ENTRY[entry](pg, t)), absent=["row_pair"])
    _ENTRY[entry](pg, t).sum().backward()
    assert bool(torch.isfinite(pg.grad).all())


def test_route_fp64_logits_compose(device):
    model = _Stub(torch.randn(10, 7, dtype=torch.float64).round())
    ids = torch.tensor([[3, 7, 8, 2]], device=device)
    special = {"mask_token_id": 1, "pad_token_id": 0, "sep_token_id": 2, "cls_token_id": 3}
    assert_route(kernels_run(lambda: _batch_distribution(model, ids, torch.ones_like(ids), None, 0.25, special, 8)), absent=["infolm_"])
