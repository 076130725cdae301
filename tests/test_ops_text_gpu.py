"""gfx950 text kernels vs PyTorch references: fused token NLL (Perplexity) and MFMA BERTScore greedy matching.
The second half pins their edges (padding, -inf identity, K tail, NaN / inf logits, misaligned views) against the
fp64 oracles of tests/helpers/oracles.py."""
import pytest
import torch

from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


@pytest.mark.parametrize("shape", [(2, 5, 7), (4, 128, 30522), (1, 3, 50257), (8, 64, 1000)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("ignore_index", [None, 0])
def test_token_nll_kernel(shape, dtype, ignore_index):
    g = torch.Generator().manual_seed(shape[-1])
    logits = (torch.randn(*shape, generator=g) * 3).to(dtype)
    target = torch.randint(0, shape[-1], shape[:2], generator=g)
    nll = torch.ops.tmx.token_nll(logits.reshape(-1, shape[-1]).cuda(), target.reshape(-1).cuda(),
                                  0 if ignore_index is None else ignore_index, ignore_index is not None)
    ref = -torch.log_softmax(logits.double().reshape(-1, shape[-1]), 1).gather(1, target.reshape(-1, 1)).squeeze(1)
    if ignore_index is not None:
        ref = torch.where(target.reshape(-1) == ignore_index, torch.zeros_like(ref), ref)
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    torch.testing.assert_close(nll.double().cpu(), ref, atol=tol, rtol=tol)


def test_perplexity_gpu_matches_cpu():
    from torchmetrics_forked_amd.functional.text import perplexity

    g = torch.Generator().manual_seed(1)
    preds = torch.randn(4, 33, 517, generator=g)
    target = torch.randint(0, 517, (4, 33), generator=g)
    torch.testing.assert_close(perplexity(preds.cuda(), target.cuda(), ignore_index=3).cpu(), perplexity(preds, target, ignore_index=3),
                               atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("shape", [(3, 40, 50, 32), (2, 1000, 1024, 40), (1, 256, 768, 776), (3, 512, 512, 64), (2, 128, 64, 768), (5, 17, 33, 24), (64, 512, 512, 768), (2, 300, 129, 72), (2, 130, 257, 20)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bert_greedy_match_kernel(shape, dtype):
    b, lp, lr, d = shape
    g = torch.Generator().manual_seed(lp * lr)
    p = torch.nn.functional.normalize(torch.randn(b, lp, d, generator=g), dim=-1)
    r = torch.nn.functional.normalize(torch.randn(b, lr, d, generator=g), dim=-1)
    p[:, 0] = 0  # masked special token
    pq, rq = p.to(dtype), r.to(dtype)
    rowmax, colmax = torch.ops.tmx.bert_greedy_match(pq.cuda(), rq.cuda())
    sim = torch.bmm(pq.double(), rq.double().transpose(1, 2))
    tol = 1e-5 if dtype == torch.float32 else 2e-3
    torch.testing.assert_close(rowmax.cpu().double(), sim.max(2).values, atol=tol, rtol=0)
    torch.testing.assert_close(colmax.cpu().double(), sim.max(1).values, atol=tol, rtol=0)


def test_bert_score_gpu_matches_cpu():
    transformers = pytest.importorskip("transformers")
    from torchmetrics_forked_amd.functional.text import bert_score

    cfg = transformers.BertConfig(vocab_size=100, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128)
    torch.manual_seed(0)
    model = transformers.BertModel(cfg).eval()
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(5, 100, (6, 24), generator=g)
    mask = torch.ones_like(ids)
    mask[:, 18:] = 0
    tids = torch.randint(5, 100, (6, 24), generator=g)
    preds, target = {"input_ids": ids, "attention_mask": mask}, {"input_ids": tids, "attention_mask": torch.ones_like(tids)}
    cpu = bert_score(preds, target, model=model, idf=True)
    gpu = bert_score(preds, target, model=model.cuda(), idf=True, device="cuda")
    for k in ("precision", "recall", "f1"):
        torch.testing.assert_close(gpu[k].cpu(), cpu[k], atol=1e-4, rtol=0)


@pytest.mark.parametrize("max_len,vocab,n", [(20, 6, 500), (64, 3, 300), (65, 4, 200), (300, 5, 64), (1024, 8, 16), (200, 1000, 50)])
def test_levenshtein_gpu_matches_host(max_len, vocab, n):
    """One wave per pair, multi-word bit-parallel DP (csrc/text_gpu.hip) vs the host kernel (Myers / two-row DP)."""
    from torchmetrics_forked_amd.functional.text.helper import _levenshtein_many

    g = torch.Generator().manual_seed(max_len * 7 + vocab)
    preds = [torch.randint(0, vocab, (int(torch.randint(0, max_len + 1, (1,), generator=g)),), generator=g).tolist() for _ in range(n)]
    target = [torch.randint(0, vocab, (int(torch.randint(0, max_len + 1, (1,), generator=g)),), generator=g).tolist() for _ in range(n)]
    target[0], preds[1] = [], []  # empty sides
    host = _levenshtein_many(preds, target)
    dev = _levenshtein_many(preds, target, torch.device("cuda"), force_gpu=True)
    assert dev.is_cuda
    assert torch.equal(dev.cpu(), host)


def test_wer_family_gpu_states_large_batch_matches_cpu():
    import torchmetrics_forked_amd.text as T

    g = torch.Generator().manual_seed(0)
    words = ["w%d" % i for i in range(30)]
    mk = lambda k: " ".join(words[int(i)] for i in torch.randint(0, 30, (k,), generator=g))  # noqa: E731
    preds = [mk(int(torch.randint(1, 90, (1,), generator=g))) for _ in range(3000)]
    target = [mk(int(torch.randint(1, 90, (1,), generator=g))) for _ in range(3000)]
    for cls in (T.WordErrorRate, T.CharErrorRate, T.MatchErrorRate, T.WordInfoLost, T.WordInfoPreserved):
        gpu, cpu = cls().cuda(), cls()
        gpu.update(preds, target)
        cpu.update(preds, target)
        torch.testing.assert_close(gpu.compute().cpu(), cpu.compute(), atol=1e-6, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------
# Edge cases against the independent fp64 oracles of tests/helpers/oracles.py (not the library's own CPU path).
from tests.helpers import oracles as O  # noqa: E402

_TILE_W = 256  # edge of the wide tile (kW in csrc/bertscore.hip)


def _bert_route(shape, dtype, aligned=True):
    """The kernel csrc/bertscore.hip is expected to pick for this call (labels the measured errors;
    ``test_bert_edge_shapes_reach_every_route`` holds it against the kernels that ran)."""
    _, lp, lr, d = shape
    if dtype == torch.float32:
        return "f32"
    if d % 8 or not aligned:
        return "half-fallback"
    wm, wn = -(-lp // _TILE_W), -(-lr // _TILE_W)
    if lp >= _TILE_W and lr >= _TILE_W and 4 * wm * wn * _TILE_W * _TILE_W <= 5 * lp * lr:
        return "w256"
    return "tile128"


def _off_by_one_element(t):
    """The same values in a contiguous GPU tensor whose base pointer sits one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == t.element_size()
    return view


# (B, Lp, Lr, D): ragged edges of the 256-wide tile (the first two; D = 72 ends in a K slice of 8), of the 128 tile (the
# next three: 256 x 300 would waste more than 25 % of two wide tiles), D % 8 != 0; the last case runs misaligned
BERT_EDGE_SHAPES = [(2, 470, 500, 40), (1, 256, 500, 72), (1, 256, 300, 72), (2, 257, 300, 40), (3, 129, 130, 8), (2, 130, 257, 20)]
BERT_EDGE_CASES = [(s, True) for s in BERT_EDGE_SHAPES] + [((2, 257, 300, 40), False)]


_BERT_KERNELS = {"f32": "greedy_match_f32_kernel", "half-fallback": "greedy_match_half_kernel",
                 "tile128": "greedy_match_tiled_kernel", "w256": "greedy_match_w256_kernel"}


def test_bert_edge_shapes_reach_every_route():
    """The kernels that RAN for every edge case (profiled launches, not the restated rule): each case launches exactly
    the one matching kernel its label names, and the cases together launch all four."""
    from tests.helpers.routes import kernels_run

    seen = set()
    for shape, aligned in BERT_EDGE_CASES:
        b, lp, lr, d = shape
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            p, r = torch.randn(b, lp, d).to(dtype), torch.randn(b, lr, d).to(dtype)
            pd, rd = (p.cuda(), r.cuda()) if aligned else (_off_by_one_element(p), _off_by_one_element(r))
            names = kernels_run(lambda: torch.ops.tmx.bert_greedy_match(pd, rd))
            ran = {label for label, kernel in _BERT_KERNELS.items() if any(kernel in n for n in names)}
            assert ran == {_bert_route(shape, dtype, aligned)}, (shape, dtype, aligned, sorted(set(names)))
            seen |= ran
    assert seen == set(_BERT_KERNELS)


def _check_greedy(pq, rq, shape, dtype, aligned, what):
    """Both maxima against fp64 on the quantised inputs.  16-bit inputs have exact products, so the only error is the
    fp32 accumulation, at most D * 2^-24 * |p_i| |r_j|, plus one fp32 ulp of the result; fp32 keeps the 1e-5 of the
    existing test."""
    d = shape[3]
    pd, rd = (pq.cuda(), rq.cuda()) if aligned else (_off_by_one_element(pq), _off_by_one_element(rq))
    rowmax, colmax = torch.ops.tmx.bert_greedy_match(pd, rd)
    row_ref, col_ref = O.greedy_match_fp64(pq, rq)
    pn, rn = pq.double().norm(dim=2), rq.double().norm(dim=2)
    for got, ref, mine, other in ((rowmax, row_ref, pn, rn), (colmax, col_ref, rn, pn)):
        got = got.cpu().double()
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
        if dtype == torch.float32:
            tol = torch.full_like(ref, 1e-5)
        else:
            tol = d * 2.0 ** -24 * mine * other.max(dim=1, keepdim=True).values + 2.0 ** -23 * ref.abs()
        err = (got - ref).abs()[~nan]
        ratio = float((err / tol[~nan]).max()) if err.numel() else 0.0
        print(f"bert_greedy_match {what} route={_bert_route(shape, dtype, aligned)} dtype={dtype} shape={shape}: "
              f"max err {float(err.max()) if err.numel() else 0.0:.3e}, err/bound {ratio:.3f}")
        assert ratio <= 1.0, f"{what}: error {float(err.max()):.3e} is {ratio:.2f} x the bound"
    return rowmax, colmax


@pytest.mark.parametrize("shape,aligned", BERT_EDGE_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bert_greedy_match_all_negative(shape, aligned, dtype):
    """Every similarity is below zero: a kernel that lets zero padding take part in a maximum, or starts from 0
    instead of -inf, returns 0 somewhere."""
    b, lp, lr, d = shape
    g = torch.Generator().manual_seed(lp + lr + d)
    u = torch.nn.functional.normalize(torch.randn(b, 1, d, generator=g), dim=-1)
    p = u + 0.05 * torch.randn(b, lp, d, generator=g) / d ** 0.5
    r = -(u + 0.05 * torch.randn(b, lr, d, generator=g) / d ** 0.5)
    pq, rq = p.to(dtype), r.to(dtype)
    assert float(torch.bmm(pq.double(), rq.double().transpose(1, 2)).max()) < -0.5
    _check_greedy(pq, rq, shape, dtype, aligned, "all-negative")


@pytest.mark.parametrize("shape,aligned", BERT_EDGE_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bert_greedy_match_planted_maxima(shape, aligned, dtype):
    """Identical rows planted at the tile and fragment edges of both operands, their whole norm in the last 8
    features, over a background of |similarity| <= 0.3: a dropped K tail or edge row reads the background."""
    b, lp, lr, d = shape
    g = torch.Generator().manual_seed(lp * lr + d)
    p = 0.3 * torch.nn.functional.normalize(torch.randn(b, lp, d, generator=g), dim=-1)
    r = 0.3 * torch.nn.functional.normalize(torch.randn(b, lr, d, generator=g), dim=-1)
    edges = [0, 15, 16, 63, 64, 127, 128, 255, 256]
    rows = [e for e in edges if e < lp - 1] + [lp - 1]
    cols = [e for e in edges if e < lr - 1] + [lr - 1]
    for t in range(max(len(rows), len(cols))):
        i, j = rows[t % len(rows)], cols[t % len(cols)]
        if t >= len(rows):  # the shorter side goes round again: reuse the vector already planted there
            r[:, j] = p[:, i]
        elif t >= len(cols):
            p[:, i] = r[:, j]
        else:
            v = torch.zeros(b, d)
            v[:, d - 8:] = torch.nn.functional.normalize(torch.randn(b, 8, generator=g), dim=-1)
            p[:, i] = v
            r[:, j] = v
    pq, rq = p.to(dtype), r.to(dtype)
    rowmax, colmax = _check_greedy(pq, rq, shape, dtype, aligned, "planted")
    assert float(rowmax[:, rows].min()) > 0.98 and float(colmax[:, cols].min()) > 0.98
    others = [i for i in range(lp) if i not in rows]
    assert float(rowmax[:, others].max()) <= 0.31  # background rows: |p_i| |r_j| <= 0.3 (+ 16-bit rounding)


@pytest.mark.parametrize("shape,aligned", [(s, a) for s, a in BERT_EDGE_CASES if s[0] >= 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bert_greedy_match_nan_propagates(shape, aligned, dtype):
    """One NaN in p[0, 3]: row 3's maximum and every column maximum of pair 0 are NaN (torch.max semantics); every
    other row and the other pairs keep their finite maxima."""
    b, lp, lr, d = shape
    g = torch.Generator().manual_seed(lp + 3 * lr)
    p = torch.nn.functional.normalize(torch.randn(b, lp, d, generator=g), dim=-1)
    r = torch.nn.functional.normalize(torch.randn(b, lr, d, generator=g), dim=-1)
    p[0, 3, d - 1] = float("nan")
    rowmax, colmax = _check_greedy(p.to(dtype), r.to(dtype), shape, dtype, aligned, "nan")
    rowmax, colmax = rowmax.cpu(), colmax.cpu()
    assert torch.isnan(rowmax[0, 3]) and torch.isnan(colmax[0]).all()
    assert int(torch.isnan(rowmax).sum()) == 1 and not torch.isnan(colmax[1:]).any()


NLL_VOCABS = [1, 3, 255, 256, 257, 2049]


def _nll_rows(v, dtype, seed):
    """Logit rows [N, V] and targets that walk the branches of csrc/perplexity.hip; returns also the row numbers whose
    result must be exactly 0.  Written for any V >= 1 (at V = 1 several rows coincide; the oracle decides)."""
    g = torch.Generator().manual_seed(seed)
    inf, nan = float("inf"), float("nan")
    big = 6e4 if dtype == torch.float16 else 1e4
    rows, tgt, zero_rows = [], [], []

    def add(x, t, exact_zero=False):
        if exact_zero:
            zero_rows.append(len(rows))
        rows.append(x)
        tgt.append(t)

    rnd = lambda: torch.randn(v, generator=g) * 3  # noqa: E731
    t0 = int(torch.randint(0, v, (1,), generator=g))
    other = (t0 + 1) % v
    add(rnd(), t0)
    x = rnd(); x[::2] = -inf; x[t0] = 1.5; add(x, t0)                      # some logits masked
    x = torch.full((v,), -inf); x[t0] = 2.25; add(x, t0, True)            # everything but the target masked: exactly 0
    x = rnd(); x[t0] = -inf; add(x, t0)                                    # the target masked: +inf (NaN when V == 1)
    add(torch.full((v,), -inf), t0)                                        # everything masked: NaN
    x = rnd(); x[other] = inf; add(x, t0)                                  # one +inf logit
    x = rnd(); x[other] = inf; x[v // 2] = inf; add(x, t0)                 # two +inf logits
    x = rnd(); x[t0] = inf; add(x, t0)                                     # +inf at the target: inf - inf
    x = rnd(); x[other] = nan; add(x, t0)                                  # one NaN logit
    x = rnd(); x[v - 1] = nan; add(x, 0)                                   # NaN as the last element a thread sees
    add((torch.rand(v, generator=g) * 2 - 1) * big, t0)                    # large logits: a naive exp overflows
    x = torch.zeros(v); x[t0] = 1e4; add(x, t0, True)                      # one-hot: exactly 0, never negative
    x = rnd(); x[v - 1] = x.max() + 5; add(x, v - 1)                       # maximum in the scalar tail
    x = rnd(); x[v - 1] = x.max() + 5; add(x, 0)
    add(rnd(), -100)                                                       # ignored row
    add(rnd(), v)                                                          # out-of-range targets: NaN
    add(rnd(), -1)
    add(rnd(), other)                                                      # an ordinary row after the poisoned ones
    return torch.stack(rows).to(dtype), torch.tensor(tgt, dtype=torch.long), zero_rows


@pytest.mark.parametrize("v", NLL_VOCABS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
def test_token_nll_edges_vs_fp64_oracle(v, dtype):
    """Masked (-inf), +inf and NaN logits, large logits, ignore_index = -100 and out-of-range targets at vocabulary
    sizes around the 256-thread block and the vector width, on an aligned and a misaligned base pointer.
    Bound: eps * 2 (|lse| + |x_t|) for the rounding of m + log s and of the subtraction, plus (V / 256 + 32) eps for a
    serial sum of V / 256 terms per thread and the merges; eps = 2^-23 (fp32 accumulation) or 2^-52 (fp64)."""
    logits, target, zero_rows = _nll_rows(v, dtype, 1000 + v)
    ref = O.nll_fp64(logits, target, -100)
    xt = logits.double().gather(1, target.clamp(0, v - 1).view(-1, 1)).squeeze(1)
    eps = 2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23
    finite = torch.isfinite(ref)
    lse = torch.where(finite, ref + xt, torch.zeros_like(ref))
    tol = 2 * eps * (lse.abs() + torch.where(finite, xt, torch.zeros_like(xt)).abs()) + (v / 256 + 32) * eps
    for aligned in (True, False):
        dev = logits.cuda() if aligned else _off_by_one_element(logits)
        got = torch.ops.tmx.token_nll(dev, target.cuda(), -100, True).cpu().double()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (got, ref)
        assert torch.equal(torch.isposinf(got), torch.isposinf(ref)) and not torch.isneginf(got).any(), (got, ref)
        err = (got - ref).abs()[finite]
        ratio = float((err / tol[finite]).max())
        print(f"token_nll V={v} dtype={dtype} aligned={aligned}: max err {float(err.max()):.3e}, err/bound {ratio:.3f}")
        assert ratio <= 1.0, (got, ref)
        assert all(float(got[i]) == 0.0 for i in zero_rows), got[zero_rows]
