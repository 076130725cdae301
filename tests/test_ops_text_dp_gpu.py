"""GPU text DPs (csrc/text_dp.hip) vs their host ops: extended edit distance (one thread per pair, bit-identical
fp64) and clipped n-gram overlap (one wave per hypothesis, 128-bit keys); module-level EED / chrF / ROUGE-N with
GPU states equal the CPU metrics."""
import random

import pytest
import torch

from tests.helpers.routes import count_calls
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

_WORDS = "the a cat sat on mat dog ran far away home blue sky today , . ! ? and of to in it is was".split()


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _sent(rnd, lo=3, hi=30):
    return " ".join(rnd.choice(_WORDS) for _ in range(rnd.randint(lo, hi)))


def _pack(strings):
    from torchmetrics_forked_amd.functional.text.helper import _pack_codepoints

    return _pack_codepoints(strings)


@pytest.mark.parametrize("n_pairs", [1, 37, 700])
def test_eed_gpu_bit_identical_to_host(n_pairs):
    rnd = random.Random(n_pairs)
    hyps = [" " + _sent(rnd) + " " for _ in range(n_pairs)]
    refs = [" " + _sent(rnd) + " " for _ in range(n_pairs)]
    hyps[0] = " "  # degenerate rows
    h, ho = _pack(hyps)
    r, ro = _pack(refs)
    args = (ord(" "), 2.0, 0.3, 0.2, 1.0)
    host = torch.ops.tmx.eed_batch(h, ho, r, ro, *args)
    dev = torch.ops.tmx.eed_gpu(h.cuda(), ho.cuda(), r.cuda(), ro.cuda(), *args, max(len(x) for x in hyps))
    assert torch.equal(dev.cpu(), host)


@pytest.mark.parametrize("n_order,tok", [(6, "char"), (2, "word"), (4, "word"), (9, "word")])
def test_ngram_overlap_gpu_equals_host(n_order, tok):
    from torchmetrics_forked_amd.functional.text.helper import _pack as pack_ids
    from torchmetrics_forked_amd.functional.text.helper import _Vocab

    rnd = random.Random(n_order)
    hyps, groups, refs = [], [0], []
    for _ in range(300):
        s = _sent(rnd)
        hyps.append(list(s) if tok == "char" else s.split())
        k = rnd.randint(1, 3)
        for _ in range(k):
            t = _sent(rnd)
            refs.append(list(t) if tok == "char" else t.split())
        groups.append(groups[-1] + k)
    vocab = _Vocab()
    h, ho = pack_ids(hyps, vocab)
    r, ro = pack_ids(refs, vocab)
    g = torch.tensor(groups)
    host = torch.ops.tmx.ngram_overlap(h, ho, r, ro, g, n_order)
    bits = max(1, len(vocab._ids).bit_length())
    if n_order * bits > 128:
        pytest.skip("keys do not fit 128 bits")
    dev = torch.ops.tmx.ngram_overlap_gpu(h.cuda(), ho.cuda(), r.cuda(), ro.cuda(), g.cuda(), n_order, bits, max(len(x) for x in hyps))
    for a, b in zip(dev, host):
        assert torch.equal(a.cpu(), b)


def test_text_modules_gpu_equal_cpu():
    import torchmetrics_forked_amd.text as T

    rnd = random.Random(5)
    preds = [_sent(rnd, 10, 40) for _ in range(200)]
    target = [[_sent(rnd, 10, 40), _sent(rnd, 10, 40)] for _ in range(200)]
    for make in (lambda: T.ExtendedEditDistance(), lambda: T.CHRFScore(), lambda: T.CHRFScore(n_word_order=0),
                 lambda: T.ROUGEScore(rouge_keys=("rouge1", "rouge2", "rougeL"))):
        cpu, gpu = make(), make().cuda()
        cpu.update(preds, target)
        gpu.update(preds, target)
        a, b = cpu.compute(), gpu.compute()
        if isinstance(a, dict):
            for k in a:
                assert torch.allclose(a[k].float(), b[k].float().cpu(), atol=1e-6), k
        else:
            assert torch.allclose(a.float(), b.float().cpu(), atol=1e-6)


@pytest.mark.parametrize("sub", [1, 2, 5])
@pytest.mark.parametrize("n_pairs", [1, 37, 600])
def test_levenshtein_beam_gpu_identical_to_host(sub, n_pairs):
    """EditDistance's Tercom beam DP on the GPU (one thread per pair) vs the host op: identical integers, including
    empty strings, pairs far off the diagonal (|n - m| > beam) and a long reference (beam widened by m / 2n)."""
    rnd = random.Random(sub * 1000 + n_pairs)
    preds = [_sent(rnd, 1, 40) for _ in range(n_pairs)]
    refs = [_sent(rnd, 1, 40) for _ in range(n_pairs)]
    preds[0] = ""
    if n_pairs > 2:
        refs[1] = ""
        preds[2] = "ab"
        refs[2] = _sent(rnd, 60, 80)  # ratio m / n >> 50: wide beam
    p, po = _pack(preds)
    r, ro = _pack(refs)
    host = torch.ops.tmx.levenshtein_beam_batch(p, po, r, ro, 1, 1, sub)
    dev = torch.ops.tmx.levenshtein_beam_gpu(p.cuda(), po.cuda(), r.cuda(), ro.cuda(), 1, 1, sub, max(len(x) for x in refs))
    assert torch.equal(dev.cpu(), host)


def test_edit_distance_module_gpu_states_equal_cpu(monkeypatch):
    import torchmetrics_forked_amd as tm

    dev_op = count_calls(monkeypatch, torch.ops.tmx, "levenshtein_beam_gpu")
    host_op = count_calls(monkeypatch, torch.ops.tmx, "levenshtein_beam_batch")
    rnd = random.Random(3)
    batches = [([_sent(rnd) for _ in range(120)], [_sent(rnd) for _ in range(120)]) for _ in range(3)]
    for red in ("mean", "none"):
        g = tm.text.EditDistance(substitution_cost=2, reduction=red).cuda()
        c = tm.text.EditDistance(substitution_cost=2, reduction=red)
        for p, t in batches:
            before = len(dev_op), len(host_op)
            g.update(p, t)
            assert (len(dev_op), len(host_op)) == (before[0] + 1, before[1])  # the device op ran, the host op did not
            c.update(p, t)
        torch.testing.assert_close(g.compute().cpu(), c.compute(), rtol=0, atol=0)


def _ter_pairs(rnd, n_pairs, lo=2, hi=25):
    refs, hyps = [], []
    for k in range(n_pairs):
        r = _sent(rnd, lo, hi).split()
        h = list(r)
        # block moves, substitutions, drops: the shift search has work to do
        if len(h) > 4:
            s = rnd.randrange(len(h) - 2)
            ln = rnd.randint(1, min(4, len(h) - s))
            blk = h[s:s + ln]
            del h[s:s + ln]
            t = rnd.randrange(len(h) + 1)
            h[t:t] = blk
        for _ in range(rnd.randint(0, 3)):
            if h:
                h[rnd.randrange(len(h))] = rnd.choice(_WORDS)
        if k % 7 == 3 and h:
            h.pop()
        refs.append(r)
        hyps.append(h)
    return refs, hyps


@pytest.mark.parametrize("n_pairs,hi", [(1, 12), (64, 25), (700, 30), (40, 120)])
def test_ter_gpu_identical_to_host(n_pairs, hi):
    """Tercom shift search on the GPU (one wave per pair, candidate DPs across lanes) vs the host op: identical edit
    counts, incl. empty hypotheses / references and long repetitive sentences that hit the 1000-candidate limit."""
    from torchmetrics_forked_amd.functional.text.helper import _pack as pack_ids
    from torchmetrics_forked_amd.functional.text.helper import _Vocab

    rnd = random.Random(n_pairs + hi)
    refs, hyps = _ter_pairs(rnd, n_pairs, 2, hi)
    if n_pairs > 3:
        hyps[1] = []
        refs[2] = []
        refs[3] = ["the"] * 60
        hyps[3] = ["the", "a"] * 30
    vocab = _Vocab()
    a, ao = pack_ids(refs, vocab)
    b, bo = pack_ids(hyps, vocab)
    groups = torch.arange(n_pairs + 1)
    host, _ = torch.ops.tmx.ter_batch(b, bo, a, ao, groups)
    dev = torch.ops.tmx.ter_gpu(a.int().cuda(), ao.cuda(), b.int().cuda(), bo.cuda(), max(map(len, refs)), max(map(len, hyps)))
    assert torch.equal(dev.cpu(), host), (dev.cpu() - host).abs().max()


def test_ter_module_gpu_states_equal_cpu(monkeypatch):
    import torchmetrics_forked_amd as tm

    dev_op = count_calls(monkeypatch, torch.ops.tmx, "ter_gpu")
    host_op = count_calls(monkeypatch, torch.ops.tmx, "ter_batch")
    rnd = random.Random(5)
    batches = []
    for _ in range(2):
        refs, hyps = _ter_pairs(rnd, 150)
        batches.append(([" ".join(h) for h in hyps], [[" ".join(r), _sent(rnd)] for r in refs]))
    g = tm.text.TranslationEditRate(return_sentence_level_score=True).cuda()
    c = tm.text.TranslationEditRate(return_sentence_level_score=True)
    for p, t in batches:
        before = len(dev_op), len(host_op)
        g.update(p, t)
        assert (len(dev_op), len(host_op)) == (before[0] + 1, before[1])  # the device op ran, the host op did not
        c.update(p, t)
    (gs, gsent), (cs, csent) = g.compute(), c.compute()
    torch.testing.assert_close(gs.cpu(), cs, rtol=0, atol=0)
    torch.testing.assert_close(gsent.cpu(), csent, rtol=0, atol=0)


# ---- which op ran: a GPU-resident text metric sends large batches to the device op and small ones to the host op ----
def _long(rnd, n, lo=300, hi=400):
    return [_sent(rnd, lo, hi) for _ in range(n)]


def _text_route_cases():
    import torchmetrics_forked_amd.text as T

    rnd = random.Random(11)
    many = [_sent(rnd, 10, 40) for _ in range(200)]
    many_refs = [[_sent(rnd, 10, 40), _sent(rnd, 10, 40)] for _ in range(200)]
    few, few_refs = many[:3], many_refs[:3]
    long_p, long_t = _long(rnd, 60), _long(rnd, 60)  # 60 pairs x >= 250 tokens x >= 4 reference words of 64: >= 2^16 DP cells
    ter_refs, ter_hyps = _ter_pairs(rnd, 150)
    ter_p, ter_t = [" ".join(h) for h in ter_hyps], [[" ".join(r), _sent(rnd)] for r in ter_refs]  # 300 pairs
    # (id, metric, device op, host op, batch for the device op, batch for the host op, metric for the host batch)
    return [
        ("edit", lambda: T.EditDistance(), "levenshtein_beam_gpu", "levenshtein_beam_batch", (many, [r[0] for r in many_refs]),
         (few, [r[0] for r in few_refs]), None),
        ("ter", lambda: T.TranslationEditRate(), "ter_gpu", "ter_batch", (ter_p, ter_t), (ter_p[:20], ter_t[:20]), None),
        ("eed", lambda: T.ExtendedEditDistance(), "eed_gpu", "eed_batch", (many, many_refs), (few, few_refs), None),
        ("chrf", lambda: T.CHRFScore(), "ngram_overlap_gpu", "ngram_overlap", (many, many_refs), (few, few_refs), None),
        ("rouge2", lambda: T.ROUGEScore(rouge_keys=("rouge2",)), "ngram_overlap_gpu", "ngram_overlap", (many, many_refs), (few, few_refs), None),
        ("rougeL", lambda: T.ROUGEScore(rouge_keys=("rougeL",)), "lcs_gpu", "lcs_batch", (long_p, long_t), (few, few_refs), None),
        ("wer", lambda: T.WordErrorRate(), "levenshtein_gpu", "levenshtein_batch", (long_p, long_t), (few, [r[0] for r in few_refs]), None),
        # BLEU has no size threshold: the device op holds keys of up to 4 tokens, longer n-grams go to the host op
        ("bleu", lambda: T.BLEUScore(n_gram=4), "bleu_stats_gpu", "bleu_stats", (many, many_refs), (many, many_refs), lambda: T.BLEUScore(n_gram=5)),
    ]


@pytest.mark.parametrize("case", range(8), ids=["edit", "ter", "eed", "chrf", "rouge2", "rougeL", "wer", "bleu"])
def test_text_module_routes(monkeypatch, case):
    _, make, dev_name, host_name, big, small, make_small = _text_route_cases()[case]
    dev_op = count_calls(monkeypatch, torch.ops.tmx, dev_name)
    host_op = count_calls(monkeypatch, torch.ops.tmx, host_name)
    for batch, mk, on_device in ((big, make, True), (small, make_small or make, False)):
        gpu, cpu = mk().cuda(), mk()
        before = len(dev_op), len(host_op)
        gpu.update(*batch)
        ran = len(dev_op) - before[0], len(host_op) - before[1]
        assert (ran[0] > 0, ran[1] > 0) == (on_device, not on_device), (dev_name, host_name, ran)
        cpu.update(*batch)
        a, b = cpu.compute(), gpu.compute()
        for k in (a if isinstance(a, dict) else [None]):
            x, y = (a[k], b[k]) if k is not None else (a, b)
            assert torch.allclose(x.float(), y.float().cpu(), atol=1e-6), (dev_name, k)
