"""The seven GPU string kernels (csrc/text_gpu.hip, csrc/text_dp.hip, csrc/ter.hip) against the plain oracles and plants
of tests/helpers/text_oracle.py and against their host ops, at the edges the corpus-like tests do not reach:

* ``levenshtein_gpu`` / ``lcs_gpu``: reference lengths on both sides of every 64-token word and at the 1024-token limit,
  mismatches planted on bit 63 / bit 0 of a word, a partial last block;
* ``levenshtein_beam_gpu``: insertion cost != deletion cost, the widened beam, a scratch stride above every length;
* ``ngram_overlap_gpu``: keys that spill into the high word of the 128-bit key (and ``bits = 64``), hypotheses that
  fill all 8 slots of a lane, first occurrences across slots;
* ``bleu_stats_gpu``: ids at the 16-bit field limit, ties of the closest reference length;
* ``ter_gpu``: several pairs per wave (grid stride) on scratch left behind by longer pairs, the scratch cap that
  shrinks the grid, the 1024-wave cap;
* ``eed_gpu``: empty sides, rows that all jump;
* every op's own limit checks.

Every assertion is exact (integers, or ``torch.equal`` on fp64)."""
import random

import pytest
import torch

from tests.helpers import text_oracle as TO
from tests.helpers.routes import count_calls
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _cuda(*tensors):
    return [t.cuda() for t in tensors]


# ------------------------------------------------------------------------------------------------ Levenshtein / LCS
@pytest.fixture(scope="module")
def lev_calls():
    """(packed host tensors, longest reference, oracle distances, oracle LCS lengths, planted values) per call."""
    out = []
    for call in TO.lev_calls():
        a, ao = TO.pack([c[1] for c in call])
        b, bo = TO.pack([c[2] for c in call])
        want = [TO.lev_oracle(c[1], c[2]) for c in call]
        for (label, _, _, dist, lcs), w in zip(call, want):
            assert dist is None or (dist, lcs) == w, label
        out.append(((a, ao, b, bo), max(len(c[2]) for c in call), [w[0] for w in want], [w[1] for w in want], [c[0] for c in call]))
    return out


def test_levenshtein_gpu_word_edges(lev_calls):
    for packed, max_ref, dist, _, labels in lev_calls:
        assert len(labels) % 4 != 0  # partial last block
        got = torch.ops.tmx.levenshtein_gpu(*_cuda(*packed), max_ref).tolist()
        assert got == dist, [(lb, g, w) for lb, g, w in zip(labels, got, dist) if g != w][:8]
        assert got == torch.ops.tmx.levenshtein_batch(*packed).tolist()


def test_lcs_gpu_word_edges(lev_calls):
    for packed, max_ref, _, lcs, labels in lev_calls:
        got = torch.ops.tmx.lcs_gpu(*_cuda(*packed), max_ref).tolist()
        assert got == lcs, [(lb, g, w) for lb, g, w in zip(labels, got, lcs) if g != w][:8]
        assert got == torch.ops.tmx.lcs_batch(*packed).tolist()


# ------------------------------------------------------------------------------------------------------------- beam
@pytest.mark.parametrize("costs", TO.BEAM_COSTS)
def test_levenshtein_beam_gpu_costs_and_band(costs):
    pairs = TO.beam_cases()
    a, ao = TO.pack([p for p, _ in pairs])
    b, bo = TO.pack([r for _, r in pairs])
    longest = max(len(r) for _, r in pairs)
    want = [TO.levenshtein_band(p, r, *costs) for p, r in pairs]
    for max_ref in (longest, longest + 37):  # the scratch stride equals / exceeds the longest reference
        got = torch.ops.tmx.levenshtein_beam_gpu(*_cuda(a, ao, b, bo), *costs, max_ref).tolist()
        assert got == want, [(k, len(pairs[k][0]), len(pairs[k][1]), g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    assert want == torch.ops.tmx.levenshtein_beam_batch(a, ao, b, bo, *costs).tolist()
    for k, (p, r) in enumerate(pairs):
        if len(p) <= 20 and len(r) <= 20:  # the band covers the table
            assert want[k] == TO.levenshtein_full(p, r, *costs), k


# ---------------------------------------------------------------------------------------------------------- n-grams
@pytest.mark.parametrize("n_order,bits", TO.NGRAM_CONFIGS)
def test_ngram_overlap_gpu_wide_keys_and_slots(n_order, bits):
    ids = TO.ngram_ids(bits, random.Random(bits))
    hyps, refs, groups = TO.ngram_cases(n_order, ids, TO.ngram_hyp_lens(n_order), seed=100 * n_order + bits, bits=bits)
    long_hyp = hyps[-1]
    assert len(long_hyp) == 512 and len({tuple(long_hyp[p:p + n_order]) for p in TO.NGRAM_SLOT_SPOTS}) == 1  # slots 0, 1, 7
    assert any(len(r) < n_order for r in refs) and any(len(r) == 600 for r in refs)
    h, ho = TO.pack(hyps)
    r, ro = TO.pack(refs)
    g = torch.tensor(groups)
    want = TO.ngram_overlap_counts(hyps, refs, groups, n_order)
    host = torch.ops.tmx.ngram_overlap(h, ho, r, ro, g, n_order)
    dev = torch.ops.tmx.ngram_overlap_gpu(*_cuda(h, ho, r, ro, g), n_order, bits, 512)
    for name, d, w, hst in zip(("match", "hyp_tot", "ref_tot"), dev, want, host):
        assert d.cpu().tolist() == w, (name, n_order, bits)
        assert torch.equal(d.cpu(), hst), name


# ------------------------------------------------------------------------------------------------------------- BLEU
@pytest.mark.parametrize("n_gram", [1, 2, 3, 4])
def test_bleu_stats_gpu_field_limit_and_ties(n_gram):
    hyps, refs, groups = TO.bleu_cases()
    assert max(max(s) for s in hyps + refs if s) == 65534 and max(len(x) for x in hyps) == 256
    h, ho = TO.pack(hyps)
    r, ro = TO.pack(refs)
    g = torch.tensor(groups)
    want = TO.bleu_counts(hyps, refs, groups, n_gram)
    host = torch.ops.tmx.bleu_stats(h, ho, r, ro, g, n_gram)
    dev = torch.ops.tmx.bleu_stats_gpu(*_cuda(h, ho, r, ro, g), n_gram, 256)
    for name, d, w, hst in zip(("num", "den", "lens"), dev, want, host):
        assert torch.equal(d.cpu(), torch.tensor(w, dtype=torch.float64).reshape(d.shape)), name
        assert torch.equal(d.cpu(), hst), name
    assert dev[2][-3:].cpu().tolist() == [[64.0, 60.0], [65.0, 70.0], [7.0, 0.0]]  # equal distance: the first reference wins


# -------------------------------------------------------------------------------------------------------------- TER
def _ter_packed(plants):
    a, ao = TO.pack([p[0] for p in plants], torch.int32)  # references: the side that is shifted
    b, bo = TO.pack([p[1] for p in plants], torch.int32)
    return a, ao, b, bo


def _host_ter(packed, count):
    a, ao, b, bo = packed
    return torch.ops.tmx.ter_batch(b.long(), bo, a.long(), ao, torch.arange(count + 1))[0]


@pytest.fixture(scope="module")
def ter_natural():
    """Run (a): the plants with one pair per wave (scratch sized by the longest sentence of the batch)."""
    plants = TO.ter_plants()
    packed = _ter_packed(plants)
    max_a, max_b = max(len(p[0]) for p in plants), max(len(p[1]) for p in plants)
    return plants, packed, torch.ops.tmx.ter_gpu(*_cuda(*packed), max_a, max_b).cpu()


def test_ter_gpu_plants_one_pair_per_wave(ter_natural):
    plants, packed, got = ter_natural
    want = [float(p[2]) for p in plants]
    assert got.tolist() == want, [(k, len(plants[k][0]), g, w) for k, (g, w) in enumerate(zip(got.tolist(), want)) if g != w][:8]
    assert torch.equal(got, _host_ter(packed, len(plants)))


def test_ter_gpu_grid_stride_on_capped_scratch(ter_natural):
    """The same pairs with 1023-word scratch: the 128 Mi-int cap leaves 92 waves, every wave walks two or three pairs,
    and the short and empty pairs at the end of the batch land on scratch that long pairs left behind."""
    plants, packed, natural = ter_natural
    assert len(plants) > 2 * 92 and all(max(len(p[0]), len(p[1])) <= 3 for p in plants[-6:])
    assert len(plants[0][0]) == 100 and not plants[-6][1] and not plants[-5][0]  # longest first; empty sides past the grid
    got = torch.ops.tmx.ter_gpu(*_cuda(*packed), 1023, 1023).cpu()
    assert torch.equal(got, natural)


def test_ter_gpu_wave_cap():
    """1100 short pairs at their natural maxima: the grid stops at 1024 waves and 76 of them take a second pair."""
    plants = TO.ter_short_batch(1100)
    packed = _ter_packed(plants)
    got = torch.ops.tmx.ter_gpu(*_cuda(*packed), max(len(p[0]) for p in plants), max(len(p[1]) for p in plants)).cpu()
    assert got.tolist() == [float(p[2]) for p in plants]
    assert torch.equal(got, _host_ter(packed, len(plants)))


def test_ter_module_strides_with_one_long_pair(monkeypatch):
    """600 pairs through the metric, one of them 400 words long: the scratch cap leaves fewer than 600 waves, so the
    production call itself strides."""
    import torchmetrics_forked_amd as tm

    dev_op = count_calls(monkeypatch, torch.ops.tmx, "ter_gpu")
    host_op = count_calls(monkeypatch, torch.ops.tmx, "ter_batch")
    plants = TO.ter_short_batch(599)
    plants.insert(300, TO.ter_long_pair(400))
    text = lambda ids: " ".join(f"w{x}" for x in ids)  # noqa: E731
    preds, target = [text(p[1]) for p in plants], [[text(p[0])] for p in plants]
    g = tm.text.TranslationEditRate(return_sentence_level_score=True).cuda()
    c = tm.text.TranslationEditRate(return_sentence_level_score=True)
    g.update(preds, target)
    assert (len(dev_op), len(host_op)) == (1, 0)
    args = dev_op[0][0]
    assert args[1].numel() - 1 == 600 and max(args[4], args[5]) == 400
    c.update(preds, target)
    assert len(dev_op) == 1
    (gs, gsent), (cs, csent) = g.compute(), c.compute()
    torch.testing.assert_close(gs.cpu(), cs, rtol=0, atol=0)
    torch.testing.assert_close(gsent.cpu(), csent, rtol=0, atol=0)
    want = torch.tensor([float(p[2]) for p in plants]) / torch.tensor([float(len(p[0])) for p in plants])  # fp32, as the metric
    assert torch.equal(torch.stack([s.cpu().reshape(()) for s in gsent]), want)


# -------------------------------------------------------------------------------------------------------------- EED
def test_eed_gpu_empty_sides_and_jump_rows():
    from torchmetrics_forked_amd.functional.text.helper import _pack_codepoints

    hyps, refs = TO.eed_cases()
    assert len(hyps) == 257 and hyps[0] == "" and refs[1] == "" and (hyps[2], refs[2]) == ("", "") and set(refs[3]) == {" "}
    h, ho = _pack_codepoints(hyps)
    r, ro = _pack_codepoints(refs)
    host = torch.ops.tmx.eed_batch(h, ho, r, ro, *TO.EED_ARGS)
    longest = max(len(x) for x in hyps)
    for max_hyp in (longest, longest + 19):
        dev = torch.ops.tmx.eed_gpu(*_cuda(h, ho, r, ro), *TO.EED_ARGS, max_hyp)
        assert torch.equal(dev.cpu(), host)


# ----------------------------------------------------------------------------------------------------- limit checks
# name -> call on (t = torch.ops.tmx, a3 / o3: one sequence of 3 ids, a10 / o10: one of 10, i3 / i10: the same as int32,
# g1: one group of one reference).  Each must be refused by the op's own checks, before anything is launched.
_REFUSED = {
    "levenshtein-ref-1025": lambda t, a3, o3, a10, o10, i3, i10, g1: t.levenshtein_gpu(a3, o3, a3, o3, 1025),
    "lcs-ref-1025": lambda t, a3, o3, a10, o10, i3, i10, g1: t.lcs_gpu(a3, o3, a3, o3, 1025),
    "bleu-hyp-257": lambda t, a3, o3, a10, o10, i3, i10, g1: t.bleu_stats_gpu(a3, o3, a3, o3, g1, 4, 257),
    "bleu-order-5": lambda t, a3, o3, a10, o10, i3, i10, g1: t.bleu_stats_gpu(a3, o3, a3, o3, g1, 5, 3),
    "ngram-129-bits": lambda t, a3, o3, a10, o10, i3, i10, g1: t.ngram_overlap_gpu(a3, o3, a3, o3, g1, 3, 43, 3),
    "ngram-hyp-513": lambda t, a3, o3, a10, o10, i3, i10, g1: t.ngram_overlap_gpu(a3, o3, a3, o3, g1, 2, 8, 513),
    "ngram-hyp-above-declared": lambda t, a3, o3, a10, o10, i3, i10, g1: t.ngram_overlap_gpu(a10, o10, a3, o3, g1, 2, 8, 9),
    "beam-ref-above-declared": lambda t, a3, o3, a10, o10, i3, i10, g1: t.levenshtein_beam_gpu(a3, o3, a10, o10, 1, 1, 1, 9),
    "eed-hyp-above-declared": lambda t, a3, o3, a10, o10, i3, i10, g1: t.eed_gpu(a10, o10, a3, o3, *TO.EED_ARGS, 9),
    "ter-max-a-4096": lambda t, a3, o3, a10, o10, i3, i10, g1: t.ter_gpu(i3, o3, i3, o3, 4096, 3),
    "ter-ref-above-max-a": lambda t, a3, o3, a10, o10, i3, i10, g1: t.ter_gpu(i10, o10, i3, o3, 9, 3),
    "ter-hyp-above-max-b": lambda t, a3, o3, a10, o10, i3, i10, g1: t.ter_gpu(i3, o3, i10, o10, 3, 9),
}


@pytest.fixture(scope="module")
def tiny():
    a3, o3, a10, o10, g1 = _cuda(*TO.pack([[1, 2, 3]]), *TO.pack([list(range(10))]), torch.tensor([0, 1]))
    return torch.ops.tmx, a3, o3, a10, o10, a3.int(), a10.int(), g1


@pytest.mark.parametrize("name", sorted(_REFUSED))
def test_op_refuses_what_its_kernel_cannot_hold(tiny, name):
    with pytest.raises(RuntimeError):
        _REFUSED[name](*tiny)


def test_ops_accept_the_same_arguments_within_the_limits(tiny):
    t, a3, o3, a10, o10, i3, i10, g1 = tiny
    assert t.levenshtein_gpu(a10, o10, a3, o3, 1024).tolist() == [7] and t.lcs_gpu(a10, o10, a3, o3, 1024).tolist() == [3]
    assert t.ngram_overlap_gpu(a10, o10, a3, o3, g1, 2, 8, 10)[0].tolist() == [[3, 2]]
    assert t.levenshtein_beam_gpu(a3, o3, a10, o10, 1, 1, 1, 10).tolist() == [7]
    assert t.ter_gpu(i10, o10, i3, o3, 10, 3).tolist() == [7.0]
