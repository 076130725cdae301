"""The plain oracles of tests/helpers/text_oracle.py against the host string ops (csrc/text.cpp) on the planted cases
that tests/test_text_kernels_gpu.py sends to the device kernels, and, where the reference package is at hand, the band
rule and the TER plants against the reference's pure-Python functions.  No GPU."""
import random

import pytest
import torch

from tests.helpers import text_oracle as TO
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.skipif(not ops.load(), reason="native library not built")


@pytest.fixture(scope="module")
def lev_calls():
    return TO.lev_calls()


def test_numpy_rows_equal_the_full_tables(lev_calls):
    """The numpy forms used for the long pairs give the textbook tables' values wherever both are affordable, and the
    planted distance / LCS of every pair is what its oracle computes."""
    for call in lev_calls:
        for label, a, b, dist, lcs in call:
            if len(a) * len(b) <= TO.LEV_NP_ABOVE:
                assert TO.levenshtein_unit_np(a, b) == TO.levenshtein_full(a, b), label
                assert TO.lcs_np(a, b) == TO.lcs_full(a, b), label
            if dist is not None:
                assert TO.lev_oracle(a, b) == (dist, lcs), label
    rng = random.Random(1)
    for _ in range(40):  # a weighted table at unit costs is the unit table
        a, b = [rng.randrange(3) for _ in range(rng.randint(0, 30))], [rng.randrange(3) for _ in range(rng.randint(0, 30))]
        assert TO.levenshtein_full(a, b, 1, 1, 1) == TO.levenshtein_unit_np(a, b)


def test_host_levenshtein_and_lcs_equal_oracles(lev_calls):
    for call in lev_calls:
        a, ao = TO.pack([c[1] for c in call])
        b, bo = TO.pack([c[2] for c in call])
        want = [TO.lev_oracle(c[1], c[2]) for c in call]
        assert torch.ops.tmx.levenshtein_batch(a, ao, b, bo).tolist() == [w[0] for w in want]
        assert torch.ops.tmx.lcs_batch(a, ao, b, bo).tolist() == [w[1] for w in want]


@pytest.mark.parametrize("costs", TO.BEAM_COSTS)
def test_host_beam_equals_band_oracle(costs):
    pairs = TO.beam_cases()
    a, ao = TO.pack([p for p, _ in pairs])
    b, bo = TO.pack([r for _, r in pairs])
    got = torch.ops.tmx.levenshtein_beam_batch(a, ao, b, bo, *costs).tolist()
    assert got == [TO.levenshtein_band(p, r, *costs) for p, r in pairs]
    small = [k for k, (p, r) in enumerate(pairs) if len(p) <= 20 and len(r) <= 20]
    assert len(small) > 40
    for k in small:  # the band covers the whole table
        assert got[k] == TO.levenshtein_full(*pairs[k], *costs), k


@pytest.mark.parametrize("costs", [(2, 3, 1), (3, 2, 5)])
def test_band_oracle_equals_reference(reference, costs):
    from torchmetrics.functional.text.helper import _LevenshteinEditDistance

    ins, dele, sub = costs
    for k, (p, r) in enumerate(TO.beam_cases()[::2]):
        ref = _LevenshteinEditDistance([str(x) for x in r], op_insert=ins, op_delete=dele, op_substitute=sub)
        assert ref([str(x) for x in p])[0] == TO.levenshtein_band(p, r, ins, dele, sub), (k, len(p), len(r))


@pytest.mark.parametrize("n_order,bits", TO.NGRAM_CONFIGS)
def test_host_ngram_overlap_equals_counter_oracle(n_order, bits):
    ids = TO.ngram_ids(bits, random.Random(bits))
    hyps, refs, groups = TO.ngram_cases(n_order, ids, TO.ngram_hyp_lens(n_order), seed=100 * n_order + bits, bits=bits)
    h, ho = TO.pack(hyps)
    r, ro = TO.pack(refs)
    got = torch.ops.tmx.ngram_overlap(h, ho, r, ro, torch.tensor(groups), n_order)
    for g, w in zip(got, TO.ngram_overlap_counts(hyps, refs, groups, n_order)):
        assert g.tolist() == w


@pytest.mark.parametrize("n_order,bits", TO.NGRAM_CONFIGS)
def test_ngram_plants_reach_the_high_key_word(n_order, bits):
    """The 128-bit key written out with Python integers (fields of id + 1, first token most significant): the first two
    plants differ above bit 63 only whenever the key is wider than 64 bits, and both occur in a hypothesis and a reference."""
    ids = TO.ngram_ids(bits, random.Random(bits))
    plants = TO.ngram_plants(n_order, ids, bits)

    def key(gram):
        k = 0
        for t in gram:
            field = (t + 1) % 2 ** 64
            assert 0 < field < 2 ** bits
            k = (k << bits) | field
        return k

    assert len({key(g) for g in plants}) == len(plants)
    if n_order * bits > 64:
        diff = key(plants[0]) ^ key(plants[1])
        assert diff and diff % 2 ** 64 == 0
    hyps, refs, _ = TO.ngram_cases(n_order, ids, TO.ngram_hyp_lens(n_order), seed=100 * n_order + bits, bits=bits)
    grams = lambda seqs: {tuple(s[j:j + n_order]) for s in seqs for j in range(len(s) - n_order + 1)}  # noqa: E731
    assert {tuple(plants[0]), tuple(plants[1])} <= grams(hyps) & grams(refs)


@pytest.mark.parametrize("n_gram", [1, 2, 3, 4])
def test_host_bleu_stats_equal_counter_oracle(n_gram):
    hyps, refs, groups = TO.bleu_cases()
    h, ho = TO.pack(hyps)
    r, ro = TO.pack(refs)
    got = torch.ops.tmx.bleu_stats(h, ho, r, ro, torch.tensor(groups), n_gram)
    for g, w in zip(got, TO.bleu_counts(hyps, refs, groups, n_gram)):
        assert torch.equal(g, torch.tensor(w, dtype=torch.float64).reshape(g.shape))
    assert got[2][-3:].tolist() == [[64.0, 60.0], [65.0, 70.0], [7.0, 0.0]]  # equal distance: the first reference wins


def _host_ter(plants):
    a, ao = TO.pack([p[0] for p in plants])  # references: the side that is shifted
    b, bo = TO.pack([p[1] for p in plants])
    edits, _ = torch.ops.tmx.ter_batch(b, bo, a, ao, torch.arange(len(plants) + 1))
    return edits.tolist()


def test_host_ter_scores_the_plants():
    for plants in (TO.ter_plants(), TO.ter_short_batch(), [TO.ter_long_pair()]):
        assert _host_ter(plants) == [float(p[2]) for p in plants]


def test_reference_ter_scores_the_plants(reference):
    """A spread of the plants (every eighth of the long ones, all degenerate ones, 40 short ones) in the reference's
    pure-Python shift search."""
    from torchmetrics.functional.text.ter import _translation_edit_rate

    plants = TO.ter_plants()
    for ref, hyp, edits in plants[::8] + plants[-6:] + TO.ter_short_batch()[:40]:
        got = _translation_edit_rate([str(x) for x in ref], [str(x) for x in hyp])
        assert float(got) == float(edits), (ref, hyp)
