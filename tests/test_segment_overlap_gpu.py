"""The class-overlap ops of ``csrc/segment_overlap.hip`` and the segmentation metrics on the GPU.

Counts are integers and are held to ``torch.equal`` against the per-pixel loop oracle of ``tests/helpers/segmentation_oracle.py``.  Scores
are held to ``|got - oracle| <= 2^-24 |oracle| + 1e-12``: the one fp32 rounding of an fp64 value (derived, not measured; the 1e-12 covers the
fp64 summation order).  Shapes come from the constants the library exports: every dtype's vector width, the chunk edges under
``TMX_SEGMENT_CHUNK``, the class cap.  Routes are proven with ``tests/helpers/routes.py``.
"""
import itertools
import pickle

import pytest
import torch

from tests.helpers import segmentation_oracle as so
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

THREADS, PIXELS, CAP, CHUNK = 256, 16, 4096, 4096  # asserted against segment_overlap_tile() below: parametrisation happens before the library is loaded
_INDEX_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)
_ONEHOT_DTYPES = (torch.bool, torch.uint8, torch.int32, torch.int64)
_I64 = torch.iinfo(torch.int64)


def _op():
    from torchmetrics_forked_amd.ops import segmentation as op

    ops.require()
    return op


def _functionals():
    from torchmetrics_forked_amd.functional.segmentation import dice_score, generalized_dice_score, mean_iou

    return mean_iou, dice_score, generalized_dice_score


def _index(p, t, C):
    return _op().segment_overlap_index(p.cuda(), t.cuda(), C).cpu()


def _onehot(p, t):
    return _op().segment_overlap_onehot(p.cuda(), t.cuda()).cpu()


def _pair(shape, C, seed, dp=torch.int64, dt=torch.int64, void=()):
    """Random preds against blocky-ish target (target = preds with a quarter of the pixels redrawn), with planted void labels."""
    p = so.random_labels(shape, C, seed)
    t = torch.where(so.random_labels(shape, 4, seed + 1) == 0, so.random_labels(shape, C, seed + 2), p)
    if void:
        p, t = so.plant(p, void, seed + 3, 0.05), so.plant(t, void, seed + 4, 0.05)
    return p.to(dp), t.to(dt)


def test_tile_is_what_the_shapes_assume():
    from torchmetrics_forked_amd.functional.segmentation import utils

    assert _op().segment_overlap_tile() == (THREADS, PIXELS, CAP, CHUNK)
    assert utils._SEGMENT_MAX_CLASSES == CAP
    assert CHUNK == THREADS * PIXELS


# ----------------------------------------------------------------------------------------------------- index form: sizes
@pytest.mark.parametrize("dtype", _INDEX_DTYPES)
def test_index_counts_at_the_vector_edges(dtype):
    """Spatial sizes 1, V - 1, V, V + 1, 2V + 1 for the dtype's vector width V; three rows (rows start unaligned: the generic kernel) and one row
    (the vector kernel with a run cut by the end of the row)."""
    V = 16 // torch.empty(0, dtype=dtype).element_size()
    C = 5
    for n in sorted({1, max(V - 1, 1), V, V + 1, 2 * V + 1}):
        for B in (1, 3):
            p, t = _pair((B, n), C, 10 * n + B, dtype, dtype, void=(C, 255))
            assert torch.equal(_index(p, t, C), so.counts(p, t, C)), (dtype, n, B)


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_index_counts_at_the_chunk_edges(monkeypatch, n):
    monkeypatch.setenv("TMX_SEGMENT_CHUNK", str(CHUNK))
    C = 21
    assert _op().segment_overlap_chunks(2, n, C, False) == (n + CHUNK - 1) // CHUNK
    for dp, dt in ((torch.int64, torch.int64), (torch.int64, torch.uint8), (torch.uint8, torch.uint8)):
        for B in (1, 2):
            p, t = _pair((B, n), C, n + B, dp, dt, void=(C, 255))
            assert torch.equal(_index(p, t, C), so.counts(p, t, C)), (dp, dt, B)


def test_index_counts_with_the_hosts_chunking():
    n = 5 * 2 * CHUNK + 17  # five minimum chunks and a little: cut in 5, rounded up to the alignment, makes 4 chunks of 3 steps
    assert _op().segment_overlap_chunks(3, n, 21, False) == 4
    p, t = _pair((3, n), 21, 5, void=(-1, 21))
    assert torch.equal(_index(p, t, 21), so.counts(p, t, 21))
    p, t = so.blocky_labels((3, 97, n // 97 + 1), 21, 32, 6), so.blocky_labels((3, 97, n // 97 + 1), 21, 24, 7)
    assert torch.equal(_index(p, t, 21), so.counts(p, t, 21))


def test_chunks_are_a_function_of_the_shape(monkeypatch):
    op = _op()
    assert op.segment_overlap_chunks(16, 512 * 512, 21, False) == op.segment_overlap_chunks(16, 512 * 512, 21, False)
    assert op.segment_overlap_chunks(1, 100, 3, False) == 1 and op.segment_overlap_chunks(70000, 4, 3, False) == 1
    assert op.segment_overlap_chunks(1, 64 * 2 * CHUNK, 3, False) == 64
    assert op.segment_overlap_chunks(1, 64 * 2 * CHUNK, 4, True) == 64  # one-hot: B·C rows share the grid
    monkeypatch.setenv("TMX_SEGMENT_CHUNK", "1")  # rounded up to the alignment
    assert op.segment_overlap_chunks(1, 3 * CHUNK, 3, False) == 3
    monkeypatch.setenv("TMX_SEGMENT_CHUNK", str(CHUNK + 1))
    assert op.segment_overlap_chunks(1, 4 * CHUNK, 3, False) == 2


# --------------------------------------------------------------------------------------------------- index form: classes
@pytest.mark.parametrize("C", [1, 2, 3, 21, 256, 257, CAP])
def test_index_counts_by_class_count(C):
    dt = torch.uint8 if C <= 257 else torch.int16  # uint8 reaches 255: the last class of 256, a middle class of 257
    p, t = _pair((2, 3001), C, C, torch.int64, torch.int64, void=(-1, C))
    t = t.clamp(-1, torch.iinfo(dt).max).to(dt)
    want = so.counts(p, t, C)
    got = _index(p, t, C)
    assert torch.equal(got, want)
    assert int(got[..., 1].sum()) == int(((p >= 0) & (p < C)).sum())  # every in-range pixel of preds is counted once


def test_above_the_cap_keeps_the_composition(monkeypatch):
    mean_iou, _, _ = _functionals()
    op = _op()
    C = CAP + 1
    p, t = _pair((2, 301), C, 3)
    with pytest.raises(RuntimeError, match="num_classes"):
        op.segment_overlap_index(p.cuda(), t.cuda(), C)
    calls = [count_calls(monkeypatch, torch.ops.tmx, n, guard=_raise) for n in ("segment_overlap_index", "segment_overlap_onehot", "segment_scores")]
    got = mean_iou(p.cuda(), t.cuda(), C, input_format="index")
    assert so.within_bound(got, so.mean_iou(so.counts(p, t, C)), "C = cap + 1, composition") <= 1.0
    assert not any(calls)


def _raise(*a, **k):
    raise AssertionError("a native segmentation op was entered on a call that keeps the composition")


# ---------------------------------------------------------------------------------------- index form: dtypes and layouts
def test_index_counts_for_every_dtype_pair():
    C = 7
    for dp, dt in itertools.product(_INDEX_DTYPES, _INDEX_DTYPES):
        for shape in ((3, 37, 29), (2, 64, 48)):  # rows that start unaligned; rows of whole vectors
            p, t = _pair(shape, C, 11, dp, dt, void=(C, 255))
            assert torch.equal(_index(p, t, C), so.counts(p, t, C)), (dp, dt, shape)


def _offset(x):
    """The same values behind a base pointer one element past a fresh allocation."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    return buf[1:].view(x.shape)


def test_index_counts_for_other_layouts():
    op = _op()
    C = 6
    for dtype in (torch.int64, torch.uint8):
        p, t = _pair((2, 40, 48), C, 21, dtype, dtype, void=(C,))
        want = so.counts(p, t, C)
        pd, td = p.cuda(), t.cuda()
        assert torch.equal(op.segment_overlap_index(_offset(pd), td, C).cpu(), want)
        assert torch.equal(op.segment_overlap_index(pd, _offset(td), C).cpu(), want)
        pt, tt = pd.transpose(1, 2), td.transpose(1, 2)  # non-contiguous views
        assert not pt.is_contiguous()
        assert torch.equal(op.segment_overlap_index(pt, tt, C).cpu(), want)
        wide = so.random_labels((2, 40, 96), C, 22, dtype).cuda()
        assert torch.equal(op.segment_overlap_index(wide[..., ::2], td, C).cpu(), so.counts(wide.cpu()[..., ::2], t, C))


def test_kernel_choice_by_alignment():
    op = _op()
    p, t = _pair((2, 64, 48), 5, 2)
    pd, td = p.cuda(), t.cuda()
    vec, generic = "segment_overlap_index_vec_kernel", "segment_overlap_index_generic_kernel"
    assert_route(kernels_run(lambda: op.segment_overlap_index(pd, td, 5)), present=(vec,), absent=(generic,))
    assert_route(kernels_run(lambda: op.segment_overlap_index(_offset(pd), td, 5)), present=(generic,), absent=(vec,))
    # 63 x 47 pixels: rows of neither side are a whole number of 16-byte vectors
    assert_route(kernels_run(lambda: op.segment_overlap_index(pd.to(torch.uint8)[:, :63, :47], td[:, :63, :47], 5)), present=(generic,), absent=(vec,))
    assert_route(kernels_run(lambda: op.segment_overlap_index(pd[:, :63, :47], td[:, :63, :47], 5)), present=(generic,), absent=(vec,))
    assert_route(kernels_run(lambda: op.segment_overlap_index(pd[:, :, :47], td[:, :, :47], 5)), present=(vec,), absent=(generic,))  # made contiguous: 64 · 47 · 8 bytes
    assert_route(kernels_run(lambda: op.segment_overlap_index(pd[:1, :63, :47], td[:1, :63, :47], 5)), present=(vec,), absent=(generic,))  # one row
    m = so.to_onehot(p, 5).cuda()
    vec, generic = "segment_overlap_onehot_vec_kernel", "segment_overlap_onehot_generic_kernel"
    assert_route(kernels_run(lambda: op.segment_overlap_onehot(m, m)), present=(vec,), absent=(generic,))
    assert_route(kernels_run(lambda: op.segment_overlap_onehot(m[:, :, :63, :47], m[:, :, :63, :47])), present=(generic,), absent=(vec,))  # planes start unaligned


# ------------------------------------------------------------------------------------------------ index form: planted labels
def test_planted_out_of_range_labels():
    C = 4
    base_p, base_t = _pair((3, 33, 31), C, 31)
    void = (-1, C, 255, _I64.min, _I64.max)
    sides = ((so.plant(base_p, void, 1), base_t), (base_p, so.plant(base_t, void, 2)), (so.plant(base_p, void, 3), so.plant(base_t, void, 3)),
             (so.plant(base_p, void, 4), so.plant(base_t, void, 5)))
    for p, t in sides:  # preds alone, target alone, both on the same pixels, both on other pixels
        want = so.counts(p, t, C)
        assert torch.equal(_index(p, t, C), want)
        assert int(want[..., 1].sum()) == int(((p >= 0) & (p < C)).sum()) and int(want[..., 2].sum()) == int(((t >= 0) & (t < C)).sum())
    # 255 is a class of its own once C reaches 256, and a void label below that
    p8, t8 = so.plant(base_p, (255,), 6).to(torch.uint8), so.plant(base_t, (255,), 7).to(torch.uint8)
    for C8 in (255, 256):
        assert torch.equal(_index(p8, t8, C8), so.counts(p8, t8, C8))
    # int16 / int32 negatives
    for dtype in (torch.int16, torch.int32):
        p, t = so.plant(base_p, (-1, torch.iinfo(dtype).min, torch.iinfo(dtype).max), 8).to(dtype), base_t.to(dtype)
        assert torch.equal(_index(p, t, C), so.counts(p, t, C))


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_contention_modes_agree(monkeypatch, mode):
    """Plain atomics, the wave-uniform path and per-lane run merging count the same pixels: one class everywhere (full contention: the count
    is the pixel count), blocky maps whose blocks straddle wave and chunk edges, and random labels."""
    monkeypatch.setenv("TMX_SEGMENT_MODE", mode)
    monkeypatch.setenv("TMX_SEGMENT_CHUNK", str(CHUNK))
    C = 3
    for dtype in (torch.int64, torch.uint8):
        n = 2 * CHUNK + 3
        p = so.constant_labels((2, n), 2, dtype)
        got = _index(p, p, C)
        assert got[:, 2].tolist() == [[n, n, n]] * 2 and int(got[:, :2].sum()) == 0
        assert torch.equal(_index(p, so.constant_labels((2, n), 1, dtype), C)[0], torch.tensor([[0, 0, 0], [0, 0, n], [0, n, 0]]))
        for block in (24, 32, 100):  # 24: a block ends inside a wave's span of a row; 100-wide rows: blocks straddle the chunk edges
            p, t = so.blocky_labels((2, 90, 100), C, block, block, dtype), so.blocky_labels((2, 90, 100), C, block + 8, block + 1, dtype)
            assert torch.equal(_index(p, t, C), so.counts(p, t, C)), (dtype, block)
        p, t = _pair((2, 2 * CHUNK + 3), C, 17, dtype, dtype, void=(C,))
        assert torch.equal(_index(p, t, C), so.counts(p, t, C))


def test_more_samples_than_a_grid_axis():
    """70 000 samples of 2 x 2: the sample index does not fit a 16-bit grid axis."""
    p, t = _pair((70000, 2, 2), 3, 9, void=(3,))
    assert torch.equal(_index(p, t, 3), so.counts(p, t, 3))


# ------------------------------------------------------------------------------------------------------------ one-hot form
@pytest.mark.parametrize("C", [1, 21])
def test_onehot_counts_by_plane_size(monkeypatch, C):
    """Plane sizes around the 16-byte load and the chunk edges; with more than one plane most sizes make planes start unaligned."""
    monkeypatch.setenv("TMX_SEGMENT_CHUNK", str(CHUNK))
    for n in (1, 15, 16, 17, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        lp, lt = _pair((2, n), C + 1, n + C)  # the label C is in no plane
        for dtype in (torch.bool, torch.int64):
            p, t = so.to_onehot(lp, C, dtype), so.to_onehot(lt, C, dtype)
            want = so.counts(lp, lt, C)
            assert torch.equal(_onehot(p, t), want), (n, dtype)
            assert torch.equal(_onehot(p[:1, :1], t[:1, :1]), want[:1, :1])  # a single plane: the vector kernel with a cut run


def test_onehot_counts_for_every_dtype_pair():
    C = 3
    for shape in ((2, 37, 29), (2, 64, 48)):
        lp, lt = _pair(shape, C + 1, 13)
        want = so.counts(lp, lt, C)
        for dp, dt in itertools.product(_ONEHOT_DTYPES, _ONEHOT_DTYPES):
            p, t = so.to_onehot(lp, C, dp), so.to_onehot(lt, C, dt)
            assert torch.equal(_onehot(p, t), want), (dp, dt, shape)
            if dp != torch.bool and dt != torch.bool:  # nonzero values other than 1, negative ones and the high byte alone
                p2 = p * torch.tensor(2 if dp == torch.uint8 else -7, dtype=dp)
                t2 = t * torch.tensor(128 if dt == torch.uint8 else 1 << 24, dtype=dt)
                assert torch.equal(_onehot(p2, t2), want), (dp, dt, shape)


def test_onehot_all_zero_and_all_one_planes():
    n = CHUNK + 17
    for dtype in _ONEHOT_DTYPES:
        p = torch.zeros(2, 3, n, dtype=dtype)
        p[:, 1] = 1
        t = torch.ones(2, 3, n, dtype=dtype)
        t[:, 2] = 0
        assert _onehot(p, t).tolist() == [[[0, 0, n], [n, n, n], [0, 0, 0]]] * 2
    big = torch.full((1, 2, 3 * CHUNK), 255, dtype=torch.uint8)
    assert _onehot(big, big).tolist() == [[[3 * CHUNK] * 3] * 2]


def test_both_forms_agree_and_runs_are_bit_equal():
    C = 21
    lp, lt = _pair((3, 50, 64), C, 41, void=(-1, C))
    pd, td = lp.cuda(), lt.cuda()
    op = _op()
    a = op.segment_overlap_index(pd, td, C)
    b = op.segment_overlap_index(pd, td, C)
    c = op.segment_overlap_onehot(so.to_onehot(lp, C).cuda(), so.to_onehot(lt, C, torch.uint8).cuda())
    d = op.segment_overlap_onehot(so.to_onehot(lp, C).cuda(), so.to_onehot(lt, C, torch.uint8).cuda())
    assert a.dtype == torch.int64 and a.shape == (3, C, 3)
    assert torch.equal(a, b) and torch.equal(c, d) and torch.equal(a, c) and torch.equal(a.cpu(), so.counts(lp, lt, C))


def test_empty_inputs_return_zeros_without_a_launch():
    op = _op()
    z = torch.zeros(0, 8, 8, dtype=torch.int64, device="cuda")
    assert op.segment_overlap_index(z, z, 3).shape == (0, 3, 3)
    e = torch.zeros(2, 0, 8, dtype=torch.int64, device="cuda")
    assert torch.equal(op.segment_overlap_index(e, e, 3).cpu(), torch.zeros(2, 3, 3, dtype=torch.int64))
    m = torch.zeros(2, 3, 0, dtype=torch.bool, device="cuda")
    assert torch.equal(op.segment_overlap_onehot(m, m).cpu(), torch.zeros(2, 3, 3, dtype=torch.int64))
    assert op.segment_scores(op.segment_overlap_index(z, z, 3), 0, 0, True).shape == (0,)
    names = kernels_run(lambda: (op.segment_overlap_index(e, e, 3), op.segment_overlap_onehot(m, m)))  # the result's fill only
    assert_route(names, absent=("segment_overlap",))


# ------------------------------------------------------------------------------------------------------------------ scores
def _forms(include_background_values=(True, False)):
    mean_iou, dice_score, generalized_dice_score = _functionals()
    out = []
    for bg in include_background_values:
        for pc in (False, True):
            kw = {"include_background": bg, "per_class": pc}
            out.append((mean_iou, kw, so.mean_iou, kw))
        for avg in ("micro", "macro", "weighted", "none", None):
            kw = {"include_background": bg, "average": avg}
            out.append((dice_score, kw, so.dice, kw))
        for wt in ("square", "simple", "linear"):
            for pc in (False, True):
                kw = {"include_background": bg, "per_class": pc, "weight_type": wt}
                out.append((generalized_dice_score, kw, so.generalized_dice, kw))
    return out


def _score_case():
    """Six samples of 23 x 19 and five classes with the planted cases: class 3 absent from the target of sample 1 only (weight replacement),
    sample 2 with an empty target throughout (no finite weight: generalized Dice 0), class 2 absent from both sides of sample 3 (its term
    is 0), sample 4 = a perfect prediction, sample 5 with one class only."""
    C = 5
    p, t = _pair((6, 23, 19), C, 77, void=(-1, C))
    t[1][t[1] == 3] = 0
    t[2] = -1
    p[3][p[3] == 2] = 1
    t[3][t[3] == 2] = 1
    p[4] = t[4]
    p[5], t[5] = 4, 4
    return C, p, t


@pytest.mark.parametrize("input_format", ["index", "one-hot"])
def test_scores_against_the_fp64_oracle(input_format):
    C, p, t = _score_case()
    k = so.counts(p, t, C)
    assert int(k[1, 3, 2]) == 0 and int(k[1, 3, 1]) > 0 and int(k[2, :, 2].sum()) == 0 and int(k[3, 2].sum()) == 0  # the planted cases are there
    pd, td = (p.cuda(), t.cuda()) if input_format == "index" else (so.to_onehot(p, C).cuda(), so.to_onehot(t, C, torch.uint8).cuda())
    for fn, kwargs, oracle, okw in _forms():
        got = fn(pd, td, C, input_format=input_format, **kwargs)
        want = oracle(k, **okw)
        per_class = kwargs.get("per_class", False) or kwargs.get("average", "micro") in ("none", None)
        assert got.dtype == torch.float32 and got.is_cuda
        assert got.shape == ((6, C - (0 if kwargs["include_background"] else 1)) if per_class else (6,))
        assert so.within_bound(got, want, f"{fn.__name__} {kwargs} {input_format}") <= 1.0
    mean_iou, dice_score, generalized_dice_score = _functionals()
    assert float(generalized_dice_score(pd, td, C, input_format=input_format)[2]) == 0.0  # an empty target: no finite weight
    assert float(mean_iou(pd, td, C, per_class=True, input_format=input_format)[3, 2]) == 0.0  # absent from both sides
    assert float(dice_score(pd, td, C, input_format=input_format)[4]) == 1.0 and float(mean_iou(pd, td, C, input_format=input_format)[5]) == float(torch.tensor(0.2, dtype=torch.float32))


def test_score_kernel_alone_with_many_classes():
    """More classes than a wave has lanes, so a lane takes several: 130 classes, every form, against the oracle on the same counts."""
    op = _op()
    g = torch.Generator().manual_seed(3)
    i = torch.randint(0, 50, (4, 130), generator=g)
    k = torch.stack([i, i + torch.randint(0, 50, (4, 130), generator=g), i + torch.randint(0, 50, (4, 130), generator=g)], dim=-1)
    k[0, 5:40] = 0
    k[1, :, 2] = 0
    k[1, :, 0] = 0
    kd = k.cuda()
    for bg in (True, False):
        for pc in (0, 1):
            assert so.within_bound(op.segment_scores(kd, op.METRIC_IOU, pc, bg), so.mean_iou(k, bg, bool(pc)), f"scores iou {pc} {bg}") <= 1.0
        for avg, code in op.DICE_OPTIONS.items():
            assert so.within_bound(op.segment_scores(kd, op.METRIC_DICE, code, bg), so.dice(k, bg, avg), f"scores dice {avg} {bg}") <= 1.0
        for wt, code in op.WEIGHT_OPTIONS.items():
            for pc in (0, 1):
                got = op.segment_scores(kd, op.METRIC_GENERALIZED_DICE, code + 3 * pc, bg)
                assert got.dtype == torch.float64
                assert so.within_bound(got, so.generalized_dice(k, bg, bool(pc), wt), f"scores gds {wt} {pc} {bg}") <= 1.0


# ------------------------------------------------------------------------------------------------------------------ routes
_NATIVE_MARKS = ("segment_overlap_", "segment_scores_kernel")
_COMPOSITION_MARKS = ("CompareEq", "reduce_kernel")  # aten's comparison expansion and reduction of the composition
_EXPANSION_MARKS = ("CompareEq", "reduce_kernel", "one_hot", "scatter", "BitwiseAnd")


def test_routes(monkeypatch):
    from torchmetrics_forked_amd.segmentation import DiceScore, GeneralizedDiceScore, MeanIoU

    C, p, t = _score_case()
    pd, td = p.cuda(), t.cuda()
    po, to = so.to_onehot(p, C).cuda(), so.to_onehot(t, C).cuda()
    index_calls = count_calls(monkeypatch, torch.ops.tmx, "segment_overlap_index")
    onehot_calls = count_calls(monkeypatch, torch.ops.tmx, "segment_overlap_onehot")
    score_calls = count_calls(monkeypatch, torch.ops.tmx, "segment_scores")
    n = 0
    for fn, kwargs, _, _ in _forms((True,)):
        names = kernels_run(lambda: fn(pd, td, C, input_format="index", **kwargs))  # (two calls: a warm-up and the profiled one)
        assert_route(names, present=("segment_overlap_index", "segment_scores_kernel"), absent=_EXPANSION_MARKS)
        names = kernels_run(lambda: fn(po, to, C, **kwargs))
        assert_route(names, present=("segment_overlap_onehot", "segment_scores_kernel"), absent=_EXPANSION_MARKS)
        n += 2
        assert len(index_calls) == n and len(onehot_calls) == n and len(score_calls) == 2 * n  # one overlap call per functional call
    for cls, kwargs in ((MeanIoU, {}), (DiceScore, {"average": "macro"}), (GeneralizedDiceScore, {"per_class": True})):
        m = cls(C, input_format="index", **kwargs).cuda()
        before = len(index_calls)
        m.update(pd, td)
        assert len(index_calls) == before + 1 and len(onehot_calls) == n  # one overlap call per update
        m(pd, td)
        assert len(index_calls) == before + 2  # forward: one update's worth, the batch value comes from the same counts
    # kept on the composition, with every op made to raise: unsupported dtypes (the two forms have their own sets), CPU tensors
    for name in ("segment_overlap_index", "segment_overlap_onehot", "segment_scores"):
        monkeypatch.setattr(torch.ops.tmx, name, _raise)
    mean_iou, dice_score, _ = _functionals()
    names = kernels_run(lambda: mean_iou(pd.to(torch.int8), td, C, input_format="index"))
    for mark in _COMPOSITION_MARKS:  # the guard is live: every mark is a real kernel name of the composition
        assert any(mark in k for k in names), (mark, sorted(set(names)))
    assert_route(names, absent=_NATIVE_MARKS)
    assert_route(kernels_run(lambda: dice_score(po.to(torch.int16), to, C)), absent=_NATIVE_MARKS)
    k = so.counts(p, t, C)
    assert so.within_bound(mean_iou(pd.to(torch.int8), td, C, input_format="index"), so.mean_iou(k), "kept: int8 labels") <= 1.0
    assert so.within_bound(dice_score(po.to(torch.int16), to, C), so.dice(k), "kept: int16 masks") <= 1.0
    assert so.within_bound(mean_iou(p, t, C, input_format="index"), so.mean_iou(k), "kept: CPU") <= 1.0
    # the composition on the GPU agrees with the CPU on out-of-range labels, and neither raises
    from torchmetrics_forked_amd.functional.segmentation import utils

    void = so.plant(p, (-1, C, 255, _I64.min, _I64.max), 5)
    on_gpu = utils._overlap_composition(void.cuda(), td.to(torch.uint8), C, "index")
    assert torch.equal(on_gpu.cpu(), utils._overlap_composition(void, t.to(torch.uint8), C, "index"))
    assert torch.equal(on_gpu.cpu(), so.counts(void, t.to(torch.uint8), C))


# ------------------------------------------------------------------------------------------------- memory and host reads
def test_no_expansion():
    """4 x 512 x 512 int64 labels, 21 classes: one input is 8 MiB.  The native route allocates the [4, 21, 3] counts and the scores only; the
    one-hot composition would allocate two 176 MiB tensors."""
    mean_iou, _, _ = _functionals()
    pd, td = (x.cuda() for x in _pair((4, 512, 512), 21, 8))
    mean_iou(pd, td, 21, input_format="index")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = mean_iou(pd, td, 21, input_format="index")
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f"mean_iou peak growth {grew} bytes, one input {pd.numel() * pd.element_size()}")
    assert grew < pd.numel() * pd.element_size()
    assert out.shape == (4,)


def test_no_host_read():
    from torchmetrics_forked_amd.segmentation import DiceScore, GeneralizedDiceScore, MeanIoU

    C, p, t = _score_case()
    pd, td = p.cuda(), t.cuda()
    po, to = so.to_onehot(p, C).cuda(), so.to_onehot(t, C, torch.int32).cuda()
    modules = [MeanIoU(C, input_format="index").cuda(), DiceScore(C, average="none", input_format="index").cuda(),
               GeneralizedDiceScore(C, input_format="index").cuda()]

    def run():
        out = [fn(pd, td, C, input_format="index", **kw) for fn, kw, _, _ in _forms((True,))]
        out += [fn(po, to, C, **kw) for fn, kw, _, _ in _forms((False,))]
        for m in modules:
            m.update(pd, td)
        return out

    want = run()  # (first calls outside the guarded region)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ----------------------------------------------------------------------------------------------------------------- modules
def test_modules_end_to_end():
    from torchmetrics_forked_amd.segmentation import DiceScore, GeneralizedDiceScore, MeanIoU

    C = 5
    p, t = _pair((8, 23, 19), C, 55, void=(C,))
    pd, td = p.cuda(), t.cuda()
    k = so.counts(p, t, C)
    cases = ((MeanIoU, {}, so.mean_iou, {}), (MeanIoU, {"per_class": True, "include_background": False}, so.mean_iou, {"per_class": True, "include_background": False}),
             (DiceScore, {"average": "weighted"}, so.dice, {"average": "weighted"}), (DiceScore, {"average": None}, so.dice, {"average": None}),
             (GeneralizedDiceScore, {"weight_type": "simple"}, so.generalized_dice, {"weight_type": "simple"}),
             (GeneralizedDiceScore, {"per_class": True}, so.generalized_dice, {"per_class": True}))
    for cls, kwargs, oracle, okw in cases:
        want = oracle(k, **okw)
        m = cls(C, input_format="index", **kwargs).cuda()
        first = m(pd[:3], td[:3])  # forward returns the batch value
        assert first.dtype == torch.float32 and so.within_bound(first, want[:3].mean(0), f"{cls.__name__} forward") <= 1.0
        m.update(pd[3:], td[3:])  # 3 + 5 samples: the mean over all 8, not the mean of two batch means
        got = m.compute()
        assert got.dtype == torch.float32 and got.is_cuda and int(m.samples) == 8
        assert so.within_bound(got, want.mean(0), f"{cls.__name__} {kwargs} 3 + 5") <= 1.0
        assert m.score.dtype == torch.float64 and m.samples.dtype == torch.int64
        twin = m.clone()
        assert torch.equal(twin.compute(), got)
        assert m.state_dict() == {}  # states are not persistent by default, as every metric's
        m.persistent(True)
        fresh = cls(C, input_format="index", **kwargs).cuda()
        fresh.persistent(True)
        fresh.load_state_dict(m.state_dict())
        assert torch.equal(fresh.compute(), got)
        assert torch.equal(pickle.loads(pickle.dumps(m)).compute(), got)
        m.reset()
        assert int(m.samples) == 0 and not bool(m.score.any())
        m.update(pd, td)
        assert so.within_bound(m.compute(), want.mean(0), f"{cls.__name__} after reset") <= 1.0


# ------------------------------------------------------------------------------------------------------------- host checks
def test_host_checks(monkeypatch):
    from torchmetrics_forked_amd.segmentation import MeanIoU

    op = _op()
    lab = torch.zeros(2, 8, 8, dtype=torch.int64, device="cuda")
    mask = torch.zeros(2, 3, 8, 8, dtype=torch.bool, device="cuda")
    for bad_p, bad_t, C, match in ((lab.cpu(), lab.cpu(), 3, "'CPU' backend"), (lab, lab.cpu(), 3, "GPU tensors"), (lab, lab[..., :7], 3, "matching shapes"),
                                   (lab[:, 0, 0], lab[:, 0, 0], 3, "matching shapes"), (lab.float(), lab, 3, "unsupported label dtype"),
                                   (lab, lab.to(torch.int8), 3, "unsupported label dtype"), (lab, lab, 0, "num_classes")):
        with pytest.raises(RuntimeError, match=match):
            op.segment_overlap_index(bad_p, bad_t, C)
    for bad_p, bad_t, match in ((mask, mask.cpu(), "GPU tensors"), (mask, mask[:, :2], "matching shapes"), (mask[:, :, 0, 0], mask[:, :, 0, 0], "matching shapes"),
                                (mask.half(), mask, "unsupported mask dtype"), (mask, mask.to(torch.int16), "unsupported mask dtype")):
        with pytest.raises(RuntimeError, match=match):
            op.segment_overlap_onehot(bad_p, bad_t)
    k = torch.zeros(2, 3, 3, dtype=torch.int64, device="cuda")
    for bad, metric, option, bg, match in ((k.int(), 0, 0, True, "int64 counts"), (k[..., :2], 0, 0, True, "int64 counts"), (k, 3, 0, True, "metric"),
                                           (k, 0, 2, True, "option"), (k, 1, 4, True, "option"), (k, 2, 6, True, "option"), (k[:, :1], 0, 0, False, "no class left")):
        with pytest.raises(RuntimeError, match=match):
            op.segment_scores(bad, metric, option, bg)
    # the functionals and modules raise ValueError before any launch
    calls = [count_calls(monkeypatch, torch.ops.tmx, n, guard=_raise) for n in ("segment_overlap_index", "segment_overlap_onehot", "segment_scores")]
    mean_iou, dice_score, generalized_dice_score = _functionals()
    for fn in (mean_iou, dice_score, generalized_dice_score):
        for args, kwargs in (((mask.float(), mask, 3), {}), ((mask, mask[..., :7], 3), {}), ((mask, mask, 4), {}), ((mask[:, :1], mask[:, :1], 1), {"include_background": False}),
                             ((lab, lab.double(), 3), {"input_format": "index"}), ((lab, lab, 3), {"input_format": "labels"})):
            with pytest.raises(ValueError):
                fn(*args, **kwargs)
    with pytest.raises(ValueError, match="average"):
        dice_score(mask, mask, 3, average="mean")
    with pytest.raises(ValueError, match="weight_type"):
        generalized_dice_score(mask, mask, 3, weight_type="cubic")
    with pytest.raises(ValueError, match="per_class"):
        mean_iou(mask, mask, 3, per_class=None)
    m = MeanIoU(3).cuda()
    with pytest.raises(ValueError, match="channels"):
        m.update(mask[:, :2], mask[:, :2])
    assert not any(calls)
