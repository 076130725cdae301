"""Segmentation metrics on the CPU: the oracle on a hand-computed case, the package's composition against the oracle (counts exact,
scores within one fp32 rounding), the native gate arm by arm, no native call for CPU tensors, the modules on 2 gloo ranks and pickle."""
import pickle

import pytest
import torch

import torchmetrics_forked_amd.functional.segmentation.utils as seg_utils
import torchmetrics_forked_amd.ops.segmentation as ops_seg
from tests.helpers import segmentation_oracle as so
from tests.helpers.ddp import run_ddp
from tests.helpers.routes import count_calls
from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.functional.segmentation import dice_score, generalized_dice_score, mean_iou
from torchmetrics_forked_amd.segmentation import DiceScore, GeneralizedDiceScore, MeanIoU

_I64 = torch.iinfo(torch.int64)


def _forms(include_background_values=(True, False)):
    """(functional, kwargs, oracle function, oracle kwargs) of every metric, option and ``include_background``."""
    out = []
    for bg in include_background_values:
        for pc in (False, True):
            out.append((mean_iou, {"include_background": bg, "per_class": pc}, so.mean_iou, {"include_background": bg, "per_class": pc}))
        for avg in ("micro", "macro", "weighted", "none", None):
            out.append((dice_score, {"include_background": bg, "average": avg}, so.dice, {"include_background": bg, "average": avg}))
        for wt in ("square", "simple", "linear"):
            for pc in (False, True):
                kw = {"include_background": bg, "per_class": pc, "weight_type": wt}
                out.append((generalized_dice_score, kw, so.generalized_dice, kw))
    return out


def test_oracle_on_a_hand_computed_case():
    # sample 0: preds 0 1 / 1 2, target 0 1 / 2 2;  sample 1: preds all 1, target 0 0 / 7 1 (7: no class), class 2 absent from both
    p = torch.tensor([[[0, 1], [1, 2]], [[1, 1], [1, 1]]])
    t = torch.tensor([[[0, 1], [2, 2]], [[0, 0], [7, 1]]])
    k = so.counts(p, t, 3)
    assert k.dtype == torch.int64
    assert k.tolist() == [[[1, 1, 1], [1, 2, 1], [1, 1, 2]], [[0, 0, 2], [1, 4, 1], [0, 0, 0]]]
    assert torch.equal(so.counts(so.to_onehot(p, 3), so.to_onehot(t, 3, torch.int32) * 5, 3, "one-hot"), k)
    f64 = torch.float64
    assert torch.allclose(so.mean_iou(k), torch.tensor([(1 + 0.5 + 0.5) / 3, (0 + 0.25 + 0) / 3], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.mean_iou(k, per_class=True), torch.tensor([[1, 0.5, 0.5], [0, 0.25, 0]], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.mean_iou(k, include_background=False), torch.tensor([0.5, 0.125], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.dice(k), torch.tensor([6 / 8, 2 / 7], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.dice(k, average="none"), torch.tensor([[1, 2 / 3, 2 / 3], [0, 0.4, 0]], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.dice(k, average="macro"), torch.tensor([7 / 9, 0.4 / 3], dtype=f64), rtol=0, atol=1e-15)
    # weighted: T / ΣT = (1/4, 1/4, 1/2) and (2/3, 1/3, 0)
    assert torch.allclose(so.dice(k, average="weighted"), torch.tensor([0.25 + 1 / 6 + 1 / 3, 0.4 / 3], dtype=f64), rtol=0, atol=1e-15)
    # square weights: (1, 1, 1/4); sample 1: (1/4, 1, and class 2 absent from the target -> the largest finite weight, 1)
    assert torch.allclose(so.generalized_dice(k), torch.tensor([4.5 / 5.75, 2 / (0.5 + 5)], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.generalized_dice(k, weight_type="simple"), torch.tensor([(2 + 2 + 1) / (2 + 3 + 1.5), 2 / (1 + 5)], dtype=f64), rtol=0, atol=1e-15)
    assert torch.allclose(so.generalized_dice(k, weight_type="linear"), so.dice(k), rtol=0, atol=1e-15)
    # a sample with an empty target: no finite weight, so every weight is 0 and the value is 0
    empty = so.counts(p[:1], torch.full_like(t[:1], -1), 3)
    assert empty[..., 2].sum() == 0 and so.generalized_dice(empty).tolist() == [0.0] and so.generalized_dice(empty, per_class=True).tolist() == [[0.0] * 3]
    # the fp32 evaluation is another number
    assert so.dice(k, dtype=torch.float32).dtype == torch.float32


def _cases():
    C = 5
    p = so.plant(so.random_labels((4, 9, 11), C, 1), (-1, C, 255, _I64.min, _I64.max), 2, 0.05)
    t = so.plant(so.blocky_labels((4, 9, 11), C, 4, 3), (-1, C, 255, _I64.min, _I64.max), 4, 0.05)
    t[1][t[1] == 3] = 0  # class 3 absent from the target of sample 1 only
    t[2] = -1  # an empty target throughout
    p[3][p[3] == 2] = 1
    t[3][t[3] == 2] = 1  # class 2 absent from both sides of sample 3
    return C, p, t


def test_composition_counts_equal_the_oracle():
    C, p, t = _cases()
    want = so.counts(p, t, C)
    assert torch.equal(seg_utils._overlap_composition(p, t, C, "index"), want)
    assert torch.equal(seg_utils._overlap_composition(p, t.clamp(-1, 255).to(torch.uint8), C, "index"), so.counts(p, t.clamp(-1, 255).to(torch.uint8), C))
    for dp, dt in ((torch.bool, torch.bool), (torch.uint8, torch.int64), (torch.int32, torch.bool)):
        got = seg_utils._overlap_composition(so.to_onehot(p, C, dp) * (1 if dp == torch.bool else 3), so.to_onehot(t, C, dt), C, "one-hot")
        assert got.dtype == torch.int64 and torch.equal(got, want)
    assert seg_utils._overlap_composition(p[:0], t[:0], C, "index").shape == (0, C, 3)
    assert torch.equal(seg_utils._overlap_composition(p[:, :0], t[:, :0], C, "index"), torch.zeros(4, C, 3, dtype=torch.int64))


@pytest.mark.parametrize("input_format", ["index", "one-hot"])
def test_composition_scores_within_one_fp32_rounding(input_format):
    C, p, t = _cases()
    k = so.counts(p, t, C)
    if input_format == "one-hot":
        p, t = so.to_onehot(p, C), so.to_onehot(t, C, torch.uint8)
    for fn, kwargs, oracle, okw in _forms():
        got = fn(p, t, C, input_format=input_format, **kwargs)
        want = oracle(k, **okw)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert so.within_bound(got, want, f"cpu {fn.__name__} {kwargs} {input_format}") <= 1.0


def test_default_format_is_one_hot():
    C, p, t = _cases()
    assert torch.equal(mean_iou(so.to_onehot(p, C), so.to_onehot(t, C), C), mean_iou(p, t, C, input_format="index"))


def test_host_checks():
    p = torch.zeros(2, 3, 4, 4, dtype=torch.int64)
    for fn in (mean_iou, dice_score, generalized_dice_score):
        with pytest.raises(ValueError, match="dtype"):
            fn(p.float(), p, 3)
        with pytest.raises(ValueError, match="dtype"):
            fn(p[:, 0], p[:, 0].double(), 3, input_format="index")
        with pytest.raises(ValueError, match="same shape"):
            fn(p, p[..., :3], 3)
        with pytest.raises(ValueError, match="channels"):
            fn(p, p, 4)
        with pytest.raises(ValueError, match="spatial"):
            fn(p[:, 0, 0, 0], p[:, 0, 0, 0], 3, input_format="index")
        with pytest.raises(ValueError, match="leaves no class"):
            fn(p[:, :1], p[:, :1], 1, include_background=False)
        with pytest.raises(ValueError, match="input_format"):
            fn(p, p, 3, input_format="onehot")
        with pytest.raises(ValueError, match="num_classes"):
            fn(p, p, 0)
    with pytest.raises(ValueError, match="average"):
        dice_score(p, p, 3, average="mean")
    with pytest.raises(ValueError, match="weight_type"):
        generalized_dice_score(p, p, 3, weight_type="cubic")
    with pytest.raises(ValueError, match="per_class"):
        mean_iou(p, p, 3, per_class="yes")
    for cls, kw in ((MeanIoU, {"per_class": 1}), (DiceScore, {"average": "mean"}), (GeneralizedDiceScore, {"weight_type": "cubic"}),
                    (MeanIoU, {"include_background": False, "num_classes": 1}), (DiceScore, {"input_format": "labels"})):
        with pytest.raises(ValueError):
            cls(**{"num_classes": 3, **kw})


class _OnGpu(torch.Tensor):
    """A plain CPU tensor that answers ``is_cuda`` with True: reaches the gate's later arms without a GPU."""

    is_cuda = property(lambda self: True)


def _gpu_like(*shape, dtype=torch.int64):
    return torch.randint(0, 2, shape).to(dtype).as_subclass(_OnGpu)


def test_gate_arm_by_arm(monkeypatch):
    ok = seg_utils._native_segment_ok
    seen = []

    def use_native(*tensors):
        seen.append(tensors)
        return True

    monkeypatch.setattr(seg_utils.ops, "use_native", use_native)
    monkeypatch.setattr(seg_utils, "_SEGMENT_NATIVE", True)
    p, t = _gpu_like(2, 8, 8), _gpu_like(2, 8, 8, dtype=torch.uint8)
    assert ok(p, t, 3, "index") and len(seen) == 1 and seen[0][0] is p and seen[0][1] is t
    for dtype in (torch.uint8, torch.int16, torch.int32, torch.int64):
        assert ok(_gpu_like(2, 8, dtype=dtype), p[:, 0], 3, "index")
    for dtype in (torch.bool, torch.uint8, torch.int32, torch.int64):
        assert ok(_gpu_like(2, 3, 8, dtype=dtype), _gpu_like(2, 3, 8), 3, "one-hot")
    # device
    assert not ok(torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64), 3, "index")
    assert not ok(p, torch.zeros(2, 8, 8, dtype=torch.int64), 3, "index") and not ok(torch.zeros(2, 8, 8, dtype=torch.int64), t, 3, "index")
    # dtype: each form has its own set
    assert not ok(_gpu_like(2, 8, dtype=torch.int8), _gpu_like(2, 8), 3, "index") and not ok(_gpu_like(2, 8), _gpu_like(2, 8, dtype=torch.bool), 3, "index")
    assert not ok(_gpu_like(2, 3, 8, dtype=torch.int16), _gpu_like(2, 3, 8), 3, "one-hot") and not ok(_gpu_like(2, 3, 8), _gpu_like(2, 3, 8, dtype=torch.int8), 3, "one-hot")
    # the class cap binds the index form only
    cap = seg_utils._SEGMENT_MAX_CLASSES
    assert ok(p, t, cap, "index") and not ok(p, t, cap + 1, "index")
    assert ok(_gpu_like(1, cap + 1, 2, dtype=torch.bool), _gpu_like(1, cap + 1, 2, dtype=torch.bool), cap + 1, "one-hot")
    # the library's own answer and the knob
    n = len(seen)
    monkeypatch.setattr(seg_utils.ops, "use_native", lambda *a: False)
    assert not ok(p, t, 3, "index")
    monkeypatch.setattr(seg_utils.ops, "use_native", use_native)
    monkeypatch.setattr(seg_utils, "_SEGMENT_NATIVE", False)
    assert not ok(p, t, 3, "index") and len(seen) == n


def test_functionals_behind_the_gate(monkeypatch):
    """With the gate open a functional is one overlap call and one score call with the metric's codes; validation stays ahead of both."""
    C, p, t = _cases()
    calls = []

    def overlap_index(preds, target, num_classes):
        calls.append(("index", num_classes))
        return so.counts(preds, target, num_classes)

    def overlap_onehot(preds, target):
        calls.append(("one-hot", preds.shape[1]))
        return so.counts(preds, target, preds.shape[1], "one-hot")

    def scores(counts, metric, option, include_background):
        calls.append(("scores", metric, option, include_background))
        return seg_utils._scores_composition(counts, metric, option, include_background)

    monkeypatch.setattr(seg_utils, "_native_segment_ok", lambda *a: True)
    monkeypatch.setattr(ops_seg, "segment_overlap_index", overlap_index)
    monkeypatch.setattr(ops_seg, "segment_overlap_onehot", overlap_onehot)
    monkeypatch.setattr(ops_seg, "segment_scores", scores)
    mean_iou(p, t, C, input_format="index")
    assert calls == [("index", C), ("scores", 0, 0, True)]
    del calls[:]
    dice_score(so.to_onehot(p, C), so.to_onehot(t, C), C, include_background=False, average="weighted")
    assert calls == [("one-hot", C), ("scores", 1, 2, False)]
    del calls[:]
    generalized_dice_score(p, t, C, per_class=True, weight_type="simple", input_format="index")
    assert calls == [("index", C), ("scores", 2, 4, True)]
    del calls[:]
    with pytest.raises(ValueError):
        mean_iou(p.float(), t, C, input_format="index")
    with pytest.raises(ValueError):
        dice_score(p, t, C, average="bad", input_format="index")
    assert not calls


def _no_native(*a, **k):
    raise AssertionError("a native segmentation op was entered for CPU tensors")


def test_cpu_calls_never_reach_the_op(monkeypatch):
    names = ("segment_overlap_index", "segment_overlap_onehot", "segment_scores")
    calls = [count_calls(monkeypatch, ops_seg, n, guard=_no_native) for n in names]
    if ops.available():
        calls += [count_calls(monkeypatch, torch.ops.tmx, n, guard=_no_native) for n in names]
    C, p, t = _cases()
    k = so.counts(p, t, C)
    for fn, kwargs, oracle, okw in _forms((True,)):
        assert so.within_bound(fn(p, t, C, input_format="index", **kwargs), oracle(k, **okw), f"cpu route {fn.__name__} {kwargs}") <= 1.0
    m = MeanIoU(C, input_format="index")
    m.update(p, t)
    assert so.within_bound(m.compute(), so.mean_iou(k).mean(), "cpu route MeanIoU") <= 1.0
    assert not any(calls)


_MODULES = [
    (MeanIoU, {"per_class": False}, so.mean_iou, {"per_class": False}),
    (MeanIoU, {"per_class": True, "include_background": False}, so.mean_iou, {"per_class": True, "include_background": False}),
    (DiceScore, {"average": "micro"}, so.dice, {"average": "micro"}),
    (DiceScore, {"average": "none"}, so.dice, {"average": "none"}),
    (GeneralizedDiceScore, {"weight_type": "square"}, so.generalized_dice, {"weight_type": "square"}),
    (GeneralizedDiceScore, {"weight_type": "simple", "per_class": True}, so.generalized_dice, {"weight_type": "simple", "per_class": True}),
]


@pytest.mark.parametrize("cls,kwargs,oracle,okw", _MODULES)
def test_modules_mean_over_samples(cls, kwargs, oracle, okw):
    C, p, t = _cases()
    want = oracle(so.counts(p, t, C), **okw).mean(0)
    m = cls(C, input_format="index", **kwargs)
    assert m.is_differentiable is False and m.higher_is_better is True and m.full_state_update is False
    assert m.plot_lower_bound == 0.0 and m.plot_upper_bound == 1.0
    assert m.score.dtype == torch.float64 and m.samples.dtype == torch.int64
    first = m(p[:1], t[:1])  # forward returns the batch value
    assert so.within_bound(first, oracle(so.counts(p[:1], t[:1], C), **okw).mean(0), f"{cls.__name__} forward") <= 1.0
    m.update(p[1:], t[1:])  # 1 + 3 samples: a mean over samples, not of batch means
    got = m.compute()
    assert got.dtype == torch.float32 and so.within_bound(got, want, f"{cls.__name__} {kwargs} uneven batches") <= 1.0
    assert int(m.samples) == 4
    again = pickle.loads(pickle.dumps(m))
    assert torch.equal(again.compute(), got)
    m.reset()
    assert int(m.samples) == 0 and not bool(m.score.any())


def _ddp_body(rank, world, cls, kwargs, C, p, t):
    m = cls(C, input_format="index", **kwargs)
    shard = slice(0, 1) if rank == 0 else slice(1, None)  # disjoint, uneven shards
    m.update(p[shard], t[shard])
    return m.compute()


@pytest.mark.parametrize("cls,kwargs,oracle,okw", _MODULES)
def test_modules_on_two_gloo_ranks(cls, kwargs, oracle, okw):
    C, p, t = _cases()
    one = cls(C, input_format="index", **kwargs)
    one.update(p, t)
    # both sides are fp32 roundings of fp64 sums in another order, so each is held to the fp64 oracle of all the data
    want = oracle(so.counts(p, t, C), **okw).mean(0)
    assert so.within_bound(one.compute(), want, f"{cls.__name__} {kwargs} 1 process") <= 1.0
    for got in run_ddp(_ddp_body, cls, kwargs, C, p, t):
        assert got.dtype == torch.float32 and so.within_bound(got, want, f"{cls.__name__} {kwargs} 2 ranks") <= 1.0


def test_exports_stay_in_the_two_subpackages():
    import torchmetrics_forked_amd as tm
    import torchmetrics_forked_amd.functional as F

    for name in ("MeanIoU", "DiceScore", "GeneralizedDiceScore"):
        assert not hasattr(tm, name)
    for name in ("mean_iou", "dice_score", "generalized_dice_score"):
        assert name not in getattr(F, "__all__", ())
