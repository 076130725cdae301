"""The order of the gates in ``_CurveMetric._fast_hist_update``, without a GPU: the cached state is armed by hand on
CPU tensors and ``torch.ops.tmx.curve_hist_update`` is a counting stub, so the test sees whether the native call would
have been made.  Task shape checks come first (multiclass ``[N, C]`` / ``[N]``; binary equal shapes, unconditionally),
then the hand-over to the update lanes, then the join of pending side work, then the launch."""
import torch

from torchmetrics_forked_amd.classification import BinaryPrecisionRecallCurve, MulticlassPrecisionRecallCurve


def _arm(m, classes, dtype=torch.bfloat16):
    """What ``_arm_fast_update`` leaves behind after a GPU update, on CPU tensors (the gates compare identities only)."""
    hist = torch.zeros(classes, 2, 8, dtype=torch.long)
    m.score_hist = hist
    m._set_range(hist, torch.zeros(classes, 2, dtype=torch.int32), 0)
    m.__dict__["_spec_mode"] = torch.zeros(8, dtype=torch.int32)
    m.__dict__["_fast_update"] = (hist, dtype, -1)  # (-1: ``Tensor.get_device()`` of a CPU tensor)
    return hist


def _stub(monkeypatch):
    calls = []
    monkeypatch.setattr(torch.ops.tmx, "curve_hist_update", lambda *a: calls.append(a), raising=False)
    return calls


def test_multiclass_rows_and_labels_take_the_native_call(monkeypatch):
    calls = _stub(monkeypatch)
    n, c = 32, 10
    m = MulticlassPrecisionRecallCurve(num_classes=c, validate_args=False)
    hist = _arm(m, c)
    preds, target = torch.randn(n, c).bfloat16(), torch.randint(0, c, (n,))
    assert m._fast_hist_update(preds, target) is True
    assert len(calls) == 1
    assert calls[0][0] is preds and calls[0][1] is target and calls[0][2] is hist and calls[0][3] == 0  # (0: multiclass)
    assert m._rows_bound == n
    # the task shape checks still send everything else to the full path
    assert m._fast_hist_update(preds[:, :9], target) is False
    assert m._fast_hist_update(preds, target[:-1]) is False
    assert m._fast_hist_update(preds, target.float()) is False
    assert len(calls) == 1


def test_unknown_row_bound_stays_unknown_and_fast(monkeypatch):
    """A loaded / merged histogram has no host-side row count (``_rows_bound is None``): the update is still one native
    call, and the bound stays unknown (the sync then bounds the bins on the device)."""
    calls = _stub(monkeypatch)
    n, c = 16, 4
    m = MulticlassPrecisionRecallCurve(num_classes=c, validate_args=False)
    hist = _arm(m, c)
    m._set_range(hist, m._code_range, None)
    assert m._fast_hist_update(torch.randn(n, c).bfloat16(), torch.randint(0, c, (n,))) is True
    assert len(calls) == 1 and m._rows_bound is None


def test_multiclass_pending_side_work_is_joined_then_launched(monkeypatch):
    calls = _stub(monkeypatch)
    n, c = 16, 4
    m = MulticlassPrecisionRecallCurve(num_classes=c, validate_args=False)
    _arm(m, c)
    ran = []
    m.__dict__["_side_event"] = lambda: ran.append(len(calls))
    assert m._fast_hist_update(torch.randn(n, c).bfloat16(), torch.randint(0, c, (n,))) is True
    assert ran == [0] and len(calls) == 1  # joined once, before the launch
    assert m.__dict__["_side_event"] is None


def test_binary_shape_check_does_not_depend_on_pending_side_work(monkeypatch):
    calls = _stub(monkeypatch)
    n = 64
    m = BinaryPrecisionRecallCurve(validate_args=False)
    _arm(m, 1)
    ran = []
    m.__dict__["_side_event"] = lambda: ran.append(1)
    preds, target = torch.randn(n).bfloat16(), torch.randint(0, 2, (n,))
    assert m._fast_hist_update(preds, target[:-1]) is False
    assert len(ran) <= 1 and not calls
    # equal shapes: joined, launched
    m.__dict__["_side_event"] = lambda: ran.append(1)
    ran.clear()
    assert m._fast_hist_update(preds, target) is True
    assert ran == [1] and len(calls) == 1 and calls[0][3] == 1  # (1: binary)
    assert m._rows_bound == n
