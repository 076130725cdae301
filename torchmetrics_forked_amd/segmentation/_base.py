"""Mean-over-samples segmentation metric base: an fp64 ``sum`` state of the per-sample values and an int64 sample count."""
from typing import Any, Optional, Sequence, Union

import torch
from torch import Tensor

from torchmetrics_forked_amd.functional.segmentation.utils import _check_arguments, _kept_classes
from torchmetrics_forked_amd.metric import Metric
from torchmetrics_forked_amd.utilities.plot import _AX_TYPE, _PLOT_OUT_TYPE


class _MeanSegmentationMetric(Metric):
    full_state_update: bool = False
    is_differentiable: bool = False
    higher_is_better: bool = True
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0

    def __init__(self, num_classes: int, include_background: bool, input_format: str, per_class: bool, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        _check_arguments(num_classes, include_background, input_format)  # the functional's own checks, at construction
        self.num_classes = num_classes
        self.include_background = include_background
        self.input_format = input_format
        shape = (_kept_classes(num_classes, include_background),) if per_class else ()
        self.add_state("score", default=torch.zeros(shape, dtype=torch.float64), dist_reduce_fx="sum")
        self.add_state("samples", default=torch.zeros((), dtype=torch.int64), dist_reduce_fx="sum")

    def _values(self, preds: Tensor, target: Tensor) -> Tensor:
        """fp64 per-sample values ``[B]`` or ``[B, C']``."""
        raise NotImplementedError

    def update(self, preds: Tensor, target: Tensor) -> None:
        v = self._values(preds, target)
        self.score += v.sum(dim=0)
        self.samples += v.shape[0]

    def compute(self) -> Tensor:
        """Mean over all samples seen (not a mean of batch means), fp32."""
        return (self.score / self.samples).float()

    def plot(self, val: Optional[Union[Tensor, Sequence[Tensor]]] = None, ax: Optional[_AX_TYPE] = None) -> _PLOT_OUT_TYPE:
        return self._plot(val, ax)
