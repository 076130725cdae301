"""``image/generative.py`` ``_rowmax_fused_wins`` at its boundaries (shapes and dtype only: meta tensors, no GPU).

* fp32 with >= 256 output tiles of 128 x 128: always the fused kernel (the f16-split matrix-core route);
* fp32 below: ``work < 2^32 and d <= 1024`` -- with fewer than 256 tiles ``n * m < 2^22``, so only the depth limit
  can be reached;
* fp64: ``work <= 2^29 and d <= 256`` (beyond, the fp64 loop loses to the library GEMM);
* bf16 / fp16: ``work <= 2^29`` at any depth."""
import pytest
import torch

from torchmetrics_forked_amd.image.generative import _rowmax_fused_wins

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16

CASES = [
    # (dtype, n, m, d, fused)
    (F32, 1921, 2048, 4096, True),  # 256 tiles: any depth
    (F32, 1920, 2048, 1024, True),  # 240 tiles: the exact kernel up to d = 1024 ...
    (F32, 1920, 2048, 1025, False),  # ... and the library beyond
    (F32, 300, 200, 1024, True),
    (F32, 300, 200, 1025, False),
    (F64, 2048, 1024, 256, True),  # work = 2^29
    (F64, 2049, 1024, 256, False),
    (F64, 1024, 1024, 257, False),
    (F64, 1921, 2048, 64, True),  # 256 tiles do not matter for fp64: work = 2^27.9
    (F64, 4096, 4096, 64, False),  # work = 2^30
    (BF16, 2048, 1024, 256, True),
    (BF16, 2049, 1024, 256, False),
    (F16, 64, 64, 4096, True),  # no depth limit for 16-bit
    (F16, 2049, 1024, 256, False),
]


@pytest.mark.parametrize("dtype,n,m,d,fused", CASES)
def test_rowmax_fused_wins_boundaries(dtype, n, m, d, fused):
    f1 = torch.empty(n, d, dtype=dtype, device="meta")
    f2 = torch.empty(m, d, dtype=dtype, device="meta")
    assert _rowmax_fused_wins(f1, f2) is fused
