"""The COCO loop oracle lives in ``tests/helpers/coco_oracle.py`` (shared with the GPU tests); re-exported here."""
from tests.helpers.coco_oracle import AREA, Oracle, _iou, coco_eval, summarize  # noqa: F401
