"""CPU reference of the YOLOv8 detection graph -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Upstream's ``cfg/models/v8/yolov8.yaml`` is, layer for layer, the backbone and neck of ``yolov8-seg.yaml`` (entries 0-21) under
a ``Detect`` head at entry 22.  So the model here is assembled from the YOLOv8-seg oracle's own modules
(``yolov8_seg_oracle.SegmentationModel``'s entries 0-21 and its ``features``) and the ``Detect`` class of
``yolov5u_det_ref`` (YOLOv8's head, which YOLOv5u shares).  Scale tags "8n" .. "8x".  No product code is imported.
"""
from __future__ import annotations

import torch.nn as nn

import yolov8_seg_oracle as orc
from yolov5u_det_ref import Detect

SCALES = {"8" + k: v for k, v in orc.SCALES.items()}
non_max_suppression = orc.non_max_suppression


class DetectionModelV8(nn.Module):
    """The 23-entry YOLOv8 detect graph; layer i is ``self.model[i]`` (upstream's state-dict names)."""

    def __init__(self, scale: str = "8n", nc: int = 80):
        super().__init__()
        _, width, maxc = SCALES[scale]
        fch = tuple(orc.make_divisible(min(c, maxc) * width, 8) for c in (256, 512, 1024))
        body = orc.SegmentationModel(scale[1:], 1).model[:22]          # the oracle's own backbone / neck modules
        self.model = nn.ModuleList(list(body) + [Detect(nc, fch)])
        self.nc, self.scale = nc, scale
        self.model[22].bias_init(640)

    features = orc.SegmentationModel.features                           # (reads self.model[0..21] only)

    def forward(self, x):
        """Inference forward: preds (B, 4 + nc, A)."""
        return self.model[22](self.features(x))

    def forward_raw(self, x):
        """raw per-level maps (B, 64 + nc, h, w)."""
        return self.model[22].forward_raw(self.features(x))


def count_parameters(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters())
