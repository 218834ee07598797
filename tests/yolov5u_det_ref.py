"""CPU reference of the YOLOv5u detection graph -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates upstream's ``cfg/models/v5/yolov5.yaml`` (the anchor-free ``u`` variant: YOLOv8's Detect head) in plain
PyTorch-CPU fp32 from the published structure, reusing the YOLOv8-seg oracle's ``Conv`` / ``SPPF`` / ``DFL`` /
``make_anchors`` / ``non_max_suppression``.  Pinned by the published parameter counts and GFLOPs at nc = 80, 640 x 640:
n 2 654 816 / 7.7, s 9 153 152 / 24.0, m 25 111 456 / 64.2 (tests/test_v5u_host.py).
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

import yolov8_seg_oracle as orc
from yolov8_seg_oracle import DFL, REG_MAX, SPPF, Conv, make_anchors, make_divisible

SCALES = {"5n": (0.33, 0.25, 1024), "5s": (0.33, 0.50, 1024), "5m": (0.67, 0.75, 1024)}
PARAMS_NC80 = {"5n": 2_654_816, "5s": 9_153_152, "5m": 25_111_456}
GFLOPS_640 = {"5n": 7.7, "5s": 24.0, "5m": 64.2}


class Stem6(nn.Module):
    """model.0: Conv2d(3, c2, 6, 2, padding=2, bias=False) + BN + SiLU (autopad(6) would be 3: upstream's yaml passes p = 2)."""

    def __init__(self, c2: int):
        super().__init__()
        self.conv = nn.Conv2d(3, c2, 6, 2, 2, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)

    def forward(self, x):
        return F.silu(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    """C3's Bottleneck (e = 1.0): 1x1 then 3x3, residual when shortcut."""

    def __init__(self, c: int, shortcut: bool):
        super().__init__()
        self.cv1 = Conv(c, c, 1, 1)
        self.cv2 = Conv(c, c, 3, 1)
        self.add = shortcut

    def forward(self, x):
        y = self.cv2(self.cv1(x))
        return x + y if self.add else y


class C3(nn.Module):
    def __init__(self, c1: int, c2: int, n: int, shortcut: bool = True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, shortcut) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class Detect(nn.Module):
    """YOLOv8's Detect: ``orc.Segment`` without cv4 and Proto."""

    def __init__(self, nc: int, ch: Sequence[int]):
        super().__init__()
        self.nc, self.nl, self.no = nc, len(ch), nc + REG_MAX * 4
        self.stride = torch.tensor([8.0, 16.0, 32.0])
        c2 = max(16, ch[0] // 4, REG_MAX * 4)
        c3 = max(ch[0], min(nc, 100))
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * REG_MAX, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1)) for x in ch)
        self.dfl = DFL(REG_MAX)

    def bias_init(self, imgsz: int = 640):
        for a, b, s in zip(self.cv2, self.cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (imgsz / float(s)) ** 2)

    def forward_raw(self, feats: List[torch.Tensor]):
        """raw per-level maps (B, 64 + nc, h, w)."""
        return [torch.cat((self.cv2[i](feats[i]), self.cv3[i](feats[i])), 1) for i in range(self.nl)]

    def forward(self, feats: List[torch.Tensor]):
        """predictions (B, 4 + nc, A): xywh in input pixels, class sigmoids."""
        raw = self.forward_raw(feats)
        bs = raw[0].shape[0]
        shapes = [(r.shape[2], r.shape[3]) for r in raw]
        x_cat = torch.cat([r.view(bs, self.no, -1) for r in raw], 2)
        box, cls = x_cat.split((REG_MAX * 4, self.nc), 1)
        anchors, strides = make_anchors(shapes, [int(s) for s in self.stride])
        lt, rb = self.dfl(box).chunk(2, 1)
        a = anchors.t().unsqueeze(0)
        x1y1, x2y2 = a - lt, a + rb
        dbox = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * strides.t().unsqueeze(0)
        return torch.cat((dbox, cls.sigmoid()), 1)


class DetectionModelV5u(nn.Module):
    """The 25-entry YOLOv5u graph; layer i is ``self.model[i]`` (upstream's state-dict names)."""

    def __init__(self, scale: str = "5s", nc: int = 80):
        super().__init__()
        depth, width, maxc = SCALES[scale]

        def ch(c):
            return make_divisible(min(c, maxc) * width, 8)

        def rep(n):
            return max(round(n * depth), 1) if n > 1 else n

        c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        m: List[nn.Module] = [
            Stem6(c64),                                   # 0
            Conv(c64, c128, 3, 2),                        # 1
            C3(c128, c128, rep(3)),                       # 2
            Conv(c128, c256, 3, 2),                       # 3
            C3(c256, c256, rep(6)),                       # 4
            Conv(c256, c512, 3, 2),                       # 5
            C3(c512, c512, rep(9)),                       # 6
            Conv(c512, c1024, 3, 2),                      # 7
            C3(c1024, c1024, rep(3)),                     # 8
            SPPF(c1024, c1024, 5),                        # 9
            Conv(c1024, c512, 1, 1),                      # 10
            nn.Upsample(scale_factor=2, mode="nearest"),  # 11
            nn.Identity(),                                # 12 Concat[-1, 6]
            C3(c512 + c512, c512, rep(3), False),         # 13
            Conv(c512, c256, 1, 1),                       # 14
            nn.Upsample(scale_factor=2, mode="nearest"),  # 15
            nn.Identity(),                                # 16 Concat[-1, 4]
            C3(c256 + c256, c256, rep(3), False),         # 17 (P3)
            Conv(c256, c256, 3, 2),                       # 18
            nn.Identity(),                                # 19 Concat[-1, 14]
            C3(c256 + c256, c512, rep(3), False),         # 20 (P4)
            Conv(c512, c512, 3, 2),                       # 21
            nn.Identity(),                                # 22 Concat[-1, 10]
            C3(c512 + c512, c1024, rep(3), False),        # 23 (P5)
            Detect(nc, (c256, c512, c1024)),              # 24
        ]
        self.model = nn.ModuleList(m)
        self.nc, self.scale = nc, scale
        self.model[24].bias_init(640)

    def features(self, x):
        m = self.model
        x4 = m[4](m[3](m[2](m[1](m[0](x)))))
        x6 = m[6](m[5](x4))
        x10 = m[10](m[9](m[8](m[7](x6))))
        x14 = m[14](m[13](torch.cat((m[11](x10), x6), 1)))
        x17 = m[17](torch.cat((m[15](x14), x4), 1))
        x20 = m[20](torch.cat((m[18](x17), x14), 1))
        x23 = m[23](torch.cat((m[21](x20), x10), 1))
        return [x17, x20, x23]

    def forward(self, x):
        """Inference forward: preds (B, 4 + nc, A)."""
        return self.model[24](self.features(x))

    def forward_raw(self, x):
        return self.model[24].forward_raw(self.features(x))


def count_parameters(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters())


def conv_macs_per_image(scale: str, nc: int, imgsz=(640, 640)) -> int:
    """Conv MACs per image (BN folded; the DFL's fixed 1x1 excluded)."""
    model = DetectionModelV5u(scale, nc).eval()
    macs = 0
    hooks = []

    def hook(mod, inp, out):
        nonlocal macs
        macs += out.shape[2] * out.shape[3] * mod.out_channels * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]

    for mod in model.modules():
        if isinstance(mod, nn.Conv2d) and mod is not model.model[24].dfl.conv:
            hooks.append(mod.register_forward_hook(hook))
    with torch.no_grad():
        model(torch.zeros(1, 3, imgsz[0], imgsz[1]))
    for h in hooks:
        h.remove()
    return macs


non_max_suppression = orc.non_max_suppression
