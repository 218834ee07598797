"""CPU reference of the YOLO11 detection graph -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates upstream's ``cfg/models/11/yolo11.yaml`` (Detect at model.23) in plain PyTorch-CPU fp32 from the published
structure, reusing the YOLOv8-seg oracle's ``Conv`` / ``SPPF`` / ``DFL`` / ``make_anchors`` / ``non_max_suppression`` as
tests/yolov5u_det_ref.py does.  Pinned by the published parameter counts and GFLOPs at nc = 80, 640 x 640:
n 2 624 080 / 6.6, s 9 458 752 / 21.7, m 20 114 688 / 68.5 (tests/test_y11_host.py).

Blocks: C3k2 (C2f's shape, shortcut on everywhere; m.0 = Bottleneck(c, c, e=0.5) or C3k(c, c, n=2)), C2PSA (one PSABlock:
multi-head self-attention with a depthwise positional term, then a 2x FFN, both residual) and the v11 Detect head whose class
branch is DWConv -> 1x1 -> DWConv -> 1x1 -> Conv2d.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

import yolov8_seg_oracle as orc
from yolov8_seg_oracle import DFL, REG_MAX, SPPF, Conv, make_anchors, make_divisible

SCALES = {"11n": (0.50, 0.25, 1024), "11s": (0.50, 0.50, 1024), "11m": (0.50, 1.00, 512)}
PARAMS_NC80 = {"11n": 2_624_080, "11s": 9_458_752, "11m": 20_114_688}
GFLOPS_640 = {"11n": 6.6, "11s": 21.7, "11m": 68.5}


class ConvGA(nn.Module):
    """Conv2d(bias=False) + BN with a group count and an optional SiLU (upstream Conv(c1, c2, k, s, g=g, act=act))."""

    def __init__(self, c1: int, c2: int, k: int = 1, s: int = 1, g: int = 1, act: bool = True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
        self.act = act

    def forward(self, x):
        y = self.bn(self.conv(x))
        return F.silu(y) if self.act else y


def DWConv(c1: int, c2: int, k: int = 3) -> ConvGA:
    return ConvGA(c1, c2, k, 1, math.gcd(c1, c2), True)


class Bottleneck(nn.Module):
    """Bottleneck(c1, c2, shortcut, k=(3, 3), e): 3x3 c1 -> c2*e, 3x3 -> c2, residual when shortcut and c1 == c2."""

    def __init__(self, c1: int, c2: int, shortcut: bool = True, e: float = 0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 3, 1)
        self.cv2 = Conv(c_, c2, 3, 1)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        y = self.cv2(self.cv1(x))
        return x + y if self.add else y


class C3k(nn.Module):
    """C3(c1, c2, n, shortcut, e=0.5) with Bottleneck(c_, c_, k=(3, 3), e=1.0)."""

    def __init__(self, c1: int, c2: int, n: int = 2, shortcut: bool = True):
        super().__init__()
        c_ = int(c2 * 0.5)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, e=1.0) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class C3k2(nn.Module):
    """C2f's shape with c = int(c2 * e): cv1 c1 -> 2c, n blocks m, cv2 (2 + n) c -> c2."""

    def __init__(self, c1: int, c2: int, n: int = 1, c3k: bool = False, e: float = 0.5, shortcut: bool = True):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1, 1)
        self.m = nn.ModuleList(C3k(self.c, self.c, 2, shortcut) if c3k else Bottleneck(self.c, self.c, shortcut)
                               for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        y.extend(m(y[-1]) for m in self.m)
        return self.cv2(torch.cat(y, 1))


class Attention(nn.Module):
    """Multi-head self-attention over the H*W tokens; head h's qkv channels are [q 32 | k 32 | v 64] at offset 128 h."""

    def __init__(self, dim: int, num_heads: int = 8, attn_ratio: float = 0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim ** -0.5
        h = dim + self.key_dim * num_heads * 2
        self.qkv = ConvGA(dim, h, 1, act=False)
        self.proj = ConvGA(dim, dim, 1, act=False)
        self.pe = ConvGA(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x):
        B, C, H, W = x.shape
        N = H * W
        qkv = self.qkv(x)
        q, k, v = qkv.view(B, self.num_heads, self.key_dim * 2 + self.head_dim, N).split(
            [self.key_dim, self.key_dim, self.head_dim], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * self.scale).softmax(dim=-1)
        x = (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self.pe(v.reshape(B, C, H, W))
        return self.proj(x)


class PSABlock(nn.Module):
    def __init__(self, c: int, attn_ratio: float = 0.5, num_heads: int = 4):
        super().__init__()
        self.attn = Attention(c, num_heads, attn_ratio)
        self.ffn = nn.Sequential(ConvGA(c, 2 * c, 1), ConvGA(2 * c, c, 1, act=False))

    def forward(self, x):
        x = x + self.attn(x)
        return x + self.ffn(x)


class C2PSA(nn.Module):
    def __init__(self, c1: int, c2: int, n: int = 1, e: float = 0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), dim=1)
        return self.cv2(torch.cat((a, self.m(b)), 1))


class Detect(nn.Module):
    """The v11 Detect head: YOLOv8's box branch; class branch DWConv, 1x1, DWConv, 1x1, Conv2d."""

    def __init__(self, nc: int, ch: Sequence[int]):
        super().__init__()
        self.nc, self.nl, self.no = nc, len(ch), nc + REG_MAX * 4
        self.stride = torch.tensor([8.0, 16.0, 32.0])
        c2 = max(16, ch[0] // 4, REG_MAX * 4)
        c3 = max(ch[0], min(nc, 100))
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * REG_MAX, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(nn.Sequential(DWConv(x, x, 3), Conv(x, c3, 1)),
                                               nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)),
                                               nn.Conv2d(c3, nc, 1)) for x in ch)
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


class DetectionModelY11(nn.Module):
    """The 24-entry YOLO11 graph; layer i is ``self.model[i]`` (upstream's state-dict names)."""

    def __init__(self, scale: str = "11s", nc: int = 80):
        super().__init__()
        depth, width, maxc = SCALES[scale]

        def ch(c):
            return make_divisible(min(c, maxc) * width, 8)

        def rep(n):
            return max(round(n * depth), 1) if n > 1 else n

        c3k_all = scale[-1] in "mlx"     # upstream parse_model: C3k2 of the m / l / x scales always use C3k
        c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        n = rep(2)
        m: List[nn.Module] = [
            Conv(3, c64, 3, 2),                                          # 0
            Conv(c64, c128, 3, 2),                                       # 1
            C3k2(c128, c256, n, c3k_all, 0.25),                          # 2
            Conv(c256, c256, 3, 2),                                      # 3
            C3k2(c256, c512, n, c3k_all, 0.25),                          # 4
            Conv(c512, c512, 3, 2),                                      # 5
            C3k2(c512, c512, n, True),                                   # 6
            Conv(c512, c1024, 3, 2),                                     # 7
            C3k2(c1024, c1024, n, True),                                 # 8
            SPPF(c1024, c1024, 5),                                       # 9
            C2PSA(c1024, c1024, n),                                      # 10
            nn.Upsample(scale_factor=2, mode="nearest"),                 # 11
            nn.Identity(),                                               # 12 Concat[-1, 6]
            C3k2(c1024 + c512, c512, n, c3k_all),                        # 13
            nn.Upsample(scale_factor=2, mode="nearest"),                 # 14
            nn.Identity(),                                               # 15 Concat[-1, 4]
            C3k2(c512 + c512, c256, n, c3k_all),                         # 16 (P3)
            Conv(c256, c256, 3, 2),                                      # 17
            nn.Identity(),                                               # 18 Concat[-1, 13]
            C3k2(c256 + c512, c512, n, c3k_all),                         # 19 (P4)
            Conv(c512, c512, 3, 2),                                      # 20
            nn.Identity(),                                               # 21 Concat[-1, 10]
            C3k2(c512 + c1024, c1024, n, True),                          # 22 (P5)
            Detect(nc, (c256, c512, c1024)),                             # 23
        ]
        self.model = nn.ModuleList(m)
        self.nc, self.scale = nc, scale
        self.model[23].bias_init(640)

    def features(self, x):
        m = self.model
        x4 = m[4](m[3](m[2](m[1](m[0](x)))))
        x6 = m[6](m[5](x4))
        x10 = m[10](m[9](m[8](m[7](x6))))
        x13 = m[13](torch.cat((m[11](x10), x6), 1))
        x16 = m[16](torch.cat((m[14](x13), x4), 1))
        x19 = m[19](torch.cat((m[17](x16), x13), 1))
        x22 = m[22](torch.cat((m[20](x19), x10), 1))
        return [x16, x19, x22]

    def forward(self, x):
        """Inference forward: preds (B, 4 + nc, A)."""
        return self.model[23](self.features(x))

    def forward_raw(self, x):
        return self.model[23].forward_raw(self.features(x))


def count_parameters(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters())


def conv_macs_per_image(scale: str, nc: int, imgsz=(640, 640)) -> int:
    """Conv MACs per image (BN folded; grouped convs count cin / groups per output; the DFL's fixed 1x1 and the
    attention's two matrix products excluded, as upstream's GFLOPs figure excludes them)."""
    model = DetectionModelY11(scale, nc).eval()
    macs = 0
    hooks = []

    def hook(mod, inp, out):
        nonlocal macs
        macs += (out.shape[2] * out.shape[3] * mod.out_channels * (mod.in_channels // mod.groups) *
                 mod.kernel_size[0] * mod.kernel_size[1])

    for mod in model.modules():
        if isinstance(mod, nn.Conv2d) and mod is not model.model[23].dfl.conv:
            hooks.append(mod.register_forward_hook(hook))
    with torch.no_grad():
        model(torch.zeros(1, 3, imgsz[0], imgsz[1]))
    for h in hooks:
        h.remove()
    return macs


def upstream_gflops(scale: str, nc: int = 80, imgsz=(640, 640)) -> float:
    """Upstream's GFLOPs figure (its thop count of the unfused model): 2 x conv MACs + 8 x the elements every BatchNorm2d
    writes (thop counts an affine norm as 2 x 2 ops per element; the total is doubled like the MACs)."""
    model = DetectionModelY11(scale, nc).eval()
    bn = 0

    def hook(mod, inp, out):
        nonlocal bn
        bn += out[0].numel()

    hooks = [mod.register_forward_hook(hook) for mod in model.modules() if isinstance(mod, nn.BatchNorm2d)]
    with torch.no_grad():
        model(torch.zeros(1, 3, imgsz[0], imgsz[1]))
    for h in hooks:
        h.remove()
    return (2 * conv_macs_per_image(scale, nc, imgsz) + 8 * bn) / 1e9


non_max_suppression = orc.non_max_suppression
