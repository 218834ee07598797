"""Plain CPU references of the forward glue kernels (csrc/misc_kernels.hip): the 3x3 stem on the uint8 image, SPPF pooling, the
nearest 2x upsample, the Detect decode and ADown's pooling front.  A plain module (no fixtures, no GPU needed to import).

float64 throughout, except adown_ref: include/mi355yolo.h fixes the fp32 operation order of the averages, IEEE fp32 adds in a fixed
association are reproducible, so the reference follows it in float32 and the comparison is bit for bit.  All maps are NHWC.
"""
import torch
import torch.nn.functional as F

import launch_ref as lr


# The SPPF cases of tests/test_glue_kernels_gpu.py, each named after the kernel instance it must reach: (B, C, H, W), the
# (cg, owned) m355_sppf_pool_form must report at the slice strides of sppf_strides (M355_SPPF_MINBLOCKS at its default, 256).
SPPF_CASES = [
    ("owned1_window_taller_than_map", (2, 24, 5, 7), (1, 1)),        # three groups: no wider chunk divides them
    ("owned1_second_slot_partly_used", (2, 24, 23, 31), (1, 1)),     # 713 elements on 512 threads
    ("owned1_2048_elements_96KB", (1, 8, 32, 64), (1, 1)),           # every slot of every thread on, LDS 96 KB
    ("owned2_six_groups", (86, 48, 6, 9), (2, 1)),                   # 6 % 4 != 0; 86 x 3 = 258 blocks
    ("owned2_522_pixels", (32, 128, 18, 29), (2, 1)),                # 4 groups would be 2088 elements and 128 blocks
    ("owned4_small_plane", (16, 512, 5, 4), (4, 1)),
    ("owned4_lds_76KB", (16, 512, 19, 21), (4, 1)),                  # 3 x 399 x 64 bytes: above 64 KB, prepare_kernel
    ("generic1_2079_pixels", (2, 16, 33, 63), (1, 0)),               # just past the 2048-element limit of the owned form
    ("generic1_lds_108KB", (1, 8, 47, 49), (1, 0)),
]


def sppf_strides(C: int):
    """(ldx, x channel offset, ldy, y channel offset) of the SPPF slice cases."""
    return C + 16, 8, 3 * C + 24, 16


def stem_ref(img_u8: torch.Tensor, w: torch.Tensor, b: torch.Tensor):
    """(ref, bound) of m355_stem_fwd: img (B, H, W, 3) uint8, w (cout, 3, 3, 3) fp32, b (cout) -> (B, H/2, W/2, cout) float64.
    ref = silu(conv(u8, fp16(w)) / 255 + b), the weights rounded to fp16 once as pack_stem3x3 stores them; S = the same
    convolution over |u8| and |fp16(w)|, / 255; bound = the conv bound of launch_ref with SiLU's slope (K = 27 products)."""
    x = img_u8.double()
    w16 = w.half().double()
    ref = lr.silu(lr.conv_ref(x, w16, 2, 1) / 255.0 + b.double())
    S = lr.conv_ref(x.abs(), w16.abs(), 2, 1) / 255.0
    return ref, lr.elem_bound(ref, S, 27, lipschitz=1.1)


def sppf_ref(x16: torch.Tensor) -> torch.Tensor:
    """x (B, H, W, C) fp16 -> (B, H, W, 3C) fp32 = [mp5(x), mp5(mp5(x)), mp5^3(x)]: three F.max_pool2d(5, 1, 2) on the values."""
    x = x16.float().permute(0, 3, 1, 2)
    p1 = F.max_pool2d(x, 5, 1, 2)
    p2 = F.max_pool2d(p1, 5, 1, 2)
    p3 = F.max_pool2d(p2, 5, 1, 2)
    return torch.cat((p1, p2, p3), 1).permute(0, 2, 3, 1).contiguous()


def upsample_ref(x: torch.Tensor) -> torch.Tensor:
    """x (B, H, W, C) -> (B, 2H, 2W, C): output pixel (ho, wo) is input pixel (ho // 2, wo // 2)."""
    _, H, W, _ = x.shape
    return x[:, torch.arange(2 * H) // 2][:, :, torch.arange(2 * W) // 2].contiguous()


def decode_anchors(in_h: int, in_w: int):
    """(anchor centres (A, 2) as (x, y) in cells, strides (A)) of the three levels, float64: level of stride s has (in_h / s) x
    (in_w / s) cells, row-major, centre (gx + 0.5, gy + 0.5)."""
    pts, st = [], []
    for s in (8, 16, 32):
        h, w = in_h // s, in_w // s
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
        pts.append(torch.stack((gx.reshape(-1) + 0.5, gy.reshape(-1) + 0.5), 1))
        st.append(torch.full((h * w,), float(s), dtype=torch.float64))
    return torch.cat(pts), torch.cat(st)


def decode_ref(raw: torch.Tensor, in_h: int, in_w: int, nc: int, nm: int) -> torch.Tensor:
    """raw (B, A, 64 + nc + nm) -> (B, A, 4 + nc + nm) float64: cxcywh in pixels from the softmax expectation over 16 bins of each of
    l, t, r, b around the anchor, sigmoid class scores, the nm coefficients copied through (exactly: fp32 -> fp64)."""
    raw = raw.double()
    B, A, _ = raw.shape
    anchors, strides = decode_anchors(in_h, in_w)
    assert anchors.shape[0] == A
    p = torch.softmax(raw[..., :64].reshape(B, A, 4, 16), 3)
    ltrb = (p * torch.arange(16, dtype=torch.float64)).sum(3)
    x1y1 = anchors - ltrb[..., :2]
    x2y2 = anchors + ltrb[..., 2:]
    box = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 2) * strides[:, None]
    return torch.cat((box, torch.sigmoid(raw[..., 64:64 + nc]), raw[..., 64 + nc:]), 2)


def adown_ref(x16: torch.Tensor):
    """x (B, H, W, C) fp16, H and W even -> (a (B, H-1, W-1, C/2), m (B, H/2, W/2, C/2)) fp16, the bits the kernel must produce:
    t = fp16(((p00 + p01) + (p10 + p11)) * 0.25) in float32, a = t[..., :C/2], m = the max of t[..., C/2:] over the 3x3 / stride-2
    window at (2y - 1, 2x - 1), clipped to the (H-1) x (W-1) map."""
    x = x16.float()
    B, H, W, C = x.shape
    t = (((x[:, :-1, :-1] + x[:, :-1, 1:]) + (x[:, 1:, :-1] + x[:, 1:, 1:])) * 0.25).half()
    a = t[..., :C // 2].contiguous()
    u = t[..., C // 2:].float()
    Hm, Wm = H // 2, W // 2
    up = F.pad(u, (0, 0, 1, 1, 1, 1), value=float("-inf"))   # row / column -1 and H-1 / W-1: outside the map, never the maximum
    m = torch.full((B, Hm, Wm, C // 2), float("-inf"))
    for dy in range(3):
        for dx in range(3):
            m = torch.maximum(m, up[:, dy:dy + 2 * Hm:2, dx:dx + 2 * Wm:2])
    return a, m.half()
