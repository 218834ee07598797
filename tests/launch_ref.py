"""Shared helpers of the per-launch parity tests of the raw strided C-ABI (m355_conv_launch, m355_wgrad_launch,
m355_bn_train_fwd_launch / _bwd_launch; include/mi355yolo.h, "raw strided launches").

A plain module (no fixtures, no GPU needed to import):
  - guard-banded NHWC buffers: the output slice lives inside a larger buffer whose every other element holds a sentinel NaN
    bit pattern no kernel produces; after a launch the slice is compared with the reference and everything outside it must
    still be the sentinel, bit for bit;
  - packers of the weight layouts, written from the header text (not from train_engine.py), and plain torch restatements of
    the kernels' arithmetic over those layouts (the host tests check packer + restatement against F.conv2d / autograd);
  - fp32 references on fp16-rounded operands, with the magnitude sum S behind every output element;
  - the per-element bound |got - ref| <= 2^-10 |ref| + c S, c = min(2^-13, 1 / (2 K)), K = products per output element.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

SENT16 = 0x7E5A                 # fp16 NaN with a payload no kernel writes
SENT32 = 0x7FC0DEAD             # fp32 NaN with a payload no kernel writes
GUARD = 256                     # sentinel elements before and after every allocation


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------- guard-banded buffers
class Guarded:
    """A (B, H, W, ctot) NHWC buffer with image stride `bstride` (>= H W ctot) in a flat allocation of fp16 or fp32, GUARD
    elements of sentinel before and after it.  Slices are handed to a kernel as (ptr(off), ld = ctot, bstride)."""

    def __init__(self, B, H, W, ctot, device, f32=False, bstride=None):
        self.B, self.H, self.W, self.ctot = B, H, W, ctot
        self.bstride = H * W * ctot if bstride is None else bstride
        assert self.bstride >= H * W * ctot
        self.f32 = f32
        self.esize = 4 if f32 else 2
        self.n = GUARD + B * self.bstride + GUARD
        self.bits = torch.full((self.n,), SENT32 if f32 else SENT16, dtype=torch.int32 if f32 else torch.int16, device=device)

    @property
    def sentinel(self) -> int:
        return SENT32 if self.f32 else SENT16

    def ptr(self, off: int = 0) -> int:
        return self.bits.data_ptr() + (GUARD + off) * self.esize

    def _nhwc(self, t: torch.Tensor) -> torch.Tensor:
        body = t[GUARD:GUARD + self.B * self.bstride]
        return body.as_strided((self.B, self.H, self.W, self.ctot), (self.bstride, self.W * self.ctot, self.ctot, 1))

    def values(self) -> torch.Tensor:
        return self._nhwc(self.bits.view(torch.float32 if self.f32 else torch.float16))

    def write(self, off: int, v: torch.Tensor) -> None:
        """v (B, H, W, c) -> channels [off, off + c)."""
        self.values()[..., off:off + v.shape[-1]].copy_(v.to(self.values().dtype))

    def fill_random(self, gen: torch.Generator, scale: float = 64.0) -> None:
        """Finite garbage everywhere (inputs: a kernel reading outside its slice picks up large wrong values, not NaN)."""
        r = ((torch.rand(self.n, generator=gen) * 2 - 1) * scale).to(torch.float32 if self.f32 else torch.float16)
        self.bits.copy_(r.view(self.bits.dtype).to(self.bits.device))

    def slice_and_guard(self, off: int, c: int) -> Tuple[torch.Tensor, int, Optional[int]]:
        """(slice values (B, H, W, c) as fp32 on the CPU, number of elements outside the slice that lost the sentinel,
        flat index of the first of them)."""
        bits = self.bits.cpu()
        inside = torch.zeros(self.n, dtype=torch.bool)
        self._nhwc(inside)[..., off:off + c] = True
        bad = (bits != self.sentinel) & ~inside
        nbad = int(bad.sum())
        first = int(bad.nonzero()[0, 0]) - GUARD if nbad else None
        vals = self._nhwc(bits.view(torch.float32 if self.f32 else torch.float16))[..., off:off + c].float().clone()
        return vals, nbad, first


def guard_report(buf: Guarded, nbad: int, first: Optional[int]) -> str:
    if not nbad:
        return "guard intact"
    b, r = divmod(first, buf.bstride)
    return (f"{nbad} element(s) outside the slice overwritten; first at image {b}, pixel {r // buf.ctot}, channel {r % buf.ctot} "
            f"(flat {first} of bstride {buf.bstride})")


# ---------------------------------------------------------------------------------------------------- packers (header text)
def pack_fwd(w: torch.Tensor) -> torch.Tensor:
    """Forward conv weight (cout, cin, k, k) -> fp16 [ceil128(cout)][kpad], K = (kh * k + kw) * cin + ci, kpad % 64 == 0."""
    cout, cin, k, _ = w.shape
    out = torch.zeros(ceil_to(cout, 128), ceil_to(k * k * cin, 64), dtype=torch.float16)
    out[:cout, :k * k * cin] = w.permute(0, 2, 3, 1).reshape(cout, k * k * cin).half()
    return out


def pack_dgrad_s1(w: torch.Tensor) -> torch.Tensor:
    """Input gradient of a stride-1 conv (cout, cin, k, k) as a conv over dY: rows ci, K = (flipped tap) * cout + co,
    flipped tap = (k - 1 - kh) * k + (k - 1 - kw): the forward layout of the flipped, channel-transposed weight."""
    return pack_fwd(w.flip(2, 3).transpose(0, 1))


def pack_dgrad_gather(w: torch.Tensor) -> torch.Tensor:
    """tmode 1 (transposed-stride gather of a 3x3 / s2 / p1 conv): rows ci, K = (kh * 3 + kw) * cout + co, taps NOT flipped."""
    return pack_fwd(w.transpose(0, 1))


def pack_dgrad_phase(w: torch.Tensor, compact: bool) -> torch.Tensor:
    """tmode 2: rows [phase q = 2a + b][ci] (4 cin rows, padded to 128), columns [(slot)][co] with slot ty * (1 + b) + tx (compact)
    or ty * 2 + tx (window slots).  Phase (a, b) = dX pixels (2i + a, 2j + b); window tap ty reads dY row i + ty.  From dX row
    2i + a = 2 o - 1 + kh: a = 0 takes kh = 1 at ty = 0; a = 1 takes kh = 2 at ty = 0 and kh = 0 at ty = 1 (columns alike)."""
    cout, cin, _, _ = w.shape
    out = torch.zeros(ceil_to(4 * cin, 128), ceil_to(4 * cout, 64), dtype=torch.float16)
    taps = {0: [(0, 1)], 1: [(0, 2), (1, 0)]}          # parity -> [(window tap, forward tap)]
    for a in (0, 1):
        for b in (0, 1):
            q = 2 * a + b
            for ty, kh in taps[a]:
                for tx, kw in taps[b]:
                    slot = ty * (1 + b) + tx if compact else ty * 2 + tx
                    out[q * cin:(q + 1) * cin, slot * cout:(slot + 1) * cout] = w[:, :, kh, kw].t().half()
    return out


def pack_convt(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(k = 2, s = 2) weight (cin, cout, 2, 2) -> rows (dy, dx, co) = 4 cout virtual channels, K = ci."""
    cin, cout, _, _ = w.shape
    out = torch.zeros(ceil_to(4 * cout, 128), ceil_to(cin, 64), dtype=torch.float16)
    out[:4 * cout, :cin] = w.permute(2, 3, 1, 0).reshape(4 * cout, cin).half()
    return out


def phase_form(cin: int, cout: int, res: bool) -> int:
    """The tmode-2 form the header promises for forward channels (cin, cout): 3 compact, 2 window slots, 0 = not accepted."""
    if cin % 64 == 0:
        return 3 if cout % 64 == 0 else 2
    return 2 if (128 % cin == 0 and 4 * cin >= 64 and not res) else 0


# ---------------------------------------------------------------------------------------------------- host restatements
def igemm_conv(x: torch.Tensor, packed: torch.Tensor, cout: int, k: int, stride: int, pad: int) -> torch.Tensor:
    """The implicit GEMM over a forward-layout matrix: x (B, H, W, cin) fp32 NHWC -> (B, Ho, Wo, cout); patch column
    (kh * k + kw) * cin + ci, out-of-map taps zero."""
    B, H, W, cin = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    cols = []
    for kh in range(k):
        for kw in range(k):
            cols.append(xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :])
    patch = torch.cat(cols, dim=-1)                                     # (B, Ho, Wo, k k cin)
    return patch @ packed[:cout, :k * k * cin].float().t()


def igemm_gather(dy: torch.Tensor, packed: torch.Tensor, H: int, W: int, cin: int) -> torch.Tensor:
    """tmode 1: dX(h, w) = sum over taps (kh, kw) with h + 1 - kh = 2 i, w + 1 - kw = 2 j inside dY of dY(i, j) . row (kh, kw)."""
    B, Ho, Wo, cout = dy.shape
    out = torch.zeros(B, H, W, cin)
    for kh in range(3):
        for kw in range(3):
            wt = packed[:cin, (kh * 3 + kw) * cout:(kh * 3 + kw + 1) * cout].float()     # (cin, cout)
            for h in range(H):
                if (h + 1 - kh) % 2 or not 0 <= (h + 1 - kh) // 2 < Ho:
                    continue
                i = (h + 1 - kh) // 2
                ws = [w_ for w_ in range(W) if (w_ + 1 - kw) % 2 == 0 and 0 <= (w_ + 1 - kw) // 2 < Wo]
                js = [(w_ + 1 - kw) // 2 for w_ in ws]
                out[:, h, ws, :] += dy[:, i, js, :] @ wt.t()
    return out


def igemm_phase(dy: torch.Tensor, packed: torch.Tensor, cin: int, compact: bool) -> torch.Tensor:
    """tmode 2: the four 2x2 phase convs over dY (windows at (i, j), dY zero past the map), rows (q, ci), slot columns."""
    B, Ho, Wo, cout = dy.shape
    dyp = F.pad(dy, (0, 0, 0, 1, 0, 1))
    out = torch.zeros(B, 2 * Ho, 2 * Wo, cin)
    for a in (0, 1):
        for b in (0, 1):
            q = 2 * a + b
            acc = torch.zeros(B, Ho, Wo, cin)
            for ty in (0, 1):
                for tx in (0, 1):
                    slot = ty * (1 + b) + tx if compact else ty * 2 + tx
                    if compact and (ty > a or tx > b):
                        continue                                        # past the phase's (1 + a)(1 + b) taps: the K loop ends
                    wt = packed[q * cin:(q + 1) * cin, slot * cout:(slot + 1) * cout].float()
                    acc += dyp[:, ty:ty + Ho, tx:tx + Wo, :] @ wt.t()
            out[:, a::2, b::2, :] = acc
    return out


def igemm_convt(x: torch.Tensor, packed: torch.Tensor, cout: int) -> torch.Tensor:
    """ConvT forward as a 1x1 GEMM to 4 cout virtual channels (dy, dx, co), scattered to pixel (2h + dy, 2w + dx)."""
    B, H, W, cin = x.shape
    v = x @ packed[:4 * cout, :cin].float().t()                          # (B, H, W, 4 cout)
    v = v.view(B, H, W, 2, 2, cout)
    return v.permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, cout)


# ---------------------------------------------------------------------------------------------------- references + bound
def conv_ref(x, w, stride, pad):
    """x (B, H, W, cin) NHWC, w (cout, cin, k, k): forward conv, fp32/fp64 NHWC."""
    return F.conv2d(x.permute(0, 3, 1, 2), w, None, stride, pad).permute(0, 2, 3, 1)


def dgrad_ref(dy, w, H, W, stride, pad):
    """Input gradient of conv2d(x (B, cin, H, W), w) for dY (B, Ho, Wo, cout) NHWC -> (B, H, W, cin)."""
    B, _, _, _ = dy.shape
    dx = torch.nn.grad.conv2d_input((B, w.shape[1], H, W), w, dy.permute(0, 3, 1, 2), stride, pad)
    return dx.permute(0, 2, 3, 1)


def convt_ref(x, w):
    """ConvTranspose2d(k = 2, s = 2) of x (B, H, W, cin) with w (cin, cout, 2, 2) -> (B, 2H, 2W, cout)."""
    return F.conv_transpose2d(x.permute(0, 3, 1, 2), w, None, 2).permute(0, 2, 3, 1)


def silu(v):
    return v * torch.sigmoid(v)


def elem_bound(ref: torch.Tensor, S: torch.Tensor, K: int, lipschitz: float = 1.0) -> torch.Tensor:
    """2^-10 |ref| + c S, c = min(2^-13, 1 / (2K)): one dropped or doubled product term of a K-term sum exceeds the c S slack
    whenever it is at least half the average |term|; fp16 x fp16 products are exact in fp32 and the fp32 summation error
    (~ sqrt(K) 2^-24 S) is far below it; the 2^-10 |ref| term covers the final rounding to fp16."""
    c = min(2.0 ** -13, 1.0 / (2 * K))
    return 2.0 ** -10 * ref.abs() + c * lipschitz * S


def check_elementwise(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> Tuple[float, float, str]:
    """(worst |got - ref| / bound, rel-L2, description of the worst element)."""
    err = (got.double() - ref.double()).abs()
    ratio = err / bound.double().clamp_min(1e-30)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.flatten().argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    desc = f"worst at {idx}: got {float(got[idx]):.6g} ref {float(ref[idx]):.6g} bound {float(bound[idx]):.3g}"
    return float(ratio.max()), rel_l2(got, ref), desc


# ---------------------------------------------------------------------------------------------------- conv launch geometry
@dataclass
class ConvGeom:
    """One m355_conv_launch geometry.  Offsets / ld / bstride are in elements of the buffer's dtype; bstride None = H W ld."""
    batch: int
    hi: int
    wi: int
    cin: int
    ho: int
    wo: int
    cout: int
    k: int
    stride: int
    pad: int
    tmode: int = 0
    convt_co: int = 0
    out_f32: int = 0
    act: int = 0
    fwd_cout: int = 0          # tmode 1 / 2: forward output channels (= cin of the launch); informational
    ldx: int = 0
    x_off: int = 0
    x_bs: Optional[int] = None
    ldy: int = 0
    y_off: int = 0
    y_bs: Optional[int] = None
    res: str = "none"          # "none" | "own" (a slice of its own buffer) | "inplace" (res == y: y += conv)
    ldr: int = 0
    r_off: int = 0
    r_bs: Optional[int] = None
    bias: bool = True
    name: str = ""

    def key(self):
        d = dict(self.__dict__)
        d.pop("name")
        return tuple(sorted(d.items()))


def _kind(g: ConvGeom) -> str:
    if g.tmode == 1:
        return "gather"
    if g.tmode == 2:
        return "phase"
    if g.convt_co > 0:
        return "convt"
    return "conv"


def conv_operands(g: ConvGeom, seed: int):
    """Random fp16-rounded operands of geometry g, as fp64 CPU tensors in the FORWARD-op orientation:
    (x NHWC (B, hi, wi, cin), w, bias or None, packed fp16 rows, y map (H, W, C) of the output slice, K products per output)."""
    gen = torch.Generator().manual_seed(seed)
    kind = _kind(g)
    x = torch.randn(g.batch, g.hi, g.wi, g.cin, generator=gen).half().double()
    if kind == "conv":
        w = (torch.randn(g.cout, g.cin, g.k, g.k, generator=gen) / (g.cin * g.k * g.k) ** 0.5).half().double()
        packed, ymap, K = pack_fwd(w), (g.ho, g.wo, g.cout), g.k * g.k * g.cin
    elif kind == "convt":
        w = (torch.randn(g.cin, g.convt_co, 2, 2, generator=gen) / g.cin ** 0.5).half().double()
        packed, ymap, K = pack_convt(w), (2 * g.hi, 2 * g.wi, g.convt_co), g.cin
    elif kind == "gather":
        # x = dY of a 3x3 / s2 / p1 conv with forward weights (fwd cout = launch cin, fwd cin = launch cout)
        w = (torch.randn(g.cin, g.cout, 3, 3, generator=gen) / (g.cin * 9) ** 0.5).half().double()
        packed, ymap, K = pack_dgrad_gather(w), (g.ho, g.wo, g.cout), 9 * g.cin
    else:
        w = (torch.randn(g.cin, g.convt_co, 3, 3, generator=gen) / (g.cin * 9) ** 0.5).half().double()
        form = phase_form(g.convt_co, g.cin, g.res != "none")
        packed, ymap, K = pack_dgrad_phase(w, form == 3), (2 * g.ho, 2 * g.wo, g.convt_co), 4 * g.cin
    bias = None
    if g.bias and kind in ("conv", "convt"):
        bias = (torch.randn(ymap[2], generator=gen) * 0.5).float().double()
    if g.tmode == 2:
        assert g.ho == g.hi and g.wo == g.wi and g.cout == 4 * g.convt_co and g.k == 2
    return x, w, bias, packed, ymap, K


def conv_reference(g: ConvGeom, x, w, bias):
    """(ref without residual / act, S the magnitude sum) of the forward-orientation op of g, fp64 NHWC."""
    kind = _kind(g)
    if kind == "conv":
        f = lambda a, b: conv_ref(a, b, g.stride, g.pad)
    elif kind == "convt":
        f = convt_ref
    elif kind == "gather":
        f = lambda a, b: dgrad_ref(a, b, g.ho, g.wo, 2, 1)
    else:
        f = lambda a, b: dgrad_ref(a, b, 2 * g.ho, 2 * g.wo, 2, 1)
    ref, S = f(x, w), f(x.abs(), w.abs())
    if bias is not None:
        ref, S = ref + bias, S + bias.abs()
    return ref, S


def last_error(capi) -> str:
    m = capi.lib.m355_last_error(None)
    return m.decode() if m else ""


def run_conv_geom(capi, g: ConvGeom, device, seed: int = 0, stream=None):
    """Launch geometry g on guard-banded buffers with random operands, compare with the fp64 reference.  Returns a dict:
    rc, ratio (worst |err| / bound), rel, guard (number of clobbered elements outside the slices), desc."""
    x, w, bias, packed, (Hy, Wy, Cy), K = conv_operands(g, seed)
    gen = torch.Generator().manual_seed(seed + 7)
    ldx = g.ldx or g.cin
    xb = Guarded(g.batch, g.hi, g.wi, ldx, device, bstride=g.x_bs)
    xb.fill_random(gen)
    xb.write(g.x_off, x.half())
    ldy = g.ldy or Cy
    yb = Guarded(g.batch, Hy, Wy, ldy, device, f32=bool(g.out_f32), bstride=g.y_bs)
    ref, S = conv_reference(g, x, w, bias)
    lip = 1.1 if g.act else 1.0
    if g.act:
        ref = silu(ref)
    rb = None
    if g.res == "own":
        rb = Guarded(g.batch, Hy, Wy, g.ldr, device, bstride=g.r_bs)
        rb.fill_random(gen)
        r = torch.randn(g.batch, Hy, Wy, Cy, generator=gen).half()
        rb.write(g.r_off, r)
        ref = ref + r.double()
        res_ptr, r_bs, ldr = rb.ptr(g.r_off), rb.bstride, rb.ctot
    elif g.res == "inplace":
        prior = torch.randn(g.batch, Hy, Wy, Cy, generator=gen).half()
        yb.write(g.y_off, prior)
        ref = ref + prior.double()
        res_ptr, r_bs, ldr = yb.ptr(g.y_off), yb.bstride, yb.ctot
    else:
        res_ptr, r_bs, ldr = 0, 0, 0
    d_w = packed.to(device)
    nb = ceil_to(max(g.cout, Cy), 128) + 128
    d_bias = torch.zeros(nb, dtype=torch.float32, device=device)
    if bias is not None:
        d_bias[:Cy] = bias.float().to(device)
    zero = torch.zeros(256, dtype=torch.uint8, device=device)
    a = capi.ConvLaunchArgs()
    a.x, a.x_bstride, a.ldx, a.hi, a.wi, a.cin = xb.ptr(g.x_off), xb.bstride, ldx, g.hi, g.wi, g.cin
    a.w_packed, a.kpad = d_w.data_ptr(), d_w.shape[1]
    a.bias = d_bias.data_ptr()
    a.y, a.y_bstride, a.ldy, a.ho, a.wo, a.cout = yb.ptr(g.y_off), yb.bstride, ldy, g.ho, g.wo, g.cout
    a.res, a.r_bstride, a.ldr = res_ptr, r_bs, ldr
    a.ksize, a.stride, a.pad, a.batch = g.k, g.stride, g.pad, g.batch
    a.act, a.out_f32, a.convt_co, a.tmode = g.act, g.out_f32, g.convt_co, g.tmode
    a.zero_page = zero.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    rc = int(capi.lib.m355_conv_launch(C.byref(a), st))
    out = {"rc": rc, "err": last_error(capi) if rc else ""}
    if rc:
        return out
    torch.cuda.synchronize()
    got, nbad, first = yb.slice_and_guard(g.y_off, Cy)
    gbad = nbad
    desc = guard_report(yb, nbad, first)
    ratio, rel, wdesc = check_elementwise(got, ref, elem_bound(ref, S, K, lip))
    out.update(ratio=ratio, rel=rel, guard=gbad, desc=f"{desc}; {wdesc}", K=K)
    return out


# ---------------------------------------------------------------------------------------------------- wgrad launch geometry
@dataclass
class WgradGeom:
    batch: int
    hi: int
    wi: int
    cin: int
    ho: int
    wo: int
    cout: int
    k: int
    stride: int
    pad: int
    ldx: int = 0
    x_off: int = 0
    x_bs: Optional[int] = None
    lddz: int = 0
    dz_off: int = 0
    dz_bs: Optional[int] = None
    name: str = ""

    def key(self):
        d = dict(self.__dict__)
        d.pop("name")
        return tuple(sorted(d.items()))


def wgrad_reference(x, dz, k, stride, pad, cout):
    """dW (cout, k, k, cin) KRSC of conv2d(x, w) for the output gradient dz, both NHWC fp64; and S on |x|, |dz|."""
    def f(a, b):
        dw = torch.nn.grad.conv2d_weight(a.permute(0, 3, 1, 2), (cout, a.shape[3], k, k), b.permute(0, 3, 1, 2), stride, pad)
        return dw.permute(0, 2, 3, 1)
    return f(x, dz), f(x.abs(), dz.abs())


def run_wgrad_geom(capi, g: WgradGeom, device, seed: int = 0, ws_delta: int = 0, repeat: bool = True):
    """m355_wgrad_launch of geometry g with random slices inside larger buffers; a workspace of exactly
    m355_wgrad_workspace_bytes + ws_delta bytes.  Returns rc, ratio, rel, bitwise (repeat run identical), K, need."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.batch, g.hi, g.wi, g.cin, generator=gen).half()
    dz = torch.randn(g.batch, g.ho, g.wo, g.cout, generator=gen).half()
    ldx, lddz = g.ldx or g.cin, g.lddz or g.cout
    xb = Guarded(g.batch, g.hi, g.wi, ldx, device, bstride=g.x_bs)
    xb.fill_random(gen)
    xb.write(g.x_off, x)
    zb = Guarded(g.batch, g.ho, g.wo, lddz, device, bstride=g.dz_bs)
    zb.fill_random(gen)
    zb.write(g.dz_off, dz)
    need = int(capi.lib.m355_wgrad_workspace_bytes(g.batch, g.ho, g.wo, g.cin, g.cout, g.k))
    wsb = need + ws_delta
    ws = torch.empty(max(wsb, 4) // 4 + 1, dtype=torch.float32, device=device)
    zero = torch.zeros(256, dtype=torch.uint8, device=device)
    # dW inside an fp32 guard band: no write past the cout x k x k x cin result
    n = g.cout * g.k * g.k * g.cin
    dwb = torch.full((GUARD + n + GUARD,), SENT32, dtype=torch.int32, device=device)

    def launch():
        a = capi.WgradLaunchArgs()
        a.dz, a.dz_bstride, a.lddz = zb.ptr(g.dz_off), zb.bstride, lddz
        a.x, a.x_bstride, a.ldx = xb.ptr(g.x_off), xb.bstride, ldx
        a.hi, a.wi, a.cin, a.ho, a.wo, a.cout = g.hi, g.wi, g.cin, g.ho, g.wo, g.cout
        a.ksize, a.stride, a.pad, a.batch = g.k, g.stride, g.pad, g.batch
        a.dw, a.zero_page = dwb.data_ptr() + GUARD * 4, zero.data_ptr()
        a.ws, a.ws_bytes = (ws.data_ptr() if wsb > 0 else 0), wsb
        return int(capi.lib.m355_wgrad_launch(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    rc = launch()
    out = {"rc": rc, "need": need, "err": last_error(capi) if rc else ""}
    if rc:
        return out
    torch.cuda.synchronize()
    bits = dwb.cpu()
    out["guard"] = int((bits[:GUARD] != SENT32).sum() + (bits[GUARD + n:] != SENT32).sum())
    got = bits[GUARD:GUARD + n].view(torch.float32).view(g.cout, g.k, g.k, g.cin).double()
    ref, S = wgrad_reference(x.double(), dz.double(), g.k, g.stride, g.pad, g.cout)
    K = g.batch * g.ho * g.wo
    out["ratio"], out["rel"], out["desc"] = check_elementwise(got, ref, elem_bound(ref, S, K))
    out["K"] = K
    if repeat:
        dwb.fill_(SENT32)
        assert launch() == 0
        torch.cuda.synchronize()
        out["bitwise"] = bool(torch.equal(dwb.cpu()[GUARD:GUARD + n], bits[GUARD:GUARD + n]))
    return out
