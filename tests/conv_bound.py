"""Per-element bound for the output of a conv kernel (host only, no GPU code).

A whole-tensor rel-L2 of 1e-3 catches a wrong tile; it does not catch ONE wrong element (a border pixel, the last channel of a
ragged tile).  This module bounds every element against a float64 reference of the same fp16-rounded operands.

What a correct kernel computes (the epilogue of csrc/device_prims.h):
    z32 = fp32 sum, in any order (MFMA's internal adds included), of the K = cin*k*k products x*w, plus the bias in fp32
    a32 = SiLU(z32) in fp32 with the hardware exp2 / rcp approximations        (if act)
    y32 = a32 + residual in fp32                                               (if a residual is given)
    out = y32 rounded ONCE to fp16 (or kept as fp32 for out_f32)

Derivation of the bound, term by term, with S = sum |x||w| + |bias| (float64):
  * accumulation.  The products of fp16 operands are exact in fp32.  K products and one bias are K + 1 terms; every partial sum of any
    summation tree is bounded by S, each add rounds by at most 2^-24 of its result, and a term passes through at most K adds:
    |z32 - z64| <= K * 2^-24 * S to first order.  (K + 1) * 2^-23 * S doubles that, so the bound holds for any order, for MFMA's
    internal adds (which need not round each add to nearest) and for the second-order terms.
  * SiLU is Lipschitz with constant max |silu'| = 1.0998 < L = 1.1 (L = 1 without activation), so the accumulation error reaches the
    output as at most L * (K + 1) * 2^-23 * S.
  * exp2 / rcp approximations, the multiply by log2(e), the 1 + e add and the final multiply: a few fp32 ulp of the result,
    2^-20 * |silu(z64)| = 16 ulp (drops out without SiLU).
  * the fp16 rounding of y32: 2^-11 * |y32| for normal results, half the subnormal spacing 2^-25 below 2^-14.
    |y32| <= |y64| + (the two middle terms), hence the last term 2^-11 * (the two middle terms).
    (The fp32 rounding of the residual add, 2^-24 * |y|, is far inside the doubled accumulation term.)

    tol = 2^-11 |y64| + 2^-25 + L (K+1) 2^-23 S + 2^-20 |silu(z64)| + 2^-11 (L (K+1) 2^-23 S + 2^-20 |silu(z64)|)

For fp32 output nothing is rounded to fp16: 2^-11 becomes 2^-24 and the subnormal term drops (the first two terms become
2^-24 |y64|).

These constants are derived, not tuned.  A later change may tighten them with a derivation; it may not loosen them without one.
"""
import torch
import torch.nn.functional as F


def _silu64(z):
    return z * torch.sigmoid(z)


def conv_ref(x16, w16, bias, k, stride, act, res16=None):
    """x16 (B, cin, H, W) and w16 (cout, cin, k, k) hold fp16-representable values (any float dtype), bias (cout,) fp32,
    res16 (B, cout, Ho, Wo) fp16-representable or None.  Returns (y64, z64, S), each (B, cout, Ho, Wo) float64:
    y64 the conv + bias (+ SiLU) (+ residual), z64 the value before the activation, S = conv(|x|, |w|) + |bias|."""
    x, w, b = x16.double(), w16.double(), bias.double()
    assert torch.equal(x, x.half().double()) and torch.equal(w, w.half().double()), "operands must be fp16-rounded"
    z64 = F.conv2d(x, w, b, stride=stride, padding=k // 2)
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=k // 2)
    y64 = _silu64(z64) if act else z64.clone()
    if res16 is not None:
        y64 = y64 + res16.double()
    return y64, z64, S


def conv_tol(y64, z64, S, K, act, res16=None, out_f32=False):
    """The per-element bound of the module docstring.  K = cin * k * k.  (res16 enters through y64 only.)"""
    L = 1.1 if act else 1.0
    acc = L * (K + 1) * 2.0 ** -23 * S
    apx = 2.0 ** -20 * _silu64(z64).abs() if act else torch.zeros_like(S)
    mid = acc + apx
    if out_f32:
        return 2.0 ** -24 * y64.abs() + mid + 2.0 ** -24 * mid
    return 2.0 ** -11 * y64.abs() + 2.0 ** -25 + mid + 2.0 ** -11 * mid


def worst_ratio(got, y64, tol):
    """(worst |got - y64| / tol, its (image, channel, row, col), count of elements above 1).  A non-finite element counts as inf."""
    ratio = (got.double() - y64).abs() / tol
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    idx = []
    for n in reversed(ratio.shape):
        idx.append(flat % n)
        flat //= n
    return float(ratio.max()), tuple(reversed(idx)), int((ratio > 1.0).sum())


def check_elements(got, y64, tol, what=""):
    """got (B, cout, Ho, Wo).  Asserts that no element misses its bound; returns (worst ratio, index, count)."""
    assert got.shape == y64.shape == tol.shape, (got.shape, y64.shape, tol.shape)
    worst, idx, bad = worst_ratio(got, y64, tol)
    assert bad == 0, (f"{what}: {bad} of {got.numel()} elements beyond their bound; worst |err|/tol {worst:.3g} at (image, channel, row, col) "
                      f"= {idx}: got {float(got[idx]):.6g}, want {float(y64[idx]):.6g}, tol {float(tol[idx]):.3g}")
    return worst, idx, bad


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-12))


def draw_operands(case_key, B, H, W, cin, cout, k, use_res, stride=1):
    """Operands drawn as tests/test_ops_gpu.py::test_conv2d_fwd draws them: x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias ~ 0.1 N(0, 1),
    residual ~ N(0, 1); x, w and the residual rounded to fp16.  Returns fp32 tensors (x16, w16, bias, res16 or None)."""
    g = torch.Generator().manual_seed(hash(case_key) % (2 ** 31))
    x = torch.randn(B, cin, H, W, generator=g).half().float()
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half().float()
    b = torch.randn(cout, generator=g) * 0.1
    res = None
    if use_res:
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        res = torch.randn(B, cout, Ho, Wo, generator=g).half().float()
    return x, w, b, res
