"""Float64 reference, per-element bounds, input families and launch geometry for the train-mode BatchNorm(+SiLU)(+residual)
kernels of csrc/train_kernels.hip (host only, no GPU code; in the style of tests/conv_bound.py).

Everything works on (npix, C) matrices of fp16-representable values held as float64; channels are columns.

What a correct forward computes, given the statistics `mean` and `invstd` it returns (fp32 values, exact in float64):
    sc = fl(gamma * invstd)                 sh = fl(beta - fl(mean * sc))
    t  = fl(fl(z * sc) + sh)                (or one fused multiply-add: fewer roundings)
    a  = SiLU(t) with the hardware exp2 / rcp approximations      (if act)
    y  = fp16(fl(a + residual))
The reference is u = (z - mean) * invstd * gamma + beta, y = silu(u) + residual in float64 WITH THE SAME mean AND invstd: the apply
arithmetic is judged on its own, the statistics are judged against float64 statistics by their own tolerances.

Bound for y, term by term, with A = |z||sc| + |mean||sc| + |beta| and one fp32 rounding = 2^-24 relative:
  * sc is rounded once (touches z sc and mean sc), mean * sc once, the subtraction that gives sh once (touches mean sc and beta),
    z * sc once, the final add once (touches all three): at most 3 roundings touch |z||sc|, 4 touch |mean||sc|, 2 touch |beta|.
    5 * 2^-24 * A covers the worst count and the second-order terms: E_u.  It scales with |mean||sc|: it is large exactly at the
    channels with |mean| >> std, where sc = gamma / std is large.
  * SiLU is Lipschitz with max |silu'| = 1.0998 < L = 1.1 (L = 1 without activation): L * E_u reaches the output.
  * exp2 / rcp, the 1 + e add and the final multiply: 2^-20 |silu(u)| (16 ulp), as in conv_bound.py.  The exponent's argument
    t * -log2(e) is rounded too; that moves sigmoid by at most |t| sg (1 - sg) 2^-24 and SiLU by t^2 sg (1 - sg) 2^-24
    <= 0.55 * 2^-24 absolute (max of t^2 e^-|t| is 0.54): 2^-24 added.
  * the fp32 residual add: 2^-24 (|silu(u)| + |residual|).
  * the fp16 rounding of the result: 2^-11 |y32| for normal results, 2^-25 below 2^-14; |y32| <= |y64| + (the terms above).

    mid = L * 5 * 2^-24 * A + [2^-20 |silu(u)| + 2^-24] + 2^-24 (|act(u)| + |residual|)
    tol = 2^-11 |y64| + 2^-25 + mid + 2^-11 mid

What a correct backward computes, given mean, invstd and the reduced sums dbeta, dgamma it returns (fp32, exact in float64):
    xh = fl(fl(z - mean) * invstd)          t = fl(fl(gamma * xh) + beta)
    du = dy                                  (no activation)
    du = fl(dy * g~),  g~ = fl(sg~ * fl(1 + fl(t * fl(1 - sg~))))  ~  silu'(t) = sg (1 + t (1 - sg))      (SiLU)
    k1 = fl(gamma * invstd), k2 = fl(dbeta * fl(1 / n)), k3 = fl(dgamma * fl(1 / n))
    dz = fp16(fl(k1 * fl(fl(du - k2) - fl(xh * k3))))
    dbeta = sum du, dgamma = sum fl(du * xh), fp32, in some fixed order over the npix pixels
Bound for dz with T1 = |du|, T2 = |dbeta| / n, T3 = |xh||dgamma| / n:
  * xh carries 2 roundings, k2 and k3 carry 2 each, xh * k3 one more (5 on T3); du - k2 one (T1, T2), the second subtraction one
    (all), k1 one and the last product one (all): 4 roundings touch T1 (beyond du's own error), 6 touch T2, 8 touch T3.
    9 * 2^-24 * (T1 + T2 + T3) covers the worst count and the second-order terms.
  * du's own error E_du (zero without activation, dy is exact):
      t is off by at most dt = 5 * 2^-24 (|gamma xh| + |beta|) (xh 2, the product 1, the add 1 touching both; 5 as above), and
      |silu''| <= 1/2, so silu'(t) moves by dt / 2;
      sg~ = sg (1 + e1), e1 <= (1 - sg) |t| 2^-23 + 2^-22 (argument rounding and the rounded constant; exp2, the add, rcp);
      with B = 1 + |t| (1 - sg) >= |1 + t (1 - sg)|: fl(1 - sg~) is off by sg e1 + 2^-24 (1 - sg); times t and rounded:
      |t| sg e1 + 2^-23 |t| (1 - sg); the 1 + add: 2^-24 B; the product with sg~: sg e1 B + 2^-24 |g|:
        dg = sg e1 (B + |t| sg) + sg 2^-23 |t| (1 - sg) + sg 2^-24 B + 2^-24 |g|
      E_du = |dy| (dg + dt / 2) + 2^-24 |du|
  * E = |k1| (E_du + 9 * 2^-24 (T1 + T2 + T3));   tol = 2^-11 |dz64| + 2^-25 + E + 2^-11 E
Bound for dbeta / dgamma per channel: a recursive sum of n fp32 terms in ANY order is within gamma_n = n 2^-24 / (1 - n 2^-24) of
sum |term| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), plus what each term carries in:
    tol_dbeta  = sum E_du + gamma_n sum |du|
    tol_dgamma = sum (|xh| E_du + 3 * 2^-24 |du xh|) + gamma_n sum |du xh|          (xh 2 roundings, the product 1)

These constants are derived, not tuned.  A later change may tighten them with a derivation; it may not loosen them without one.

Geometry: lanes_px, red_rows, red_stride and apply_blocks restate grid_red / grid_px and the launchers of csrc/train_kernels.hip
(BN_THREADS = 256, BN_ROWS = 512, four pixels per trip).  They MUST follow that file: the tests use them to put spikes on the
seams of the kernels' pixel walks.
"""
import math

import torch

BN_THREADS = 256
BN_ROWS = 512
EPS = 1e-3                       # the training graph's BatchNorm eps
U24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- launch geometry
def lanes_px(C):
    """pixel lanes of a block: a thread owns one 8-channel group, BN_THREADS // (C / 8) pixels side by side."""
    return BN_THREADS // (C // 8)


def idle_threads(C):
    return BN_THREADS - lanes_px(C) * (C // 8)


def red_rows(npix, C):
    """blocks (= partial rows) of the two reduction kernels: grid_red(npix * BN_THREADS / lanes_px / 4)."""
    work = npix * BN_THREADS // lanes_px(C) // 4
    g = min(max((work + BN_THREADS - 1) // BN_THREADS, 1), 256 * 8)
    return min(g, BN_ROWS)


def red_stride(npix, C):
    """pixels between two visits of one reduction thread: thread (block b, lane l) walks b * lanes_px + l + k * stride."""
    return red_rows(npix, C) * lanes_px(C)


def apply_blocks(npix, C):
    """grid_px: blocks of the two apply kernels (at least 16 pixels per thread, at most 2048 blocks)."""
    lp = lanes_px(C)
    return min(max((npix + lp * 16 - 1) // (lp * 16), 1), 256 * 8)


def seam_pixels(npix, C):
    """Pixels on the seams of the reduction walk, one spike each: the first and last pixel, both sides of the first stride and
    of the first four-pixel trip, the first pixel that the tail loop (one pixel per trip) takes, and one pixel of the last
    active thread of block 0 (lane lanes_px - 1; the threads behind it idle when C / 8 does not divide 256)."""
    st = red_stride(npix, C)
    main_trips = max((npix - 3 * st + 4 * st - 1) // (4 * st), 0) if npix > 3 * st else 0   # trips of thread 0's main loop
    tail0 = 4 * st * main_trips
    want = [0, npix - 1, st - 1, st, 4 * st - 1, 4 * st, tail0, lanes_px(C) - 1]
    return [p if 0 <= p < npix else (7 * i + 3) % npix for i, p in enumerate(want)]


# ---------------------------------------------------------------------------------------------------- input families
FAMILIES = [(0.3, 1.7), (8.0, 0.05), (30.0, 0.05), (-60.0, 0.5), (100.0, 0.1), (4.0, 0.02), (1000.0, 2.0), (2048.0, 16.0),
            (1e-3, 1e-4), (-0.02, 30.0), (0.0, 0.0), (12.5, 0.0)]
# gamma: zero, both signs, and 25 / -30, which take |u| to about 100 at four standard deviations (SiLU saturated on both
# sides).  The outlier pixels sit at 0.5 sqrt(npix) <= 128 standard deviations for npix <= 65 792: |u| <= 3 843, far from the
# fp16 limit 65 504.  Cycles of 12, 7 and 5: each family meets every gamma and beta as the channel index grows.
GAMMAS = [1.0, 0.0, -1.5, 25.0, 0.7, -30.0, 2.0]
BETAS = [0.0, 0.5, -2.0, 3.0, -0.1]


def family_params(C, shift=0):
    """Per-channel (mean, std, gamma, beta), float64 tensors of C; channel c takes family (c + shift) mod 12, so different
    families share every 8-channel group.  family_name(c, shift) names it for failure messages."""
    fam = [FAMILIES[(c + shift) % len(FAMILIES)] for c in range(C)]
    mean = torch.tensor([f[0] for f in fam], dtype=torch.float64)
    std = torch.tensor([f[1] for f in fam], dtype=torch.float64)
    gamma = torch.tensor([GAMMAS[c % len(GAMMAS)] for c in range(C)], dtype=torch.float32).double()
    beta = torch.tensor([BETAS[c % len(BETAS)] for c in range(C)], dtype=torch.float32).double()
    return mean, std, gamma, beta


def family_name(c, shift=0):
    """shift None: the inputs are not drawn from FAMILIES (spike and constant-channel cases)."""
    if shift is None:
        return "(not a family case)"
    m, s = FAMILIES[(c + shift) % len(FAMILIES)]
    return f"(mean {m:g}, std {s:g})"


def draw_z(npix, C, variant, seed, shift=0):
    """z (npix, C) float64 of fp16-representable values: channel c ~ N(mean_c, std_c), rounded to fp16.  variant "outliers":
    pixel 0 and the last pixel sit at mean - 0.5 std sqrt(npix) (a statistic shifted by one channel-wide pivot taken from pixel 0
    cancels as badly as the unshifted one).  Returns (z, gamma, beta)."""
    assert variant in ("plain", "outliers")
    mean, std, gamma, beta = family_params(C, shift)
    g = torch.Generator().manual_seed(seed)
    z = mean + std * torch.randn(npix, C, generator=g, dtype=torch.float64)
    if variant == "outliers":
        z[0] = z[-1] = mean - 0.5 * std * math.sqrt(npix)
    return z.half().double(), gamma, beta


def stats64(z, eps=EPS):
    """(mean, biased variance, unbiased variance, invstd) per channel in float64."""
    n = z.shape[0]
    mean = z.mean(0)
    var_b = ((z - mean) ** 2).mean(0)
    var_u = var_b * (n / max(n - 1, 1))
    return mean, var_b, var_u, 1.0 / torch.sqrt(var_b + eps)


# the project's statistic tolerances (tests/test_strided_launch_gpu.py::test_bn_train_launch_slices)
STAT_TOL = {"mean": (1e-5, 1e-6), "invstd": (1e-5, 0.0), "running_mean": (1e-5, 1e-7), "running_var": (1e-5, 1e-7)}


def stat_ratio(got, want, what):
    """per-channel |got - want| / (atol + rtol |want|) (torch.allclose's criterion); non-finite counts as inf."""
    rtol, atol = STAT_TOL[what]
    r = (got.double() - want).abs() / (atol + rtol * want.abs())
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))


def check_stat(got, want, what, shift=0, note=""):
    r = stat_ratio(got, want, what)
    c = int(r.argmax())
    assert float(r.max()) <= 1.0, (f"{note}{what}: {int((r > 1).sum())} of {r.numel()} channels beyond rtol {STAT_TOL[what][0]:g}; worst channel {c} "
                                   f"{family_name(c, shift)}: got {float(got[c]):.9g}, want {float(want[c]):.9g}, "
                                   f"relative error {abs(float(got[c]) - float(want[c])) / max(abs(float(want[c])), 1e-300):.3g}, "
                                   f"{float(r.max()):.3g} x the tolerance")
    return float(r.max()), c


# ---------------------------------------------------------------------------------------------------- forward
def _sig(u):
    return torch.sigmoid(u)


def fwd_ref(z, mean, invstd, gamma, beta, act, res=None):
    """(y64, u64) with the statistics given (the kernel's own, cast to double, to judge the apply alone)."""
    u = (z - mean) * invstd * gamma + beta
    y = u * _sig(u) if act else u.clone()
    if res is not None:
        y = y + res
    return y, u


def fwd_tol(z, y64, u64, mean, invstd, gamma, beta, act, res=None):
    sc = (gamma * invstd).abs()
    A = z.abs() * sc + mean.abs() * sc + beta.abs()
    L = 1.1 if act else 1.0
    a = (u64 * _sig(u64)).abs() if act else u64.abs()
    mid = L * 5 * U24 * A + U24 * (a + (res.abs() if res is not None else 0.0))
    if act:
        mid = mid + 2.0 ** -20 * a + U24
    return 2.0 ** -11 * y64.abs() + 2.0 ** -25 + mid + 2.0 ** -11 * mid


# ---------------------------------------------------------------------------------------------------- backward
def bwd_terms(z, dy, mean, invstd, gamma, beta, act):
    """(xh, du, E_du) in float64: du = dy * silu'(u) (or dy), E_du the bound of the module docstring on a kernel's du."""
    xh = (z - mean) * invstd
    if not act:
        return xh, dy.clone(), torch.zeros_like(dy)
    t = gamma * xh + beta
    sg = _sig(t)
    g = sg * (1 + t * (1 - sg))
    dt = 5 * U24 * ((gamma * xh).abs() + beta.abs())
    e1 = (1 - sg) * t.abs() * 2.0 ** -23 + 2.0 ** -22
    B = 1 + t.abs() * (1 - sg)
    dg = sg * e1 * (B + t.abs() * sg) + sg * 2.0 ** -23 * t.abs() * (1 - sg) + sg * U24 * B + U24 * g.abs()
    du = dy * g
    return xh, du, dy.abs() * (dg + dt / 2) + U24 * du.abs()


def bwd_sums_ref(xh, du, e_du):
    """(dbeta, dgamma, tol_dbeta, tol_dgamma) per channel."""
    n = xh.shape[0]
    gam = n * U24 / (1 - n * U24)
    t2 = du * xh
    return (du.sum(0), t2.sum(0), e_du.sum(0) + gam * du.abs().sum(0),
            (xh.abs() * e_du + 3 * U24 * t2.abs()).sum(0) + gam * t2.abs().sum(0))


def bwd_dz_ref(xh, du, e_du, invstd, gamma, dbeta, dgamma):
    """(dz64, tol) with the reduced sums given (the kernel's own, cast to double, to judge the apply alone)."""
    n = xh.shape[0]
    k1 = gamma * invstd
    dz = k1 * (du - dbeta / n - xh * dgamma / n)
    T = du.abs() + dbeta.abs() / n + xh.abs() * dgamma.abs() / n
    E = k1.abs() * (e_du + 9 * U24 * T)
    return dz, 2.0 ** -11 * dz.abs() + 2.0 ** -25 + E + 2.0 ** -11 * E


# ---------------------------------------------------------------------------------------------------- judging
def worst_ratio(got, want, tol):
    """(worst |got - want| / tol, its index tuple, count of elements above 1).  A non-finite element counts as inf."""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)      # an exact result meets a bound of 0 (constant channels)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    idx = []
    for n in reversed(ratio.shape):
        idx.append(flat % n)
        flat //= n
    return float(ratio.max()), tuple(reversed(idx)), int((ratio > 1.0).sum())


def check_elements(got, want, tol, what="", shift=0):
    """got, want, tol (npix, C) or (C,).  Asserts that no element misses its bound; returns the worst ratio."""
    assert got.shape == want.shape == tol.shape, (got.shape, want.shape, tol.shape)
    worst, idx, bad = worst_ratio(got, want, tol)
    assert bad == 0, (f"{what}: {bad} of {got.numel()} elements beyond their bound; worst |err|/tol {worst:.3g} at {idx} "
                      f"(channel family {family_name(idx[-1], shift)}): got {float(got[idx]):.6g}, want {float(want[idx]):.6g}, "
                      f"tol {float(tol[idx]):.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------- cases
# The smallest shapes that reach each path of the launches (rows = red_rows(npix, C)):
SHAPES = {
    "a": (8, (1, 3, 7)),          # one channel group: lanes_px = 256, most threads without a pixel
    "b": (576, (2, 5, 7)),        # 72 channel groups: lanes_px = 3, 40 idle threads (the m-scale width)
    "c": (256, (2, 40, 48)),      # 120 rows: waves 0-7 of the row walk take its 8-way unrolled trip, waves 8-15 do not
    "d": (256, (2, 100, 101)),    # 632 -> capped at 512 rows, ragged: a four-pixel trip and a tail pixel per thread
    "e": (64, (1, 256, 257)),     # the cap at lanes_px = 32: four-pixel trip + tail loop
    "f": (2048, (2, 3, 3)),       # lanes_px = 1: the largest C the launcher accepts
}
# (shape, family shift): eight channels see only eight of the twelve families, so shape a runs twice
STAT_CASES = [("a", 0), ("a", 6), ("b", 0), ("c", 0), ("d", 0), ("e", 0), ("f", 0)]
VARIANTS = ("plain", "outliers")


def case_npix(name):
    B, H, W = SHAPES[name][1]
    return B * H * W
