"""Selector-weight probes for the fused multi-stage launches (host only, no GPU code).

A fused launch (bneck_pair, c2f_c32, s2c64_cv1, stem_s2c32_cv1, proto_phase) keeps a hidden fp16 tensor in LDS.  A float64 reference of
the whole chain cannot be judged element by element: a hidden value may land on either side of an fp16 rounding boundary, and one fp16
ulp per hidden element carried through sum |w2| of a 3x3 stage gives a bound (4.5e-2 at 64 channels) looser than the 2e-2 the old tests
assert.  A probe chooses the weights so that this ambiguity disappears:

  exact-hidden       the stages BEFORE the judged one are selectors: a 0/1 weight on one tap and a zero bias.  Such a stage computes
                     SiLU(one input element) (the fp32 sum of one product x * 1 and zeros is exact).  The inputs are drawn from the fp16
                     values whose SiLU rounds to fp16 unambiguously (silu_safe_values), so the hidden tensor is known bit for bit: a table
                     lookup of the zero-padded, shifted input.  The judged stage then is a plain conv of known fp16 operands:
                     conv_bound.conv_ref / conv_tol with the K of that stage alone.
  transparent-tail   the stages AFTER the judged one are selectors: every output element is SiLU(one hidden element) (+ residual), so every
                     hidden element is seen, its zero-padding ring included (through the off-centre taps).  The bound of the judged stage is
                     carried through each later stage (tail, below).

Bound of a transparent later stage.  Let v be the float64 reference of a hidden element, t its bound, h the kernel's fp16 value,
|h - v| <= t.  The selector stage computes z = h exactly (one product h * 1, zeros, bias 0), then in fp32
    a32 = SiLU(h) with the hardware exp2 / rcp:  |a32 - silu64(h)| <= 2^-20 |silu64(h)|       (conv_bound.py, third term)
    |silu64(h) - silu64(v)| <= 1.1 t                                                          (SiLU is Lipschitz, max |silu'| = 1.0998)
    so |a32 - silu64(v)| <= mid := 1.1 t + 2^-20 (|silu64(v)| + 1.1 t)
    y32 = a32 + residual in fp32 (where the launch adds one): one fp32 rounding, 2^-24 (|y64| + mid)
    out = fp16(y32): 2^-11 |y32| + 2^-25 with |y32| <= |y64| + mid + the fp32 rounding
    t' = mid + r + 2^-11 (|y64| + mid + r) + 2^-25,   r = 2^-24 (|y64| + mid) with a residual, else 0
with y64 = silu64(v) (+ residual).  A padded position has v = 0 and t = 0: the output must be the residual (or 0) to 2^-25.
Nothing here is tuned; the constants are those of conv_bound.py.

Safe values.  With s = silu64(v) and h = fp16(s), v is safe when s is farther from both rounding boundaries of h (the midpoints to its
fp16 neighbours) than 2^-18 |s| -- four times the 2^-20 |silu| that conv_bound.py allows the hardware exp2 / rcp path -- and h is not
subnormal (|s| >= 2^-14, or v == 0).  Any SiLU within 2^-20 |s| of s, fp32 F.silu included, then rounds to the same h.  depth = 2 keeps the
values whose h is itself safe: two selector stages in a row (c2f_c32 with the 1x1 stage judged) are then exact too.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_bound as cb

L_SILU = 1.1
TAPS = ((0, 0), (2, 2), (0, 2), (1, 1))         # the off-centre taps see the padding ring; the centre tap does not


def silu64(z):
    return z * torch.sigmoid(z)


@functools.lru_cache(maxsize=None)
def _safe_table(depth):
    bits = np.concatenate((np.arange(0x0000, 0x4601), np.arange(0x8001, 0xC601))).astype(np.uint16)      # |v| <= 6, one zero
    v16 = bits.view(np.float16)
    v = torch.from_numpy(v16.astype(np.float64))
    s = silu64(v)
    h16 = s.numpy().astype(np.float16)
    h = torch.from_numpy(h16.astype(np.float64))
    with np.errstate(over="ignore"):
        up = torch.from_numpy(np.nextafter(h16, np.float16(np.inf)).astype(np.float64))
        dn = torch.from_numpy(np.nextafter(h16, np.float16(-np.inf)).astype(np.float64))
    margin = torch.minimum((h + up) / 2 - s, s - (h + dn) / 2)
    ok = ((margin > 2.0 ** -18 * s.abs()) & (s.abs() >= 2.0 ** -14)) | (v == 0)
    order = torch.argsort(v)
    v, h, ok = v[order], h[order], ok[order]
    if depth == 2:
        v1, _, _ = _safe_table(1)
        pos = torch.searchsorted(v1, h).clamp(max=v1.numel() - 1)
        ok = ok & (v1[pos] == h)
    total = int(v.numel()) + 1                    # the fp16 values in [-6, 6], -0 counted as the issue counts it
    return v[ok].contiguous(), h[ok].contiguous(), total


def silu_safe_values(depth=1):
    """(sorted fp16 values v with |v| <= 6 whose SiLU rounds to fp16 unambiguously, their exact fp16 SiLU), both float64."""
    v, h, _ = _safe_table(depth)
    return v, h


def safe_fraction(depth=1):
    v, _, total = _safe_table(depth)
    return v.numel() / total


def snap_safe(x, depth=1):
    """Every element of x moved to the nearest safe value (float32 holding fp16 values)."""
    v, _ = silu_safe_values(depth)
    xd = x.double().clamp(float(v[0]), float(v[-1]))
    hi = torch.searchsorted(v, xd).clamp(1, v.numel() - 1)
    lo = hi - 1
    pick = torch.where((xd - v[lo]).abs() <= (v[hi] - xd).abs(), lo, hi)
    return v[pick].float()


def draw_safe(shape, gen, hot_border=False, depth=1):
    """N(0, 0.8) snapped to the nearest safe value; shape (B, C, H, W).  hot_border: the first and last rows and columns times 4 before
    snapping (as tests/test_dwconv_gpu.py heats its border), so a wrong padding or a wrapped neighbour reads a large value."""
    x = torch.randn(shape, generator=gen) * 0.8
    if hot_border:
        x = heat_border(x)
    return snap_safe(x, depth)


def heat_border(x):
    x = x.clone()
    x[:, :, 0] *= 4
    x[:, :, -1] *= 4
    x[:, :, :, 0] *= 4
    x[:, :, :, -1] *= 4
    return x


def silu_exact(x16):
    """The exact fp16 SiLU (float64 tensor) of a tensor of safe values (zeros included): the table lookup."""
    v, h = silu_safe_values(1)
    xd = x16.double()
    pos = torch.searchsorted(v, xd).clamp(max=v.numel() - 1)
    assert torch.equal(v[pos], xd), "silu_exact: an element is no safe value"
    return h[pos]


# ---- selector weights (every selector bias is 0)
def delta3x3(cout, cin, tap):
    """w[c, c % cin, ky, kx] = 1 and nothing else.  tap = (ky, kx), or a sequence of taps of which output channel c takes the
    (c // cin)-th (the stride-2 64 -> 128 selector: two taps per probe)."""
    taps = [tap] if isinstance(tap[0], int) else list(tap)
    w = torch.zeros(cout, cin, 3, 3)
    for c in range(cout):
        ky, kx = taps[(c // cin) % len(taps)]
        w[c, c % cin, ky, kx] = 1.0
    return w


def select1x1(cout, cin, offset):
    """w[o, offset + o % (cin - offset)] = 1 and nothing else."""
    w = torch.zeros(cout, cin, 1, 1)
    for o in range(cout):
        w[o, offset + o % (cin - offset), 0, 0] = 1.0
    return w


def zero_bias(n):
    return torch.zeros(n)


def select(t64, w_sel, stride=1):
    """A selector applied to a float64 tensor: the zero-padded, shifted (strided) copy.  Exact: every output is one input times 1."""
    assert bool(((w_sel == 0) | (w_sel == 1)).all()) and bool((w_sel.flatten(1).sum(1) == 1).all()), "not a selector"
    return F.conv2d(t64.double(), w_sel.double(), None, stride=stride, padding=w_sel.shape[-1] // 2)


# ---- reference and bound
def judged(x16, w16, bias, k, stride=1, res16=None):
    """The judged stage: float64 reference and per-element bound of SiLU(conv(x16; w16) + bias) (+ res16), conv_bound's own, with the K
    of this stage alone."""
    y64, z64, S = cb.conv_ref(x16, w16, bias, k, stride, 1, res16)
    return y64, cb.conv_tol(y64, z64, S, w16.shape[1] * k * k, 1, res16)


def stem_stage0(img_u8_nchw, w0, b0):
    """Float64 reference and bound of the stem's first stage, SiLU(conv3x3/s2(u8 image; w0) / 255 + b0).  The products u8 * fp16 are exact
    in fp32 (8 + 11 bits); the fp32 sum is scaled by the fp32 constant 1/255 in the epilogue: the constant's own rounding and the
    multiply's are two more roundings of a value bounded by S, so K + 1 becomes K + 3 in the accumulation term."""
    y, z, S = cb.conv_ref(img_u8_nchw.float(), w0, zero_bias(w0.shape[0]), 3, 2, 0, None)
    bb = b0.double().view(1, -1, 1, 1)
    z64, S = z / 255.0 + bb, S / 255.0 + bb.abs()
    y64 = silu64(z64)
    return y64, cb.conv_tol(y64, z64, S, 27 + 2, 1)


def tail(v64, t, w_sel=None, stride=1, res16=None):
    """One transparent later stage (module docstring): the selector w_sel (None: the identity) applied to the hidden reference v64 and its
    bound t, SiLU, the residual where the launch adds one, one fp16 rounding.  Returns (y64, t')."""
    if w_sel is not None:
        v64, t = select(v64, w_sel, stride), select(t, w_sel, stride)
    s = silu64(v64)
    y64 = s if res16 is None else s + res16.double()
    mid = L_SILU * t + 2.0 ** -20 * (s.abs() + L_SILU * t)
    r = 2.0 ** -24 * (y64.abs() + mid) if res16 is not None else torch.zeros_like(mid)
    return y64, mid + r + 2.0 ** -11 * (y64.abs() + mid + r) + 2.0 ** -25


def summary(got, y64, tol):
    """(worst |err|/tol, its index, elements beyond the bound, median tolerance)."""
    worst, idx, bad = cb.worst_ratio(got, y64, tol)
    return worst, idx, bad, float(tol.median())


# ---- proto_phase: ConvTranspose2d(2x2, s2) -> Conv3x3 as four 2x2 phase convs over the low-resolution input
def proto_phase_weights(wt, w3, rounded=True):
    """The composed phase weights, float64 sums rounded to fp16 ONCE (as include/mi355yolo.h says the host does):
    Weff[q = py * 2 + px][co, ci, a, b] = sum over the taps (kh, kw) of w3 whose high-resolution row py + kh - 1 lies in low-resolution row
    offset a - 1 + py (columns alike) of sum_c w3[co, c, kh, kw] * wt[ci, c, dy, dx], (dy, dx) the parity of that tap's position."""
    n = w3.shape[0]
    weff = torch.zeros(4, n, n, 2, 2, dtype=torch.float64)
    w3d, wtd = w3.double(), wt.double()
    for py in range(2):
        for px in range(2):
            for kh in range(3):
                ty = py + kh - 1
                a, dy = (ty // 2) + 1 - py, ty % 2
                for kw in range(3):
                    tx = px + kw - 1
                    b, dx = (tx // 2) + 1 - px, tx % 2
                    weff[py * 2 + px, :, :, a, b] += w3d[:, :, kh, kw] @ wtd[:, :, dy, dx].t()
    if not rounded:
        return weff
    r16 = weff.half().double()
    assert torch.equal(weff.float().half().double(), r16), "a composed weight rounds differently through fp32: draw other weights"
    return r16


def proto_phase_conv(x, weff, absolute=False):
    """The four 2x2 phase convs of the zero-padded low-resolution x (B, n, H, W) -> (B, n, 2H, 2W), float64 (absolute: of |x|, |weff|)."""
    B, n, H, W = x.shape
    xp = F.pad(x.double(), (1, 1, 1, 1))
    out = torch.zeros(B, weff.shape[1], 2 * H, 2 * W, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            wq = weff[py * 2 + px]
            full = F.conv2d(xp.abs(), wq.abs()) if absolute else F.conv2d(xp, wq)
            out[:, :, py::2, px::2] = full[:, :, py:py + H, px:px + W]
    return out


def proto_hidden(x16, wt, bt, w3, b3):
    """Float64 reference and bound of proto_phase's hidden tile SiLU(cv2(upsample(x))), (B, n, 2H, 2W): per phase a 2x2 conv (K = 4 n) of
    the zero-padded input with the composed fp16 weights; the bias of a pixel is b3 + the w3 . bt of the 3x3 taps inside the image."""
    B, n, H, W = x16.shape
    weff = proto_phase_weights(wt, w3)
    up_b = bt.double().view(1, n, 1, 1).expand(1, n, 2 * H, 2 * W)
    bmap = (F.conv2d(up_b, w3.double(), b3.double(), padding=1)).float().double().expand(B, n, 2 * H, 2 * W)
    z64, S = proto_phase_conv(x16, weff), proto_phase_conv(x16, weff, absolute=True)
    z64, S = z64 + bmap, S + bmap.abs()
    y64 = silu64(z64)
    return y64, cb.conv_tol(y64, z64, S, 4 * n, 1)


def weak_stage(v64, t, w16, bias, k, stride=1):
    """WEAK: a random 3x3 stage behind a hidden tensor that is only known to its bound t.  The hidden error is carried through the
    stage in L1 (sum |w| t over the window: every hidden element off by its whole bound, all with the worst sign), which no kernel does;
    the result bounds a correct kernel but is an order of magnitude looser than an fp16 ulp of the output.  Returns (y64, tol)."""
    wd, bd = w16.double(), bias.double()
    z64 = F.conv2d(v64, wd, bd, stride=stride, padding=k // 2)
    dz = F.conv2d(t, wd.abs(), None, stride=stride, padding=k // 2)
    S = F.conv2d(v64.abs() + t, wd.abs(), bd.abs(), stride=stride, padding=k // 2)
    y64 = silu64(z64)
    return y64, cb.conv_tol(y64, z64, S, w16.shape[1] * k * k, 1) + L_SILU * dz * (1 + 2.0 ** -11)


# ---- the probes of each launch: operands in the order of the C-ABI entry, the float64 reference and the bound
def _r16(t):
    return t.half().float()


def rand_w(gen, cout, cin, k):
    return _r16(torch.randn((cout, cin, k, k), generator=gen) * (2.0 / (k * k * cin)) ** 0.5)


def rand_b(gen, n):
    return torch.randn(n, generator=gen) * 0.3


def hot_x(gen, shape):
    return _r16(heat_border(torch.randn(shape, generator=gen) * 0.8))


ONLY_EXACT = 2.0 ** -25      # half the smallest fp16 spacing: only the tabulated value itself passes


def bneck_probe(kind, B, H, W, C, tap, shortcut, seed=0):
    """m355_bneck_pair_fwd.  'exact': stage 1 a selector on safe inputs, stage 2 random and judged (K = 9 C).  'tail': stage 1 random with
    a non-zero bias and judged (a computed halo element would be SiLU(bias + partial window), not 0), stage 2 a selector."""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        x = draw_safe((B, C, H, W), g, hot_border=True)
        wa, ba, wb, bb = delta3x3(C, C, tap), zero_bias(C), rand_w(g, C, C, 3), rand_b(g, C)
        hidden = silu_exact(select(x, wa))
        y64, tol = judged(hidden, wb, bb, 3, res16=x if shortcut else None)
    else:
        x = hot_x(g, (B, C, H, W))
        wa, ba, wb, bb = rand_w(g, C, C, 3), rand_b(g, C), delta3x3(C, C, tap), zero_bias(C)
        v, t = judged(x, wa, ba, 3)
        y64, tol = tail(v, t, wb, res16=x if shortcut else None)
    return dict(x=x, w=(wa, ba, wb, bb), y64=y64, tol=tol)


def c2f_probe(kind, B, H, W, tap, seed=0):
    """m355_c2f_c32_fwd: x = [y0, y1]; t = SiLU(conv3x3(y1; wa)); y2 = fp16(SiLU(conv3x3(t; wb)) (+ y1)); out = SiLU(conv1x1([y0, y1, y2]; wc)).
      'a'     wa random (judged), wb a selector, wc selects the y2 third; shortcut on (transparent tail with the residual y1)
      'b'     wa a selector on safe y1 (hidden exact), wb random (judged, with the shortcut as its residual), wc selects y2
      'c'     wa and wb selectors on depth-2 safe y1, shortcut OFF (fp16(SiLU(t) + y1) would be ambiguous): y2 exact, wc random (judged)
      'pass'  wa, wb random, wc selects [y0, y1]: the pass-through channels arrive as fp16(SiLU(x)) bit for bit
    Returns the shortcut flag with the operands."""
    g = torch.Generator().manual_seed(seed)
    sel_y2, zeros = select1x1(64, 96, 64), zero_bias
    if kind == "a":
        x, shortcut = hot_x(g, (B, 64, H, W)), True
        wa, ba, wb, bb, wc, bc = rand_w(g, 32, 32, 3), rand_b(g, 32), delta3x3(32, 32, tap), zeros(32), sel_y2, zeros(64)
        v, t = judged(x[:, 32:], wa, ba, 3)
        y2, t2 = tail(v, t, wb, res16=x[:, 32:])
    elif kind == "b":
        x, shortcut = draw_safe((B, 64, H, W), g, hot_border=True), True
        wa, ba, wb, bb, wc, bc = delta3x3(32, 32, tap), zeros(32), rand_w(g, 32, 32, 3), rand_b(g, 32), sel_y2, zeros(64)
        y2, t2 = judged(silu_exact(select(x[:, 32:], wa)), wb, bb, 3, res16=x[:, 32:])
    elif kind == "c":
        x, shortcut = draw_safe((B, 64, H, W), g, hot_border=True, depth=2), False
        wa, ba, wb, bb = delta3x3(32, 32, tap), zeros(32), delta3x3(32, 32, (2 - tap[0], 2 - tap[1])), zeros(32)
        wc, bc = rand_w(g, 64, 96, 1), rand_b(g, 64)
        y2 = silu_exact(select(silu_exact(select(x[:, 32:], wa)), wb))
        y64, tol = judged(torch.cat((x.double(), y2), 1), wc, bc, 1)
        return dict(x=x, w=(wa, ba, wb, bb, wc, bc), shortcut=shortcut, y64=y64, tol=tol)
    else:
        x, shortcut = draw_safe((B, 64, H, W), g, hot_border=True), True
        wa, ba, wb, bb = rand_w(g, 32, 32, 3), rand_b(g, 32), rand_w(g, 32, 32, 3), rand_b(g, 32)
        wc, bc = select1x1(64, 96, 0), zeros(64)
        y64 = silu_exact(x)
        return dict(x=x, w=(wa, ba, wb, bb, wc, bc), shortcut=shortcut, y64=y64, tol=torch.full_like(y64, ONLY_EXACT))
    xd = x.double()
    y64, tol = tail(torch.cat((xd, y2), 1), torch.cat((torch.zeros_like(xd), t2), 1), wc)
    return dict(x=x, w=(wa, ba, wb, bb, wc, bc), shortcut=shortcut, y64=y64, tol=tol)


def s2c64_probe(kind, B, H, W, taps, seed=0):
    """m355_s2c64_cv1_fwd (3x3 / s2 64 -> 128, then 1x1 128 -> 128).  'exact': the stride-2 selector maps output channel c to input c % 64
    with the tap taps[c // 64]; the 1x1 stage is random and judged (K = 128).  'tail': the 3x3 stage random with a bias and judged,
    the 1x1 stage the identity."""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        x = draw_safe((B, 64, H, W), g, hot_border=True)
        w3, b3, w1, b1 = delta3x3(128, 64, taps), zero_bias(128), rand_w(g, 128, 128, 1), rand_b(g, 128)
        y64, tol = judged(silu_exact(select(x, w3, 2)), w1, b1, 1)
    else:
        x = hot_x(g, (B, 64, H, W))
        w3, b3, w1, b1 = rand_w(g, 128, 64, 3), rand_b(g, 128), select1x1(128, 128, 0), zero_bias(128)
        v, t = judged(x, w3, b3, 3, stride=2)
        y64, tol = tail(v, t)
    return dict(x=x, w=(w3, b3, w1, b1), y64=y64, tol=tol)


def stem_probe(kind, B, H, W, taps, seed=0):
    """m355_stem_s2c32_cv1_fwd (uint8 image -> 3x3 / s2 3 -> 32 with the 1/255 inside -> 3x3 / s2 32 -> 64 -> 1x1 64 -> 64).  The uint8 / 255
    input cannot be made exact, so both probes are transparent-tail.  'a': w0 random (judged, with its zero padding), w1 the stride-2
    selector (output channel c reads channel c % 32 through the tap taps[c // 32]), w2 the identity.  'b', WEAK: w0 and w1 random, w2 the
    identity: stage 0's bound goes through the random 3x3 stage in L1 (weak_stage)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    img[:, 0], img[:, -1], img[:, :, 0], img[:, :, -1] = 255, 255, 255, 255      # a hot border
    w0, b0 = _r16(torch.randn((32, 3, 3, 3), generator=g) * (2.0 / 27) ** 0.5 * 2.0), rand_b(g, 32)
    v, t = stem_stage0(img.permute(0, 3, 1, 2), w0, b0)
    if kind == "a":
        w1, b1 = delta3x3(64, 32, taps), zero_bias(64)
        v, t = tail(v, t, w1, stride=2)
    else:
        w1, b1 = rand_w(g, 64, 32, 3), rand_b(g, 64)
        v, t = weak_stage(v, t, w1, b1, 3, stride=2)
    y64, tol = tail(v, t)
    return dict(x=img, w=(w0, b0, w1, b1, select1x1(64, 64, 0), zero_bias(64)), y64=y64, tol=tol)


def proto_probe(B, H, W, quarter, with_bt, seed=0):
    """m355_proto_phase_fwd.  The ConvTranspose weight wt[c, c, a, b] = 1 makes the upsampling nearest-neighbour (+ bt); w3 is random; wc
    selects hidden channels [32 quarter, 32 quarter + 32): every element of the hidden SiLU(cv2) tile is judged, borders included.
    with_bt: a non-zero ConvTranspose bias, which reaches a pixel only through the 3x3 taps inside the image."""
    g = torch.Generator().manual_seed(seed)
    x = hot_x(g, (B, 128, H, W))
    wt = torch.zeros(128, 128, 2, 2)
    wt[torch.arange(128), torch.arange(128)] = 1.0
    w3, b3 = rand_w(g, 128, 128, 3), rand_b(g, 128)
    bt = rand_b(g, 128) if with_bt else zero_bias(128)
    wc = select1x1(32, 128, 32 * quarter)
    v, t = proto_hidden(x, wt, bt, w3, b3)
    y64, tol = tail(v, t, wc)
    return dict(x=x, w=(wt, bt, w3, b3, wc, zero_bias(32)), y64=y64, tol=tol)
