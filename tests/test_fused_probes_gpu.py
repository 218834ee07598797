"""Per-element parity of the fused multi-stage launches through selector-weight probes (tests/fused_probe.py; what a probe is and which
fault each one sees: DESIGN.md, "Selector probes"; the proof that they discriminate: tests/test_fused_probe_host.py).

Entries: m355_bneck_pair_fwd, m355_c2f_c32_fwd, m355_s2c64_cv1_fwd, m355_stem_s2c32_cv1_fwd (both forms), m355_proto_phase_fwd, at the
smallest shapes that still hold a seam of every kind.  Every launch
  * writes into a NaN-filled body between 0xA5 guard bands whose bytes must not change, and reads its fp16 input from between NaN guard
    bands (the helpers of test_narrow_maps_gpu.py), so a read outside the tensor that feeds a result poisons it.  Two exceptions, by
    construction: the uint8 image of the stem cannot hold a NaN (it sits between bands of 255), and in the 384-channel concat case of
    bneck_pair input and output share ONE buffer, whose other channels hold the sentinel 7.0 and must keep it;
  * is judged element by element (conv_bound.check_elements) against the float64 reference and the derived bound of its probe;
  * still meets the old whole-tensor bound (rel-L2 <= 1e-3; 1.5e-3 for proto_phase);
  * is run twice for identical bits;
  * prints its worst |err|/tol, the index of that element and the median tolerance;
  * must be accepted: a refusal (M355_ERR_INVALID) of one of these shapes fails the test.

Measured on an MI355X (worst |err|/tol over the cases of the row, median tolerance; every bound is derived, a ratio above 1 is a finding):
(kernels of commit 7cd3901; this change touches no kernel source.)

  entry                  probe                       cases  worst |err|/tol  at (image, channel, row, col) of case            median tol
  bneck_pair             exact-hidden                   12  0.815            (0, 4, 0, 9)     tap22 (2, 23, 51, 64)           1.0e-3 .. 2.5e-3
  bneck_pair             transparent-tail               12  0.637            (0, 46, 0, 50)   tap11 (2, 23, 51, 64)           2.0e-3 .. 5.0e-3
  c2f_c32                a: wa judged (tail)             8  0.746            (1, 13, 3, 0)    tap11 (2, 16, 32)               1.5e-3 .. 2.0e-3
  c2f_c32                b: wb judged (exact + tail)     8  0.863            (1, 8, 15, 13)   tap02 (2, 16, 32)               8.9e-4 .. 1.1e-3
  c2f_c32                c: wc judged (exact)            8  0.925            (0, 53, 15, 13)  tap00 (2, 16, 32)               2.1e-4 .. 2.8e-4
  c2f_c32                pass-through                    2  0 (bit-exact)    -                                                3.0e-8
  s2c64_cv1              exact-hidden                    4  0.905            (0, 64, 0, 6)    tap0211 (2, 32, 48)             1.8e-4 .. 2.0e-4
  s2c64_cv1              transparent-tail                2  0.552            (1, 40, 0, 19)   (2, 32, 48)                     1.7e-3 .. 2.3e-3
  stem, two_team = 1     a: stage 0 (tail)               2  0.783            (1, 21, 5, 16)   tap0022 (2, 64, 128)            2.6e-4 .. 2.7e-4
  stem, two_team = 0     a: stage 0 (tail)               2  0.760            (1, 25, 3, 9)    tap0022 (2, 64, 128)            3.1e-4 .. 3.2e-4
  stem, two_team = 1     b: two random stages, WEAK      1  0.335            (1, 36, 5, 28)   (2, 64, 128)                    6.5e-3
  stem, two_team = 0     b: two random stages, WEAK      1  0.293            (1, 58, 0, 14)   (2, 64, 128)                    1.1e-2
  proto_phase            hidden quarter 0, bt = 0 / bt   4  0.644            (2, 14, 4, 44)   bt (3, 16, 32)                  1.5e-3 .. 2.7e-3
  proto_phase            hidden quarter 1                4  0.668            (1, 1, 10, 34)   bt0 (3, 16, 32)                 1.5e-3 .. 2.7e-3
  proto_phase            hidden quarter 2                4  0.643            (1, 11, 23, 21)  bt0 (3, 16, 32)                 1.5e-3 .. 2.7e-3
  proto_phase            hidden quarter 3                4  0.678            (1, 29, 25, 11)  bt0 (3, 16, 32)                 1.5e-3 .. 2.6e-3
No probe found a fault: no ratio above 1, no NaN from an input guard band, every guard byte intact, every second run bit-identical.  The
hot-border reruns of the random / random cases under the old assertions: bneck_pair rel-L2 2.1e-4, max |d| 7.8e-3 (bound 2e-2); c2f_c32
2.1e-4, 7.8e-3; s2c64_cv1 2.1e-4.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_bound as cb
import fused_probe as fp
from conv_harness import banded_input as _banded_input, guarded_output as _guarded_output, guards_intact as _guards_intact

pytestmark = pytest.mark.gpu

TAP_PAIRS = (((0, 0), (2, 2)), ((0, 2), (1, 1)))          # stride-2 selectors take two taps per probe (channel c: taps[c // cin])
_tid = lambda t: "tap" + "".join(str(i) for i in np.ravel(t))          # noqa: E731


def _np(ws):
    return [t.contiguous().numpy().astype(np.float32).copy() for t in ws]


def _h(a):
    return a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc(body, B, H, W, Cc):
    return body.view(torch.float16).reshape(B, H, W, Cc).permute(0, 3, 1, 2).float()


def _accepted(rc, what):
    from defectdetection_viaobjectdetection_amd import _capi
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc} ({(_capi.lib.m355_last_error(None) or b'').decode()!r}); the existing tests run this shape, a refusal is a failure"


def _judge(what, run, out_dims, y64, tol, dev, rel_bound=1e-3):
    """run(y pointer) launches the entry.  Output in a fresh guard-banded NaN body, judged per element, the old rel-L2 bound, a second
    run for identical bits, the figures printed."""
    B, Cc, Ho, Wo = out_dims
    outs = []
    for _ in range(2):
        raw, body = _guarded_output(B * Ho * Wo * Cc * 2, torch.float16, dev)
        _accepted(run(body.data_ptr()), what)
        outs.append(_guards_intact(raw, what))
    got = _nhwc(outs[0], B, Ho, Wo, Cc)
    _report(what, got, y64, tol, rel_bound)
    assert torch.equal(outs[0], outs[1]), f"{what}: two runs differ"


def _report(what, got, y64, tol, rel_bound):
    worst, idx, bad, med = fp.summary(got, y64, tol)
    rel = cb.rel_l2(got, y64)
    print(f"PROBE {what}: worst |err|/tol {worst:.3f} at (image, channel, row, col) = {idx}, median tol {med:.2e}, rel-L2 {rel:.2e}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (an element not written, or a read outside the input feeds it)"
    cb.check_elements(got, y64, tol, what)
    assert rel <= rel_bound, f"{what}: rel-L2 {rel}"


# ---- m355_bneck_pair_fwd
BNECK_SHAPES = [(1, 13, 37, 128, None), (2, 23, 51, 64, None), (1, 13, 37, 128, (128, 256, 384))]


def _bneck(what, x, w, shortcut, cat, y64, tol, dev, old_ref=None):
    """cat None: dense x between NaN bands, dense guard-banded output.  cat (xo, yo, total): x = channels [xo, xo + C) and the output =
    channels [yo, yo + C) of ONE guard-banded buffer of `total` channels; the other channels hold 7.0 and must keep it."""
    from defectdetection_viaobjectdetection_amd import _capi
    B, Cc, H, W = x.shape
    a = _np(w)

    def call(xp, ldx, yp, ldy):
        return _capi.lib.m355_bneck_pair_fwd(C.c_void_p(xp), B, H, W, Cc, ldx, _h(a[0]), _h(a[1]), _h(a[2]), _h(a[3]), int(shortcut),
                                             C.c_void_p(yp), ldy, _stream())
    if cat is None:
        xd, xp = _banded_input(x, dev)
        if old_ref is None:
            return _judge(what, lambda yp: call(xp, Cc, yp, Cc), (B, Cc, H, W), y64, tol, dev)
        raw, body = _guarded_output(B * H * W * Cc * 2, torch.float16, dev)
        _accepted(call(xp, Cc, body.data_ptr(), Cc), what)
        return _nhwc(_guards_intact(raw, what), B, H, W, Cc)
    xo, yo, tot = cat
    outs = []
    for _ in range(2):
        raw, body = _guarded_output(B * H * W * tot * 2, torch.float16, dev)
        buf = body.view(B, H, W, tot)
        buf[..., :xo] = 7.0
        buf[..., xo:xo + Cc] = x.permute(0, 2, 3, 1).to(dev).half()
        buf[..., xo + Cc:yo] = 7.0
        buf[..., yo + Cc:] = 7.0
        _accepted(call(body.data_ptr() + 2 * xo, tot, body.data_ptr() + 2 * yo, tot), what)
        outs.append(_guards_intact(raw, what))
    full = outs[0].view(torch.float16).reshape(B, H, W, tot)
    other = torch.cat((full[..., :xo], full[..., xo + Cc:yo], full[..., yo + Cc:]), -1)
    assert bool((other == 7.0).all()), f"{what}: a channel outside the output lost its sentinel"
    assert torch.equal(full[..., xo:xo + Cc].float(), x.permute(0, 2, 3, 1)), f"{what}: the input channels changed"
    got = full[..., yo:yo + Cc].permute(0, 3, 1, 2).float()
    if old_ref is not None:
        return got
    _report(what, got, y64, tol, 1e-3)
    assert torch.equal(outs[0], outs[1]), f"{what}: two runs differ"


@pytest.mark.parametrize("tap", fp.TAPS, ids=_tid)
@pytest.mark.parametrize("kind", ["exact", "tail"])
@pytest.mark.parametrize("B,H,W,Cc,cat", BNECK_SHAPES)
def test_bneck_pair_probe(cuda_device, B, H, W, Cc, cat, kind, tap):
    p = fp.bneck_probe(kind, B, H, W, Cc, tap, True, seed=B * 1000 + H * 10 + Cc)
    _bneck(f"bneck_pair {kind} {_tid(tap)} {(B, H, W, Cc)} cat={cat}", p["x"], p["w"], True, cat, p["y64"], p["tol"], cuda_device)


@pytest.mark.parametrize("B,H,W,Cc,cat", BNECK_SHAPES)
def test_bneck_pair_hot_border_old_assertions(cuda_device, B, H, W, Cc, cat):
    """The random / random case of test_bneck_pair_gpu.py with a hot border, under its assertions (rel-L2 1e-3, max |d| 2e-2)."""
    from test_bneck_pair_gpu import _ref
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cc)
    x = fp.hot_x(g, (B, Cc, H, W))
    w = (fp.rand_w(g, Cc, Cc, 3), fp.rand_b(g, Cc), fp.rand_w(g, Cc, Cc, 3), fp.rand_b(g, Cc))
    got = _bneck(f"bneck_pair hot {(B, H, W, Cc)} cat={cat}", x, w, True, cat, None, None, cuda_device, old_ref=True)
    want = _ref(x, *w, True)
    rel, worst = cb.rel_l2(got, want), float((got - want.half().float()).abs().max())
    print(f"PROBE bneck_pair hot border {(B, H, W, Cc)} cat={cat}: rel-L2 {rel:.2e}, max |d| vs the fp16-rounded reference {worst:.2e}")
    assert bool(torch.isfinite(got).all()) and rel <= 1e-3 and worst <= 2e-2


# ---- m355_c2f_c32_fwd
C2F_SHAPES = [(2, 16, 32), (1, 8, 16)]


def _c2f(what, p, dev, judge=True):
    from defectdetection_viaobjectdetection_amd import _capi
    x = p["x"]
    B, _, H, W = x.shape
    a = _np(p["w"])
    xd, xp = _banded_input(x, dev)

    def run(yp):
        return _capi.lib.m355_c2f_c32_fwd(C.c_void_p(xp), B, H, W, _h(a[0]), _h(a[1]), _h(a[2]), _h(a[3]), _h(a[4]), _h(a[5]),
                                          int(p["shortcut"]), C.c_void_p(yp), _stream())
    if judge:
        return _judge(what, run, (B, 64, H, W), p["y64"], p["tol"], dev)
    raw, body = _guarded_output(B * H * W * 64 * 2, torch.float16, dev)
    _accepted(run(body.data_ptr()), what)
    return _nhwc(_guards_intact(raw, what), B, H, W, 64)


@pytest.mark.parametrize("tap", fp.TAPS, ids=_tid)
@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("B,H,W", C2F_SHAPES)
def test_c2f_c32_probe(cuda_device, B, H, W, kind, tap):
    """Each of the three stages in turn random and judged, the other two selectors (fused_probe.c2f_probe)."""
    _c2f(f"c2f_c32 {kind} {_tid(tap)} {(B, H, W)}", fp.c2f_probe(kind, B, H, W, tap, seed=B * 1000 + H), cuda_device)


@pytest.mark.parametrize("B,H,W", C2F_SHAPES)
def test_c2f_c32_pass_through_channels(cuda_device, B, H, W):
    """wc selects [y0, y1]: the pass-through channels arrive unchanged, fp16(SiLU(x)) bit for bit, whatever the two 3x3 stages do."""
    _c2f(f"c2f_c32 pass {(B, H, W)}", fp.c2f_probe("pass", B, H, W, (1, 1), seed=B * 1000 + H), cuda_device)


@pytest.mark.parametrize("B,H,W", C2F_SHAPES)
def test_c2f_c32_hot_border_old_assertions(cuda_device, B, H, W):
    from test_c2f_fused_gpu import _ref
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = fp.hot_x(g, (B, 64, H, W))
    w = (fp.rand_w(g, 32, 32, 3), fp.rand_b(g, 32), fp.rand_w(g, 32, 32, 3), fp.rand_b(g, 32), fp.rand_w(g, 64, 96, 1), fp.rand_b(g, 64))
    got = _c2f(f"c2f_c32 hot {(B, H, W)}", dict(x=x, w=w, shortcut=True), cuda_device, judge=False)
    want = _ref(x, *w, True)
    rel, worst = cb.rel_l2(got, want), float((got - want.half().float()).abs().max())
    print(f"PROBE c2f_c32 hot border {(B, H, W)}: rel-L2 {rel:.2e}, max |d| vs the fp16-rounded reference {worst:.2e}")
    assert bool(torch.isfinite(got).all()) and rel <= 1e-3 and worst <= 2e-2


# ---- m355_s2c64_cv1_fwd
S2C64_SHAPES = [(2, 32, 48), (1, 16, 16)]


def _s2c64(what, p, dev, judge=True):
    from defectdetection_viaobjectdetection_amd import _capi
    x = p["x"]
    B, _, H, W = x.shape
    a = _np(p["w"])
    xd, xp = _banded_input(x, dev)

    def run(yp):
        return _capi.lib.m355_s2c64_cv1_fwd(C.c_void_p(xp), B, H, W, _h(a[0]), _h(a[1]), _h(a[2]), _h(a[3]), C.c_void_p(yp), _stream())
    if judge:
        return _judge(what, run, (B, 128, H // 2, W // 2), p["y64"], p["tol"], dev)
    raw, body = _guarded_output(B * (H // 2) * (W // 2) * 128 * 2, torch.float16, dev)
    _accepted(run(body.data_ptr()), what)
    return _nhwc(_guards_intact(raw, what), B, H // 2, W // 2, 128)


@pytest.mark.parametrize("taps", TAP_PAIRS, ids=_tid)
@pytest.mark.parametrize("B,H,W", S2C64_SHAPES)
def test_s2c64_cv1_exact_hidden(cuda_device, B, H, W, taps):
    _s2c64(f"s2c64_cv1 exact {_tid(taps)} {(B, H, W)}", fp.s2c64_probe("exact", B, H, W, taps, seed=H + B), cuda_device)


@pytest.mark.parametrize("B,H,W", S2C64_SHAPES)
def test_s2c64_cv1_transparent_tail(cuda_device, B, H, W):
    _s2c64(f"s2c64_cv1 tail {(B, H, W)}", fp.s2c64_probe("tail", B, H, W, None, seed=H + B), cuda_device)


@pytest.mark.parametrize("B,H,W", S2C64_SHAPES)
def test_s2c64_cv1_hot_border_old_assertions(cuda_device, B, H, W):
    g = torch.Generator().manual_seed(H + B)
    x = fp.hot_x(g, (B, 64, H, W))
    w = (fp.rand_w(g, 128, 64, 3), fp.rand_b(g, 128), fp.rand_w(g, 128, 128, 1), fp.rand_b(g, 128))
    got = _s2c64(f"s2c64_cv1 hot {(B, H, W)}", dict(x=x, w=w), cuda_device, judge=False)
    t = F.silu(F.conv2d(x, w[0], w[1], stride=2, padding=1)).half().float()
    want = F.silu(F.conv2d(t, w[2], w[3]))
    rel = cb.rel_l2(got, want)
    print(f"PROBE s2c64_cv1 hot border {(B, H, W)}: rel-L2 {rel:.2e}")
    assert bool(torch.isfinite(got).all()) and rel <= 1e-3


# ---- m355_stem_s2c32_cv1_fwd, both forms
def _stem(what, p, two_team, dev):
    from defectdetection_viaobjectdetection_amd import _capi
    img = p["x"]
    B, H, W, _ = img.shape
    a = _np(p["w"])
    band = 32768
    buf = torch.full((img.numel() + 2 * band,), 255, dtype=torch.uint8)
    buf[band:band + img.numel()] = img.reshape(-1)
    xd = buf.to(dev)

    def run(yp):
        return _capi.lib.m355_stem_s2c32_cv1_fwd(C.c_void_p(xd.data_ptr() + band), B, H, W, _h(a[0]), _h(a[1]), _h(a[2]), _h(a[3]), _h(a[4]),
                                                 _h(a[5]), C.c_void_p(yp), two_team, _stream())
    _judge(what, run, (B, 64, H // 4, W // 4), p["y64"], p["tol"], dev)


@pytest.mark.parametrize("two_team", [1, 0])
@pytest.mark.parametrize("taps", TAP_PAIRS, ids=_tid)
def test_stem_probe_stage0_through_selectors(cuda_device, taps, two_team):
    """(a) w1 the stride-2 selector, w2 the identity, w0 random: stage 0 and its zero padding judged through two SiLUs."""
    _stem(f"stem two_team={two_team} a {_tid(taps)} (2, 64, 128)", fp.stem_probe("a", 2, 64, 128, taps, seed=64 + two_team), two_team, cuda_device)


@pytest.mark.parametrize("two_team", [1, 0])
def test_stem_probe_weak_two_random_stages(cuda_device, two_team):
    """(b) WEAK: w0 and w1 random, w2 the identity.  Stage 0's bound is carried through the random 3x3 stage in L1 (fused_probe.weak_stage),
    so the tolerance (its median is printed) is an order of magnitude looser than an fp16 ulp of the output: this probe sees a wrong or
    missing element of stage 1, not a hidden value off by a few ulp."""
    _stem(f"stem two_team={two_team} b WEAK (2, 64, 128)", fp.stem_probe("b", 2, 64, 128, None, seed=64 + two_team), two_team, cuda_device)


# ---- m355_proto_phase_fwd
@pytest.mark.parametrize("with_bt", [False, True], ids=["bt0", "bt"])
@pytest.mark.parametrize("quarter", [0, 1, 2, 3])
@pytest.mark.parametrize("B,H,W", [(3, 16, 32), (1, 8, 16)])
def test_proto_phase_probe(cuda_device, B, H, W, quarter, with_bt):
    """wt the identity (nearest-neighbour upsampling), wc selects 32 of the 128 hidden channels: every element of the hidden SiLU(cv2)
    tile judged, borders included; with_bt: the ConvTranspose bias through the zero-padded 3x3 (the border classes of the bias table)."""
    from defectdetection_viaobjectdetection_amd import _capi
    p = fp.proto_probe(B, H, W, quarter, with_bt, seed=W + quarter)
    a = _np(p["w"])
    xd, xp = _banded_input(p["x"], cuda_device)

    def run(yp):
        return _capi.lib.m355_proto_phase_fwd(C.c_void_p(xp), B, H, W, _h(a[0]), _h(a[1]), _h(a[2]), _h(a[3]), _h(a[4]), _h(a[5]),
                                              C.c_void_p(yp), _stream())
    _judge(f"proto_phase q{quarter} {'bt' if with_bt else 'bt0'} {(B, H, W)}", run, (B, 32, 2 * H, 2 * W), p["y64"], p["tol"], cuda_device,
           rel_bound=1.5e-3)
