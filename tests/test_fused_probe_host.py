"""The selector probes of tests/fused_probe.py pass an honest fused launch and flag the faults a fused kernel makes.  CPU only.

The launch is emulated in torch fp32 with the documented rounding points (fp16 operands, fp32 sums, the hidden tensor rounded to fp16
where the kernel keeps it in LDS, the output rounded once), for a bneck-pair-shaped problem (two images, C = 64, 23 x 51, slabs of 5 rows) and a
c2f-shaped one (two images of 16 x 48: 2 x 3 tiles of 8 x 16).

  * The honest emulation has ZERO elements beyond its bound in every probe (a condition of the probes, not a measurement).
  * Every seeded fault is flagged (check_elements fails) by at least one named probe.  The faults, each at two extents:
      ring      the padding ring of the hidden tensor computed (SiLU(bias + partial window)) where it should be zero
      stale     hidden row r of one 32-channel block replaced by row r + 1, at a slab (tile) seam of image 0
      swap      two hidden channels of the last 32-channel block swapped
      nores     the residual (shortcut) missing at one pixel
      ulp8      one output element off by 8 fp16 ulp
    `ring`, `stale` and `swap` exist whole (every element of the ring / row / channel pair) and as `*_one` (ONE hidden element of it).
  * rel-L2 is about (rms error of the touched outputs) * sqrt(touched / all) / rms(y).  ONE wrong hidden element of size ~0.2 moves the
    9 C outputs of its window by ~0.01 each, one output 8 ulp off moves one: at these sizes (150 000 and 98 000 outputs) that is a few
    1e-4, below the 1e-3 that the whole-tensor assertion allows.  So for `ring_one`, `stale_one`, `swap_one` and `ulp8` the test asserts
    that at least one probe flags the fault in a run whose own rel-L2 stays <= 1e-3: the old assertion alone would have passed that
    very output.  The whole ring, row or channel pair touches hundreds of hidden elements, and a missing residual moves C outputs by ~0.8
    each (0.8 * 8 / (0.85 * sqrt(150 000)) = 2e-2): no whole-tensor 1e-3 can pass those at these sizes, by that arithmetic; they are
    asserted as flagged and their rel-L2 is printed (the probes add the element index and margins of 10^2 .. 10^4 over the bound).
    What the old test's own i.i.d. operands give for each fault (rel-L2 of the faulty against the honest output) is printed too.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_bound as cb
import fused_probe as fp

ONE = ("ring_one", "stale_one", "swap_one", "ulp8")          # faults that a probe must flag in a run that passes rel-L2 <= 1e-3
FAULTS = ("ring", "stale", "swap", "nores") + ONE
SEAM = {"bneck": 4, "c2f": 7}                                # the last row of the first slab / tile


def _r16(t):
    return t.half().float()


def _hidden(x, wa, ba, fault, seam):
    """The zero-padded hidden tensor (B, C, H + 2, W + 2) = fp16(SiLU(conv3x3(x; wa) + ba)) with one of the hidden-tensor faults."""
    C, H, W = wa.shape[0], x.shape[2], x.shape[3]
    tp = F.pad(_r16(F.silu(F.conv2d(x, wa, ba, padding=1))), (1, 1, 1, 1))
    if fault in ("ring", "ring_one"):
        full = _r16(F.silu(F.conv2d(F.pad(x, (2, 2, 2, 2)), wa, ba)))          # the hidden tensor computed one pixel beyond the map
        if fault == "ring":
            full[:, :, 1:H + 1, 1:W + 1] = tp[:, :, 1:H + 1, 1:W + 1]
            tp = full
        else:                                                # one element of the halo row below the map: that of median magnitude
            row = full[0, :, H + 1, 1:W + 1]
            flat = int(row.abs().flatten().argsort()[row.numel() // 2])
            c, j = flat // W, flat % W
            tp[0, c, H + 1, j + 1] = row[c, j]
    elif fault == "stale":
        tp[0, C - 32:, seam + 1, :] = tp[0, C - 32:, seam + 2, :].clone()
    elif fault == "stale_one":
        tp[0, C - 3, seam + 1, 6] = tp[0, C - 3, seam + 2, 6]
    elif fault == "swap":
        tp[:, [C - 1, C - 2]] = tp[:, [C - 2, C - 1]]
    elif fault == "swap_one":
        tp[0, [C - 1, C - 2], 6, 9] = tp[0, [C - 2, C - 1], 6, 9]
    return tp


def _ulp8(y):
    flat = y.view(-1)
    i = int(((flat.abs() >= 0.5) & (flat.abs() < 1.0)).nonzero()[7])           # an element with ulp 2^-11 ... 2^-10
    flat[i] += 8 * 2.0 ** -11 * (2.0 if abs(float(flat[i])) >= 1.0 else 1.0)
    return y


def bneck_emul(x, w, shortcut, fault=None):
    wa, ba, wb, bb = w
    tp = _hidden(x, wa, ba, fault, SEAM["bneck"])
    y = F.silu(F.conv2d(tp, wb, bb))
    if shortcut:
        res = x.clone()
        if fault == "nores":
            res[0, :, 6, 9] = 0
        y = y + res
    y = _r16(y)
    return _ulp8(y) if fault == "ulp8" else y


def c2f_emul(x, w, shortcut, fault=None):
    wa, ba, wb, bb, wc, bc = w
    y1 = x[:, 32:]
    tp = _hidden(y1, wa, ba, fault, SEAM["c2f"])
    y2 = F.silu(F.conv2d(tp, wb, bb))
    if shortcut:
        res = y1.clone()
        if fault == "nores":
            res[0, :, 6, 9] = 0
        y2 = y2 + res
    y = _r16(F.silu(F.conv2d(torch.cat((x, _r16(y2)), 1), wc, bc)))
    return _ulp8(y) if fault == "ulp8" else y


def _random_ops(kind, gen):
    """The i.i.d. operands of the old tests (test_bneck_pair_gpu.py, test_c2f_fused_gpu.py)."""
    rw = lambda co, ci, k: _r16(torch.randn((co, ci, k, k), generator=gen) * (2.0 / (k * k * ci)) ** 0.5)
    rb = lambda n: torch.randn(n, generator=gen) * 0.3
    if kind == "bneck":
        x = _r16(torch.randn((2, 64, 23, 51), generator=gen) * 0.8)
        return x, (rw(64, 64, 3), rb(64), rw(64, 64, 3), rb(64))
    x = _r16(torch.randn((2, 64, 16, 48), generator=gen) * 0.8)
    return x, (rw(32, 32, 3), rb(32), rw(32, 32, 3), rb(32), rw(64, 96, 1), rb(64))


def _probes(kind):
    """(name, operands x, weights, shortcut, y64, tol) of every probe of a launch."""
    out = []
    if kind == "bneck":
        for which in ("exact", "tail"):
            for tap in fp.TAPS:
                p = fp.bneck_probe(which, 2, 23, 51, 64, tap, True, seed=11)
                out.append((f"bneck {which} tap {tap}", p["x"], p["w"], True, p["y64"], p["tol"]))
    else:
        for which in ("a", "b", "c"):
            for tap in fp.TAPS:
                p = fp.c2f_probe(which, 2, 16, 48, tap, seed=12)
                out.append((f"c2f {which} tap {tap}", p["x"], p["w"], p["shortcut"], p["y64"], p["tol"]))
        p = fp.c2f_probe("pass", 2, 16, 48, (1, 1), seed=12)
        out.append(("c2f pass", p["x"], p["w"], p["shortcut"], p["y64"], p["tol"]))
    return out


EMUL = {"bneck": bneck_emul, "c2f": c2f_emul}


@pytest.fixture(scope="module", params=["bneck", "c2f"])
def launch(request):
    return request.param, _probes(request.param)


def test_honest_emulation_has_no_element_out_of_bound(launch):
    kind, probes = launch
    for name, x, w, shortcut, y64, tol in probes:
        got = EMUL[kind](x, w, shortcut)
        worst, idx, bad, med = fp.summary(got, y64, tol)
        print(f"{name}: honest worst |err|/tol {worst:.3f} at {idx}, median tol {med:.2e}, rel-L2 {cb.rel_l2(got, y64):.2e}")
        cb.check_elements(got, y64, tol, name)
        assert cb.rel_l2(got, y64) <= 1e-3


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_fault_is_flagged(launch, fault):
    kind, probes = launch
    x, w = _random_ops(kind, torch.Generator().manual_seed(5))
    old = cb.rel_l2(EMUL[kind](x, w, True, fault), EMUL[kind](x, w, True))
    print(f"{kind} {fault}: the old test (i.i.d. operands, whole-tensor rel-L2) sees {old:.2e}: {'PASSES' if old <= 1e-3 else 'fails'} 1e-3")
    flagged = []
    for name, px, pw, shortcut, y64, tol in probes:
        got = EMUL[kind](px, pw, shortcut, fault)
        worst, idx, bad, _ = fp.summary(got, y64, tol)
        rel = cb.rel_l2(got, y64)
        if bad:
            flagged.append((name, rel))
            with pytest.raises(AssertionError):
                cb.check_elements(got, y64, tol, name)
        print(f"{kind} {fault} under {name}: {bad} elements beyond the bound, worst |err|/tol {worst:.3g} at {idx}, rel-L2 {rel:.2e}")
    assert flagged, f"{fault} slipped through every probe of {kind}"
    if fault in ONE:
        quiet = [n for n, rel in flagged if rel <= 1e-3]
        assert quiet, f"{fault}: no probe flags it while its own rel-L2 stays below 1e-3: {flagged}"


def test_the_other_launches_honest_emulation():
    """s2c64_cv1, the stem and proto_phase, emulated honestly in fp32 at their smallest shapes: zero elements beyond the bound."""
    for kind, taps in (("exact", ((0, 0), (2, 2))), ("exact", ((0, 2), (1, 1))), ("tail", None)):
        p = fp.s2c64_probe(kind, 1, 16, 16, taps, seed=3)
        w3, b3, w1, b1 = p["w"]
        got = _r16(F.silu(F.conv2d(_r16(F.silu(F.conv2d(p["x"], w3, b3, stride=2, padding=1))), w1, b1)))
        worst, idx, _ = cb.check_elements(got, p["y64"], p["tol"], f"s2c64 {kind} {taps}")
        print(f"s2c64_cv1 {kind} {taps}: honest worst |err|/tol {worst:.3f}, median tol {float(p['tol'].median()):.2e}")
    for kind, taps in (("a", ((0, 0), (2, 2))), ("a", ((0, 2), (1, 1))), ("b", None)):
        p = fp.stem_probe(kind, 1, 32, 64, taps, seed=4)
        w0, b0, w1, b1, w2, b2 = p["w"]
        x = p["x"].permute(0, 3, 1, 2).float()
        t0 = _r16(F.silu(F.conv2d(x, w0, None, stride=2, padding=1) * (1.0 / 255.0) + b0.view(1, -1, 1, 1)))
        got = _r16(F.silu(F.conv2d(_r16(F.silu(F.conv2d(t0, w1, b1, stride=2, padding=1))), w2, b2)))
        worst, idx, _ = cb.check_elements(got, p["y64"], p["tol"], f"stem {kind} {taps}")
        print(f"stem {kind} {taps}: honest worst |err|/tol {worst:.3f}, median tol {float(p['tol'].median()):.2e}{' (WEAK)' if kind == 'b' else ''}")
    for with_bt in (False, True):
        p = fp.proto_probe(1, 8, 16, 2, with_bt, seed=6)
        wt, bt, w3, b3, wc, bc = p["w"]
        weff = fp.proto_phase_weights(wt, w3).float()
        bmap = F.conv2d(bt.view(1, -1, 1, 1).expand(1, 128, 16, 32), w3, b3, padding=1)
        z = _r16(F.silu(fp.proto_phase_conv(p["x"], weff.double()).float() + bmap))
        got = _r16(F.silu(F.conv2d(z, wc, bc)))
        worst, idx, _ = cb.check_elements(got, p["y64"], p["tol"], f"proto bt={with_bt}")
        print(f"proto_phase bt={with_bt}: honest worst |err|/tol {worst:.3f}, median tol {float(p['tol'].median()):.2e}")


def test_proto_phase_composition_equals_upsample_then_conv():
    """The four composed 2x2 phase convs (unrounded, float64, ANY ConvTranspose weight) are ConvTranspose2d(2x2, s2) then Conv3x3, to
    float64 rounding: the reference's phase indexing is right independently of the kernel."""
    g = torch.Generator().manual_seed(1)
    n, H, W = 8, 5, 7
    x, wt, w3 = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((2, n, H, W), (n, n, 2, 2), (n, n, 3, 3)))
    want = F.conv2d(F.conv_transpose2d(x, wt, None, stride=2), w3, None, padding=1)
    got = fp.proto_phase_conv(x, fp.proto_phase_weights(wt, w3, rounded=False))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_safe_values():
    v, h = fp.silu_safe_values()
    frac = fp.safe_fraction()
    print(f"{v.numel()} safe values, {frac:.1%} of the fp16 values in [-6, 6]; depth 2: {fp.silu_safe_values(2)[0].numel()}")
    assert frac >= 0.8
    assert torch.equal(F.silu(v.float()).half().double(), h)                   # fp32 F.silu agrees with the table on all of it
    assert bool((v[1:] > v[:-1]).all()) and float(v.abs().max()) <= 6.0
    assert bool(((h.abs() >= 2.0 ** -14) | (v == 0)).all())                    # no subnormal hidden value
    v2, h2 = fp.silu_safe_values(2)
    assert torch.equal(fp.silu_exact(h2.float()), fp.silu_exact(fp.silu_exact(v2.float()).float()))
    g = torch.Generator().manual_seed(0)
    x = fp.draw_safe((2, 3, 7, 9), g, hot_border=True)
    assert torch.equal(x, x.half().float()) and float(x[:, :, 0].abs().mean()) > 2 * float(x[:, :, 3].abs().mean())
    fp.silu_exact(x)                                                           # every drawn value is in the table


def test_selectors():
    w = fp.delta3x3(128, 64, ((0, 0), (2, 2)))
    assert float(w.sum()) == 128 and w[3, 3, 0, 0] == 1 and w[67, 3, 2, 2] == 1
    s = fp.select1x1(64, 96, 64)
    assert float(s.sum()) == 64 and s[0, 64, 0, 0] == 1 and s[33, 65, 0, 0] == 1
    t = torch.arange(12.0).view(1, 1, 3, 4) + 1
    sh = fp.select(t, fp.delta3x3(1, 1, (0, 0)))                               # out[p] = t[p + (-1, -1)], zero outside
    assert torch.equal(sh[0, 0, 1:, 1:], t[0, 0, :2, :3].double()) and float(sh[0, 0, 0].abs().sum()) == 0
