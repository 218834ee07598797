"""The per-element conv checker (tests/conv_bound.py) passes a correct implementation and fails subtly wrong ones.  CPU only.

Correct implementation: F.conv2d in fp32 of the fp16-rounded operands, the epilogue in fp32, one rounding to fp16.
Mutants, each on its own, each at every shape where it exists (the residual one needs a residual, the batch one B >= 2):
  tap       one (ky, kx) tap dropped for one output channel at the corner pixel (0, 0) of image 0
  k_tail    the last 32 input channels dropped for the last output channel only
  swap      two neighbouring pixels of one row swapped (all channels, image 0)
  bias      the bias missing on the last output channel
  res_left  the residual read from the pixel to the left
  batch     one image computed from the previous image's input

The old whole-tensor bound (rel-L2 <= 1e-3) is printed for every mutant and shape, with the shapes at which it would have let the
mutant through.  Measured here: it lets `tap` through at (2,8,160,64,64) and (2,16,160,32,32) (rel-L2 2.1e-4 and 5.0e-4, where a
correct result has 2.1e-4 from the fp16 rounding alone) -- a defect of ONE element in 163 840 that is 10 x and 126 x its element
bound -- and that is asserted.  For the other five mutants no shape of the narrow-map lists can
show it, by arithmetic: rel-L2 of a defect is about (rms error of the touched elements) * sqrt(touched / all) / (rms of y), the largest
case has 163 840 elements, and these mutants move at least 2 elements by O(1) (2 / sqrt(163 840) = 4.9e-3) or a whole channel / image.
The old bound does catch them here; what the new bound adds for them is the index of the element and a margin of orders of magnitude
(the printed worst ratios) instead of a factor 5-50 over a whole-tensor threshold.  Their rel-L2 is printed, not asserted.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_bound as cb

SHAPES = [
    # B, H, W, cin, cout, k, act, residual     (from the case lists of tests/test_narrow_maps_gpu.py)
    (2, 1, 20, 256, 256, 3, 1, True),
    (2, 2, 2, 128, 64, 3, 1, False),
    (2, 4, 20, 256, 224, 3, 0, False),
    (3, 1, 20, 384, 256, 1, 1, False),
    (2, 8, 160, 64, 64, 3, 1, True),
    (2, 16, 160, 32, 32, 3, 1, True),
]
MUTANTS = ("tap", "k_tail", "swap", "bias", "res_left", "batch")


def _epilogue(z, act, res):
    y = F.silu(z) if act else z
    if res is not None:
        y = y + res
    return y.half().float()


def _implementation(x, w, b, k, act, res, mutant=None):
    """fp32 conv + epilogue, rounded to fp16; `mutant` plants one defect.  Returns None where the mutant does not exist."""
    pad = k // 2
    B, cin, H, W = x.shape
    cout = w.shape[0]
    z = F.conv2d(x, w, b, padding=pad)
    if mutant == "tap":
        ky, kx = (min(H - 1, 1) + pad, min(W - 1, 1) + pad) if k == 3 else (0, 0)     # a tap that lies inside the map
        iy, ix = ky - pad, kx - pad
        z[0, cout - 1, 0, 0] -= (x[0, :, iy, ix] * w[cout - 1, :, ky, kx]).sum()
    elif mutant == "k_tail":
        if cin < 64:
            return None
        z[:, cout - 1] -= F.conv2d(x[:, cin - 32:], w[cout - 1:, cin - 32:], None, padding=pad)[:, 0]
    elif mutant == "bias":
        z[:, cout - 1] -= b[cout - 1]
    elif mutant == "batch":
        if B < 2:
            return None
        z[B - 1] = z[B - 2]
        y = _epilogue(z, act, res)
        return y
    elif mutant == "res_left":
        if res is None:
            return None
        res = torch.cat((res[..., :1], res[..., :-1]), -1)
    y = _epilogue(z, act, res)
    if mutant == "swap":
        if W < 2:
            return None
        c = W // 2
        y[0, :, H - 1, [c - 1, c]] = y[0, :, H - 1, [c, c - 1]]
    return y


@pytest.fixture(scope="module")
def cases():
    out = []
    for shp in SHAPES:
        B, H, W, cin, cout, k, act, use_res = shp
        x, w, b, res = cb.draw_operands(shp, B, H, W, cin, cout, k, use_res)
        y64, z64, S = cb.conv_ref(x, w, b, k, 1, act, res)
        tol = cb.conv_tol(y64, z64, S, cin * k * k, act, res)
        out.append((shp, (x, w, b, res), y64, tol))
    return out


def test_correct_implementation_passes(cases):
    for shp, (x, w, b, res), y64, tol in cases:
        got = _implementation(x, w, b, shp[5], shp[6], res)
        worst, idx, _ = cb.check_elements(got, y64, tol, str(shp))
        print(f"{shp}: correct implementation, worst |err|/tol {worst:.3f} at {idx}, rel-L2 {cb.rel_l2(got, y64):.2e}")
        assert cb.rel_l2(got, y64) <= 1e-3


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_fails_the_element_bound(cases, mutant):
    through, ran = [], 0
    for shp, (x, w, b, res), y64, tol in cases:
        got = _implementation(x, w, b, shp[5], shp[6], res, mutant)
        if got is None:
            continue
        ran += 1
        worst, idx, bad = cb.worst_ratio(got, y64, tol)
        rel = cb.rel_l2(got, y64)
        if rel <= 1e-3:
            through.append(shp)
        print(f"{mutant} {shp}: {bad} elements beyond the bound, worst |err|/tol {worst:.3g} at (image, channel, row, col) = {idx}; "
              f"rel-L2 {rel:.2e} ({'PASSES' if rel <= 1e-3 else 'fails'} the old 1e-3 bound)")
        assert bad > 0 and worst > 1.0, f"{mutant} at {shp} slipped through the element bound"
        with pytest.raises(AssertionError):
            cb.check_elements(got, y64, tol, f"{mutant} {shp}")
    print(f"{mutant}: the old rel-L2 bound lets it through at {through if through else 'none of these shapes'}")
    assert ran >= 2
    if mutant == "tap":
        assert through, "a one-element defect in 163 840 must pass the whole-tensor bound (module docstring)"


def test_fp32_output_bound():
    """out_f32: nothing is rounded to fp16, so the bound is the accumulation term alone and a bias off by one fp16 ulp of the
    output fails it."""
    shp = (2, 1, 20, 128, 65, 1, 0, False)
    x, w, b, _ = cb.draw_operands(shp, 2, 1, 20, 128, 65, 1, False)
    y64, z64, S = cb.conv_ref(x, w, b, 1, 1, 0, None)
    tol = cb.conv_tol(y64, z64, S, 128, 0, None, out_f32=True)
    got = F.conv2d(x, w, b)
    worst, idx, _ = cb.check_elements(got, y64, tol, "fp32 out")
    print(f"fp32 output: worst |err|/tol {worst:.3f} at {idx}")
    assert cb.worst_ratio(got.half().float(), y64, tol)[2] > 0      # an fp16-rounded result is not an fp32 one
