"""The per-element bounds the conv-family GPU tests apply, checked on the CPU at the shapes those tests use.  No device is touched: the
case lists are imported from the GPU test modules.

Reference within bound: a plain fp32 CPU implementation (F.conv2d / conv2d_input rounded once to fp16, conv2d_weight and the fp32-output
head kept in fp32) passes the bound at every seam shape, plain and with hot seams, and at the heaviest shapes of the forward, dgrad and
wgrad lists -- so a GPU failure at one of them is the kernel's, not the bound's.  The worst ratios are printed.

The gap closed: defects that the old whole-tensor bound (rel-L2 <= 1e-3) lets through and the element bound catches.
  seam     ONE output element next to a tile boundary takes the value of its neighbour across the boundary -- on one workload-sized
           shape per family, with that family's boundary (16 x 16 grid tiles: the halo / 32x32x16 and wide kernels; linear
           128-pixel tiles: the implicit GEMM and the dispatcher; row slabs: the slab kernel and tile 33; linear 64-pixel tiles: the 1x1
           weights-in-registers kernel) and on the heaviest dgrad shape (the 64-column chunks of conv_dgrad_s2c32).  The channel is the
           one whose two values differ by the median amount: a defect of ordinary size.
  product  ONE product dropped from ONE wgrad element, at a pixel on a tile / chunk boundary -- on the seam shape of each wgrad kernel.
           The dropped product is the one of its boundary column nearest the rms magnitude 1: launch_ref.elem_bound promises to see a
           product of at least half the average magnitude beyond its c S slack, and has the 2^-10 |ref| rounding term on top.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_bound as cb
import conv_harness as ch
import launch_ref as lr
from test_backward_ops_gpu import DGRAD_CASES, WGRAD_CASES
from test_bneck_pair_gpu import SINGLE_CASES
from test_conv_seams_gpu import SEAM_CASES, hot_mask, seam_geometry, seam_operands
from test_ops_gpu import CONV_CASES, CONVT_SHAPES

# the three heaviest forward cases, and the largest case of the families they do not cover (wide, row slabs of tile 33).  The largest
# Cin = Cout = 32 case, (1, 160, 160, 32, 32), has 819 200 elements: one median-sized seam defect alone is rel-L2 1.08e-3 there (measured),
# which the old bound does catch; its 16 x 16 grid boundary is the wide kernel's.
_HEAVY = {((6, 160, 160, 64, 64), 26), ((300, 20, 20, 64, 64), 25), ((24, 40, 40, 512, 256), 32), ((1, 160, 160, 128, 128), 19)}
HEAVY_FWD = [c for c in CONV_CASES if (c[:5], c[9]) in _HEAVY] + [c[:5] + (3, 1, 1, c[5], 33) for c in SINGLE_CASES if c[0] == 40]
HEAVY_DGRAD = (9, 320, 320, 32, 64, 3, 2)
HEAVY_WGRAD = (4, 320, 512, 8, 32, 3, 2)
DGRAD_SEAMS = [(1, 8, 64, 32, 64, 3, 2), (1, 6, 192, 32, 64, 3, 2)]
WGRAD_SEAMS = [(2, 23, 45, 48, 96, 3, 1), (2, 17, 33, 48, 96, 3, 1), (1, 16, 128, 8, 48, 3, 2), (1, 8, 160, 32, 64, 3, 2)]


def _fp32_conv(case, ops):
    """The correct implementation: fp32 conv and epilogue, one rounding to fp16 (none for fp32 output)."""
    B, H, W, cin, cout, k, s, act, use_res, f32 = case
    x, w, b, res = ops[:4]
    z = F.conv2d(x, w, b, stride=s, padding=k // 2)
    y = F.silu(z) if act else z
    if res is not None:
        y = y + res
    return y if f32 else y.half().float()


@pytest.fixture(scope="module")
def heavy():
    """The heavy forward cases: (the test's case, the harness case, operands + float64 reference, the fp32 implementation's output)."""
    out = []
    for c in HEAVY_FWD:
        c10 = c[:9] + (False,)
        ops = ch.reference(c10, key=c, keep=False)
        out.append((c, c10, ops, _fp32_conv(c10, ops)))
    return out


def test_the_lists_hold_what_the_files_say():
    assert len(HEAVY_FWD) == 5 and HEAVY_DGRAD in DGRAD_CASES and HEAVY_WGRAD in WGRAD_CASES
    assert all(c in DGRAD_CASES for c in DGRAD_SEAMS) and all(c in WGRAD_CASES for c in WGRAD_SEAMS)
    assert sorted(SEAM_CASES) == [-1, 0, 1, 2, 3, 5, 16, 17, 18, 19, 20, 25, 26, 27, 28, 29, 32, 33]
    for tile, cases in SEAM_CASES.items():
        assert len(cases) >= 2, tile
        if tile != -1:
            assert all(c in SEAM_CASES[-1] for c in cases), tile
        n_seamed = sum(bool(hot_mask(tile, c).any()) for c in cases)
        assert n_seamed >= 1 and (n_seamed >= 2 or tile == 33), f"tile {tile}: {n_seamed} shapes with a boundary inside"
        for c in cases:                                         # a hot seam is a proper part of the map, not all of it
            assert not bool(hot_mask(tile, c).all()), (tile, c)


def test_fp32_forward_within_the_bound_at_every_seam_shape():
    worst_all, seen = 0.0, set()
    for tile in sorted(SEAM_CASES):
        for case in SEAM_CASES[tile]:
            for hot in (False, True):
                key = (case, seam_geometry(tile, case) if hot else None)
                if key in seen:
                    continue
                seen.add(key)
                ops = seam_operands(tile, case, hot)
                worst, idx, _ = cb.check_elements(_fp32_conv(case, ops), ops[4], ops[5], f"{case} hot={hot}")
                worst_all = max(worst_all, worst)
    print(f"{len(seen)} seam references: worst |err|/tol of the fp32 implementation {worst_all:.3f}")
    assert worst_all <= 1.0


def test_fp32_forward_within_the_bound_at_the_heaviest_shapes(heavy):
    for c, c10, ops, got in heavy:
        worst, idx, _ = cb.check_elements(got, ops[4], ops[5], str(c))
        print(f"{c}: fp32 implementation, worst |err|/tol {worst:.3f} at {idx}, rel-L2 {cb.rel_l2(got, ops[4]):.2e}")
        assert worst <= 1.0


def test_fp32_head_and_convt_within_their_bounds():
    for cout in (1, 3, 64, 65):                                   # test_conv2d_f32_out_small_cout
        g = torch.Generator().manual_seed(cout)
        x = torch.randn(2, 128, 20, 20, generator=g).half().float()
        w = (torch.randn(cout, 128, 1, 1, generator=g) / 128 ** 0.5).half().float()
        b = torch.randn(cout, generator=g)
        y64, z64, S = cb.conv_ref(x, w, b, 1, 1, 0, None)
        worst, _, _ = cb.check_elements(F.conv2d(x, w, b), y64, cb.conv_tol(y64, z64, S, 128, 0, None, out_f32=True), f"fp32 out {cout}")
        print(f"fp32 output, cout {cout}: worst |err|/tol {worst:.3f}")
    for shape in CONVT_SHAPES:                                    # test_convt2x2
        B, H, W, cin, cout = shape
        g = torch.Generator().manual_seed(5)
        x = torch.randn(B, cin, H, W, generator=g).half()
        w = (torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5).half()
        b = torch.randn(cout, generator=g) * 0.1
        got = F.conv_transpose2d(x.float(), w.float(), b, stride=2).half().permute(0, 2, 3, 1)
        x64 = x.double().permute(0, 2, 3, 1)
        ref = lr.convt_ref(x64, w.double()) + b.double()
        S = lr.convt_ref(x64.abs(), w.double().abs()) + b.double().abs()
        ratio, rel, desc = lr.check_elementwise(got, ref, lr.elem_bound(ref, S, cin))
        print(f"convt {shape}: worst |err|/bound {ratio:.3f}; {desc}")
        assert ratio <= 1.0


def _dgrad_draw(case):
    """The draw of test_conv2d_dgrad: (w, dY (B, cout, Ho, Wo)), both fp16-rounded."""
    B, H, W, cin, cout, k, s = case
    g = torch.Generator().manual_seed(sum(case))
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half().float()
    torch.randn(B, cin, H, W, generator=g)
    Ho, Wo = ch.out_hw(H, W, k, s)
    return w, torch.randn(B, cout, Ho, Wo, generator=g).half().float()


def _dgrad_case(case):
    """(float64 reference NHWC, bound, the fp32 implementation rounded to fp16) of a dgrad case."""
    from test_backward_ops_gpu import _dgrad_reference
    B, H, W, cin, cout, k, s = case
    w, dy = _dgrad_draw(case)
    ref, bound = _dgrad_reference(dy, w, H, W, s)
    got = torch.nn.grad.conv2d_input((B, cin, H, W), w, dy, s, k // 2).half().permute(0, 2, 3, 1)
    return ref, bound, got


@pytest.fixture(scope="module")
def heavy_dgrad():
    return _dgrad_case(HEAVY_DGRAD)


def test_fp32_dgrad_within_the_bound(heavy_dgrad):
    for case in DGRAD_SEAMS + [HEAVY_DGRAD]:
        ref, bound, got = heavy_dgrad if case == HEAVY_DGRAD else _dgrad_case(case)
        ratio, rel, desc = lr.check_elementwise(got, ref, bound)
        print(f"dgrad {case}: fp32 implementation, worst |err|/bound {ratio:.3f}, rel-L2 {rel:.2e}")
        assert ratio <= 1.0, desc


def _wgrad_case(case):
    """The draw of test_conv2d_wgrad: (x, dY NHWC fp16-rounded, float64 reference KRSC, S, K)."""
    B, H, W, cin, cout, k, s = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    x = torch.randn(B, cin, H, W, generator=g).half().float()
    torch.randn(cout, cin, k, k, generator=g)
    Ho, Wo = ch.out_hw(H, W, k, s)
    dy = torch.randn(B, cout, Ho, Wo, generator=g).half().float()
    xn, dn = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    ref, S = lr.wgrad_reference(xn.double(), dn.double(), k, s, k // 2, cout)
    return xn, dn, ref, S, B * Ho * Wo


def _wgrad_fp32(xn, dn, case):
    B, H, W, cin, cout, k, s = case
    return lr.wgrad_reference(xn, dn, k, s, k // 2, cout)[0]


def test_fp32_wgrad_within_the_bound():
    for case in WGRAD_SEAMS + [HEAVY_WGRAD]:
        xn, dn, ref, S, K = _wgrad_case(case)
        B, H, W, cin, cout, k, s = case
        got = torch.nn.grad.conv2d_weight(xn.permute(0, 3, 1, 2), (cout, cin, k, k), dn.permute(0, 3, 1, 2), s, k // 2).permute(0, 2, 3, 1)
        ratio, rel, desc = lr.check_elementwise(got, ref, lr.elem_bound(ref, S, K))
        print(f"wgrad {case}: fp32 implementation, K = {K}, worst |err|/bound {ratio:.3f}, rel-L2 {rel:.2e}")
        assert ratio <= 1.0, desc


# ---- the gap closed
def _median_channel(a, b):
    """The channel (last axis of two vectors) whose |a - b| is the median: a defect of ordinary size, never zero by accident."""
    d = (a.double() - b.double()).abs()
    return int(d.argsort()[d.numel() // 2])


def _seam_pair(geom, Ho, Wo):
    """Two output pixels (image 0) either side of the first boundary of a geometry, as (row, col) pairs."""
    if geom[0] == "linear":
        p = geom[1]
        return divmod(p - 1, Wo), divmod(p, Wo)
    return (geom[1] - 1, Wo // 2), (geom[1], Wo // 2)


def test_one_seam_element_passes_rel_l2_and_fails_the_element_bound(heavy, heavy_dgrad):
    ran = 0
    for c, c10, ops, good in heavy:
        y64, tol = ops[4], ops[5]
        Ho, Wo = y64.shape[2:]
        tiles = [17, 0] if c[9] == 26 else [c[9]]                    # the grid and the linear family both take the 64-channel 160 x 160 case
        for tile in tiles:
            (r0, c0), (r1, c1) = _seam_pair(seam_geometry(tile, c10), Ho, Wo)
            chn = _median_channel(good[0, :, r0, c0], good[0, :, r1, c1])
            got = good.clone()
            got[0, chn, r0, c0] = good[0, chn, r1, c1]
            worst, idx, bad = cb.worst_ratio(got, y64, tol)
            rel = cb.rel_l2(got, y64)
            print(f"seam mutant, {c[:5]} with the boundary of tile {tile}: element {(0, chn, r0, c0)} <- {(0, chn, r1, c1)}: rel-L2 {rel:.2e} "
                  f"(correct: {cb.rel_l2(good, y64):.2e}), {bad} element beyond the bound, worst |err|/tol {worst:.3g} at {idx}")
            assert rel <= 1e-3, "the old bound was expected to let this through"
            assert bad == 1 and idx == (0, chn, r0, c0) and worst > 1.0
            ran += 1
    ref, bound, good = heavy_dgrad                                   # NHWC; a chunk of 32 dY pixels is 64 dX columns
    chn = _median_channel(good[0, 10, 63], good[0, 10, 64])
    got = good.clone()
    got[0, 10, 63, chn] = good[0, 10, 64, chn]
    ratio, rel, desc = lr.check_elementwise(got, ref, bound)
    print(f"seam mutant, dgrad {HEAVY_DGRAD}: rel-L2 {rel:.2e}, worst |err|/bound {ratio:.3g}; {desc}")
    assert rel <= 1e-3 and ratio > 1.0 and lr.rel_l2(good, ref) <= 1e-3
    assert ran == 6


@pytest.mark.parametrize("case,ow", [((2, 23, 45, 48, 96, 3, 1), 16),      # patch kernel: the first column of the second 16-wide tile
                                     ((1, 16, 128, 8, 48, 3, 2), 0),       # stem kernel: the first pixel of every row's 64-pixel chunk
                                     ((1, 8, 160, 32, 64, 3, 2), 64)])     # wgrad_s2c32: the first pixel of the partial last chunk
def test_one_dropped_product_passes_rel_l2_and_fails_the_element_bound(case, ow):
    B, H, W, cin, cout, k, s = case
    xn, dn, ref, S, K = _wgrad_case(case)
    good = _wgrad_fp32(xn, dn, case)
    co, ci = cout - 1, cin - 1
    prod = dn[0, :, ow, co] * xn[0, 0:s * dn.shape[1]:s, ow * s, ci]      # the centre tap (1, 1) reads x at (oh * s, ow * s)
    oh = int((prod.abs() - 1.0).abs().argmin())                           # an ordinary product: the rms of x dY is 1
    got = good.clone()
    got[co, 1, 1, ci] -= prod[oh]
    bound = lr.elem_bound(ref, S, K)
    ratio, rel, desc = lr.check_elementwise(got, ref, bound)
    ratio0, rel0, _ = lr.check_elementwise(good, ref, bound)
    print(f"product mutant, wgrad {case}: dY(0, {oh}, {ow}, {co}) x(0, {oh * s}, {ow * s}, {ci}) = {float(prod[oh]):.3f} of K = {K} dropped: "
          f"rel-L2 {rel:.2e} (correct: {rel0:.2e}), worst |err|/bound {ratio:.3g} (correct: {ratio0:.3g}); {desc}")
    assert ratio0 <= 1.0 and rel <= 1e-3, "the old bound was expected to let this through"
    assert ratio > 1.0 and desc.startswith(f"worst at ({co}, 1, 1, {ci})")
