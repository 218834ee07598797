"""The conv kernels and the fused entries on the narrow and tiny maps that predict() reaches on long, thin B-scans (net shapes such
as 64 x 640, 32 x 640, 32 x 32: pyramid maps of 8 x 80 down to 1 x 20 and 1 x 1), through the per-op C-ABI entries.

Every accepted conv case is judged element by element (tests/conv_bound.py: float64 reference of the fp16-rounded operands, a
derived bound per element), keeps the whole-tensor rel-L2 bound of 1e-3, and is run twice for identical bits.  The output sits in
a NaN-filled buffer between guard bands whose bytes must stay untouched; the input and the residual sit between NaN guard bands
too, so a read outside them poisons the output.

A forced tile may refuse a shape: m355_conv2d_fwd then returns M355_ERR_INVALID and m355_last_error() reads "conv launch failed:
-1" (the launcher's -1).  A refusal is recorded and printed and the case is skipped; any other nonzero rc fails the test; every
tile id must accept at least one of its shapes, and the dispatcher (tile -1) must accept every one."""
import pytest
import torch

import conv_bound as cb
from conv_harness import ERR_INVALID, REFUSED_TEXT, banded_input as _banded_input, launch as _launch, reference as _reference

pytestmark = pytest.mark.gpu

def _c(B, H, W, cin, cout, k=3, s=1, act=1, res=False, f32=False):
    return (B, H, W, cin, cout, k, s, act, res, f32)


S1 = [  # 3x3 stride 1
    _c(2, 1, 20, 256, 256, res=True),        # one row: no tap above or below
    _c(2, 20, 1, 256, 256),                  # one column
    _c(3, 1, 1, 64, 64),                     # one pixel: the centre tap alone
    _c(2, 2, 2, 128, 64),                    # every pixel a corner
    _c(2, 4, 20, 256, 224, act=0),           # the fused head-level convs of a 32 x 160 net shape; ragged channel tile
    _c(2, 2, 40, 128, 128),
    _c(2, 8, 160, 64, 64, res=True),         # one tile row of the 8-row tiles, ten tile columns
    _c(2, 8, 160, 128, 128),
    _c(2, 16, 160, 32, 32, res=True),
    _c(2, 1, 1, 512, 512),
]
S2 = [  # 3x3 stride 2
    _c(1, 2, 2, 64, 128, s=2),               # a 1 x 1 output
    _c(2, 2, 40, 128, 256, s=2),
    _c(2, 40, 2, 256, 512, s=2),
    _c(2, 4, 80, 64, 128, s=2),
    _c(1, 17, 3, 64, 128, s=2),              # odd sizes on a 3-wide map
]
P1 = [  # 1x1
    _c(1, 1, 1, 256, 256, k=1),
    _c(3, 1, 20, 384, 256, k=1),
    _c(2, 2, 2, 96, 64, k=1),
    _c(2, 1, 20, 128, 1, k=1, act=0, f32=True),
    _c(2, 1, 20, 128, 65, k=1, f32=True),
]
EVERY = S1 + S2 + P1
HALO_IDS = (16, 17, 18, 19, 26, 27, 28, 29)
TILE_CASES = {-1: EVERY}
TILE_CASES.update({t: EVERY for t in (0, 1, 2, 3, 5)})
TILE_CASES.update({t: S1 for t in HALO_IDS})
# The wide kernel (19) needs Cin % 64 == 0, Cout >= 128 and 16-row tiles that waste at most 30 %: it refuses every map of S1 (measured:
# ten refusals; 8 x 160 covers 16 x 160 = 2 x the map).  The narrowest maps its predicate takes: one row of 16-row tiles, full and
# ragged (13 rows: 16 x 160 <= 1.3 x 13 x 160).
TILE_CASES[19] = S1 + [_c(2, 16, 160, 128, 128, res=True), _c(2, 13, 160, 64, 128)]
TILE_CASES[20] = [_c(2, 16, 160, 32, 32, res=True), _c(3, 16, 16, 32, 32)]
TILE_CASES[25] = [c for c in S1 if c[2] <= 26]
TILE_CASES[32] = [_c(2, 1, 20, 256, 256, k=1), _c(1, 1, 1, 128, 128, k=1), _c(2, 4, 80, 256, 128, k=1)]
# The row-slab kernel (33) always runs its 256 (128-channel stride-2 form: 224) pixels per block and refuses a slab that fills less than
# 60 % of them: R x (Wo + 1) >= 154 storage columns.  It refuses all eight maps of the first two rows (measured).  The last row is the
# narrowest maps the rule takes, by its arithmetic: 8 x 20 (8 x 21 = 168), a 2-wide column of 64 rows (64 x 3 = 192), and the same
# two as stride-2 outputs.
TILE_CASES[33] = [_c(2, 2, 20, 256, 256), _c(2, 4, 20, 256, 64), _c(2, 20, 2, 256, 256), _c(2, 1, 20, 256, 256),
                  _c(2, 8, 40, 128, 256, s=2), _c(2, 4, 40, 256, 512, s=2), _c(2, 40, 4, 128, 128, s=2), _c(2, 2, 2, 64, 128, s=2),
                  _c(2, 8, 20, 256, 256, res=True), _c(2, 64, 2, 64, 64), _c(2, 16, 40, 128, 256, s=2), _c(1, 128, 4, 64, 128, s=2)]

@pytest.mark.parametrize("tile", sorted(TILE_CASES))
def test_conv_on_narrow_maps(tile, cuda_device):
    from defectdetection_viaobjectdetection_amd import _capi as capi
    accepted, refused, failures = [], [], []
    for case in TILE_CASES[tile]:
        x, w, b, res, y64, tol = _reference(case)
        xd, xp = _banded_input(x, cuda_device)
        rd, rp = _banded_input(res, cuda_device) if res is not None else (None, 0)
        rc, got = _launch(capi, case, tile, xp, rp, w, b, y64.shape, cuda_device)
        if rc != 0:
            text = (capi.lib.m355_last_error(None) or b"").decode()
            assert rc == ERR_INVALID and text == REFUSED_TEXT, f"tile {tile} {case}: rc {rc} is no refusal: {text!r}"
            refused.append(case)
            print(f"tile {tile} {case}: refused")
            continue
        accepted.append(case)
        worst, idx, bad = cb.worst_ratio(got, y64, tol)
        rel = cb.rel_l2(got, y64)
        print(f"tile {tile} {case}: accepted, worst |err|/tol {worst:.3f} at (image, channel, row, col) = {idx}, rel-L2 {rel:.2e}")
        try:
            assert bool(torch.isfinite(got).all()), "non-finite output (an element not written, or a read outside the input)"
            cb.check_elements(got, y64, tol, f"tile {tile} {case}")
            assert rel <= 1e-3, f"rel-L2 {rel}"
            rc2, got2 = _launch(capi, case, tile, xp, rp, w, b, y64.shape, cuda_device)
            assert rc2 == 0 and torch.equal(got.contiguous().view(torch.int32 if case[9] else torch.int16),
                                            got2.contiguous().view(torch.int32 if case[9] else torch.int16)), "two runs differ"
        except AssertionError as e:
            failures.append(f"tile {tile} {case}: {e}")
    print(f"tile {tile}: accepted {len(accepted)}, refused {len(refused)}: {refused}")
    assert not failures, "\n".join(failures)
    assert accepted, f"tile {tile} accepted none of its shapes: the list tests nothing"
    if tile == -1:
        assert not refused, f"the dispatcher refused {refused}"


# ---- the fused entries, each through the reference of its own test module (imported, not copied)
def _raises_refusal(fn, *args):
    from defectdetection_viaobjectdetection_amd import _capi
    with pytest.raises(_capi.M355Error, match=r"error -1:"):
        fn(*args)


@pytest.mark.parametrize("B,H,W", [(2, 16, 160), (1, 16, 16)])
def test_s2c64_cv1_narrow(cuda_device, B, H, W):
    from test_fused_ops_gpu import test_s2c64_cv1_against_torch as ref_test
    ref_test(cuda_device, B, H, W)


@pytest.mark.parametrize("two_team", [1, 0])
@pytest.mark.parametrize("B,H,W", [(2, 32, 640), (3, 32, 64)])
def test_stem_launch_narrow(cuda_device, B, H, W, two_team):
    from test_fused_ops_gpu import test_stem_launch_against_torch as ref_test
    ref_test(cuda_device, B, H, W, two_team)


@pytest.mark.parametrize("B,H,W", [(2, 8, 80), (1, 8, 16)])
def test_proto_phase_narrow(cuda_device, B, H, W):
    from test_fused_ops_gpu import test_proto_phase_launch_against_torch as ref_test
    ref_test(cuda_device, B, H, W)


@pytest.mark.parametrize("B,H,W,nc,stride", [(2, 4, 80, 3, 8.0), (3, 2, 16, 1, 16.0),     # 320 and 32 pixels: the 32-pixel boundary
                                             (2, 1, 32, 20, 32.0)])
def test_head_tail_narrow_accepted(cuda_device, B, H, W, nc, stride):
    from test_fused_ops_gpu import test_head_tail_against_torch as ref_test
    ref_test(cuda_device, B, H, W, nc, stride)


def test_head_tail_refuses_a_level_below_32_pixels(cuda_device):
    from test_fused_ops_gpu import test_head_tail_against_torch as ref_test
    _raises_refusal(ref_test, cuda_device, 2, 1, 20, 1, 32.0)


def _accept_or_refuse(what, fn, *args):
    """Runs an existing test body; M355_ERR_INVALID (a refusal) is printed and accepted, everything else is the body's verdict."""
    from defectdetection_viaobjectdetection_amd import _capi
    try:
        fn(*args)
        print(f"{what}: accepted")
    except _capi.M355Error as e:
        assert "error -1:" in str(e), str(e)
        print(f"{what}: refused ({e})")


@pytest.mark.parametrize("B,H,W,Cc", [(2, 4, 40, 128), (2, 2, 20, 128)])
def test_bneck_pair_narrow(cuda_device, B, H, W, Cc):
    from test_bneck_pair_gpu import test_bneck_pair_against_torch as ref_test
    _accept_or_refuse(f"bneck_pair {(B, H, W, Cc)}", ref_test, cuda_device, B, H, W, Cc, True, None)


@pytest.mark.parametrize("B,H,W", [(2, 4, 40), (2, 2, 20), (2, 1, 20)])
def test_blockdiag_narrow(cuda_device, B, H, W):
    from test_planes_blockdiag_gpu import test_blockdiag_against_torch_and_the_three_launches as ref_test
    ref_test(cuda_device, B, H, W, 0)         # (block-diagonal mode takes any fill of its pixel blocks: no refusal)


@pytest.mark.parametrize("B,H,W", [(2, 16, 160), (2, 8, 16)])
def test_c2f_c32_narrow(cuda_device, B, H, W):
    from test_c2f_fused_gpu import test_c2f_c32_against_torch as ref_test
    ref_test(cuda_device, B, H, W, True)
