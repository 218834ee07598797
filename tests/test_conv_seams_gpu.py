"""Every forced conv tile id of m355_conv2d_fwd, and its dispatcher, on the smallest shapes that still cross every boundary inside one
launch: at least two tiles along rows and columns with a partial last tile, two channel tiles with a ragged last one where the kernel
has channel tiles, and the K-pipeline depth named beside the shape.  Each shape is a few thousand pixels.

Every case is judged on the common path of tests/conv_harness.py (input and residual between NaN bands, output NaN-filled between byte
bands, every element against the float64 reference with conv_bound's derived bound, rel-L2, a second launch for identical bits) and
runs twice: as drawn, and with "hot seams" -- the same operands with x multiplied by 4 on the two rows and two columns either side of
every tile boundary (the hot border of tests/test_dwconv_gpu.py moved to the seams), so that a neighbour fetched from the wrong side of
a seam moves the result by far more than the bound.

This file lists only shapes its tile accepts: a refusal fails.  Where a forced id refuses a shape of the starting list, the comment
beside the replacement names the predicate clause.  The persistent kernels' second tile per block needs more tiles than the grid has
blocks; the workload-sized cases of tests/test_ops_gpu.py and tests/test_bneck_pair_gpu.py do that, per element too.
"""
import pytest
import torch

import conv_harness as ch

pytestmark = pytest.mark.gpu


def _c(B, H, W, cin, cout, k=3, s=1, act=1, res=False):
    return (B, H, W, cin, cout, k, s, act, res, False)


# implicit GEMM (ids 0, 1, 5: linear pixel tiles of 128; 2, 3: of 256)
IGEMM = [
    _c(2, 17, 23, 64, 160, s=2),             # odd map, 216 output pixels = 1.7 tiles of 128, channel tiles 128 + 32 (64 + 64 + 32)
    _c(1, 19, 21, 96, 200, k=1),             # K = 96, not a multiple of 64; 399 pixels; 200 = 128 + 72
    _c(2, 13, 15, 48, 48, res=True),         # 390 pixels, K = 432 = 6.75 steps of 64
    _c(3, 11, 13, 16, 16),                   # 429 pixels, K = 144
]
# (2, 17, 23, s2) is a single partial tile of 256 pixels: one image more makes it 324 = 1.3 tiles for ids 2 and 3
IGEMM256 = IGEMM + [_c(3, 17, 23, 64, 160, s=2)]
# halo kernels (16: by shape, 17: 16 x 16 pixels, 18: 8 x 16).  conv3x3_halo_ok refuses (1, 40, 24, 128, 224): its 8 x 16 tiling covers
# 40 x 32 = 1280 pixels of 960, beyond the clause `covered * 10 <= Hi * Wi * 13`.  The nearest map that keeps 2.5 x 1.6 tiles of
# 16 x 16 and is ragged for the 8-row tiles too: 39 x 26 (1280 <= 1.3 x 1014).
HALO = [
    _c(1, 39, 26, 128, 224, res=True),       # two chunks, ragged channel tile (224 = 128 + 96)
    _c(2, 24, 40, 192, 64, act=0),           # three chunks (odd count), 1.5 x 2.5 tiles
]
WIDE = [                                     # 19: 128 channels x 16 x 16 pixels, 32-deep K steps
    _c(1, 48, 40, 128, 224, res=True),       # 3 x 2.5 tiles, four K steps, ragged channel tile
    _c(2, 29, 32, 64, 128),                  # 1.8 x 2 tiles, two K steps
]
C32 = [                                      # 20: Cin = Cout = 32, 16 x 16 tiles
    _c(2, 40, 24, 32, 32, res=True),
    _c(1, 17, 33, 32, 32, act=0),
]
SLAB = [                                     # 25: full-width row slabs, W <= 26
    _c(3, 20, 20, 128, 96, res=True),        # two slabs of 10 rows, two channel tiles with the second half full
    _c(2, 13, 7, 64, 72),                    # slabs of 10 + 3 rows, 72 = 64 + 8
]
# v_mfma_f32_32x32x16_f16 halo kernel (26: by shape, 27: 128 ch x 8 rows, 28: 64 ch x 16 rows, 29: 64 ch x 8 rows).  It shares
# conv3x3_halo_ok, which refuses (2, 40, 24, 64, 72) by the same waste clause as above: 39 x 26 instead.
M32 = [
    _c(1, 24, 40, 128, 224, res=True),       # two chunks (both patch buffers), 224 = 128 + 96 = 3 x 64 + 32
    _c(2, 39, 26, 64, 72, res=True),         # one chunk, ragged tiles in both directions, 72 = 64 + 8
    _c(1, 15, 30, 192, 64),                  # three chunks: the unpaired tail
]
W1 = [                                       # 32: 1x1 with the weights in registers, K in 128 .. 512, Cout % 128 == 0
    _c(3, 10, 13, 192, 128, k=1),            # 390 pixels = 3.05 tiles of 128, the last almost empty
    _c(1, 10, 10, 384, 256, k=1),            # 100 pixels = 1.6 tiles of 64
    _c(5, 9, 9, 512, 512, k=1),              # 405 pixels = 6.3 tiles of 64, two channel tiles of 256
]
PLANES = [                                   # 33: row slabs of equal height, 64-channel tiles
    _c(1, 13, 17, 128, 192, res=True),       # one ragged slab, three channel tiles
    _c(2, 16, 40, 128, 256, s=2),            # the parity sub-planes of a stride-2 input, four channel tiles
    _c(2, 20, 20, 256, 64),                  # two slabs of 10 rows, eight input planes
]

SEAM_CASES = {0: IGEMM, 1: IGEMM, 2: IGEMM256, 3: IGEMM256, 5: IGEMM, 16: HALO, 17: HALO, 18: HALO, 19: WIDE, 20: C32, 25: SLAB,
              26: M32, 27: M32, 28: M32, 29: M32, 32: W1, 33: PLANES}
SEAM_CASES[-1] = list(dict.fromkeys(c for t in sorted(SEAM_CASES) for c in SEAM_CASES[t]))     # the dispatcher takes every one

_GRID = {17: (16, 16), 18: (8, 16), 19: (16, 16), 20: (16, 16), 27: (8, 16), 28: (16, 16), 29: (8, 16),
         # by shape: 8- or 16-row tiles of 16 columns; every 16-row boundary is an 8-row boundary
         16: (8, 16), 26: (8, 16)}
_LINEAR = {0: 128, 1: 128, 2: 256, 3: 256, 5: 128}


def seam_geometry(tile, case):
    """Where the tile boundaries of one launch lie, in output pixels: ("grid", rows, cols), ("rows", R) or ("linear", pixels); from
    conv_forced_tile_extent and the launchers (conv_pick_tile, slab_rows, planes_geometry, launch_w1)."""
    B, H, W, cin, cout, k, s = case[:7]
    Ho, Wo = ch.out_hw(H, W, k, s)
    if tile in _GRID:
        return ("grid",) + _GRID[tile]
    if tile in _LINEAR:
        return ("linear", _LINEAR[tile])
    if tile == -1:                                               # conv_pick_tile: 128-pixel tiles above 32 channels, else 32 x 256
        return ("linear", 128 if cout > 32 else 256)
    if tile == 25:                                               # slab_rows
        return ("rows", min(256 // W, 10, H))
    if tile == 32:                                               # eight channel blocks run 64-pixel tiles, four 128
        return ("linear", 64 if cout % 256 == 0 else 128)
    if tile == 33:                                               # planes_geometry: R (Wo + 1) <= 256, then equal slabs
        R = min(256 // (Wo + 1), Ho)
        nslab = -(-Ho // R)
        return ("rows", -(-Ho // nslab))
    raise KeyError(tile)


def hot_mask(tile, case):
    """(B, 1, H, W) bool: the input pixels on the two rows and two columns either side of every tile boundary of seam_geometry
    (output boundary o = input row / column o * stride)."""
    B, H, W, cin, cout, k, s = case[:7]
    Ho, Wo = ch.out_hw(H, W, k, s)
    m = torch.zeros(B, 1, H, W, dtype=torch.bool)

    def rows(b, o):
        m[b, :, max(0, o * s - 2):o * s + 2, :] = True

    def cols(b, o):
        m[b, :, :, max(0, o * s - 2):o * s + 2] = True

    geom = seam_geometry(tile, case)
    if geom[0] == "linear":
        for p in range(geom[1], B * Ho * Wo, geom[1]):
            b, rem = divmod(p, Ho * Wo)
            rows(b, rem // Wo)
            cols(b, rem % Wo)
    else:
        for o in range(geom[1], Ho, geom[1]):
            rows(slice(None), o)
        if geom[0] == "grid":
            for o in range(geom[2], Wo, geom[2]):
                cols(slice(None), o)
    return m


def seam_operands(tile, case, hot):
    """Operands and float64 reference of a seam case: the plain draw is shared by every tile id, the hot one by every id with the same
    geometry."""
    if not hot:
        return ch.reference(case)
    return ch.reference(case, hot=(seam_geometry(tile, case), hot_mask(tile, case)))


@pytest.mark.parametrize("tile", sorted(SEAM_CASES))
def test_conv_seams(tile, cuda_device):
    from defectdetection_viaobjectdetection_amd import _capi as capi
    assert len(SEAM_CASES[tile]) >= 2
    failures, worst_all = [], 0.0
    for case in SEAM_CASES[tile]:
        for hot in (False, True):
            what = f"tile {tile} {case}{' hot seams' if hot else ''}"
            try:
                worst, _, _ = ch.judge(capi, case, tile, seam_operands(tile, case, hot), cuda_device, what)
                worst_all = max(worst_all, worst)
            except ch.NotLaunched as e:
                if not e.refused:
                    raise                                        # a runtime error: nothing more is launched
                failures.append(f"{e} (this file lists only shapes its tile accepts)")
                break
            except AssertionError as e:
                failures.append(str(e))
    print(f"tile {tile}: {len(SEAM_CASES[tile])} seam shapes, plain and hot: worst |err|/tol {worst_all:.3f}")
    assert not failures, "\n".join(failures)
