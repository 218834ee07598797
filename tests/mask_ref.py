"""CPU restatement (fp64) of the letterboxed mask assembly (upstream ``process_mask``, the oracle's ``process_mask``), written
from the semantics, for the host test and the per-pixel GPU comparison of ``m355_proto_masks``; and the inputs both use.

One detection with coefficients c (32), prototypes P (mh, mw, 32), network input (in_h, in_w) = (4 mh, 4 mw) and box
(x1, y1, x2, y2) in input pixels:
  1. cell logit L = P @ c, scale S = |P| @ |c| (the size of the rounding a fp32 / split-fp16 evaluation may make);
  2. the box is scaled to the prototype grid in float32: x * (mw / in_w), y * (mh / in_h) -- the factor is exactly 0.25, so the
     product is exact; a cell (y, x) is kept iff x1 <= x < x2 and y1 <= y < y2, every other cell is zeroed BEFORE the upsample;
  3. bilinear interpolation to (in_h, in_w), align_corners=False: source coordinate (Y + 0.5) / 4 - 0.5 clamped at 0, upper
     neighbour clamped to the last row / column (``native_mask_ref.src_axis``: the one place that rule lives), applied alike
     to L and S;
  4. mask = v > 0.
A pixel with S == 0 lies outside the upsampled support of the kept cells and must be exactly 0.  Elsewhere a fp32 evaluation
may differ from this one only where |v| <= rel * S (``compare``, the rule of ``native_mask_ref.compare_native``), rel = 2^-16:
32 fp32 products per cell, two MFMAs and three lerps round to a few 2^-24 each, 32 * 2^-24 = 2^-19 in all, times 8 headroom.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from native_mask_ref import src_axis

REL = 2.0 ** -16


def kept_cells(boxes: np.ndarray, mh: int, mw: int, in_hw: Tuple[int, int]) -> np.ndarray:
    """bool (n, mh, mw): the cells each box keeps."""
    in_h, in_w = in_hw
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    wr, hr = np.float32(mw / in_w), np.float32(mh / in_h)
    x1, y1, x2, y2 = b[:, 0] * wr, b[:, 1] * hr, b[:, 2] * wr, b[:, 3] * hr
    x = np.arange(mw, dtype=np.float32)[None, None, :]
    y = np.arange(mh, dtype=np.float32)[None, :, None]
    return ((x >= x1[:, None, None]) & (x < x2[:, None, None]) & (y >= y1[:, None, None]) & (y < y2[:, None, None]))


def upsample(m: np.ndarray, out_hw: Tuple[int, int]) -> np.ndarray:
    """(n, mh, mw) fp64 -> (n, H, W): bilinear, align_corners=False, clamped indices."""
    H, W = out_hw
    y0, y1, fy = src_axis(H, m.shape[1])
    x0, x1, fx = src_axis(W, m.shape[2])
    rows = (1 - fy)[None, :, None] * m[:, y0] + fy[None, :, None] * m[:, y1]
    return (1 - fx)[None, None, :] * rows[:, :, x0] + fx[None, None, :] * rows[:, :, x1]


def process_mask_ref(coefs: np.ndarray, protos: np.ndarray, boxes: np.ndarray, in_hw: Tuple[int, int]):
    """coefs (n, 32), protos (mh, mw, 32) (both taken as fp64), boxes (n, 4) in input pixels.  Returns (masks uint8
    (n, in_h, in_w), v, S): v the fp64 interpolated logit and S the same interpolation of sum_k |c_k P_k|."""
    mh, mw, nm = protos.shape
    n = len(coefs)
    if n == 0:
        z = np.zeros((0,) + tuple(in_hw))
        return z.astype(np.uint8), z, z
    P = protos.astype(np.float64).reshape(mh * mw, nm)
    c = np.asarray(coefs, np.float64)
    keep = kept_cells(boxes, mh, mw, in_hw)
    L = (c @ P.T).reshape(n, mh, mw) * keep
    S = (np.abs(c) @ np.abs(P).T).reshape(n, mh, mw) * keep
    v, s = upsample(L, in_hw), upsample(S, in_hw)
    return (v > 0).astype(np.uint8), v, s


def band(v: np.ndarray, S: np.ndarray, rel: float = REL):
    """(pixels with S > 0, those of them inside the margin band |v| <= rel * S): a property of the inputs alone."""
    sup = S > 0
    return int(sup.sum()), int((sup & (np.abs(v) <= rel * S)).sum())


def compare(got: np.ndarray, ref: np.ndarray, v: np.ndarray, S: np.ndarray, rel: float = REL):
    """Returns (number of differing pixels, worst |v| / S over the differing pixels with S > 0, pixels with S == 0 that
    are not 0).  The caller asserts worst <= rel and unsupported == 0."""
    assert got.shape == ref.shape == v.shape == S.shape, (got.shape, ref.shape, v.shape, S.shape)
    sup = S > 0
    unsupported = int(np.count_nonzero(got[~sup]))
    d = (got != ref) & sup
    worst = float((np.abs(v[d]) / S[d]).max()) if d.any() else 0.0
    return int((got != ref).sum()), worst, unsupported


# ----------------------------------------------------------------------------------------------- inputs of the edge tests
# (in_h, in_w): the smallest inputs that reach every tile case of the kernel's 8 x 32-cell tile.  (80, 160) -> 20 x 40 cells:
# 2 tiles in x, the last 8 columns wide, 3 in y, the last 4 rows high; (96, 272) -> 24 x 68: 3 in x, the last 4 columns wide,
# y exact.  Both have the tile seams x = 128 px (cells 31 | 32) and y = 32 px (cell rows 7 | 8).
SHAPES = [(80, 160), (96, 272)]
# (counts per image, max_det): the early return, one partial chunk of 16, exactly one, one + 1, several, the clamp of
# counts[b] to max_det; the last pair holds every crafted box in image 0 and four whole chunks in image 1.
COUNT_CASES = [((0, 1), 300), ((15, 16), 300), ((17, 40), 300), ((20, 33), 20), ((23, 64), 300)]
# "mixed": random boxes reaching 10 % beyond the image, interleaved with the crafted ones; "full": every box covers the whole
# image (and more), so that every detection touches every tile and the chunks of 16 are exactly what the counts say.
KINDS = ["mixed", "full"]


def crafted_boxes(in_h: int, in_w: int) -> np.ndarray:
    """Boxes (x1, y1, x2, y2) in input pixels at the kernel's edges; cells are 4 px, the seams x = 128 and y = 32."""
    return np.asarray([
        (0, 0, in_w, in_h),                        # the whole image
        (8, 12, 100, 60),                          # edges at multiples of 4 px: cells 2..24 x 3..14
        (128, 32, in_w - 4, in_h - 8),             # first edges on the seams
        (20, 8, 128, 32),                          # last edges on the seams
        (127, 31, 150, 70), (129, 33, 150, 70),    # first edges one pixel to either side of the seams
        (20, 8, 127, 31), (20, 8, 129, 33),        # last edges one pixel to either side
        (41, 21, 43, 23),                          # inside one cell, between cell indices: keeps nothing
        (39, 19, 42, 22),                          # keeps the single cell (5, 10)
        (125, 10, 129, 70),                        # one cell wide right of the x seam: column 32
        (123, 10, 127, 70),                        # one cell wide left of it: column 31, whose support crosses the seam
        (10, 29, 100, 33),                         # one cell high below the y seam: row 8
        (10, 27, 100, 31),                         # row 7
        (50, 10, 50, 40), (60, 10, 40, 40),        # x2 <= x1
        (20, 40, 90, 40),                          # y2 <= y1
        (-30, -20, -2, -1),                        # wholly at negative coordinates
        (in_w + 1, 10, in_w + 30, 40),             # wholly beyond in_w
        (10, in_h + 2, 60, in_h + 20),             # wholly beyond in_h
        (-5, -5, 9, 9), (in_w - 9, in_h - 9, in_w + 5, in_h + 5),   # over the corners
        (0, 0, 4, 4),                              # the first cell alone
    ], np.float32)


def edge_case(shape: Tuple[int, int], counts: Sequence[int], max_det: int, kind: str, seed: int):
    """Inputs of one case: protos fp16 (B, mh, mw, 32), dets f32 (B, max_det, 38) with every slot filled (boxes in columns
    0..3, coefficients 0.5 N(0, 1) in 6..37 -- the slots at and past counts[b] hold boxes and coefficients too, which the
    kernel must not use), n = min(counts, max_det) per image."""
    in_h, in_w = shape
    mh, mw = in_h // 4, in_w // 4
    B = len(counts)
    rng = np.random.default_rng(seed)
    protos = rng.standard_normal((B, mh, mw, 32)).astype(np.float16)
    dets = np.zeros((B, max_det, 38), np.float32)
    dets[..., 6:] = (rng.standard_normal((B, max_det, 32)) * 0.5).astype(np.float32)
    dets[..., 4] = rng.uniform(0.25, 1.0, (B, max_det))
    x = np.sort(rng.uniform(-0.1 * in_w, 1.1 * in_w, (B, max_det, 2)), -1)
    y = np.sort(rng.uniform(-0.1 * in_h, 1.1 * in_h, (B, max_det, 2)), -1)
    if kind == "full":
        x = np.stack((rng.uniform(-0.1 * in_w, 0, (B, max_det)), rng.uniform(in_w, 1.1 * in_w, (B, max_det))), -1)
        y = np.stack((rng.uniform(-0.1 * in_h, 0, (B, max_det)), rng.uniform(in_h, 1.1 * in_h, (B, max_det))), -1)
    dets[..., 0], dets[..., 2] = x[..., 0], x[..., 1]
    dets[..., 1], dets[..., 3] = y[..., 0], y[..., 1]
    n = [min(int(c), max_det) for c in counts]
    if kind == "mixed":
        cb = crafted_boxes(in_h, in_w)
        for b in range(B):
            if n[b] >= len(cb):            # room for all of them: every other slot until they are used up
                slots = [s for s in range(0, n[b], 2)][:len(cb)]
                slots += [s for s in range(1, n[b], 2)][:len(cb) - len(slots)]
                order = np.arange(len(cb))
            else:                          # as many as there are slots, a different stretch of the list per image and seed
                slots = list(range(0, n[b], 2)) if n[b] > 1 else list(range(n[b]))
                order = (np.arange(len(cb)) + 7 * b + 11 * seed) % len(cb)
            for s, k in zip(slots, order):
                dets[b, s, :4] = cb[k]
    return protos, dets, n
