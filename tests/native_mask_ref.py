"""CPU restatement (fp64) of predict(retina_masks=True) and of predict's ``classes`` filter, written from the semantics in
DESIGN.md section 14, for the host tests and the GPU comparisons.

Native masks (upstream ``process_mask_native``), one detection with coefficients c (32), prototypes P (mh, mw, 32), original
shape (h0, w0) and box (x1, y1, x2, y2) in original pixels:
  1. gain = min(mh / h0, mw / w0), pw = (mw - w0 gain) / 2, ph = (mh - h0 gain) / 2; crop the prototype grid to rows
     [int(ph), int(mh - ph)) and columns [int(pw), int(mw - pw)) (``crop``: the one place this rule lives here);
  2. logit = sum_k c_k P[.., k];
  3. bilinear interpolation to (h0, w0), align_corners=False: source coordinate (y + 0.5) ch / h0 - 0.5 clamped at 0, upper
     neighbour clamped to the last row / column (computed exactly: ((2y + 1) ch - h0) / (2 h0));
  4. pixel (r, q) kept iff x1 <= q < x2 and y1 <= r < y2;
  5. uint8(logit > 0).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def crop(mh: int, mw: int, h0: int, w0: int) -> Tuple[int, int, int, int]:
    """(top, bottom, left, right) of the prototype crop: rows [top, bottom), columns [left, right)."""
    gain = min(mh / h0, mw / w0)
    pw, ph = (mw - w0 * gain) / 2, (mh - h0 * gain) / 2
    return int(ph), int(mh - ph), int(pw), int(mw - pw)


def src_axis(o: int, c: int):
    """Per output index 0..o-1 along an axis of c cells: (lower cell, upper cell, weight of the upper cell)."""
    n = np.maximum((2 * np.arange(o, dtype=np.int64) + 1) * c - o, 0)
    i0 = n // (2 * o)
    f = (n - i0 * 2 * o).astype(np.float64) / (2 * o)
    return i0, np.minimum(i0 + 1, c - 1), f


def _interp(L: np.ndarray, rows: np.ndarray, cols: np.ndarray, h0: int, w0: int) -> np.ndarray:
    ch, cw = L.shape
    y0, y1, fy = (a[rows] for a in src_axis(h0, ch))
    x0, x1, fx = (a[cols] for a in src_axis(w0, cw))
    fy, fx = fy[:, None], fx[None, :]
    top = (1 - fx) * L[y0][:, x0] + fx * L[y0][:, x1]
    bot = (1 - fx) * L[y1][:, x0] + fx * L[y1][:, x1]
    return (1 - fy) * top + fy * bot


def box_ranges(box, h0: int, w0: int):
    """Integer pixel rows / columns of a box: x1 <= q < x2, y1 <= r < y2 (q, r pixel indices)."""
    x1, y1, x2, y2 = (float(v) for v in box[:4])
    q, r = np.arange(w0), np.arange(h0)
    return r[(r >= y1) & (r < y2)], q[(q >= x1) & (q < x2)]


def native_masks(coefs: np.ndarray, protos: np.ndarray, boxes: np.ndarray, orig_hw: Tuple[int, int]):
    """coefs (n, 32), protos (mh, mw, 32) (both taken as fp64), boxes (n, 4) in original pixels.  Returns (masks uint8
    (n, h0, w0), per detection (rows, cols, v, S)): v the fp64 interpolated logit over the box's pixels and S the same
    bilinear combination of sum_k |c_k P_k|, the scale of the rounding a fp32 evaluation may make."""
    h0, w0 = orig_hw
    mh, mw, _ = protos.shape
    t, b, l, r = crop(mh, mw, h0, w0)
    P = protos[t:b, l:r].astype(np.float64)
    out = np.zeros((len(coefs), h0, w0), np.uint8)
    info = []
    for i, (c, box) in enumerate(zip(coefs.astype(np.float64), boxes)):
        rows, cols = box_ranges(box, h0, w0)
        if rows.size == 0 or cols.size == 0:
            info.append((rows, cols, np.zeros((rows.size, cols.size)), np.zeros((rows.size, cols.size))))
            continue
        v = _interp(P @ c, rows, cols, h0, w0)
        S = _interp(np.abs(P) @ np.abs(c), rows, cols, h0, w0)
        out[i][np.ix_(rows, cols)] = v > 0
        info.append((rows, cols, v, S))
    return out, info


def compare_native(got: np.ndarray, ref: np.ndarray, info, rel: float = 2.0 ** -16):
    """Every pixel outside its box must be exactly 0; inside, a pixel may differ only where |v| <= rel * S.  Returns
    (number of differing pixels, worst |v| / S over them, pixels outside the boxes that are not 0)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n_diff, worst, outside = 0, 0.0, 0
    for i, (rows, cols, v, S) in enumerate(info):
        inside = np.zeros(got.shape[1:], bool)
        if rows.size and cols.size:
            inside[np.ix_(rows, cols)] = True
        outside += int(np.count_nonzero(got[i][~inside]))
        if not inside.any():
            continue
        d = got[i][np.ix_(rows, cols)] != ref[i][np.ix_(rows, cols)]
        if d.any():
            ratio = np.abs(v[d]) / np.maximum(S[d], 1e-300)
            n_diff += int(d.sum())
            worst = max(worst, float(ratio.max()))
    return n_diff, worst, outside


def filter_classes(pred: np.ndarray, nc: int, classes) -> np.ndarray:
    """pred (B, 4+nc+nm, A) in the oracle's layout: zero the class scores of every anchor whose argmax class is not in
    ``classes`` (None: every class; ids outside [0, nc) match nothing).  With conf >= 0 such an anchor is then never a
    candidate, which is upstream's filter on the argmax after the conf test."""
    if classes is None:
        return pred
    ids = [classes] if np.ndim(classes) == 0 else list(classes)
    keep = np.zeros(nc, bool)
    for c in ids:
        if 0 <= int(c) < nc:
            keep[int(c)] = True
    p = pred.copy()
    am = p[:, 4:4 + nc, :].argmax(1)                     # (B, A): first maximum, as the kernel
    drop = ~keep[am]
    sc = p[:, 4:4 + nc, :]
    sc[np.broadcast_to(drop[:, None, :], sc.shape)] = 0.0
    return p


def nms_ref(pred: np.ndarray, nc: int, conf: float, iou: float, max_det: int, agnostic: bool = False,
            classes=None) -> List[np.ndarray]:
    """The oracle's NMS (oracle/yolov8_seg_oracle.py) on top of ``filter_classes``."""
    import yolov8_seg_oracle as orc
    return orc.non_max_suppression(filter_classes(pred, nc, classes), nc, conf, iou, max_det, agnostic=agnostic)


def random_case(rng: np.random.Generator, mh: int, mw: int, shapes: Sequence[Tuple[int, int]], n: int):
    """fp16 prototypes (B, mh, mw, 32), fp32 coefficients (B, n, 32) and boxes (B, n, 4) inside each original image."""
    B = len(shapes)
    protos = rng.standard_normal((B, mh, mw, 32)).astype(np.float16)
    coefs = (rng.standard_normal((B, n, 32)) * 0.5).astype(np.float32)
    boxes = np.zeros((B, n, 4), np.float32)
    for b, (h0, w0) in enumerate(shapes):
        x = np.sort(rng.uniform(-0.1 * w0, 1.1 * w0, (n, 2)), 1)
        y = np.sort(rng.uniform(-0.1 * h0, 1.1 * h0, (n, 2)), 1)
        boxes[b] = np.stack((x[:, 0].clip(0, w0), y[:, 0].clip(0, h0), x[:, 1].clip(0, w0), y[:, 1].clip(0, h0)), 1)
    return protos, coefs, boxes
