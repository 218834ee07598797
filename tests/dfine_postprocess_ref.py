"""Float64 numpy restatement of the D-FINE / RT-DETR detection post-processing (RTDetrImageProcessor.post_process_object_detection,
transformers models/rt_detr/image_processing_rt_detr.py:482-552, focal branch) with the order rule of m355_dfine_postprocess, the
reference of the dfine.topk_detections tests.  The project's own code: nothing here imports transformers.

    candidates i = q * C + c of one image, K = Q rows:
      NaN logits first, then descending logit (-0 == +0), an exact tie to the lowest i
    row: score = sigmoid(logit), label = i % C, box = corners(pred_boxes[i // C]) * (W, H, W, H)
    counts = (leading NaN rows, rows with score > float32(threshold))
"""
import numpy as np

GOLDEN = "dfine_postprocess_golden.npz"
GOLDEN_THRESHOLD = 0.3   # the reference trainers' value (temporal_dfine.py:190)

# (B, Q, C), target sizes (height, width) per image or None
CASES = [((1, 300, 3), [(480, 640)]),
         ((2, 300, 80), [(640, 640), (375, 500)]),
         ((3, 300, 2), [(1080, 1920), (512, 512), (333, 777)]),
         ((2, 37, 1), None),
         ((2, 20, 91), [(100, 200), (200, 100)]),
         ((2, 1024, 4), [(640, 480), (720, 1280)]),
         ((2, 2048, 1), [(800, 1333), (600, 600)]),
         ((1, 1, 1), [(32, 48)])]


def case_name(shape):
    return "b%d_q%d_c%d" % tuple(shape)


def order(logits):
    """flat candidate indices of one image (Q, C) in output order, all Q * C of them"""
    x = np.asarray(logits, np.float64).ravel()
    nan = np.isnan(x)
    key = np.where(nan, 0.0, -x) + 0.0            # ascending -logit; -0.0 + 0.0 = +0.0, and lexsort compares by value anyway
    return np.lexsort((np.arange(x.size), key, ~nan))   # last key first: NaN, then logit, then index


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def corners(b):
    cx, cy, w, h = (b[..., k] for k in range(4))
    return np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def post_process(logits, pred_boxes, sizes=None, threshold=0.5):
    """logits (B, Q, C), pred_boxes (B, Q, 4), sizes None or (B, 2) (height, width)
    -> scores (B, Q) f64, labels (B, Q) i64, boxes (B, Q, 4) f64, counts (B, 2) i64, index (B, Q) i64 (the flat candidates)"""
    logits = np.asarray(logits)
    B, Q, C = logits.shape
    xyxy = corners(np.asarray(pred_boxes, np.float64))
    if sizes is not None:
        s = np.asarray(sizes, np.float64).reshape(B, 2)
        xyxy = xyxy * np.stack([s[:, 1], s[:, 0], s[:, 1], s[:, 0]], 1)[:, None, :]
    thr = float(np.float32(threshold))
    scores, labels, boxes, counts, index = [], [], [], [], []
    for b in range(B):
        i = order(logits[b])[:Q]
        sc = sigmoid(logits[b].ravel()[i])
        nan = np.isnan(sc)
        assert not nan[int(nan.sum()):].any()
        with np.errstate(invalid="ignore"):
            counts.append((int(nan.sum()), int((sc > thr).sum())))
        scores.append(sc)
        labels.append(i % C)
        boxes.append(xyxy[b][i // C])
        index.append(i)
    return np.stack(scores), np.stack(labels).astype(np.int64), np.stack(boxes), np.array(counts, np.int64), np.stack(index)


def ladder_logits(rng, Q, C):
    """One image (Q, C) fp32 whose top scores are apart by construction: a ladder of min(Q + 8, Q * C) scores evenly spaced over
    [0.05, 0.95], each moved by at most 0.2 of a step, as logits at a random permutation of the flat positions; everything else
    is min(N(-8, 1), logit(0.04))."""
    n = Q * C
    m = min(Q + 8, n)
    step = 0.9 / (m - 1) if m > 1 else 0.0
    s = np.linspace(0.05, 0.95, m) + step * rng.uniform(-0.2, 0.2, m)
    x = np.minimum(rng.normal(-8.0, 1.0, n), np.log(0.04 / 0.96))
    x[rng.permutation(n)[:m]] = np.log(s / (1.0 - s))
    return x.astype(np.float32).reshape(Q, C)


def random_boxes(rng, B, Q):
    """(B, Q, 4) fp32 cx, cy, w, h in the unit square"""
    b = 1.0 / (1.0 + np.exp(-rng.normal(size=(B, Q, 4))))
    b[..., 2:] = b[..., 2:] * 0.5 + 0.01
    return b.astype(np.float32)


def ladder_conditions(logits, threshold, min_gap=1e-4):
    """(smallest gap among the top Q + 1 float64 scores of an image, smallest distance of any of them to the threshold)"""
    Q = logits.shape[0]
    top = np.sort(sigmoid(logits.ravel()))[::-1][:Q + 1]
    gap = float(np.min(-np.diff(top))) if top.size > 1 else np.inf
    return gap, float(np.min(np.abs(top - threshold)))


def load_case(z, shape):
    """-> dict(logits, boxes, sizes (list of (h, w)) or None, kept: per image (scores, labels, boxes) at GOLDEN_THRESHOLD,
    full: the same at threshold -1, i.e. all Q rows)"""
    n = case_name(shape)
    B, Q, _ = shape
    sizes = [tuple(int(v) for v in hw) for hw in z[n + "/sizes"]] if (n + "/sizes") in z.files else None
    cnt = [int(c) for c in z[n + "/kept_counts"]]
    off = np.concatenate([[0], np.cumsum(cnt)])
    kept = [(z[n + "/kept_scores"][off[b]:off[b + 1]], z[n + "/kept_labels"][off[b]:off[b + 1]], z[n + "/kept_boxes"][off[b]:off[b + 1]])
            for b in range(B)]
    full = [(z[n + "/full_scores"][b], z[n + "/full_labels"][b], z[n + "/full_boxes"][b]) for b in range(B)]
    return dict(logits=z[n + "/logits"], boxes=z[n + "/boxes"], sizes=sizes, kept=kept, full=full)
