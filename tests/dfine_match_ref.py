"""Float64 numpy restatement of the Hungarian matcher's cost expression (RTDetrHungarianMatcher.forward,
transformers/loss/loss_rt_detr.py:99-114), the reference of the dfine.hungarian_match tests.  The project's own code:
nothing here imports transformers.

    cost = bbox_cost * L1(cxcywh) + class_cost * class_term + giou_cost * (-GIoU(xyxy))
    class_term (focal):     alpha (1 - p)^gamma (-log(p + 1e-8)) - (1 - alpha) p^gamma (-log(1 - p + 1e-8)),  p = sigmoid(logit)
    class_term (non-focal): -softmax(logits)[target class]
"""
import numpy as np

GOLDEN = "dfine_match_golden.npz"


def corners(b):
    cx, cy, w, h = (b[..., k] for k in range(4))
    return np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def generalized_iou(a, b):
    """a (N, 4), b (M, 4) xyxy -> (N, M)"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = np.clip(np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b[None] - inter
    hull = np.clip(np.maximum(a[:, None, 2:], b[None, :, 2:]) - np.minimum(a[:, None, :2], b[None, :, :2]), 0, None)
    area = hull[..., 0] * hull[..., 1]
    return inter / union - (area - union) / area


def cost_matrix(logits, boxes, labels, tboxes, class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, alpha=0.25, gamma=2.0,
                use_focal_loss=True):
    """One image: logits (Q, C), boxes (Q, 4), labels (n), tboxes (n, 4) -> float64 (Q, n)."""
    logits, boxes, tboxes = (np.asarray(x, np.float64) for x in (logits, boxes, tboxes))
    labels = np.asarray(labels, np.int64)
    if use_focal_loss:
        p = (1.0 / (1.0 + np.exp(-logits)))[:, labels]
        cls = alpha * (1 - p) ** gamma * (-np.log(p + 1e-8)) - (1 - alpha) * p ** gamma * (-np.log(1 - p + 1e-8))
    else:
        e = np.exp(logits - logits.max(-1, keepdims=True))
        cls = -(e / e.sum(-1, keepdims=True))[:, labels]
    l1 = np.abs(boxes[:, None, :] - tboxes[None, :, :]).sum(-1)
    giou = generalized_iou(corners(boxes), corners(tboxes))
    return bbox_cost * l1 + class_cost * cls + giou_cost * (-giou)


def case_names(z):
    return [str(s) for s in z["names"]]


def load_case(z, name):
    """-> dict(logits (B, Q, C) f32, boxes (B, Q, 4) f32, sizes [n_b], labels [(n_b,) i64], tboxes [(n_b, 4) f32], focal,
    rows / cols [(K_b,) i64], optimum / gap (B,) f64)"""
    sizes = [int(s) for s in z[name + "/sizes"]]
    off = np.concatenate([[0], np.cumsum(sizes)])
    ks = [min(z[name + "/logits"].shape[1], n) for n in sizes]
    koff = np.concatenate([[0], np.cumsum(ks)])
    split = lambda a, o: [a[o[i]:o[i + 1]] for i in range(len(sizes))]
    return dict(logits=z[name + "/logits"], boxes=z[name + "/boxes"], sizes=sizes, focal=bool(z[name + "/focal"]),
                labels=split(z[name + "/labels"], off), tboxes=split(z[name + "/tboxes"], off),
                rows=split(z[name + "/rows"], koff), cols=split(z[name + "/cols"], koff),
                optimum=z[name + "/optimum"], gap=z[name + "/gap"])
