"""Numpy restatement of the D-FINE encoder query selection (dfine.select_queries) and the case table of its goldens.

Order rule (the kernel's): score = max over C of the class logits, NaN if the row holds one; NaN scores first, then descending
score with -0 == +0, an exact tie to the lowest token.  Gathered rows are copies; the boxes are the float64 sigmoid."""
import numpy as np

GOLDEN = "dfine_select_golden.npz"
# (B, feature levels (h = w), C = num_labels, K = num_queries): S = sum of h * h
CASES = [
    (1, (20, 10, 5), 80, 300),    # S = 525
    (2, (32, 16, 8), 5, 300),     # S = 1344
    (1, (80, 40, 20), 2, 300),    # S = 8400, the trainers' token count
    (2, (20, 10, 5), 3, 100),     # K = 100
]
FIELDS = ("enc_outputs_class", "enc_outputs_coord_logits", "indices", "init_reference_points", "enc_topk_logits", "enc_topk_bboxes")


def case_name(case):
    B, levels, C, K = case
    return f"b{B}_s{sum(h * h for h in levels)}_c{C}_k{K}"


def load_case(z, case):
    return {f: z[f"{case_name(case)}/{f}"] for f in FIELDS}


def token_scores(class_logits):
    """(B, S, C) -> (B, S) float32: the row max, NaN where the row holds a NaN (torch.max)"""
    x = np.asarray(class_logits, np.float32)
    with np.errstate(invalid="ignore"):
        m = x.max(-1)
    return np.where(np.isnan(x).any(-1), np.float32(np.nan), m)


def select_indices(scores, K):
    """(B, S) scores -> (B, K) int64 tokens in output order"""
    s = np.asarray(scores, np.float64)
    nan = np.isnan(s)
    key = np.where(nan, np.inf, s + 0.0)   # -0 + 0 = +0: the two zeros tie
    out = np.empty((s.shape[0], K), np.int64)
    for b in range(s.shape[0]):
        # stable sort by (not NaN, -key): NaN first, descending score, lowest token among equals
        order = np.lexsort((np.arange(s.shape[1]), -key[b], ~nan[b]))
        out[b] = order[:K]
    return out


def select(class_logits, coord_logits, memory=None, K=300):
    """indices (B, K) int64, ref (B, K, 4) fp32 copies, boxes (B, K, 4) float64 sigmoid, logits (B, K, C) copies, target or None"""
    cl, co = np.asarray(class_logits, np.float32), np.asarray(coord_logits, np.float32)
    ind = select_indices(token_scores(cl), K)
    rows = lambda t: np.take_along_axis(t, ind[:, :, None], 1)
    ref = rows(co)
    with np.errstate(over="ignore"):
        boxes = 1.0 / (1.0 + np.exp(-ref.astype(np.float64)))
    return ind, ref, boxes, rows(cl), None if memory is None else rows(np.asarray(memory, np.float32))


def top_gap(scores, K):
    """smallest difference between neighbours among the K + 1 greatest scores of every image (inf when S == K)"""
    s = -np.sort(-np.asarray(scores, np.float64), axis=1)[:, :K + 1]
    return float(np.diff(-s, axis=1).min(initial=np.inf))
