"""Generates tests/golden/dfine_match_golden.npz: seeded inputs of the D-FINE Hungarian matcher and what transformers'
RTDetrHungarianMatcher (5.15.0, loss/loss_rt_detr.py:68-120, on CPU fp32 tensors, scipy's linear_sum_assignment) returns for
them, plus per image the float64 optimum and the gap to the second-best assignment (every matched pair forbidden in turn,
re-solved on the float64 cost matrix of tests/dfine_match_ref.py).  Every committed image has gap >= 1e-3, asserted here, so
an fp32 cost error of 1e-6 cannot change the answer.  Run in the build container only
(`python tests/golden/make_dfine_match_golden.py`); the .npz is data: inputs and expected outputs."""
import os
import sys

import numpy as np
import scipy
import torch
import transformers
from scipy.optimize import linear_sum_assignment
from transformers import DFineConfig
from transformers.loss.loss_rt_detr import RTDetrHungarianMatcher

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dfine_match_ref as ref  # noqa: E402

# (Q, C, targets per image, seed, use_focal_loss)
CASES = [(300, 3, [0, 1, 5, 16], 0, True), (300, 80, [40, 2, 0, 7], 1, True), (300, 1, [3, 3, 64, 1], 2, True),
         (37, 5, [37, 12], 3, True), (20, 4, [30, 5], 4, True), (300, 2, [100], 5, True),
         (300, 3, [0, 1, 5, 16], 0, False)]
MIN_GAP = 1e-3


def make_inputs(Q, C, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    logits = 2 * torch.randn(B, Q, C, generator=g)
    boxes = torch.sigmoid(torch.randn(B, Q, 4, generator=g))
    boxes[..., 2:] = boxes[..., 2:] * 0.5 + 0.01
    labels, tboxes = [], []
    for n in sizes:
        labels.append(torch.randint(0, C, (n,), generator=g))
        tb = torch.rand(n, 4, generator=g)
        tb[:, 2:] = tb[:, 2:] * 0.4 + 0.02
        tboxes.append(tb)
    return logits, boxes, labels, tboxes


def second_best_gap(cost, rows, cols, optimum):
    """smallest increase of the optimum when one matched pair is forbidden (inf where no other assignment exists)"""
    gap = np.inf
    for r, c in zip(rows, cols):
        m = cost.copy()
        m[r, c] = 1e9
        rr, cc = linear_sum_assignment(m)
        total = m[rr, cc].sum()
        if total < 1e8:
            gap = min(gap, total - optimum)
    return gap


def main():
    out = {"transformers_version": np.array(transformers.__version__), "scipy_version": np.array(scipy.__version__), "names": []}
    names, worst_gap, worst_abs = [], np.inf, 0.0
    for Q, C, sizes, seed, focal in CASES:
        name = f"q{Q}_c{C}_s{seed}_{'focal' if focal else 'softmax'}"
        names.append(name)
        logits, boxes, labels, tboxes = make_inputs(Q, C, sizes, seed)
        cfg = DFineConfig()
        cfg.use_focal_loss = focal
        matcher = RTDetrHungarianMatcher(cfg)
        assert (matcher.class_cost, matcher.bbox_cost, matcher.giou_cost, matcher.alpha, matcher.gamma) == (2, 5, 2, 0.25, 2.0)
        targets = [{"class_labels": l, "boxes": t} for l, t in zip(labels, tboxes)]
        indices = matcher({"logits": logits, "pred_boxes": boxes}, targets)
        optimum, gaps = [], []
        for b, n in enumerate(sizes):
            rows, cols = indices[b][0].numpy(), indices[b][1].numpy()
            cost = ref.cost_matrix(logits[b].numpy(), boxes[b].numpy(), labels[b].numpy(), tboxes[b].numpy(), use_focal_loss=focal)
            r64, c64 = linear_sum_assignment(cost)
            assert np.array_equal(r64, rows) and np.array_equal(c64, cols), (name, b)   # fp32 upstream == float64 restatement
            opt = float(cost[rows, cols].sum())
            gap = second_best_gap(cost, rows, cols, opt) if n else np.inf
            assert gap >= MIN_GAP, (name, b, gap)
            optimum.append(opt)
            gaps.append(gap)
            if n:
                worst_gap, worst_abs = min(worst_gap, gap), max(worst_abs, float(np.abs(cost).max()))
        out[name + "/logits"], out[name + "/boxes"] = logits.numpy(), boxes.numpy()
        out[name + "/sizes"], out[name + "/focal"] = np.array(sizes, np.int32), np.array(focal)
        out[name + "/labels"] = torch.cat(labels).numpy().astype(np.int64)
        out[name + "/tboxes"] = torch.cat(tboxes).numpy()
        out[name + "/rows"] = np.concatenate([i[0].numpy() for i in indices]).astype(np.int64)
        out[name + "/cols"] = np.concatenate([i[1].numpy() for i in indices]).astype(np.int64)
        out[name + "/optimum"], out[name + "/gap"] = np.array(optimum), np.array(gaps)
        print(name, "gaps", ["%.3g" % g for g in gaps])
    out["names"] = np.array(names)
    path = os.path.join(HERE, ref.GOLDEN)
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; smallest gap {worst_gap:.3g}, largest |cost| {worst_abs:.3g}")


if __name__ == "__main__":
    main()
