"""Generates tests/golden/dfine_loss_golden.npz: seeded inputs of the D-FINE loss terms and what transformers' own DFineLoss
methods (5.15.0: loss_labels_vfl, loss_boxes, loss_local, on the CPU) compute from them: the five term values and the gradients
of sum_k c_k * term_k (c = dfine_loss_ref.COEFFS) with respect to logits, pred_boxes and pred_corners.

Inputs are fp32-exact values, handed to upstream as float64 tensors wherever its code takes them: all of loss_labels_vfl and
loss_boxes, and in loss_local the logits, boxes and corner distributions.  loss_local forces fp32 in four places.  translate_gt
stores the bin weights in `closest_left_indices.float()`-typed tensors and refuses a float64 distance (index_put dtype mismatch),
so `ref_points` and the target boxes go into loss_local as fp32 and bbox2distance / translate_gt run in fp32;
unimodal_distribution_focal_loss takes `weight.float()` of the IoUs; `mask.sum() * batch_scale` (int tensor * Python float) makes
num_pos / num_neg fp32.  So loss_fgl, loss_ddf and the pred_corners gradient are recorded at fp32 accuracy (`fp32_terms`): the
host test holds the float64 restatement to 1e-9 on the rest and, given the same fp32 ref_points / target boxes, to 2e-6 on these.
The criterion is not moved to float64: W(n) is upstream's fp32 weighting_function, the `project` the kernel gets.

Every case must keep fp32 rounding away from a decision (asserted here, in float64): every FGL distance >= 1e-3 from every W(n),
every |src - tgt| coordinate >= 1e-4, every pair of min / max arguments of IoU / GIoU >= 1e-4 apart, every union and hull area
>= 1e-3.  A seed that misses is skipped for the next one.  Cases (a) and (g) use max_num_bins 16, the others 32: with 33 bins the
two 300-query cases alone would pass the size limit of a committed file.
Run from the repository root: `python tests/golden/make_dfine_loss_golden.py`; the .npz is data: inputs and expected outputs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dfine_loss_ref as ref  # noqa: E402


def criterion_for(C, R):
    from transformers import DFineConfig
    from transformers.loss.loss_d_fine import DFineLoss
    return DFineLoss(DFineConfig(num_labels=C, max_num_bins=R))


def draw(rng, B, Q, C, sizes, R, local, groups=1, ends=False):
    f = np.float32
    case = {"logits": rng.normal(0, 1.5, (B, Q, C)).astype(f)}
    boxes = np.concatenate([rng.uniform(0.2, 0.8, (B, Q, 2)), rng.uniform(0.05, 0.4, (B, Q, 2))], -1).astype(f)
    T = sum(sizes)
    tboxes = np.concatenate([rng.uniform(0.2, 0.8, (T, 2)), rng.uniform(0.05, 0.4, (T, 2))], -1).astype(f)
    labels = rng.integers(0, C, T).astype(np.int64)
    ref_points = np.concatenate([rng.uniform(0.2, 0.8, (B, Q, 2)), rng.uniform(0.05, 0.4, (B, Q, 2))], -1).astype(f)
    mq, mt, lens, o = [], [], [], 0
    for b, n in enumerate(sizes):
        if groups > 1:      # denoising form: every target once per group, distinct queries
            k = n * groups
            q = rng.permutation(Q)[:k]
            t = np.tile(np.arange(n), groups)
        else:               # Hungarian form: min(Q, n) pairs by ascending query, distinct targets
            k = min(Q, n)
            q = np.sort(rng.permutation(Q)[:k])
            t = rng.permutation(n)[:k]
        for qi, ti in zip(q, t):   # matched predictions and reference points sit near their target
            tb = tboxes[o + ti]
            boxes[b, qi] = (tb + np.concatenate([rng.uniform(-0.04, 0.04, 2), rng.uniform(-0.03, 0.03, 2)])).astype(f)
            ref_points[b, qi] = np.concatenate([tb[:2] + rng.uniform(-0.02, 0.02, 2), tb[2:] * rng.uniform(0.7, 1.3, 2)]).astype(f)
        mq.append(q); mt.append(t); lens.append(k); o += n
    if ends:   # FGL's end rules: target 0 far wider than its reference box, the reference point of target 1 outside its target
        b, (q0, q1) = 0, mq[0][:2]
        t0, t1 = tboxes[mt[0][0]], tboxes[mt[0][1]]
        ref_points[b, q0] = np.array([t0[0], t0[1], 0.01, 0.01], f)
        ref_points[b, q1] = np.array([t1[0] - t1[2], t1[1] - t1[3], 0.1, 0.1], f)
    case.update(pred_boxes=boxes, tboxes=tboxes, labels=labels, sizes=np.array(sizes), lens=np.array(lens),
                match_q=np.concatenate(mq).astype(np.int64) if mq else np.zeros(0, np.int64),
                match_t=np.concatenate(mt).astype(np.int64) if mt else np.zeros(0, np.int64))
    if local:
        case.update(pred_corners=rng.normal(0, 1, (B, Q, 4 * (R + 1))).astype(f), ref_points=ref_points,
                    teacher_corners=rng.normal(0, 1, (B, Q, 4 * (R + 1))).astype(f),
                    teacher_logits=rng.normal(0, 1.5, (B, Q, C)).astype(f))
    return case


def margins_ok(case, outputs, targets, indices, kw, ends):
    """the conditions of the module docstring, in float64; also that an `ends` case really reaches both end rules"""
    idx = ref._get_source_permutation_idx(indices)
    if idx[0].numel() == 0:
        return True
    src = outputs["pred_boxes"][idx].detach()
    tgt = torch.cat([t["boxes"][i] for t, (_, i) in zip(targets, indices)], 0)
    a, b = ref.center_to_corners_format(src), ref.center_to_corners_format(tgt)
    ok = bool(((src - tgt).abs() >= 1e-4).all() and ((a - b).abs() >= 1e-4).all())
    iou, union = ref.box_iou(a, b)
    hull = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0).prod(-1)
    ok = ok and bool((torch.diag(union) >= 1e-3).all() and (hull >= 1e-3).all())
    if "pred_corners" in outputs:
        d = ref.fgl_distances(outputs["ref_points"][idx], b, kw["reg_scale"]).reshape(-1)
        W = kw["project"]
        ok = ok and bool(((d.unsqueeze(1) - W.unsqueeze(0)).abs() >= 1e-3).all())
        if ends:
            ok = ok and bool((d < W[0]).any() and (d >= W[-1]).any())
    return ok


def record(name, spec, seed0, store):
    B, Q, C, sizes, R, local = spec["B"], spec["Q"], spec["C"], spec["sizes"], spec.get("R", 32), spec.get("local", True)
    groups, ends = spec.get("groups", 1), spec.get("ends", False)
    crit = criterion_for(C, R)
    for seed in range(seed0, seed0 + 200):
        case = draw(np.random.default_rng(seed), B, Q, C, sizes, R, local, groups, ends)
        if spec.get("teacher_is_pred"):
            case["teacher_corners"] = case["pred_corners"].copy()
        case.update(alpha=np.float64(crit.alpha), gamma=np.float64(crit.gamma), num_boxes=np.float64(max(sum(sizes), 1) * groups))
        if local:
            from transformers.loss.loss_d_fine import weighting_function
            case.update(project=weighting_function(R, crit.up.detach(), crit.reg_scale).numpy().astype(np.float32),
                        reg_scale=np.float64(crit.reg_scale), temperature=np.float64(5.0))
        outputs, targets, indices, kw = ref.tensors(case)
        if margins_ok(case, outputs, targets, indices, kw, ends):
            break
    else:
        raise SystemExit(f"no seed keeps the margins for case {name}")
    nb = float(case["num_boxes"])
    values = dict(crit.loss_labels_vfl(outputs, targets, indices, nb))
    values.update(crit.loss_boxes(outputs, targets, indices, nb))
    if local:
        values.update(crit.loss_local(*ref.local_fp32(outputs, targets), indices, nb))
    grads = ref.weighted_grads(values, outputs)
    case["seed"] = np.int64(seed)
    for k, v in values.items():
        assert v.dtype == torch.float64, (k, v.dtype)
        case[k] = v.detach().numpy()
    for k, g in grads.items():
        case[k] = (torch.zeros_like(outputs[k[5:]]) if g is None else g).numpy()
    case["fp32_terms"] = np.array(["loss_fgl", "loss_ddf", "grad_pred_corners"])
    drop = ()
    if spec.get("teacher_is_pred"):   # stored as a reference to case (a): same seed, same arrays
        assert seed == store["seed_of"][spec["same_inputs_as"]]
        case["same_inputs_as"] = np.array(spec["same_inputs_as"])
        drop = ("logits", "pred_boxes", "tboxes", "labels", "sizes", "lens", "match_q", "match_t", "pred_corners", "ref_points",
                "teacher_corners", "teacher_logits", "project", "reg_scale", "temperature", "alpha", "gamma", "num_boxes")
    store["seed_of"][name] = seed
    for k, v in case.items():
        if k not in drop:
            store["arrays"][f"{name}/{k}"] = v
    print(name, "seed", seed, {k: float(v.detach()) for k, v in values.items()})


CASES = {
    "a_q300": dict(B=1, Q=300, C=3, sizes=(3,), R=16),
    "b_empty_image": dict(B=2, Q=37, C=1, sizes=(0, 5)),
    "c_all_matched": dict(B=3, Q=20, C=80, sizes=(30, 2, 0)),
    "d_no_local": dict(B=2, Q=5, C=3, sizes=(1, 0), local=False),
    "e_no_targets": dict(B=2, Q=20, C=2, sizes=(0, 0)),
    "f_no_unmatched": dict(B=1, Q=4, C=2, sizes=(6,)),
    "g_teacher_is_pred": dict(B=1, Q=300, C=3, sizes=(3,), R=16, teacher_is_pred=True, same_inputs_as="a_q300"),
    "h_denoising": dict(B=2, Q=12, C=3, sizes=(2, 2), groups=3),
    "i_fgl_ends": dict(B=1, Q=8, C=2, sizes=(2,), ends=True),
}

if __name__ == "__main__":
    store = {"arrays": {}, "seed_of": {}}
    for i, (name, spec) in enumerate(CASES.items()):
        record(name, spec, 1000 if spec.get("teacher_is_pred") else 1000 + 1000 * i, store)
    path = os.path.join(HERE, ref.GOLDEN)
    np.savez_compressed(path, **store["arrays"])
    print("wrote", path, os.path.getsize(path), "bytes")
