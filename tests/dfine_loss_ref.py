"""Float64 torch restatement of the D-FINE loss terms, function by function under upstream's names (transformers 5.15.0,
loss/loss_for_object_detection.py, loss/loss_rt_detr.py:165-254, loss/loss_d_fine.py:74-301), under autograd.  What the tests measure
the HIP kernels (csrc/dfine_loss.hip) and dfine.detection_loss against.  It differs from upstream only where upstream drops to
fp32 inside a float64 call (translate_gt's `.float()` weights, `weight.float()`, the int * float `num_pos`): everything here
stays in the dtype of its inputs.  W(n) is an input (`project`), the tensor weighting_function returns."""
import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = "dfine_loss_golden.npz"
TERMS = ("loss_vfl", "loss_bbox", "loss_giou", "loss_fgl", "loss_ddf")
COEFFS = (1.0, 0.7, 1.3, 0.45, 2.1)   # the fixed unequal c_k of the recorded gradients of sum_k c_k * term_k


def center_to_corners_format(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def box_iou(boxes1, boxes2):
    area1, area2 = box_area(boxes1), box_area(boxes2)
    left_top = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    right_bottom = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    width_height = (right_bottom - left_top).clamp(min=0)
    inter = width_height[:, :, 0] * width_height[:, :, 1]
    union = area1[:, None] + area2 - inter
    return inter / union, union


def generalized_box_iou(boxes1, boxes2):
    iou, union = box_iou(boxes1, boxes2)
    top_left = torch.min(boxes1[:, None, :2], boxes2[:, :2])
    bottom_right = torch.max(boxes1[:, None, 2:], boxes2[:, 2:])
    width_height = (bottom_right - top_left).clamp(min=0)
    area = width_height[:, :, 0] * width_height[:, :, 1]
    return iou - (area - union) / area


def _get_source_permutation_idx(indices):
    batch_idx = torch.cat([torch.full_like(source, i) for i, (source, _) in enumerate(indices)])
    source_idx = torch.cat([source for (source, _) in indices])
    return batch_idx, source_idx


def loss_labels_vfl(outputs, targets, indices, num_boxes, alpha, gamma):
    idx = _get_source_permutation_idx(indices)
    src_boxes = outputs["pred_boxes"][idx]
    target_boxes = torch.cat([t["boxes"][i] for t, (_, i) in zip(targets, indices)], dim=0)
    ious = torch.diag(box_iou(center_to_corners_format(src_boxes.detach()), center_to_corners_format(target_boxes))[0])
    src_logits = outputs["logits"]
    num_classes = src_logits.shape[-1]
    target_classes_original = torch.cat([t["class_labels"][i] for t, (_, i) in zip(targets, indices)])
    target_classes = torch.full(src_logits.shape[:2], num_classes, dtype=torch.int64)
    target_classes[idx] = target_classes_original
    target = F.one_hot(target_classes, num_classes=num_classes + 1)[..., :-1]
    target_score_original = torch.zeros_like(target_classes, dtype=src_logits.dtype)
    target_score_original[idx] = ious
    target_score = target_score_original.unsqueeze(-1) * target
    pred_score = torch.sigmoid(src_logits.detach())
    weight = alpha * pred_score.pow(gamma) * (1 - target) + target_score
    loss = F.binary_cross_entropy_with_logits(src_logits, target_score, weight=weight, reduction="none")
    return {"loss_vfl": loss.mean(1).sum() * src_logits.shape[1] / num_boxes}


def loss_boxes(outputs, targets, indices, num_boxes):
    idx = _get_source_permutation_idx(indices)
    src_boxes = outputs["pred_boxes"][idx]
    target_boxes = torch.cat([t["boxes"][i] for t, (_, i) in zip(targets, indices)], dim=0)
    loss_bbox = F.l1_loss(src_boxes, target_boxes, reduction="none")
    loss_giou = 1 - torch.diag(generalized_box_iou(center_to_corners_format(src_boxes), center_to_corners_format(target_boxes)))
    return {"loss_bbox": loss_bbox.sum() / num_boxes, "loss_giou": loss_giou.sum() / num_boxes}


def translate_gt(gt, project):
    max_num_bins = project.numel() - 1
    gt = gt.reshape(-1)
    diffs = project.unsqueeze(0) - gt.unsqueeze(1)
    closest_left_indices = torch.sum(diffs <= 0, dim=1) - 1
    indices = closest_left_indices.to(gt.dtype)
    weight_right, weight_left = torch.zeros_like(indices), torch.zeros_like(indices)
    valid_idx_mask = (indices >= 0) & (indices < max_num_bins)
    valid_indices = indices[valid_idx_mask].long()
    left_diffs = torch.abs(gt[valid_idx_mask] - project[valid_indices])
    right_diffs = torch.abs(project[valid_indices + 1] - gt[valid_idx_mask])
    weight_right[valid_idx_mask] = left_diffs / (left_diffs + right_diffs)
    weight_left[valid_idx_mask] = 1.0 - weight_right[valid_idx_mask]
    neg, pos = indices < 0, indices >= max_num_bins
    weight_right[neg], weight_left[neg], indices[neg] = 0.0, 1.0, 0.0
    weight_right[pos], weight_left[pos], indices[pos] = 1.0, 0.0, max_num_bins - 0.1
    return indices, weight_right, weight_left


def fgl_distances(points, bbox, reg_scale):
    """the four_lens of bbox2distance before translate_gt: (n, 4) left, top, right, bottom"""
    reg_scale = abs(reg_scale)
    left = (points[:, 0] - bbox[:, 0]) / (points[..., 2] / reg_scale + 1e-16) - 0.5 * reg_scale
    top = (points[:, 1] - bbox[:, 1]) / (points[..., 3] / reg_scale + 1e-16) - 0.5 * reg_scale
    right = (bbox[:, 2] - points[:, 0]) / (points[..., 2] / reg_scale + 1e-16) - 0.5 * reg_scale
    bottom = (bbox[:, 3] - points[:, 1]) / (points[..., 3] / reg_scale + 1e-16) - 0.5 * reg_scale
    return torch.stack([left, top, right, bottom], -1)


def bbox2distance(points, bbox, project, reg_scale, eps=0.1):
    four_lens, weight_right, weight_left = translate_gt(fgl_distances(points, bbox, reg_scale), project)
    four_lens = four_lens.clamp(min=0, max=project.numel() - 1 - eps)
    return four_lens.reshape(-1).detach(), weight_right.detach(), weight_left.detach()


def unimodal_distribution_focal_loss(pred, label, weight_right, weight_left, weight, avg_factor):
    dis_left = label.long()
    loss = F.cross_entropy(pred, dis_left, reduction="none") * weight_left.reshape(-1) \
        + F.cross_entropy(pred, dis_left + 1, reduction="none") * weight_right.reshape(-1)
    return (loss * weight).sum() / avg_factor


def loss_local(outputs, targets, indices, num_boxes, project, reg_scale, T=5):
    nb1 = project.numel()
    idx = _get_source_permutation_idx(indices)
    target_boxes = torch.cat([t["boxes"][i] for t, (_, i) in zip(targets, indices)], dim=0)
    pred_corners = outputs["pred_corners"][idx].reshape(-1, nb1)
    ref_points = outputs["ref_points"][idx].detach()
    target_corners, weight_right, weight_left = bbox2distance(ref_points, center_to_corners_format(target_boxes), project, reg_scale)
    ious = torch.diag(box_iou(center_to_corners_format(outputs["pred_boxes"][idx]), center_to_corners_format(target_boxes))[0])
    weight_targets = ious.unsqueeze(-1).repeat(1, 1, 4).reshape(-1).detach()
    losses = {"loss_fgl": unimodal_distribution_focal_loss(pred_corners, target_corners, weight_right, weight_left, weight_targets,
                                                           num_boxes)}
    pred_corners = outputs["pred_corners"].reshape(-1, nb1)
    target_corners = outputs["teacher_corners"].reshape(-1, nb1)
    if torch.equal(pred_corners, target_corners):
        losses["loss_ddf"] = pred_corners.sum() * 0
        return losses
    weight_targets_local = outputs["teacher_logits"].sigmoid().max(dim=-1)[0]
    mask = torch.zeros_like(weight_targets_local, dtype=torch.bool)
    mask[idx] = True
    mask = mask.unsqueeze(-1).repeat(1, 1, 4).reshape(-1)
    weight_targets_local[idx] = ious.reshape_as(weight_targets_local[idx])
    weight_targets_local = weight_targets_local.unsqueeze(-1).repeat(1, 1, 4).reshape(-1).detach()
    kl = torch.nn.KLDivLoss(reduction="none")(F.log_softmax(pred_corners / T, dim=1), F.softmax(target_corners.detach() / T, dim=1))
    loss_match_local = weight_targets_local * (T ** 2) * kl.sum(-1)
    batch_scale = 1 / outputs["pred_boxes"].shape[0]
    num_pos = (mask.sum().to(kl.dtype) * batch_scale) ** 0.5
    num_neg = ((~mask).sum().to(kl.dtype) * batch_scale) ** 0.5
    loss_match_local1 = loss_match_local[mask].mean() if mask.any() else 0
    loss_match_local2 = loss_match_local[~mask].mean() if (~mask).any() else 0
    losses["loss_ddf"] = (loss_match_local1 * num_pos + loss_match_local2 * num_neg) / (num_pos + num_neg)
    return losses


# ---- the golden fixture ---------------------------------------------------------------------------------------------------
def case_names(z):
    return sorted({k.split("/")[0] for k in z.files})


def load_case(z, name):
    """one case of dfine_loss_golden.npz as a dict of numpy arrays / Python values (inputs are fp32-exact values)"""
    g = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    if "same_inputs_as" in g:   # case (g): the arrays of case (a), the teacher a copy of the prediction
        base = load_case(z, str(g["same_inputs_as"]))
        for k, v in base.items():
            if k not in g and not k.startswith("grad_") and k not in TERMS and k != "fp32_terms":
                g[k] = v
        g["teacher_corners"] = base["pred_corners"].copy()
    return g


def tensors(case, dtype=torch.float64, device="cpu", requires_grad=True):
    """(outputs, targets, indices, kwargs) of a case as torch tensors; kwargs are detection_loss's keyword arguments"""
    def t(a, dt=dtype):
        return torch.tensor(np.asarray(a), dtype=dt, device=device)
    sizes, lens = [int(v) for v in case["sizes"]], [int(v) for v in case["lens"]]
    outputs = {"logits": t(case["logits"]).requires_grad_(requires_grad), "pred_boxes": t(case["pred_boxes"]).requires_grad_(requires_grad)}
    targets, indices, o, e = [], [], 0, 0
    for n, m in zip(sizes, lens):
        targets.append({"class_labels": t(case["labels"][o:o + n], torch.int64), "boxes": t(case["tboxes"][o:o + n].reshape(n, 4))})
        indices.append((t(case["match_q"][e:e + m], torch.int64), t(case["match_t"][e:e + m], torch.int64)))
        o, e = o + n, e + m
    kw = dict(alpha=float(case["alpha"]), gamma=float(case["gamma"]))
    if "pred_corners" in case:
        outputs["pred_corners"] = t(case["pred_corners"]).requires_grad_(requires_grad)
        outputs["ref_points"], outputs["teacher_corners"] = t(case["ref_points"]), t(case["teacher_corners"])
        outputs["teacher_logits"] = t(case["teacher_logits"])
        kw.update(project=t(case["project"]), reg_scale=float(case["reg_scale"]), temperature=float(case["temperature"]))
    return outputs, targets, indices, kw


def local_fp32(outputs, targets):
    """(outputs, targets) as upstream's loss_local had them when the golden was recorded: ref_points and the target boxes in fp32
    (translate_gt refuses float64 distances), everything else unchanged"""
    if "ref_points" in outputs:   # an output without corners has none
        outputs = dict(outputs, ref_points=outputs["ref_points"].float())
    return outputs, [dict(t, boxes=t["boxes"].float()) for t in targets]


def terms(outputs, targets, indices, num_boxes, alpha, gamma, project=None, reg_scale=None, temperature=5.0, as_recorded=False):
    """all terms of one output by the restatement, in the dtype of the tensors; as_recorded: loss_local gets local_fp32's inputs"""
    out = dict(loss_labels_vfl(outputs, targets, indices, num_boxes, alpha, gamma))
    out.update(loss_boxes(outputs, targets, indices, num_boxes))
    if "pred_corners" in outputs:
        lo, lt = local_fp32(outputs, targets) if as_recorded else (outputs, targets)
        out.update(loss_local(lo, lt, indices, num_boxes, project.to(lo["ref_points"].dtype), reg_scale, temperature))
    return out


def weighted_grads(values, outputs):
    """gradients of sum_k COEFFS[k] * term_k with respect to logits, pred_boxes and (if present) pred_corners"""
    total = sum(c * values[k] for k, c in zip(TERMS, COEFFS) if k in values)
    wrt = [outputs[k] for k in ("logits", "pred_boxes", "pred_corners") if k in outputs]
    return dict(zip(("grad_logits", "grad_pred_boxes", "grad_pred_corners"), torch.autograd.grad(total, wrt, allow_unused=True)))
