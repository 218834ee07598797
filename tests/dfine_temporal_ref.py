"""The literal torch expressions of the temporal-head ops (csrc/dfine_temporal.hip, the guarded decode of csrc/dfine_kernels.hip),
restated here from the trainers' lines so that the tests do not judge the package by its own fallbacks.  Every function runs in
float64 or fp32 on any device and is differentiable by autograd."""
import torch
import torch.nn.functional as F


def temporal_fuse(fused, scores, context=None):
    """fused (T, Q, D), scores (T, Q, 1) or (T, Q): softmax over the frames, the weighted features, plus the context"""
    out = fused * F.softmax(scores.reshape(tuple(fused.shape[:2]) + (1,)), dim=0)
    return out if context is None else out + context


def guard_logits(cls_logits, anomaly=None, bound=20.0):
    """anomaly scores on all but the last class column through a slice and a cat, then the clamp and nan_to_num"""
    if anomaly is not None:
        cls_logits = torch.cat([cls_logits[..., :-1] + anomaly, cls_logits[..., -1:]], dim=-1)
    cls_logits = cls_logits.clamp(-bound, bound)
    return torch.nan_to_num(cls_logits, nan=0.0, posinf=bound, neginf=-bound)


def integral(pred_corners, project):
    """DFineIntegral.forward: softmax over the bins of every side, linear with the weighting function"""
    nb1 = project.numel()
    p = F.softmax(pred_corners.reshape(-1, nb1), dim=1)
    return F.linear(p, project.reshape(1, -1)).reshape(tuple(pred_corners.shape[:-1]) + (4,))


def distance2bbox(points, distance, reg_scale):
    reg_scale = abs(reg_scale)
    x0 = points[..., 0] - (0.5 * reg_scale + distance[..., 0]) * (points[..., 2] / reg_scale)
    y0 = points[..., 1] - (0.5 * reg_scale + distance[..., 1]) * (points[..., 3] / reg_scale)
    x1 = points[..., 0] + (0.5 * reg_scale + distance[..., 2]) * (points[..., 2] / reg_scale)
    y1 = points[..., 1] + (0.5 * reg_scale + distance[..., 3]) * (points[..., 3] / reg_scale)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1)


def guard_boxes(boxes, clamp01=True):
    """the last two guards of the chain alone: what a box coordinate goes through"""
    if clamp01:
        boxes = boxes.clamp(0, 1)
    return torch.nan_to_num(boxes, nan=0.5, posinf=1.0, neginf=0.0)


def decode_boxes(pred_corners, project, points, reg_scale, clamp01=False, guard=False, integral_fn=integral, d2b_fn=distance2bbox):
    """guard: the trainers' chain, nan_to_num -> integral -> nan_to_num -> distance2bbox [-> clamp] -> nan_to_num"""
    if guard:
        pred_corners = torch.nan_to_num(pred_corners, nan=0.0, posinf=1.0, neginf=0.0)
    distances = integral_fn(pred_corners, project)
    if guard:
        distances = torch.nan_to_num(distances, nan=0.0, posinf=1.0, neginf=0.0)
    boxes = d2b_fn(points, distances, reg_scale)
    if guard:
        return guard_boxes(boxes, clamp01)
    return boxes.clamp(0, 1) if clamp01 else boxes


def noobject_loss(cls_logits, class_index=-1):
    """(T, Q, C1) -> (T,): cross_entropy of every frame against the one class"""
    T, Q, C1 = cls_logits.shape
    target = torch.full((Q,), class_index % C1, dtype=torch.long, device=cls_logits.device)
    return torch.stack([F.cross_entropy(cls_logits[t], target) for t in range(T)])


def consistency_loss(a):
    """the improved trainer's loop: the mean over t >= 1 of mse_loss(a[t], a[t - 1]); a zero tensor for one frame"""
    T = a.shape[0]
    if T <= 1:
        return a.new_zeros(())
    loss = 0.0
    for t in range(1, T):
        loss = loss + F.mse_loss(a[t], a[t - 1])
    return loss / (T - 1)


def temporal_head(fused, init_ref, class_head, bbox_head, project, reg_scale, scores=None, context=None, anomaly_head=None, bound=20.0):
    x = fused if scores is None else temporal_fuse(fused, scores, context)
    anomaly = anomaly_head(x) if anomaly_head is not None else None
    cls_logits = guard_logits(class_head(x), anomaly, bound)
    boxes = decode_boxes(bbox_head(x), project, init_ref, reg_scale, clamp01=True, guard=True)
    return cls_logits, boxes, anomaly


LOGIT_TABLE = ([float("nan"), float("inf"), float("-inf"), 20.0, -20.0, 20.000002, 3.0, -25.0],   # in
               [0.0, 20.0, -20.0, 20.0, -20.0, 20.0, 3.0, -20.0],                                  # out
               [0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0])                                           # gradient mask
BOX_TABLE = ([float("nan"), 1.5, -0.2, 0.0, 1.0, 0.3], [0.5, 1.0, 0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
