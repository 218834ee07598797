"""CPU reference of the detection training loss -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Upstream's ``v8DetectionLoss`` (what a box-label training run minimises) restated from the pieces of the training oracle
(``oracle/yolov8_seg_train_oracle.py``: ``task_aligned_assign``, ``bbox_iou``, ``dist2bbox_xyxy``, ``bbox2dist``, ``dfl_loss``):
it is ``segmentation_loss`` there without the mask term.  Gradients come from autograd.  No product code is imported.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch
import torch.nn.functional as F

from yolov8_seg_oracle import REG_MAX, make_anchors
from yolov8_seg_train_oracle import bbox2dist, bbox_iou, dfl_loss, dist2bbox_xyxy, task_aligned_assign


def detection_loss(raw: Sequence[torch.Tensor], batch: Dict[str, torch.Tensor], nc: int, imgsz: Tuple[int, int],
                   gains=(7.5, 0.5, 1.5)):
    """raw: 3 maps (B, 64 + nc, h, w); batch: batch_idx (N,), cls (N,), bboxes (N, 4) normalised xywh.
    Returns (loss * B, items [box, cls, dfl]) in the dtype of ``raw``."""
    B, no = raw[0].shape[:2]
    dt = raw[0].dtype
    x_cat = torch.cat([r.view(B, no, -1) for r in raw], 2)
    pred_distri, pred_scores = x_cat.split((REG_MAX * 4, nc), 1)
    pred_scores = pred_scores.permute(0, 2, 1).contiguous()            # (B, A, nc)
    pred_distri = pred_distri.permute(0, 2, 1).contiguous()            # (B, A, 64)
    strides = [imgsz[0] // r.shape[2] for r in raw]
    anchor_points, stride_tensor = make_anchors([(r.shape[2], r.shape[3]) for r in raw], strides)
    anchor_points, stride_tensor = anchor_points.to(dt), stride_tensor.to(dt)
    bi = batch["batch_idx"].long()
    counts = torch.bincount(bi, minlength=B)
    G = int(counts.max()) if bi.numel() else 0
    tg = torch.zeros(B, G, 5, dtype=dt)
    scale = torch.tensor([imgsz[1], imgsz[0], imgsz[1], imgsz[0]], dtype=dt)
    for b in range(B):
        m = bi == b
        n = int(m.sum())
        if n:
            tg[b, :n, 0] = batch["cls"][m].to(dt).view(-1)
            xywh = batch["bboxes"][m].to(dt)
            tg[b, :n, 1:] = torch.cat((xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, :2] + xywh[:, 2:] / 2), 1) * scale
    gt_labels, gt_bboxes = tg[..., :1], tg[..., 1:]
    mask_gt = gt_bboxes.sum(2, keepdim=True) > 0
    proj = torch.arange(REG_MAX, dtype=dt)
    pd = pred_distri.view(B, -1, 4, REG_MAX).softmax(3).matmul(proj)   # (B, A, 4) grid units
    pred_bboxes = dist2bbox_xyxy(pd, anchor_points)
    tb, ts, fg, _ = task_aligned_assign(pred_scores.detach().sigmoid(), pred_bboxes.detach() * stride_tensor,
                                        anchor_points * stride_tensor, gt_labels, gt_bboxes, mask_gt)
    tss = max(float(ts.sum()), 1.0)
    loss = torch.zeros(3, dtype=dt)
    loss[1] = F.binary_cross_entropy_with_logits(pred_scores, ts.to(dt), reduction="none").sum() / tss
    if fg.any():
        tbg = tb / stride_tensor
        w = ts.sum(-1)[fg][:, None]
        iou = bbox_iou(pred_bboxes[fg], tbg[fg], ciou=True)
        loss[0] = ((1.0 - iou) * w).sum() / tss
        tlrb = bbox2dist(anchor_points.expand(B, -1, -1)[fg], tbg[fg], REG_MAX - 1)
        loss[2] = (dfl_loss(pred_distri[fg].view(-1, REG_MAX), tlrb) * w).sum() / tss
    loss = loss * torch.tensor(list(gains), dtype=dt)
    return loss.sum() * B, loss.detach()


def detection_loss_f64(raw_rows: torch.Tensor, batch: Dict[str, torch.Tensor], hw, nc: int, imgsz: Tuple[int, int],
                       gains=(7.5, 0.5, 1.5)):
    """The loss in float64 on head rows (B, A, 64 + nc) (levels of sizes ``hw`` one after the other): (loss * B, items, d loss * B /
    d rows), all float64.  The oracle's pieces allocate in the default dtype, which is float64 for the length of this call."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        B = raw_rows.shape[0]
        rows = raw_rows.detach().double().clone().requires_grad_(True)
        maps, o = [], 0
        for h, w in hw:
            maps.append(rows[:, o:o + h * w].permute(0, 2, 1).reshape(B, 64 + nc, h, w))
            o += h * w
        loss, items = detection_loss(maps, batch, nc, imgsz, gains)
        loss.backward()
        return loss.detach(), items, rows.grad
    finally:
        torch.set_default_dtype(prev)
