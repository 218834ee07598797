"""Segmentation and detection training losses on the head outputs of the HIP engine.

Stands where ``v8SegmentationLoss`` + ``TaskAlignedAssigner`` + ``BboxLoss`` stand upstream (reached from
/root/reference/BscanBased/yolo_seg_train.py:12).  Inputs are the engine's train-mode outputs -- raw head maps
``(B, A, 64+nc+32)`` fp32 and prototypes ``(B, mh, mw, 32)`` NHWC -- so the autograd graph of this module is only
the loss itself (a few MB of irregular gathers); its gradients w.r.t. those two tensors are what
``TrainEngine.backward`` consumes.  Plain PyTorch tensor ops, device agnostic; no convolution happens here.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

REG_MAX = 16
NM = 32
_EPS = 1e-7


def anchor_grid(imgsz: Tuple[int, int], device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cell centres (x+0.5, y+0.5) in grid units, row-major per level P3,P4,P5, and the stride per anchor."""
    pts, strides = [], []
    for s in (8, 16, 32):
        h, w = imgsz[0] // s, imgsz[1] // s
        ys, xs = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32) + 0.5,
                                torch.arange(w, device=device, dtype=torch.float32) + 0.5, indexing="ij")
        pts.append(torch.stack((xs.reshape(-1), ys.reshape(-1)), 1))
        strides.append(torch.full((h * w, 1), float(s), device=device))
    return torch.cat(pts), torch.cat(strides)


def ciou(b1: torch.Tensor, b2: torch.Tensor, complete: bool = True) -> torch.Tensor:
    """Complete-IoU of xyxy boxes (broadcasting over leading dims); returns (...,)."""
    ax1, ay1, ax2, ay2 = b1.unbind(-1)
    bx1, by1, bx2, by2 = b2.unbind(-1)
    aw, ah = ax2 - ax1, ay2 - ay1 + _EPS
    bw, bh = bx2 - bx1, by2 - by1 + _EPS
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp_min(0)
    ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp_min(0)
    inter = iw * ih
    iou = inter / (aw * ah + bw * bh - inter + _EPS)
    if not complete:
        return iou
    cw = torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)
    chh = torch.maximum(ay2, by2) - torch.minimum(ay1, by1)
    diag2 = cw * cw + chh * chh + _EPS
    centre2 = ((bx1 + bx2 - ax1 - ax2) ** 2 + (by1 + by2 - ay1 - ay2) ** 2) * 0.25
    v = (4.0 / math.pi ** 2) * (torch.atan(bw / bh) - torch.atan(aw / ah)) ** 2
    with torch.no_grad():
        alpha = v / (v - iou + (1.0 + _EPS))
    return iou - (centre2 / diag2 + v * alpha)


@torch.no_grad()
def assign_targets(scores: torch.Tensor, boxes: torch.Tensor, anchors_px: torch.Tensor, gt_cls: torch.Tensor,
                   gt_boxes: torch.Tensor, gt_valid: torch.Tensor, topk: int = 10, alpha: float = 0.5,
                   beta: float = 6.0, eps: float = 1e-9, stable_ties: bool = False):
    """Task-aligned assignment.  scores (B,A,nc) in [0,1]; boxes (B,A,4) xyxy px; anchors_px (A,2);
    gt_cls (B,G) long; gt_boxes (B,G,4) xyxy px; gt_valid (B,G) bool.
    Returns target boxes (B,A,4), target scores (B,A,nc), foreground mask (B,A), assigned GT index (B,A)."""
    B, A, nc = scores.shape
    G = gt_boxes.shape[1]
    if G == 0:
        z = torch.zeros(B, A, dtype=torch.long, device=scores.device)
        return torch.zeros_like(boxes), torch.zeros_like(scores), z.bool(), z
    d = torch.cat((anchors_px[None, None] - gt_boxes[:, :, None, :2], gt_boxes[:, :, None, 2:] - anchors_px[None, None]), -1)
    cand = (d.amin(-1) > eps) & gt_valid[:, :, None]                              # (B,G,A) centre strictly inside
    cls_score = scores.transpose(1, 2).gather(1, gt_cls.clamp(0, nc - 1)[:, :, None].expand(B, G, A))
    overlap = ciou(gt_boxes[:, :, None, :], boxes[:, None, :, :]).clamp_min(0) * cand
    metric = (cls_score * cand).pow(alpha) * overlap.pow(beta)
    top = torch.zeros_like(cand)
    if stable_ties:
        # torch.topk leaves the choice among EQUAL metrics unspecified; it matters when a truth has fewer than ten candidates with a
        # positive metric (zero-metric candidates that make the top ten stay foreground).  This form fixes it the way the device
        # kernels do (csrc/loss_kernels.hip: tal_topk_kernel): candidates before non-candidates, then the lower anchor index.
        key = torch.where(cand, metric, torch.full_like(metric, -1.0))
        top.scatter_(2, key.sort(dim=2, descending=True, stable=True).indices[..., :min(topk, A)], True)
    else:
        top.scatter_(2, metric.topk(min(topk, A), dim=2).indices, True)
    pos = top & cand
    claims = pos.sum(1)                                                          # several GTs -> highest overlap wins
    winner = torch.zeros_like(pos).scatter_(1, overlap.argmax(1, keepdim=True), True)
    pos = torch.where((claims > 1)[:, None, :], winner, pos)
    fg = pos.any(1)
    gt_idx = pos.float().argmax(1)
    bi = torch.arange(B, device=scores.device)[:, None]
    t_boxes = gt_boxes[bi, gt_idx]
    t_cls = gt_cls[bi, gt_idx].clamp(0, nc - 1)
    metric = metric * pos
    norm = (metric * (overlap * pos).amax(2, keepdim=True) / (metric.amax(2, keepdim=True) + eps)).amax(1)
    t_scores = F.one_hot(t_cls, nc).to(scores.dtype) * (fg * norm)[..., None]
    return t_boxes, t_scores, fg, gt_idx


@torch.no_grad()
def _assign_targets_device(scores, boxes, anchors_px, gt_cls, gt_boxes, gt_valid):
    """assign_targets on the device as two kernels (``m355_tal_assign_launch``): same outputs, ties of the top-10 broken towards the
    lower anchor index."""
    from ._capi import check, lib
    B, A, nc = scores.shape
    G = gt_boxes.shape[1]
    dev = scores.device
    sc, bx = scores.float().contiguous(), boxes.float().contiguous()
    t_boxes = torch.zeros((B, A, 4), dtype=torch.float32, device=dev)
    t_scores = torch.zeros((B, A, nc), dtype=torch.float32, device=dev)
    fg = torch.zeros((B, A), dtype=torch.uint8, device=dev)
    gt_idx = torch.zeros((B, A), dtype=torch.int64, device=dev)
    ws = torch.empty(B * G * 10 * 3, dtype=torch.int32, device=dev)
    # the converted copies stay referenced until the launch is queued: a temporary inside the argument list is freed (and its block
    # handed to the next conversion) as soon as its data_ptr() has been taken
    anc, gc, gb, gv = (anchors_px.float().contiguous(), gt_cls.to(torch.int32).contiguous(), gt_boxes.float().contiguous(),
                       gt_valid.to(torch.uint8).contiguous())
    check(lib.m355_tal_assign_launch(sc.data_ptr(), bx.data_ptr(), anc.data_ptr(), gc.data_ptr(), gb.data_ptr(), gv.data_ptr(), B, A, G, nc,
                                     ws.data_ptr(), t_boxes.data_ptr(), t_scores.data_ptr(), fg.data_ptr(), gt_idx.data_ptr(), _stream()))
    return t_boxes, t_scores, fg.bool(), gt_idx


_CONST_CACHE: Dict = {}


def _consts(imgsz: Tuple[int, int], mh: int, mw: int, dev, gains: Tuple[float, float, float]):
    """Small constant tensors of the loss, built once per (image size, map size, device, gains): creating them inside the loss
    would be host-to-device copies on every step."""
    key = (tuple(imgsz), mh, mw, str(dev), tuple(float(g) for g in gains))
    c = _CONST_CACHE.get(key)
    if c is None:
        anchors, strides = anchor_grid(imgsz, dev)
        c = dict(anchors=anchors, strides=strides, anchors_px=anchors * strides, strides_flat=strides.reshape(-1).contiguous(), bins=torch.arange(REG_MAX, device=dev, dtype=torch.float32),
                 wh=torch.tensor([imgsz[1], imgsz[0], imgsz[1], imgsz[0]], device=dev, dtype=torch.float32),
                 mwh=torch.tensor([mw, mh, mw, mh], device=dev, dtype=torch.float32),
                 cols=torch.arange(mw, device=dev, dtype=torch.float32).repeat(mh)[None, None, :],
                 rows=torch.arange(mh, device=dev, dtype=torch.float32).repeat_interleave(mw)[None, None, :],
                 gains=torch.tensor([gains[0], gains[0], gains[1], gains[2]], device=dev))
        _CONST_CACHE[key] = c
    return c


def pad_targets(batch: Dict[str, torch.Tensor], B: int, imgsz: Tuple[int, int], dev):
    """Labels (batch_idx, cls, bboxes xywh normalised) -> padded per-image tensors gt_cls (B,G), gt_boxes (B,G,4) xyxy px,
    gt_valid (B,G).  The ONE host synchronisation of the loss is here (G = most instances in an image)."""
    bidx = batch["batch_idx"].to(dev).long()
    n_per = torch.bincount(bidx, minlength=B) if bidx.numel() else torch.zeros(B, dtype=torch.long, device=dev)
    G = int(n_per.max()) if bidx.numel() else 0
    gt_cls = torch.zeros(B, G, dtype=torch.long, device=dev)
    gt_boxes = torch.zeros(B, G, 4, device=dev)
    gt_valid = torch.zeros(B, G, dtype=torch.bool, device=dev)
    if G:
        order = torch.argsort(bidx, stable=True)
        slot = torch.arange(bidx.numel(), device=dev) - torch.cumsum(n_per, 0)[bidx[order]] + n_per[bidx[order]]
        xywh = batch["bboxes"].to(dev).float()[order]
        scale = torch.tensor([imgsz[1], imgsz[0], imgsz[1], imgsz[0]], device=dev, dtype=torch.float32)
        xyxy = torch.cat((xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, :2] + xywh[:, 2:] / 2), 1) * scale
        gt_boxes[bidx[order], slot] = xyxy
        gt_cls[bidx[order], slot] = batch["cls"].to(dev).long().view(-1)[order]
        gt_valid[bidx[order], slot] = xyxy.sum(1) > 0
    return gt_cls, gt_boxes, gt_valid


def segmentation_loss(raw: torch.Tensor, protos: torch.Tensor, batch: Dict[str, torch.Tensor], nc: int,
                      imgsz: Tuple[int, int], box_gain: float = 7.5, cls_gain: float = 0.5, dfl_gain: float = 1.5):
    """raw (B,A,64+nc+32); protos (B,mh,mw,32).  batch: batch_idx (N,), cls (N,), bboxes (N,4) xywh normalised to the
    network input, masks (B,mh,mw) overlap-encoded (pixel value = 1 + index of the instance within its image,
    instances sorted by area descending).  Returns (loss * B, detached items [box, seg, cls, dfl])."""
    gt_cls, gt_boxes, gt_valid = pad_targets(batch, raw.shape[0], imgsz, raw.device)
    return loss_core(raw, protos, gt_cls, gt_boxes, gt_valid, batch["masks"].to(raw.device), nc, imgsz, (box_gain, cls_gain, dfl_gain))


def _loss_kernels_enabled() -> bool:
    """The HIP forms of the loss terms (device tensors only); M355_NO_LOSS_KERNELS=1 keeps the torch-op forms for A/B runs."""
    import os
    return os.environ.get("M355_NO_LOSS_KERNELS") != "1"


def _stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _decode_all(raw: torch.Tensor, anchors: torch.Tensor, strides_flat: torch.Tensor, nc: int):
    """raw (B,A,64+nc+nm) fp32 -> xyxy boxes in pixels (B,A,4) and sigmoid class scores (B,A,nc) of every anchor."""
    from ._capi import check, lib
    B, A, rw = raw.shape
    raw = raw.float().contiguous()
    boxes = torch.empty((B, A, 4), dtype=torch.float32, device=raw.device)
    scores = torch.empty((B, A, nc), dtype=torch.float32, device=raw.device)
    check(lib.m355_dfl_decode_launch(raw.data_ptr(), B * A, A, rw, nc, anchors.data_ptr(), strides_flat.data_ptr(), boxes.data_ptr(),
                                     scores.data_ptr(), _stream()))
    return boxes, scores


class _BoxTerm(torch.autograd.Function):
    """(sum_s w_s (1 - CIoU_s), sum_s w_s DFL_s) over the foreground slots with d / d logits from the same device pass
    (``m355_box_loss_launch``).  logits (B,K,4,16); anchors (B,K,2) and targets (B,K,4) in grid units; w (B,K)."""

    @staticmethod
    def forward(ctx, logits, anchors, targets, w):
        from ._capi import check, lib
        n = w.numel()
        lg = logits.detach().float().contiguous()
        an, tg, wc = anchors.float().contiguous(), targets.float().contiguous(), w.float().contiguous()
        terms = torch.empty((2, n), dtype=torch.float32, device=lg.device)
        grads = torch.empty((2, n, 4 * REG_MAX), dtype=torch.float32, device=lg.device)
        check(lib.m355_box_loss_launch(lg.data_ptr(), an.data_ptr(), tg.data_ptr(), wc.data_ptr(), n, terms[0].data_ptr(),
                                       terms[1].data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), _stream()))
        ctx.save_for_backward(grads)
        ctx.shape = logits.shape
        sums = terms.sum(1)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g_box, g_dfl):
        (grads,) = ctx.saved_tensors
        g = grads[0] * g_box + grads[1] * g_dfl
        return g.view(ctx.shape), None, None, None


class _MaskTerm(torch.autograd.Function):
    """sum_{b,k} w[b,k] * mean_p(BCE(coef[b,k] . proto[b,p], mask[b,p] == inst[b,k]) inside box[b,k]) (``m355_mask_loss_launch``).
    The gradients need only forward values: d / d coef comes out of the forward pass over the boxes with the value; the dense
    d / d protos is produced in ``backward``, already scaled by the incoming gradient.  coef (B,K,32) fp32; protos
    (B,mh,mw,32) fp16 or fp32; masks (B,mh,mw) overlap-encoded; inst (B,K); boxes (B,K,4) prototype px; w (B,K), 0 = skip."""

    @staticmethod
    def forward(ctx, coef, protos, masks, inst, boxes, w):
        from ._capi import check, lib
        B, K, _ = coef.shape
        mh, mw = protos.shape[1:3]
        assert protos.shape[3] == NM and protos.dtype in (torch.float16, torch.float32)
        coef_c, protos_c = coef.detach().float().contiguous(), protos.detach().contiguous()
        masks_i, inst_i = masks.to(torch.int32).contiguous(), inst.to(torch.int32).contiguous()
        boxes_c, w_c = boxes.float().contiguous(), w.float().contiguous()
        slot_sum = torch.empty((B, K), dtype=torch.float32, device=coef.device)
        d_coef = torch.empty((B, K, NM), dtype=torch.float32, device=coef.device)
        f16 = 1 if protos.dtype == torch.float16 else 0
        check(lib.m355_mask_loss_launch(coef_c.data_ptr(), protos_c.data_ptr(), f16, masks_i.data_ptr(), inst_i.data_ptr(),
                                        boxes_c.data_ptr(), w_c.data_ptr(), B, K, mh, mw, slot_sum.data_ptr(), d_coef.data_ptr(), None, 0,
                                        None, _stream()))
        ctx.save_for_backward(coef_c, protos_c, masks_i, inst_i, boxes_c, w_c, d_coef)
        return (slot_sum * w_c).sum() / float(mh * mw)

    @staticmethod
    def backward(ctx, g):
        # the dense prototype gradient is produced here, already multiplied by the incoming gradient (read from the device by the
        # kernel) and in the prototypes' dtype: one write of the map instead of fp32 store + multiply + cast
        from ._capi import check, lib
        coef_c, protos_c, masks_i, inst_i, boxes_c, w_c, d_coef = ctx.saved_tensors
        B, K, _ = coef_c.shape
        mh, mw = protos_c.shape[1:3]
        f16 = 1 if protos_c.dtype == torch.float16 else 0
        gs = g.detach().float().contiguous()
        d_protos = torch.empty_like(protos_c)
        check(lib.m355_mask_loss_launch(coef_c.data_ptr(), protos_c.data_ptr(), f16, masks_i.data_ptr(), inst_i.data_ptr(),
                                        boxes_c.data_ptr(), w_c.data_ptr(), B, K, mh, mw, None, None, d_protos.data_ptr(), f16,
                                        gs.data_ptr(), _stream()))
        return d_coef * g, d_protos, None, None, None, None


def _assign_all(raw, logits_box, logits_cls, gt_cls, gt_boxes, gt_valid, nc: int, k: Dict, use_kernels: bool):
    """Decoded boxes and class scores of ALL anchors (no gradient) and their task-aligned assignment: target boxes (B,A,4) px,
    target scores (B,A,nc), foreground mask (B,A), assigned GT index (B,A).  Shared by the segmentation and the detection loss."""
    B, A, _ = raw.shape
    G = gt_boxes.shape[1]
    anchors, strides, bins = k["anchors"], k["strides"], k["bins"]
    # Decoded boxes of ALL anchors feed only the assignment (no gradient).  The box / DFL / mask terms are evaluated on
    # the <= 10 G foreground slots per image: every other anchor has weight zero, and carrying the (B, A, 4, 16) logits
    # through softmax, log-softmax, two gathers and their backward passes cost ~2 ms of a 5.3 ms loss for 0.2 % of the rows.
    # expectation over the 16 bins as multiply + reduce: `softmax @ bins` runs as a (B*A*4) x 16 rocBLAS gemv, 1.4 ms
    with torch.no_grad():
        if use_kernels and raw.shape[2] <= 255:            # one pass over the raw rows (csrc/loss_kernels.hip; 64 rows in LDS)
            boxes_px, scores = _decode_all(raw.detach(), anchors, k["strides_flat"], nc)
        else:
            ltrb = (logits_box.view(B, A, 4, REG_MAX).softmax(3) * bins).sum(3)
            boxes_px = torch.cat((anchors - ltrb[..., :2], anchors + ltrb[..., 2:]), -1) * strides       # pixels
            scores = logits_cls.detach().sigmoid()
    if use_kernels and G > 0 and A <= 18000 and G <= 900:        # two launches instead of ~40 (csrc/loss_kernels.hip: tal_topk / tal_resolve)
        return _assign_targets_device(scores, boxes_px, k["anchors_px"], gt_cls, gt_boxes, gt_valid)
    return assign_targets(scores, boxes_px, k["anchors_px"], gt_cls, gt_boxes, gt_valid)


def _fg_slots(fg: torch.Tensor, w: torch.Tensor, G: int):
    """Every GT claims at most 10 anchors, so K = 10 G slots per image hold all foreground anchors: (K, anchor index (B,K), occupied
    (B,K), slot weight (B,K), 0 on an empty slot)."""
    K = min(10 * G, fg.shape[1])
    val, ai = fg.float().topk(K, dim=1)
    valid = val > 0                                                              # (B,K)
    return K, ai, valid, w.gather(1, ai) * valid


def _box_dfl_terms(logits_box, t_boxes, ai, ws, denom, k: Dict, use_kernels: bool):
    """(box loss, DFL loss) over the foreground slots `ai` with weights `ws`, both divided by `denom`."""
    B, K = ai.shape
    anchors, strides, bins = k["anchors"], k["strides"], k["bins"]
    anc = anchors[ai]                                                            # (B,K,2) grid units
    tb = (t_boxes / strides).gather(1, ai[..., None].expand(B, K, 4))
    lb = logits_box.gather(1, ai[..., None].expand(B, K, 4 * REG_MAX)).view(B, K, 4, REG_MAX)
    if use_kernels:                                    # value and gradient of both terms in one pass, one thread per slot
        box_sum, dfl_sum = _BoxTerm.apply(lb, anc, tb.detach(), ws.detach())
        return box_sum / denom, dfl_sum / denom
    ltrb_s = (lb.softmax(3) * bins).sum(3)
    pred_s = torch.cat((anc - ltrb_s[..., :2], anc + ltrb_s[..., 2:]), -1)
    loss_box = ((1.0 - ciou(pred_s, tb)) * ws).sum() / denom
    dist = torch.cat((anc - tb[..., :2], tb[..., 2:] - anc), -1).clamp(0, REG_MAX - 1 - 0.01)       # (B,K,4)
    lo = dist.long()
    logp = lb.log_softmax(3)
    ce_lo = -logp.gather(3, lo[..., None]).squeeze(3)
    ce_hi = -logp.gather(3, lo[..., None] + 1).squeeze(3)
    loss_dfl = (((ce_lo * (lo + 1 - dist) + ce_hi * (dist - lo)).mean(2)) * ws).sum() / denom
    return loss_box, loss_dfl


def loss_core(raw: torch.Tensor, protos: torch.Tensor, gt_cls: torch.Tensor, gt_boxes: torch.Tensor, gt_valid: torch.Tensor,
              masks: torch.Tensor, nc: int, imgsz: Tuple[int, int], gains: Tuple[float, float, float] = (7.5, 0.5, 1.5)):
    """The loss on padded targets: fixed shapes for a given G, no host synchronisation, no host-to-device copy."""
    dev = raw.device
    B, A, _ = raw.shape
    mh, mw = protos.shape[1:3]
    G = gt_boxes.shape[1]
    k = _consts(imgsz, mh, mw, dev, gains)
    logits_box, logits_cls, coefs = raw.split((4 * REG_MAX, nc, NM), 2)
    use_kernels = raw.is_cuda and _loss_kernels_enabled()
    t_boxes, t_scores, fg, gt_idx = _assign_all(raw, logits_box, logits_cls, gt_cls, gt_boxes, gt_valid, nc, k, use_kernels)
    # Everything below runs over ALL anchors / a fixed number of slots per image with zero weights for the background,
    # so the step has no data-dependent shapes and no host synchronisation after the one that sized the GT padding.
    denom = t_scores.sum().clamp_min(1.0)
    w = t_scores.sum(-1)                                                            # (B,A), 0 off the foreground
    loss_cls = F.binary_cross_entropy_with_logits(logits_cls, t_scores, reduction="sum") / denom
    if G == 0:
        zero = (protos * 0).sum() + (coefs * 0).sum() + (logits_box * 0).sum()
        items = torch.stack((zero, zero, loss_cls, zero))
    else:
        K, ai, valid, ws = _fg_slots(fg, w, G)
        loss_box, loss_dfl = _box_dfl_terms(logits_box, t_boxes, ai, ws, denom, k, use_kernels)
        # masks: BCE(coef . proto, gt mask of the assigned instance) inside the target box, mean over the map, divided by
        # the normalised box area; one batched GEMM (B,K,32) x (B,32,mh*mw).
        nb = t_boxes.gather(1, ai[..., None].expand(B, K, 4)) / k["wh"]
        area = ((nb[..., 2] - nb[..., 0]) * (nb[..., 3] - nb[..., 1])).masked_fill(~valid, 1.0)
        mbox = nb * k["mwh"]                                                                              # (B,K,4) prototype px
        ck = coefs.gather(1, ai[..., None].expand(B, K, NM))
        inst = gt_idx.gather(1, ai) + 1
        nfg = fg.sum().clamp_min(1)
        if use_kernels:
            # one HIP pass over the boxes' pixels gives the term and both gradients (csrc/loss_kernels.hip)
            loss_seg = _MaskTerm.apply(ck, protos, masks, inst, mbox.detach(), (valid / (area * nfg)).detach())
        else:
            mb = mbox[..., None]                                                                          # (B,K,4,1)
            cols, rows = k["cols"], k["rows"]
            inside = (cols >= mb[:, :, 0]) & (cols < mb[:, :, 2]) & (rows >= mb[:, :, 1]) & (rows < mb[:, :, 3])
            pred = torch.bmm(ck, protos.float().reshape(B, mh * mw, NM).transpose(1, 2))                # (B,K,HW)
            gt = (masks.reshape(B, 1, mh * mw) == inst[..., None]).to(pred.dtype)
            bce = F.binary_cross_entropy_with_logits(pred, gt, reduction="none")
            per_slot = (bce * inside).mean(2) / area
            loss_seg = (per_slot * valid).sum() / nfg
        items = torch.stack((loss_box, loss_seg, loss_cls, loss_dfl))
    items = items * k["gains"]
    return items.sum() * B, items.detach()


def cls_bce_device(raw: torch.Tensor, t_scores: torch.Tensor, s: torch.Tensor, d_raw: torch.Tensor) -> torch.Tensor:
    """The class term of the detection loss on the device, value and gradient in one pass (``m355_cls_bce_launch``): reads the
    class logits in place in the raw rows (B,A,rw) at column 64, writes (sigmoid(x) - t) * s into the same columns of ``d_raw`` and
    returns the sum of BCEWithLogits(x, t) as a device scalar.  ``s`` is a device scalar too, so nothing here waits for the device."""
    from ._capi import check, lib
    B, A, rw = raw.shape
    nc = t_scores.shape[2]
    assert raw.dtype == torch.float32 and raw.is_contiguous() and d_raw.dtype == torch.float32 and d_raw.is_contiguous()
    assert d_raw.shape == raw.shape and rw >= 4 * REG_MAX + nc
    tg = t_scores.float().contiguous()
    sc = s.detach().float().reshape(1).contiguous()
    out = torch.empty(int(lib.m355_cls_bce_workspace_floats()), dtype=torch.float32, device=raw.device)
    check(lib.m355_cls_bce_launch(raw.data_ptr(), rw, tg.data_ptr(), B * A, nc, sc.data_ptr(), d_raw.data_ptr(), out.data_ptr(),
                                  _stream()))
    return out[0]


def det_loss_core(raw: torch.Tensor, gt_cls: torch.Tensor, gt_boxes: torch.Tensor, gt_valid: torch.Tensor, nc: int,
                  imgsz: Tuple[int, int], gains: Tuple[float, float, float] = (7.5, 0.5, 1.5), scale: float = 1.0):
    """The detection loss (upstream v8DetectionLoss) on padded targets with its gradient: raw (B,A,64+nc) -> (detached items (3,)
    [box, cls, dfl] with the gains applied, d(scale * B * sum(items)) / d raw).  Assignment, box and DFL terms are the
    segmentation loss's own (``_assign_all`` / ``_fg_slots`` / ``_box_dfl_terms``).  On the device the class term is one HIP pass
    that writes its gradient straight into the class columns of d_raw (``cls_bce_device``); on CPU tensors (and with
    M355_NO_LOSS_KERNELS=1) it is torch's BCE under autograd."""
    dev = raw.device
    B, A, rw = raw.shape
    assert rw == 4 * REG_MAX + nc, f"raw rows of {rw} columns for a detection head of {4 * REG_MAX + nc}"
    G = gt_boxes.shape[1]
    k = _consts(imgsz, 0, 0, dev, gains)
    use_kernels = raw.is_cuda and _loss_kernels_enabled()
    r = raw.detach().float().contiguous().requires_grad_(True)   # shares the engine's buffer: the loss never writes to its inputs
    logits_box, logits_cls = r.split((4 * REG_MAX, nc), 2)
    t_boxes, t_scores, fg, _ = _assign_all(r, logits_box, logits_cls, gt_cls, gt_boxes, gt_valid, nc, k, use_kernels)
    denom = t_scores.sum().clamp_min(1.0)
    terms = []                                                   # (gain, term with a gradient path to r)
    zero = torch.zeros((), device=dev)
    loss_box = loss_dfl = zero
    if G > 0:
        _, ai, _, ws = _fg_slots(fg, t_scores.sum(-1), G)
        loss_box, loss_dfl = _box_dfl_terms(logits_box, t_boxes, ai, ws, denom, k, use_kernels)
        terms += [(gains[0], loss_box), (gains[2], loss_dfl)]
    if not use_kernels:
        loss_cls = F.binary_cross_entropy_with_logits(logits_cls, t_scores, reduction="sum") / denom
        terms.append((gains[1], loss_cls))
    if terms:
        (sum(g * t for g, t in terms) * (B * scale)).backward()
    d_raw = r.grad.contiguous() if r.grad is not None else torch.zeros_like(r)
    if use_kernels:
        loss_cls = cls_bce_device(r.detach(), t_scores, (gains[1] * B * scale) / denom, d_raw) / denom
    items = torch.stack((loss_box.detach() * gains[0], loss_cls.detach() * gains[1], loss_dfl.detach() * gains[2]))
    return items, d_raw


class SegCriterion:
    """The criterion of the training loop: loss + its backward on the engine's train-mode outputs (stands where
    ``criterion(preds, batch)`` + ``loss.backward()`` stand upstream, /root/reference/BscanBased/yolo_seg_train.py:12).

    ``prepare(batch, B, dev)`` pads the targets BEFORE the forward pass is enqueued (the loss's one host synchronisation);
    ``__call__(raw, protos, prepared_or_batch, scale)`` -> (items (4,) [box, seg, cls, dfl], d(scale * loss)/d raw,
    d(scale * loss)/d protos).  On device tensors the box / DFL / mask terms and the all-anchor decode are HIP kernels
    (``csrc/loss_kernels.hip``) wrapped as autograd Functions; the assignment and the class BCE are torch ops.

    Rounds 1-2 also carried a hipGraph capture of loss + backward (``GraphedSegLoss``, opt-in).  Its one run at batch 64 @640
    ended in a GPU hardware exception (HSA_STATUS_ERROR_EXCEPTION 0x1016) during the replays and the cause could not be
    established from that one failure; since the host no longer limits the loss (its launches are enqueued while the device
    is still in the forward convolutions) the capture had nothing left to gain, so it was deleted in round 3 rather than
    shipped as known-faulting code."""

    def __init__(self, nc: int, imgsz: Tuple[int, int], gains: Tuple[float, float, float] = (7.5, 0.5, 1.5)):
        self.nc, self.imgsz, self.gains = nc, tuple(imgsz), tuple(gains)

    def prepare(self, batch: Dict[str, torch.Tensor], B: int, dev) -> Dict[str, torch.Tensor]:
        """The padded targets of a batch, to be made BEFORE the forward pass is enqueued and handed to ``__call__`` in place of
        the batch.  ``pad_targets`` holds the loss's one host synchronisation (the padded width G): on host labels it runs on
        the CPU and only the three padded tensors are uploaded; on device labels it waits for an idle stream instead of for
        the whole forward pass -- either way the host can enqueue the small kernels of the loss while the device is still
        in the forward convolutions."""
        dev = torch.device(dev)
        gt = pad_targets(batch, B, self.imgsz, batch["batch_idx"].device)
        return {"_gt": tuple(t.to(dev, non_blocking=True) for t in gt), "masks": batch["masks"].to(dev, non_blocking=True)}

    def __call__(self, raw: torch.Tensor, protos: torch.Tensor, batch: Dict[str, torch.Tensor], scale: float = 1.0):
        dev = raw.device
        gt = batch["_gt"] if "_gt" in batch else pad_targets(batch, raw.shape[0], self.imgsz, dev)
        masks = batch["masks"].to(dev)
        r = raw.detach().requires_grad_(True)             # shares the engine's buffer: the loss never writes to its inputs
        # on the device the prototypes stay fp16 (the engine's own buffer): the mask kernel reads them as they are and the
        # gradient comes back in the dtype TrainEngine.backward stores anyway
        p = (protos.detach() if protos.is_cuda else protos.detach().float()).requires_grad_(True)
        loss, items = loss_core(r, p, *gt, masks, self.nc, self.imgsz, self.gains)
        (loss * scale).backward()
        return items, r.grad, p.grad


class DetCriterion:
    """The criterion of a box-only training run (upstream ``v8DetectionLoss``; the reference's BscanBased/yolo/yolo_bbox_retrain.py
    trains against it): same protocol as ``SegCriterion`` without the mask term.  ``prepare(batch, B, dev)`` pads the targets
    before the forward pass is enqueued; ``__call__(raw, protos, prepared_or_batch, scale)`` -> (items (3,) [box, cls, dfl],
    d(scale * loss)/d raw, None); ``protos`` is None for a detection head and is ignored."""

    def __init__(self, nc: int, imgsz: Tuple[int, int], gains: Tuple[float, float, float] = (7.5, 0.5, 1.5)):
        self.nc, self.imgsz, self.gains = nc, tuple(imgsz), tuple(gains)

    def prepare(self, batch: Dict[str, torch.Tensor], B: int, dev) -> Dict[str, torch.Tensor]:
        dev = torch.device(dev)
        gt = pad_targets(batch, B, self.imgsz, batch["batch_idx"].device)
        return {"_gt": tuple(t.to(dev, non_blocking=True) for t in gt)}

    def __call__(self, raw: torch.Tensor, protos, batch: Dict[str, torch.Tensor], scale: float = 1.0):
        gt = batch["_gt"] if "_gt" in batch else pad_targets(batch, raw.shape[0], self.imgsz, raw.device)
        items, d_raw = det_loss_core(raw, *gt, self.nc, self.imgsz, self.gains, scale)
        return items, d_raw, None
