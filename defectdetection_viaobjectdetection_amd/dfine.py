"""D-FINE decoder hot ops on the HIP library.

Same names, argument meaning and error behaviour as the functions /root/reference/D-Fine/temporal_dfine.py:11-15,
160-181 imports from / reaches through ``transformers.models.d_fine.modeling_d_fine`` (5.15.0):
``multi_scale_deformable_attention_v2`` (:150-221), ``weighting_function`` (:1091-1112), ``distance2bbox``
(:1115-1137), ``DFineIntegral.forward`` (:756-778).  Tensors are CUDA fp32; there is no CPU path (the C-ABI call
fails loudly without a gfx950 device).  The three kernel-backed ops are differentiable (torch.autograd.Function over the
HIP backward entries, bitwise-reproducible gradients); with nothing to differentiate they take the plain forward path.
A maintainer binds them with
``modeling_d_fine.multi_scale_deformable_attention_v2 = dfine.multi_scale_deformable_attention_v2`` (the attention
module keeps a reference in ``self.ms_deformable_attn_core``, :244) — see INTEGRATION.md.

``hungarian_match`` / ``matcher_forward`` are the loss's Hungarian matcher (``RTDetrHungarianMatcher.forward``,
transformers/loss/loss_rt_detr.py:68-120) in one launch: cost matrix and assignment on the device, no trip to the host.

``detection_loss`` / ``criterion_forward`` are what those indices feed: loss_vfl, loss_bbox, loss_giou, loss_fgl and loss_ddf of a
decoder output (``RTDetrLoss.loss_labels_vfl`` / ``loss_boxes``, ``DFineLoss.loss_local``) and their gradients as fused kernels,
two launches forward and one backward per output, without a synchronisation; on CPU tensors the same expressions in torch ops.

``topk_detections`` / ``post_process_detections`` / ``post_process_object_detection`` are the inference tail
(``RTDetrImageProcessor.post_process_object_detection``, models/rt_detr/image_processing_rt_detr.py:482-552): sigmoid, top-K, labels,
scaled xyxy boxes and the threshold in one launch for a whole sequence of frames, with one read-back of the kept counts.

``preprocess_images`` / ``resize_tables`` / ``preprocess_images_torch`` / ``bind_processor`` are the stage in front of the model
(``RTDetrImageProcessorPil.preprocess`` with its defaults, models/rt_detr/image_processing_pil_rt_detr.py:380-505): Pillow's 8-bit
BILINEAR resize to a fixed size and the rescale for a whole sequence of decoded frames of mixed sizes, one uint8 upload and two
launches (csrc/dfine_preprocess.hip), bit for bit the processor's pixel_values; the host path builds the same bytes in numpy.

``self_attention`` / ``add_layer_norm`` / ``relu_dropout`` / ``encoder_layer_forward`` / ``bind_encoder`` are the temporal
encoder the D-FINE trainers train (``nn.TransformerEncoderLayer``, post-norm, ReLU, head dim 32) between its torch GEMMs:
attention core with online softmax on the packed in-projection output, LayerNorm(x + dropout(y)) and dropout(relu(h)), each
with a HIP backward, and a counter-based dropout mask that the backward recomputes (``dropout_keep_mask`` shows it).

``gru_recurrence`` / ``gru_forward`` / ``bind_gru`` / ``gru_status`` are the context GRU of the improved trainer
(``nn.GRU(256, 256, batch_first=True, bidirectional=True)`` on one sequence of T * Q steps): the input projection is one torch
GEMM, the serial chain of both directions one persistent launch forward and one backward (csrc/dfine_gru.hip).

``gate_layer_norm`` / ``add_layer_norm(clamp=...)`` / ``lqe_statistics`` / ``decoder_layer_forward`` / ``lqe_forward`` /
``bind_decoder`` are the decoder layers every trainer trains (``DFineDecoderLayer``, ``DFineLQE``) between their torch GEMMs: the
self-attention core above on a packed q | k | v projection, the fused deformable attention, DFineGate behind its Linear,
LayerNorm(clamp(x + y)) and the LQE's softmax / top-k / mean, each one launch forward with a HIP backward (csrc/dfine_decoder.hip; the row LayerNorms of both layer kinds: csrc/dfine_rowln.hip).

``query_pos_hidden`` / ``refine_reference`` / ``refine_boxes`` / ``decoder_forward`` / ``bind_decoder_loop`` are the decoder's own
loop around those layers (``DFineDecoder.forward``, :1184-1293), six times per call: the K = 4 Linear + ReLU of ``query_pos_head``,
inverse_sigmoid + sigmoid at layer 0, and the corner accumulation + integral + distance2bbox of every layer with contiguous
16-byte accesses, each one launch forward and one backward (csrc/dfine_loop.hip), with W(n) cached on the instance; CPU tensors
take the same expressions in torch ops (``*_torch``).

``select_queries`` / ``select_queries_torch`` / ``model_forward`` / ``bind_model`` are the encoder query selection every call of
``DFineModel.forward`` makes between the hybrid encoder and the decoder (:1804-1828): row max of the class logits, top-k, the
gathers of the coordinate logits, class logits and memory, and the sigmoid, two launches forward and one backward
(csrc/dfine_select.hip on the block-wide selection of csrc/topk_select.h, which the post-processing shares), with a stated order
among equal scores (NaN first, descending, an exact tie to the lowest token) where ``torch.topk`` promises none.

``maps_to_tokens`` / ``tokens_to_maps`` / ``gelu`` / ``aifi_forward`` / ``bind_aifi`` / ``bind_model(assembly=...)`` / ``bind_all``
are the hybrid encoder's AIFI layer (``DFineAIFILayer``, ``DFineEncoderLayer``, :542-610, :699-753) between its torch GEMMs and the
memory assembly of ``DFineModel.forward`` (:1750-1797): NCHW maps to token rows for all levels in one launch, with ``tokens + pos``
or ``valid_mask * tokens`` from the same read, its adjoint, and the erf GELU with a backward from the saved input
(csrc/dfine_layout.hip); the layer's training clamp is unconditional, so nothing between the backbone and the loss synchronises.

``temporal_fuse`` / ``guard_logits`` / ``decode_boxes(guard=True)`` / ``noobject_loss`` / ``consistency_loss`` / ``temporal_head``
are the trainers' own stage between the temporal encoder / context GRU and the loss or the post-processing
(temp_dfine_over.py:188-285, temp_dfine_over_improved.py:219-350): the softmax over the frame axis and the fusion, the anomaly
scores and the clamp / nan_to_num of the class logits, the nan_to_num chain around the box decode, the cross-entropy of every
frame against "no object" and the frame-to-frame consistency loss, each one launch forward and one backward
(csrc/dfine_temporal.hip; the guarded decode is an instance of the decode kernels), with torch's gradients at the guards; CPU
tensors take the same expressions in torch ops (``*_torch``).

``clip_grad_norm_`` / ``bind_optimizer`` are the three lines every trainer ends its step with (``loss.backward()``,
``torch.nn.utils.clip_grad_norm_(params, 1.0)``, ``optimizer.step()`` of ``torch.optim.Adam`` / ``AdamW``): the squared norm of all
gradients, the clip and the update as multi-tensor launches over a device table with one row per tensor (csrc/dfine_optim.hip),
a number of launches that does not depend on the number of tensors, no synchronisation, the optimizer's state in torch's own
layout; anything outside the kernels' domain runs torch's own function.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from collections.abc import Mapping
from operator import itemgetter
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from ._capi import (DFINE_OPTIM_ADAM, DFINE_OPTIM_ADAMW, DFINE_OPTIM_CHUNK, DFINE_OPTIM_MAX_TENSORS, DFINE_PRE_MAX_H,
                    DFINE_PRE_MAX_TAPS, DFINE_PRE_MAX_W, DfineOptimRow, DfinePreAxis, DfinePreImage, check, lib)

_raise_on_error = check   # for hungarian_match, whose keyword `check` is upstream-facing


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor: the D-FINE ops have no CPU fallback")
    return t.to(torch.float32).contiguous()


def multi_scale_deformable_attention_v2(value: torch.Tensor, value_spatial_shapes, sampling_locations: torch.Tensor,
                                        attention_weights: torch.Tensor, num_points_list: List[int],
                                        method: str = "default") -> torch.Tensor:
    """value (B, S, heads, 32); value_spatial_shapes [(h, w)] per level (list or tensor); sampling_locations
    (B, Q, heads, 1, P, 2) or (B, Q, heads, P, 2); attention_weights (B, Q, heads, P).  Returns (B, Q, heads * 32)."""
    if method not in ("default", "discrete"):
        raise ValueError(f"unknown method {method!r}")   # the reference leaves sampling_grids undefined (NameError)
    B, S, H, D = value.shape
    loc = sampling_locations
    if loc.dim() == 6:          # the attention module passes (B, Q, heads, 1, P, 2) when reference points are 4-d
        loc = loc.reshape(loc.shape[0], loc.shape[1], loc.shape[2], -1, 2)
    Q, P = loc.shape[1], loc.shape[3]
    shapes = [(int(h), int(w)) for h, w in (value_spatial_shapes.tolist() if torch.is_tensor(value_spatial_shapes)
                                            else value_spatial_shapes)]
    if sum(h * w for h, w in shapes) != S:
        raise ValueError("spatial shapes do not add up to the value sequence length")
    if sum(num_points_list) != P or len(num_points_list) != len(shapes):
        raise ValueError("num_points_list must have one entry per level and add up to the number of points")
    if _wants_grad(value, loc, attention_weights):
        return _MsdaCore.apply(value, loc, attention_weights, shapes, [int(n) for n in num_points_list], method == "discrete")
    return _msda_forward(_f32c(value, "value"), _f32c(loc, "sampling_locations"), _f32c(attention_weights, "attention_weights"),
                         shapes, num_points_list, method == "discrete")


def _wants_grad(*tensors: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tables(shapes, num_points_list):
    sh = (C.c_int32 * (2 * len(shapes)))(*[v for hw in shapes for v in hw])
    pp = (C.c_int32 * len(shapes))(*[int(n) for n in num_points_list])
    return sh, pp


def _msda_forward(value, loc, attn, shapes, num_points_list, discrete: bool) -> torch.Tensor:
    """contiguous fp32 CUDA tensors -> (B, Q, heads * 32)"""
    B, S, H, D = value.shape
    Q, P = loc.shape[1], loc.shape[3]
    out = torch.empty((B, Q, H * D), dtype=torch.float32, device=value.device)
    sh, pp = _tables(shapes, num_points_list)
    check(lib.m355_msda_forward(_ptr(value), B, S, H, D, sh, len(shapes), _ptr(loc), _ptr(attn), pp, Q, P, int(discrete),
                                _ptr(out), _stream()))
    return out


def _backward_workspace(B, Q, H, P, device) -> torch.Tensor:
    return torch.empty(int(lib.m355_msda_backward_workspace_bytes(B, Q, H, P)), dtype=torch.uint8, device=device)


def _grad_like(need: bool, t: torch.Tensor):
    return torch.empty_like(t) if need else None


def _as_input(g, shape, dtype):
    return None if g is None else g.reshape(shape).to(dtype)


def _fp32_cuda_params(module) -> bool:
    return all(p.is_cuda and p.dtype == torch.float32 for p in module.parameters())


def _bind_forward(module, forwards: dict):
    """Set forwards[cls] as the bound `forward` of every INSTANCE of cls inside `module` (or `module` itself); the classes are
    never touched, parameters, buffers and the state dict stay as they are.  Returns the bound instances."""
    import types
    bound = []
    for m in module.modules():
        for cls, forward in forwards.items():
            if isinstance(m, cls):
                m.forward = types.MethodType(forward, m)
                bound.append(m)
                break
    return bound


def _xyxy(b: torch.Tensor) -> torch.Tensor:
    """(..., 4) cx, cy, w, h -> x0, y0, x1, y1 in upstream's order of operations (center_to_corners_format)"""
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def _packed_targets(targets, dev, *counts):
    """The targets of all images as the matcher and the loss kernels read them: class labels (T,) int64 on `dev`, boxes (T, 4)
    detached but otherwise as they are (one image: its own tensors, no cat), and an int32 table on `dev` that holds, for each
    list of per-image counts, 0 and then its running sums."""
    if len(targets) == 1:
        labels, tboxes = targets[0]["class_labels"], targets[0]["boxes"]
    else:
        labels, tboxes = torch.cat([t["class_labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])
    table = []
    for per_image in counts:
        table.append(0)
        for n in per_image:
            table.append(table[-1] + n)
    # pinned + non_blocking: the copy is queued on the stream, the host does not wait for it
    offs = torch.tensor(table, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    return labels.to(device=dev, dtype=torch.int64).contiguous(), tboxes.detach(), offs


class _MsdaCore(torch.autograd.Function):
    """multi_scale_deformable_attention_v2 with m355_msda_backward behind it; gradients for value, loc, attn."""

    @staticmethod
    def forward(ctx, value, loc, attn, shapes, pts, discrete):
        v, l, a = _f32c(value, "value"), _f32c(loc, "sampling_locations"), _f32c(attn, "attention_weights")
        ctx.save_for_backward(v, l, a)
        ctx.meta = (shapes, pts, discrete, [(t.shape, t.dtype) for t in (value, loc, attn)])
        return _msda_forward(v, l, a, shapes, pts, discrete)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        v, l, a = ctx.saved_tensors
        shapes, pts, discrete, like = ctx.meta
        B, S, H, D = v.shape
        Q, P = l.shape[1], l.shape[3]
        need = ctx.needs_input_grad
        gv, gl, ga = _grad_like(need[0], v), _grad_like(need[1], l), _grad_like(need[2], a)
        work = _backward_workspace(B, Q, H, P, v.device) if need[0] else None
        sh, pp = _tables(shapes, pts)
        go = _f32c(grad_out, "grad_output")
        check(lib.m355_msda_backward(_ptr(go), _ptr(v), B, S, H, D, sh, len(shapes), _ptr(l), _ptr(a), pp, Q, P, int(discrete),
                                     _ptr(gv), _ptr(gl), _ptr(ga), _ptr(work), work.numel() if work is not None else 0,
                                     _stream()))
        return tuple(_as_input(g, *sd) for g, sd in zip((gv, gl, ga), like)) + (None, None, None)


class _MsdaModule(torch.autograd.Function):
    """The fused module kernel with m355_msda_module_backward behind it; gradients for value, ref, offsets, logits."""

    @staticmethod
    def forward(ctx, value, ref, off, logit, n_heads, shapes, pts, offset_scale):
        v, r = _f32c(value, "encoder_hidden_states"), _f32c(ref, "reference_points")
        o, z = _f32c(off, "sampling offsets"), _f32c(logit, "attention logits")
        ctx.save_for_backward(v, r, o, z)
        ctx.meta = (n_heads, shapes, pts, offset_scale, [(t.shape, t.dtype) for t in (value, ref, off, logit)])
        return _module_forward(v, r, o, z, n_heads, shapes, pts, offset_scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        v, r, o, z = ctx.saved_tensors
        H, shapes, pts, offset_scale, like = ctx.meta
        B, S, d = v.shape
        Q, P = r.shape[1], sum(pts)
        need = ctx.needs_input_grad
        gv, gr, go_, gz = (_grad_like(n, t) for n, t in zip(need, (v, r, o, z)))
        work = _backward_workspace(B, Q, H, P, v.device) if need[0] or need[1] else None
        sh, pp = _tables(shapes, pts)
        go = _f32c(grad_out, "grad_output")
        check(lib.m355_msda_module_backward(_ptr(go), _ptr(v), B, S, H, d // H, sh, len(shapes), _ptr(r), _ptr(o), _ptr(z), pp,
                                            Q, P, float(offset_scale), _ptr(gv), _ptr(gr), _ptr(go_), _ptr(gz), _ptr(work),
                                            work.numel() if work is not None else 0, _stream()))
        return tuple(_as_input(g, *sd) for g, sd in zip((gv, gr, go_, gz), like)) + (None, None, None, None)


def _module_forward(value, ref, off, logit, n_heads, shapes, pts, offset_scale) -> torch.Tensor:
    """contiguous fp32 CUDA tensors: value (B, S, d), ref (B, Q, 4), off (B, Q, heads * P * 2), logit (B, Q, heads * P)"""
    B, S, d = value.shape
    Q, P = ref.shape[1], sum(pts)
    out = torch.empty((B, Q, d), dtype=torch.float32, device=value.device)
    sh, pp = _tables(shapes, pts)
    check(lib.m355_msda_module_forward(_ptr(value), B, S, n_heads, d // n_heads, sh, len(shapes), _ptr(ref), _ptr(off),
                                       _ptr(logit), pp, Q, P, float(offset_scale), _ptr(out), _stream()))
    return out


def deformable_attention(hidden_states: torch.Tensor, reference_points: torch.Tensor, encoder_hidden_states: torch.Tensor,
                         spatial_shapes_list, sampling_offsets: torch.nn.Linear, attention_weights: torch.nn.Linear,
                         num_points_list: List[int], n_heads: int, offset_scale: float) -> torch.Tensor:
    """DFineMultiscaleDeformableAttention.forward (modeling_d_fine.py:247-311) for 4-d reference points and method
    "default": the two linear layers run as torch GEMMs, everything behind them (softmax over the points, sampling
    locations from the reference boxes, bilinear gather-weighted-sum) is ONE kernel.
    hidden_states (B, Q, d); reference_points (B, Q, 1, 4) or (B, Q, 4); encoder_hidden_states (B, S, d) -> (B, Q, d)."""
    B, Q, d = hidden_states.shape
    S = encoder_hidden_states.shape[1]
    D = d // n_heads
    P = sum(num_points_list)
    shapes = [(int(h), int(w)) for h, w in spatial_shapes_list]
    if sum(h * w for h, w in shapes) != S:
        raise ValueError("Make sure to align the spatial shapes with the sequence length of the encoder hidden states")
    ref = reference_points.reshape(B, Q, -1)
    if ref.shape[-1] != 4:
        raise ValueError(f"Last dim of reference_points must be 4 for the fused form, but get {ref.shape[-1]} instead.")
    pts = [int(n) for n in num_points_list]
    off = sampling_offsets(hidden_states)          # (B, Q, heads * P * 2)
    logit = attention_weights(hidden_states)       # (B, Q, heads * P)
    if off.shape[-1] != n_heads * P * 2 or logit.shape[-1] != n_heads * P or d != n_heads * D:
        raise ValueError("the linear layers must produce heads * points * 2 offsets and heads * points logits")
    if _wants_grad(encoder_hidden_states, ref, off, logit):
        return _MsdaModule.apply(encoder_hidden_states, ref, off, logit, n_heads, shapes, pts, float(offset_scale))
    # (B, S, heads, D) is a view of (B, S, d)
    return _module_forward(_f32c(encoder_hidden_states, "encoder_hidden_states"), _f32c(ref, "reference_points"),
                           _f32c(off, "sampling offsets"), _f32c(logit, "attention logits"), n_heads, shapes, pts,
                           float(offset_scale))


def weighting_function(max_num_bins: int, up: torch.Tensor, reg_scale) -> torch.Tensor:
    """W(n), max_num_bins + 1 values (modeling_d_fine.py:1091-1112); a few dozen scalars: computed with torch ops on
    the device `up` lives on, in the reference's order of operations."""
    reg = reg_scale if torch.is_tensor(reg_scale) else torch.tensor(float(reg_scale), dtype=up.dtype, device=up.device)
    upper_bound1 = abs(up[0]) * abs(reg)
    upper_bound2 = abs(up[0]) * abs(reg) * 2
    step = (upper_bound1 + 1) ** (2 / (max_num_bins - 2))
    left = [-((step) ** i) + 1 for i in range(max_num_bins // 2 - 1, 0, -1)]
    right = [(step) ** i - 1 for i in range(1, max_num_bins // 2)]
    values = [-upper_bound2] + left + [torch.zeros_like(up[0][None])] + right + [upper_bound2]
    return torch.cat([v.reshape(1) for v in values], 0)


def decode_boxes(pred_corners: torch.Tensor, project: torch.Tensor, points: torch.Tensor, reg_scale: float,
                 clamp01: bool = False, guard: bool = False) -> torch.Tensor:
    """integral(pred_corners, project) -> distance2bbox(points, ., reg_scale) [-> clamp(0, 1)] in one kernel
    (temporal_dfine.py:180-181).  pred_corners (..., 4 * (bins + 1)), points (..., 4) -> boxes (..., 4).
    guard=True runs the trainers' guards in the same kernel (temp_dfine_over.py:200-222): nan_to_num(pred_corners, 0, 1, 0) ->
    integral -> nan_to_num(distances, 0, 1, 0) -> distance2bbox [-> clamp(0, 1)] -> nan_to_num(boxes, 0.5, 1, 0), with torch's
    gradients (0 into a replaced logit, 0 through a clamped or replaced coordinate); where no guard fires the bits are those of
    guard=False.  With guard=True, CPU or non-fp32 tensors and autocast take decode_boxes_torch; guard=False is the old call."""
    nb1 = project.numel()
    lead = pred_corners.shape[:-1]
    if pred_corners.shape[-1] != 4 * nb1 or tuple(points.shape) != tuple(lead) + (4,):
        raise ValueError("pred_corners must be (..., 4 * len(project)) and points (..., 4)")
    if torch.is_grad_enabled() and project.requires_grad:
        raise RuntimeError("decode_boxes treats project (the weighting function W(n)) as a constant: it has no gradient; "
                           "detach it, or use integral() + distance2bbox() to train reg_scale / up")
    if guard:
        if not (_fp32_cuda(pred_corners, project, points) and not torch.is_autocast_enabled() and nb1 >= 2 and float(reg_scale) != 0.0):
            return decode_boxes_torch(pred_corners, project, points, reg_scale, clamp01, True)
        temporal_calls["kernel"] += 1
    if _wants_grad(pred_corners, points):
        return _Decode.apply(pred_corners, project, points, float(reg_scale), bool(clamp01), bool(guard))
    return _decode_forward(_f32c(pred_corners, "pred_corners"), _f32c(project, "project"), _f32c(points, "points"),
                           float(reg_scale), bool(clamp01), bool(guard))


def _decode_forward(d, pr, pt, reg_scale: float, clamp01: bool, guard: bool = False) -> torch.Tensor:
    out = torch.empty(tuple(d.shape[:-1]) + (4,), dtype=torch.float32, device=d.device)
    entry = lib.m355_dfine_decode_guarded if guard else lib.m355_dfine_decode
    check(entry(_ptr(d), _ptr(pr), _ptr(pt), _ptr(out), out.numel() // 4, pr.numel(), reg_scale, int(clamp01), _stream()))
    return out


class _Decode(torch.autograd.Function):
    """decode_boxes with m355_dfine_decode_backward (guard: m355_dfine_decode_guarded_backward) behind it; gradients for
    pred_corners and points."""

    @staticmethod
    def forward(ctx, pred_corners, project, points, reg_scale, clamp01, guard=False):
        d, pr, pt = _f32c(pred_corners, "pred_corners"), _f32c(project, "project"), _f32c(points, "points")
        ctx.save_for_backward(d, pr, pt)
        ctx.meta = (reg_scale, clamp01, guard, [(t.shape, t.dtype) for t in (pred_corners, points)])
        return _decode_forward(d, pr, pt, reg_scale, clamp01, guard)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_boxes):
        d, pr, pt = ctx.saved_tensors
        reg_scale, clamp01, guard, like = ctx.meta
        gd, gp = _grad_like(ctx.needs_input_grad[0], d), _grad_like(ctx.needs_input_grad[2], pt)
        gb = _f32c(grad_boxes, "grad_output")
        entry = lib.m355_dfine_decode_guarded_backward if guard else lib.m355_dfine_decode_backward
        check(entry(_ptr(gb), _ptr(d), _ptr(pr), _ptr(pt), _ptr(gd), _ptr(gp), gb.numel() // 4, pr.numel(), reg_scale, int(clamp01),
                    _stream()))
        return _as_input(gd, *like[0]), None, _as_input(gp, *like[1]), None, None, None


def integral(pred_corners: torch.Tensor, project: torch.Tensor) -> torch.Tensor:
    """DFineIntegral.forward: (B, Q, 4 * (bins + 1)) logits -> (B, Q, 4) distances.  Runs the decode kernel against a
    reference point chosen so that the box IS the distances: with reg_scale 1 and points (0, 0, 1, 1) the corners are
    (-(0.5 + d0), -(0.5 + d1), 0.5 + d2, 0.5 + d3); the distances are recovered exactly only up to that affine map, so
    this entry computes them with torch softmax + matmul on the device instead (it is not a hot op on its own)."""
    nb1 = project.numel()
    b, q, _ = pred_corners.shape
    p = torch.softmax(pred_corners.reshape(-1, nb1), dim=1)
    return torch.nn.functional.linear(p, project.to(p.device).reshape(1, -1)).reshape(b, q, -1)


def distance2bbox(points: torch.Tensor, distance: torch.Tensor, reg_scale: float) -> torch.Tensor:
    """modeling_d_fine.py:1115-1137 on device tensors (elementwise; the fused form is `decode_boxes`)."""
    reg_scale = abs(reg_scale)
    x0 = points[..., 0] - (0.5 * reg_scale + distance[..., 0]) * (points[..., 2] / reg_scale)
    y0 = points[..., 1] - (0.5 * reg_scale + distance[..., 1]) * (points[..., 3] / reg_scale)
    x1 = points[..., 0] + (0.5 * reg_scale + distance[..., 2]) * (points[..., 2] / reg_scale)
    y1 = points[..., 1] + (0.5 * reg_scale + distance[..., 3]) * (points[..., 3] / reg_scale)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1)


# ---- Hungarian matcher of the loss (RTDetrHungarianMatcher.forward, transformers/loss/loss_rt_detr.py:68-120) ----------------
MATCH_MAX_QUERIES = 2048     # the limits of m355_dfine_match; anything outside them takes the torch + scipy expression
MATCH_MAX_TARGETS = 512
INVALID_COST_MESSAGE = "matrix contains invalid numeric entries"   # scipy.optimize.linear_sum_assignment's ValueError


def hungarian_match(logits: torch.Tensor, pred_boxes: torch.Tensor, targets: Sequence[dict], *, class_cost: float = 2.0,
                    bbox_cost: float = 5.0, giou_cost: float = 2.0, alpha: float = 0.25, gamma: float = 2.0,
                    use_focal_loss: bool = True, check: bool = True, return_cost: bool = False):
    """The matching of RTDetrHungarianMatcher.forward in ONE kernel launch, without the cost matrix's trip to the host.

    logits (B, Q, C), pred_boxes (B, Q, 4) cx, cy, w, h; targets: upstream's list of {"class_labels": (n_b,), "boxes": (n_b, 4)}.
    Returns a list of B tuples (query indices, target indices) of int64 DEVICE tensors, min(Q, n_b) long, ordered by ascending
    query index as scipy's linear_sum_assignment orders them; they are views of two (B, Kmax) buffers.  Sizes come from the
    tensor shapes on the host.  The result is scipy's on the same fp32 costs except where two assignments tie exactly (the
    kernel's search takes the lowest index; scipy's order is its own).

    check=True reads back the B flags (the one synchronisation of the call) and raises ValueError("matrix contains invalid
    numeric entries"), scipy's exception, if an image has a NaN or infinite cost.  Deviation: a +inf entry raises too; scipy
    tolerates +inf.  Upstream's generalized_box_iou additionally raises for boxes with negative width or height; here such a
    box is matched by its (finite) cost.
    check=False performs no device-to-host transfer and no synchronisation.  A tensor's length cannot follow a flag that is
    only on the device, so an image with a non-finite cost then keeps its min(Q, n_b) entries, all -1 (no match); the caller
    promises finite inputs or looks at the flags (return_cost=True) at a synchronisation point of its own.

    return_cost=True returns (indices, costs, flags): costs a list of B (Q, n_b) fp32 views of the matrices the kernel solved,
    flags the (B,) int32 device tensor (0 solved, 1 non-finite cost).
    Shapes outside the kernel's limits (Q > 2048 or an image with more than 512 targets) take upstream's torch + scipy
    expression, results moved to the device: the semantics do not change."""
    B, Q, Cn = logits.shape
    sizes = [int(t["boxes"].shape[0]) for t in targets]
    if len(sizes) != B or tuple(pred_boxes.shape) != (B, Q, 4):
        raise ValueError("logits (B, Q, C), pred_boxes (B, Q, 4) and one target dict per image are expected")
    costs = (class_cost, bbox_cost, giou_cost, alpha, gamma, use_focal_loss)
    if Q > MATCH_MAX_QUERIES or max(sizes, default=0) > MATCH_MAX_TARGETS or Q < 1 or Cn < 1 or B > 65535:
        return _match_torch_scipy(logits, pred_boxes, targets, sizes, costs, return_cost)
    lg, pb = _f32c(logits.detach(), "logits"), _f32c(pred_boxes.detach(), "pred_boxes")
    dev = lg.device
    nmax, total = max(sizes, default=0), sum(sizes)
    kmax = min(Q, nmax)
    ks = [min(Q, n) for n in sizes]
    rows = torch.empty((B, kmax), dtype=torch.int64, device=dev)
    cols = torch.empty((B, kmax), dtype=torch.int64, device=dev)
    cost = torch.empty((B, Q, nmax), dtype=torch.float32, device=dev) if return_cost else None
    if total == 0:   # nothing to match anywhere: no launch
        flags = torch.zeros(B, dtype=torch.int32, device=dev) if return_cost else None
    else:
        labels, tboxes, d_offs = _packed_targets(targets, dev, sizes)
        tboxes = _f32c(tboxes, "target boxes")
        h_counts = (C.c_int32 * B)(*sizes)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        wbytes = int(lib.m355_dfine_match_workspace_bytes(B, Q, nmax))
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev) if wbytes else None
        # (the keyword `check` shadows _capi.check in this function)
        _raise_on_error(lib.m355_dfine_match(_ptr(lg), _ptr(pb), B, Q, Cn, _ptr(labels), _ptr(tboxes), _ptr(d_offs), h_counts,
                                             float(class_cost), float(bbox_cost), float(giou_cost), float(alpha), float(gamma),
                                             int(bool(use_focal_loss)), _ptr(work), wbytes, _ptr(cost), _ptr(rows), _ptr(cols),
                                             kmax, _ptr(flags), _stream()))
        if check and flags.cpu().any():   # the call's one read-back
            raise ValueError(INVALID_COST_MESSAGE)
    out = [(rows[b, :k], cols[b, :k]) for b, k in enumerate(ks)]
    if return_cost:
        return out, [cost[b, :, :n] for b, n in enumerate(sizes)], flags
    return out


def match_cost_torch(logits, pred_boxes, labels, tboxes, class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, alpha=0.25, gamma=2.0,
                     use_focal_loss=True) -> torch.Tensor:
    """The cost expression of loss_rt_detr.py:99-114 in torch ops, in upstream's order, on whatever device and dtype the
    tensors have: logits (N, C), pred_boxes (N, 4), labels (T), tboxes (T, 4) -> (N, T).  What hungarian_match falls back to
    outside the kernel's limits, and what the tests measure the kernel's fp32 error against."""
    if use_focal_loss:
        p = torch.sigmoid(logits)[:, labels]
        neg = (1 - alpha) * (p ** gamma) * (-(1 - p + 1e-8).log())
        pos = alpha * ((1 - p) ** gamma) * (-(p + 1e-8).log())
        cls = pos - neg
    else:
        cls = -logits.softmax(-1)[:, labels]
    l1 = torch.cdist(pred_boxes, tboxes, p=1)
    a, b = _xyxy(pred_boxes), _xyxy(tboxes)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = area_a[:, None] + area_b - inter
    hull = (torch.max(a[:, None, 2:], b[:, 2:]) - torch.min(a[:, None, :2], b[:, :2])).clamp(min=0)
    area = hull[:, :, 0] * hull[:, :, 1]
    giou = inter / union - (area - union) / area
    return bbox_cost * l1 + class_cost * cls + giou_cost * (-giou)


def _match_torch_scipy(logits, pred_boxes, targets, sizes, costs, return_cost):
    """hungarian_match for shapes the kernel does not take: per-image torch cost + scipy on the host"""
    from scipy.optimize import linear_sum_assignment
    class_cost, bbox_cost, giou_cost, alpha, gamma, use_focal_loss = costs
    out, mats = [], []
    for b, t in enumerate(targets):
        labels = t["class_labels"].to(logits.device)
        m = match_cost_torch(logits[b].detach().float(), pred_boxes[b].detach().float(), labels, t["boxes"].detach().float(),
                             class_cost, bbox_cost, giou_cost, alpha, gamma, use_focal_loss)
        i, j = linear_sum_assignment(m.cpu())   # raises ValueError("matrix contains invalid numeric entries") itself
        out.append((torch.as_tensor(i, dtype=torch.int64, device=logits.device),
                    torch.as_tensor(j, dtype=torch.int64, device=logits.device)))
        mats.append(m)
    if return_cost:
        return out, mats, torch.zeros(len(sizes), dtype=torch.int32, device=logits.device)
    return out


@torch.no_grad()
def matcher_forward(self, outputs, targets):
    """Drop-in for RTDetrHungarianMatcher.forward (`RTDetrHungarianMatcher.forward = dfine.matcher_forward`):
    the module's own costs, one launch, index tensors on the device of the logits.  As upstream (scipy) it raises ValueError
    on a non-finite cost, which costs one read-back of B flags per call (hungarian_match(check=False) has none)."""
    return hungarian_match(outputs["logits"], outputs["pred_boxes"], targets, class_cost=self.class_cost,
                           bbox_cost=self.bbox_cost, giou_cost=self.giou_cost, alpha=self.alpha, gamma=self.gamma,
                           use_focal_loss=self.use_focal_loss, check=True)


# ---- loss terms of one decoder output (RTDetrLoss.loss_labels_vfl / loss_boxes, DFineLoss.loss_local) ---------------------------
LOSS_MAX_BINS1 = 64          # the limit of m355_dfine_loss_forward: one lane per bin
LOSS_KEYS = ("loss_vfl", "loss_bbox", "loss_giou", "loss_fgl", "loss_ddf")
loss_calls = {"kernel": 0, "torch": 0}   # how many detection_loss calls took which path (tests and tools read it)


def _pair_iou(a: torch.Tensor, b: torch.Tensor):
    """box_iou of row i of `a` with row i of `b` (xyxy): the diagonal upstream takes from the full matrix"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = area_a + area_b - inter
    return inter / union, union


def _pair_giou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    iou, union = _pair_iou(a, b)
    wh = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
    area = wh[:, 0] * wh[:, 1]
    return iou - (area - union) / area


def _translate_gt(gt: torch.Tensor, project: torch.Tensor):
    """translate_gt (loss_d_fine.py:74-134) followed by bbox2distance's clamp, with torch.where in place of the boolean-mask
    assignments (which synchronise): left bin (int64), weight_right, weight_left"""
    R = project.numel() - 1
    idx = ((project.unsqueeze(0) - gt.unsqueeze(1)) <= 0).sum(1) - 1
    ci = idx.clamp(0, R - 1)
    left_diffs, right_diffs = (gt - project[ci]).abs(), (project[ci + 1] - gt).abs()
    weight_right = left_diffs / (left_diffs + right_diffs)
    neg, pos = idx < 0, idx >= R
    one, zero = torch.ones_like(gt), torch.zeros_like(gt)
    weight_right = torch.where(neg, zero, torch.where(pos, one, weight_right))
    weight_left = torch.where(neg, one, torch.where(pos, zero, 1.0 - weight_right))
    index = torch.where(neg, zero, torch.where(pos, torch.full_like(gt, R - 0.1), idx.to(gt.dtype)))
    return index.clamp(min=0, max=R - 0.1).long(), weight_right, weight_left


def detection_loss_torch(logits, pred_boxes, targets, indices, num_boxes, *, alpha, gamma, pred_corners=None, ref_points=None,
                         teacher_corners=None, teacher_logits=None, project=None, reg_scale=None, temperature=5.0) -> dict:
    """The terms of `detection_loss` in torch ops under autograd, upstream's expressions, on whatever device and dtype the
    tensors have: what detection_loss evaluates on CPU tensors and beyond the kernel's limits, and the fp32 baseline of the
    tests.  Unlike upstream it does not synchronise; every index entry must be valid here."""
    B, Q, Cn = logits.shape
    dtype = logits.dtype
    batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)]).to(logits.device)
    src_idx = torch.cat([src for src, _ in indices]).to(logits.device)
    tgt_boxes = torch.cat([t["boxes"][j] for t, (_, j) in zip(targets, indices)], 0).to(device=logits.device, dtype=pred_boxes.dtype)
    tgt_labels = torch.cat([t["class_labels"][j] for t, (_, j) in zip(targets, indices)]).to(logits.device)
    idx = (batch_idx, src_idx)
    src_boxes = pred_boxes[idx]
    ious, _ = _pair_iou(_xyxy(src_boxes.detach()), _xyxy(tgt_boxes))
    # loss_labels_vfl
    target_classes = torch.full((B, Q), Cn, dtype=torch.int64, device=logits.device)
    target_classes[idx] = tgt_labels
    target = torch.nn.functional.one_hot(target_classes, num_classes=Cn + 1)[..., :-1]
    score = torch.zeros((B, Q), dtype=dtype, device=logits.device)
    score[idx] = ious.to(dtype)
    target_score = score.unsqueeze(-1) * target
    weight = (alpha * torch.sigmoid(logits.detach()).pow(gamma) * (1 - target) + target_score).to(dtype)
    vfl = torch.nn.functional.binary_cross_entropy_with_logits(logits, target_score, weight=weight, reduction="none")
    out = {"loss_vfl": vfl.mean(1).sum() * Q / num_boxes}
    # loss_boxes
    out["loss_bbox"] = torch.nn.functional.l1_loss(src_boxes, tgt_boxes, reduction="none").sum() / num_boxes
    out["loss_giou"] = (1 - _pair_giou(_xyxy(src_boxes), _xyxy(tgt_boxes))).sum() / num_boxes
    if pred_corners is None:
        return out
    # loss_local: FGL
    nb1 = project.numel()
    project = project.detach().to(device=logits.device, dtype=pred_corners.dtype)
    rs = abs(float(reg_scale))
    ref = ref_points[idx].detach().to(pred_corners.dtype)
    box = _xyxy(tgt_boxes).to(pred_corners.dtype)
    four = torch.stack([(ref[:, 0] - box[:, 0]) / (ref[:, 2] / rs + 1e-16) - 0.5 * rs,
                        (ref[:, 1] - box[:, 1]) / (ref[:, 3] / rs + 1e-16) - 0.5 * rs,
                        (box[:, 2] - ref[:, 0]) / (ref[:, 2] / rs + 1e-16) - 0.5 * rs,
                        (box[:, 3] - ref[:, 1]) / (ref[:, 3] / rs + 1e-16) - 0.5 * rs], -1).reshape(-1)
    left, weight_right, weight_left = _translate_gt(four, project)
    rows = pred_corners[idx].reshape(-1, nb1)
    ce = torch.nn.functional.cross_entropy
    fgl = ce(rows, left, reduction="none") * weight_left + ce(rows, left + 1, reduction="none") * weight_right
    out["loss_fgl"] = (fgl * ious.to(rows.dtype).unsqueeze(-1).repeat(1, 4).reshape(-1)).sum() / num_boxes
    # loss_local: DDF.  log q from the same log_softmax as log p: a teacher equal to the prediction gives exactly 0
    T = float(temperature)
    w_local = teacher_logits.detach().sigmoid().max(dim=-1)[0].to(pred_corners.dtype)
    mask = torch.zeros((B, Q), dtype=torch.bool, device=logits.device)
    mask[idx] = True
    w_local = w_local.clone()
    w_local[idx] = ious.to(w_local.dtype)
    log_p = torch.log_softmax(pred_corners.reshape(B, Q, 4, nb1) / T, dim=-1)
    log_q = torch.log_softmax(teacher_corners.detach().reshape(B, Q, 4, nb1).to(pred_corners.dtype) / T, dim=-1)
    rows_loss = w_local.unsqueeze(-1) * (T ** 2) * (log_q.exp() * (log_q - log_p)).sum(-1)          # (B, Q, 4)
    m4 = mask.unsqueeze(-1).to(rows_loss.dtype)
    n_pos, n_neg = 4 * mask.sum().to(rows_loss.dtype), 4 * (~mask).sum().to(rows_loss.dtype)
    num_pos, num_neg = (n_pos * (1 / B)) ** 0.5, (n_neg * (1 / B)) ** 0.5
    mean_pos = torch.where(n_pos > 0, (rows_loss * m4).sum() / n_pos.clamp(min=1), torch.zeros_like(n_pos))
    mean_neg = torch.where(n_neg > 0, (rows_loss * (1 - m4)).sum() / n_neg.clamp(min=1), torch.zeros_like(n_neg))
    out["loss_ddf"] = (mean_pos * num_pos + mean_neg * num_neg) / (num_pos + num_neg)
    return out


class _DetectionLoss(torch.autograd.Function):
    """m355_dfine_loss_forward / _backward: the five terms as five 0-d outputs; gradients for logits, pred_boxes, pred_corners.
    The backward recomputes per query; the forward keeps its inputs and the two DDF group coefficients (in `out`)."""

    @staticmethod
    def forward(ctx, logits, pred_boxes, pred_corners, consts):
        (mq, mt, M, offs, labels, tboxes, T, num_boxes, alpha, gamma, ref, tc, tl, project, nb1, reg_scale, temperature) = consts
        lg, pb = _f32c(logits, "logits"), _f32c(pred_boxes, "pred_boxes")
        pc = _f32c(pred_corners, "pred_corners") if pred_corners is not None else None
        B, Q, Cn = lg.shape
        wbytes = int(lib.m355_dfine_loss_workspace_bytes(B, Q))
        work = torch.empty(wbytes, dtype=torch.uint8, device=lg.device)
        out = torch.empty(8, dtype=torch.float32, device=lg.device)
        ctx.args = (B, Q, Cn, _ptr(mq), _ptr(mt), M, _ptr(offs), _ptr(labels), _ptr(tboxes), T, num_boxes, alpha, gamma)
        ctx.local = (_ptr(ref), _ptr(tc), _ptr(tl), _ptr(project), nb1, reg_scale, temperature)
        check(lib.m355_dfine_loss_forward(_ptr(lg), _ptr(pb), *ctx.args, _ptr(pc), *ctx.local, _ptr(work), wbytes, _ptr(out),
                                          _stream()))
        ctx.save_for_backward(lg, pb, pc, out)
        ctx.keep = consts   # the buffers behind the raw pointers
        ctx.like = [(t.shape, t.dtype) if t is not None else None for t in (logits, pred_boxes, pred_corners)]
        loss_calls["kernel"] += 1
        return tuple(out[:5].unbind(0))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        lg, pb, pc, out = ctx.saved_tensors
        zero = None
        terms = []
        for g in grads:
            if g is None:
                zero = torch.zeros((), dtype=torch.float32, device=lg.device) if zero is None else zero
                g = zero
            terms.append(g.reshape(()).to(torch.float32))
        gt = torch.stack(terms)
        need = ctx.needs_input_grad
        gl, gb = _grad_like(need[0], lg), _grad_like(need[1], pb)
        gc = _grad_like(need[2], pc) if pc is not None else None
        check(lib.m355_dfine_loss_backward(_ptr(gt), _ptr(lg), _ptr(pb), *ctx.args, _ptr(pc), *ctx.local, _ptr(out), _ptr(gl),
                                           _ptr(gb), _ptr(gc), _stream()))
        res = [None if g is None else _as_input(g, *sd) for g, sd in zip((gl, gb, gc), ctx.like)]
        return res[0], res[1], res[2], None


def detection_loss(logits: torch.Tensor, pred_boxes: torch.Tensor, targets: Sequence[dict], indices, num_boxes, *, alpha: float,
                   gamma: float, pred_corners=None, ref_points=None, teacher_corners=None, teacher_logits=None, project=None,
                   reg_scale=None, temperature: float = 5.0) -> dict:
    """The loss terms of ONE D-FINE / RT-DETR decoder output, unweighted, as 0-d tensors under upstream's keys: loss_vfl,
    loss_bbox, loss_giou (RTDetrLoss.loss_labels_vfl, loss_boxes) and, when the local group (pred_corners, ref_points,
    teacher_corners, teacher_logits, project = weighting_function(...), reg_scale) is given, loss_fgl and loss_ddf
    (DFineLoss.loss_local with T = temperature).  Differentiable in logits, pred_boxes and pred_corners.

    logits (B, Q, C), pred_boxes (B, Q, 4) cx, cy, w, h; targets: upstream's list of {"class_labels", "boxes"}; indices:
    upstream's list of B (query idx, target idx) int64 tensors, as hungarian_match and get_cdn_matched_indices return them
    (their lengths are read from the shapes on the host); num_boxes: a Python number.

    CUDA tensors: three launches forward (two kernels and the copy of 2 (B + 1) offsets), one backward, no synchronisation in
    either direction.  An entry whose query or target index is out of range (hungarian_match(check=False)'s -1 entries
    included) is skipped in every term.  The caller promises at most one entry per (b, q); with duplicates one of them wins.
    Deviations from upstream: a box with negative width or height is not refused (generalized_box_iou's ValueError is a
    synchronising check; hungarian_match documents the same), and a teacher equal to the prediction gives loss_ddf == 0.0
    by arithmetic (one log-softmax routine for both sides) where upstream compares the tensors with torch.equal.
    CPU tensors, and more than 64 bins + 1: detection_loss_torch, the same expressions in torch ops."""
    B, Q, Cn = logits.shape
    if len(indices) != B or len(targets) != B or tuple(pred_boxes.shape) != (B, Q, 4):
        raise ValueError("logits (B, Q, C), pred_boxes (B, Q, 4), one target dict and one index pair per image are expected")
    group = (pred_corners, ref_points, teacher_corners, teacher_logits, project, reg_scale)
    local = pred_corners is not None
    if any((g is None) == local for g in group):
        raise ValueError("pred_corners, ref_points, teacher_corners, teacher_logits, project and reg_scale go together")
    nb1 = int(project.numel()) if local else 0
    if local and (pred_corners.shape[-1] != 4 * nb1 or tuple(teacher_corners.shape) != tuple(pred_corners.shape)
                  or tuple(teacher_logits.shape) != (B, Q, Cn) or tuple(ref_points.shape) != (B, Q, 4)):
        raise ValueError("the local group's shapes do not fit logits / project")
    if not logits.is_cuda or nb1 > LOSS_MAX_BINS1 or B < 1 or Q < 1 or Cn < 1:
        loss_calls["torch"] += 1
        return detection_loss_torch(logits, pred_boxes, targets, indices, num_boxes, alpha=alpha, gamma=gamma,
                                    pred_corners=pred_corners, ref_points=ref_points, teacher_corners=teacher_corners,
                                    teacher_logits=teacher_logits, project=project, reg_scale=reg_scale, temperature=temperature)
    dev = logits.device
    lens = [int(i.shape[0]) for i, _ in indices]
    sizes = [int(t["boxes"].shape[0]) for t in targets]
    M, T = sum(lens), sum(sizes)
    mq = mt = offs = labels = tboxes = None
    if M > 0 and T > 0:
        mq, mt = indices[0] if B == 1 else (torch.cat([i for i, _ in indices]), torch.cat([j for _, j in indices]))
        mq, mt = (t.to(device=dev, dtype=torch.int64).contiguous() for t in (mq, mt))
        labels, tboxes, offs = _packed_targets(targets, dev, lens, sizes)
        tboxes = _f32c(tboxes.to(dev), "target boxes")
    else:
        M = 0
    if local:
        ref, tc = _f32c(ref_points.detach(), "ref_points"), _f32c(teacher_corners.detach(), "teacher_corners")
        tl, pr = _f32c(teacher_logits.detach(), "teacher_logits"), _f32c(project.detach(), "project")
        rs, temp = float(reg_scale), float(temperature)
    else:
        ref = tc = tl = pr = None
        rs, temp = 1.0, 1.0
    consts = (mq, mt, M, offs, labels, tboxes, T, float(num_boxes), float(alpha), float(gamma), ref, tc, tl, pr, nb1, rs, temp)
    terms = _DetectionLoss.apply(logits, pred_boxes, pred_corners, consts)
    return dict(zip(LOSS_KEYS[:5 if local else 3], terms))


def criterion_forward(self, outputs, targets):
    """Drop-in for RTDetrLoss.forward, which DFineLoss inherits (`RTDetrLoss.forward = dfine.criterion_forward`,
    INTEGRATION.md): upstream's control flow (the main output, `auxiliary_outputs`, `dn_auxiliary_outputs` with
    get_cdn_matched_indices and num_boxes * dn_num_group), keys, `_aux_i` / `_dn_i` suffixes and `weight_dict`; indices from
    `self.matcher`, whatever is bound there; ONE detection_loss call per output.  num_boxes is max(sum of the target counts, 1)
    from the shapes on the host, without `.item()`.  An output without `pred_corners` yields no loss_fgl / loss_ddf.
    Deviations: as detection_loss (no ValueError for a negative-size box; loss_ddf's zero by arithmetic), and
    `self.num_pos` / `self.num_neg` / `self.fgl_targets` are not set on the module.  W(n) is computed once per (module, device)
    and kept in `self._m355_project` (upstream recomputes it per output from the same constants)."""
    if not set(self.losses) <= {"vfl", "boxes", "local"}:
        raise ValueError(f"criterion_forward covers the losses vfl, boxes and local, not {self.losses}")
    outputs_without_aux = {k: v for k, v in outputs.items() if "auxiliary_outputs" not in k}
    indices = self.matcher(outputs_without_aux, targets)
    num_boxes = float(max(sum(int(t["class_labels"].shape[0]) for t in targets), 1))
    with_local = "local" in self.losses

    def project_for(device):
        key = (str(device), self.up._version, self.max_num_bins, float(self.reg_scale))
        cached = getattr(self, "_m355_project", None)
        if cached is None or cached[0] != key:
            with torch.no_grad():
                cached = (key, weighting_function(self.max_num_bins, self.up.detach().to(device), self.reg_scale).float())
            self._m355_project = cached
        return cached[1]

    def terms(out, indices, num_boxes, suffix):
        kw = {}
        if with_local and "pred_corners" in out:
            kw = dict(pred_corners=out["pred_corners"], ref_points=out["ref_points"], teacher_corners=out["teacher_corners"],
                      teacher_logits=out["teacher_logits"], project=project_for(out["logits"].device), reg_scale=self.reg_scale)
        d = detection_loss(out["logits"], out["pred_boxes"], targets, indices, num_boxes, alpha=self.alpha, gamma=self.gamma, **kw)
        return {k + suffix: v * self.weight_dict[k] for k, v in d.items() if k in self.weight_dict}

    losses = terms(outputs, indices, num_boxes, "")
    if "auxiliary_outputs" in outputs:
        for i, aux in enumerate(outputs["auxiliary_outputs"]):
            losses.update(terms(aux, self.matcher(aux, targets), num_boxes, f"_aux_{i}"))
    if "dn_auxiliary_outputs" in outputs:
        if "denoising_meta_values" not in outputs:
            raise ValueError("The output must have the 'denoising_meta_values` key. Please, ensure that 'outputs' includes a "
                             "'denoising_meta_values' entry.")
        indices = self.get_cdn_matched_indices(outputs["denoising_meta_values"], targets)
        num_boxes = num_boxes * outputs["denoising_meta_values"]["dn_num_group"]
        for i, aux in enumerate(outputs["dn_auxiliary_outputs"]):
            losses.update(terms(aux, indices, num_boxes, f"_dn_{i}"))
    return losses


# ---- detection post-processing (RTDetrImageProcessor.post_process_object_detection, image_processing_rt_detr.py:482-552) ------
POST_MAX_QUERIES = 2048          # the limits of m355_dfine_postprocess; anything outside them takes post_process_torch
POST_MAX_CANDIDATES = 1 << 24    # Q * C stays below it
TARGET_SIZES_MESSAGE = "Make sure that you pass in as many target sizes as the batch dimension of the logits"   # upstream's
post_calls = {"kernel": 0, "torch": 0}   # how many calls took which path (tests and tools read it)


def _post_kernel_takes(logits: torch.Tensor, pred_boxes: torch.Tensor) -> bool:
    B, Q, Cn = logits.shape
    return (logits.is_cuda and pred_boxes.is_cuda and B >= 1 and 1 <= Q <= POST_MAX_QUERIES and Cn >= 1
            and Q * Cn < POST_MAX_CANDIDATES and not _wants_grad(logits, pred_boxes))


def _check_post_shapes(logits, pred_boxes, target_sizes):
    if logits.dim() != 3 or tuple(pred_boxes.shape) != tuple(logits.shape[:2]) + (4,):
        raise ValueError("logits (B, Q, C) and pred_boxes (B, Q, 4) are expected")
    if target_sizes is not None and len(logits) != len(target_sizes):
        raise ValueError(TARGET_SIZES_MESSAGE)


def _device_sizes(target_sizes, B: int, dev) -> torch.Tensor:
    """(B, 2) fp32 (height, width) on `dev` without a synchronisation: a device tensor is cast there, anything on the host goes
    up as one pinned non-blocking copy"""
    if torch.is_tensor(target_sizes) and target_sizes.is_cuda:
        return target_sizes.to(device=dev, dtype=torch.float32).reshape(B, 2).contiguous()
    host = target_sizes.to(torch.float32) if torch.is_tensor(target_sizes) else torch.tensor(
        [[float(h), float(w)] for h, w in target_sizes], dtype=torch.float32)
    return host.reshape(B, 2).contiguous().pin_memory().to(dev, non_blocking=True)


def _topk_torch(logits, pred_boxes, target_sizes, use_focal_loss: bool = True):
    """upstream's expression up to the per-image masks: scores (B, K), labels (B, K), boxes (B, K, 4)"""
    boxes = _xyxy(pred_boxes)
    if target_sizes is not None:
        sizes = torch.as_tensor(target_sizes) if isinstance(target_sizes, (list, tuple)) else target_sizes
        img_h, img_w = sizes.unbind(1)
        boxes = boxes * torch.stack([img_w, img_h, img_w, img_h], dim=1).to(boxes.device)[:, None, :]
    num_top_queries, num_classes = logits.shape[1], logits.shape[2]
    if use_focal_loss:
        scores, index = torch.topk(torch.sigmoid(logits).flatten(1), num_top_queries, dim=-1)
        labels = index % num_classes
        index = index // num_classes
        boxes = boxes.gather(dim=1, index=index.unsqueeze(-1).repeat(1, 1, boxes.shape[-1]))
    else:
        scores, labels = torch.softmax(logits, dim=-1)[:, :, :-1].max(dim=-1)
        if scores.shape[1] > num_top_queries:   # never: upstream keeps the branch
            scores, index = torch.topk(scores, num_top_queries, dim=-1)
            labels = torch.gather(labels, dim=1, index=index)
            boxes = torch.gather(boxes, dim=1, index=index.unsqueeze(-1).tile(1, 1, boxes.shape[-1]))
    return scores, labels, boxes


def post_process_torch(logits: torch.Tensor, pred_boxes: torch.Tensor, target_sizes=None, threshold: float = 0.5,
                       use_focal_loss: bool = True) -> List[dict]:
    """Upstream's post_process_object_detection in torch ops, on whatever device and dtype the tensors have, its three
    boolean-mask indexings per image included (each synchronises on a device): what the kernel-backed functions fall back to
    (use_focal_loss=False, CPU tensors, shapes beyond the kernel's limits, inputs under autograd) and the fp32 baseline of the
    tests.  Among equal scores the order is torch.topk's own."""
    _check_post_shapes(logits, pred_boxes, target_sizes)
    post_calls["torch"] += 1
    scores, labels, boxes = _topk_torch(logits, pred_boxes, target_sizes, use_focal_loss)
    return [{"scores": s[s > threshold], "labels": l[s > threshold], "boxes": b[s > threshold]}
            for s, l, b in zip(scores, labels, boxes)]


def topk_detections(logits: torch.Tensor, pred_boxes: torch.Tensor, target_sizes=None, threshold: float = 0.5):
    """The focal branch of post_process_object_detection up to the threshold, in ONE kernel launch and without any
    device-to-host transfer: (scores (B, Q) fp32, labels (B, Q) int64, boxes (B, Q, 4) fp32 xyxy, counts (B, 2) int32), all on
    the device.  logits (B, Q, C), pred_boxes (B, Q, 4) cx, cy, w, h; target_sizes None, a list of (height, width), or a (B, 2)
    tensor of any integer or float dtype on the host (one pinned non-blocking copy) or on the device (cast there).

    Rows: NaN logits first (torch.topk's order), then descending logit, an exact tie to the lowest flat index q * C + c.
    counts[b] = (n_nan, n_keep): upstream's `score > threshold` masks of image b are the slice [n_nan, n_nan + n_keep) of its
    rows.  Boxes are torch's fp32 bits.  Deviation: the sizes are taken as fp32 (a float64 target_sizes tensor makes upstream
    return float64 boxes).  CPU tensors, shapes beyond the kernel's limits (Q > 2048, Q * C >= 2^24) and inputs under autograd
    take upstream's torch ops; the counts are then computed with torch ops too and ties keep torch.topk's order."""
    _check_post_shapes(logits, pred_boxes, target_sizes)
    B, Q, Cn = logits.shape
    if not _post_kernel_takes(logits, pred_boxes):
        post_calls["torch"] += 1
        scores, labels, boxes = _topk_torch(logits, pred_boxes, target_sizes)
        n_nan = torch.isnan(scores).sum(1)
        counts = torch.stack([n_nan, (scores > threshold).sum(1)], dim=1).to(torch.int32)
        return scores, labels, boxes, counts
    lg, pb = _f32c(logits.detach(), "logits"), _f32c(pred_boxes.detach(), "pred_boxes")
    dev = lg.device
    sizes = _device_sizes(target_sizes, B, dev) if target_sizes is not None else None
    scores = torch.empty((B, Q), dtype=torch.float32, device=dev)
    labels = torch.empty((B, Q), dtype=torch.int64, device=dev)
    boxes = torch.empty((B, Q, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    check(lib.m355_dfine_postprocess(_ptr(lg), _ptr(pb), B, Q, Cn, _ptr(sizes), float(threshold), _ptr(scores), _ptr(labels),
                                     _ptr(boxes), _ptr(counts), _stream()))
    post_calls["kernel"] += 1
    return scores, labels, boxes, counts


def post_process_detections(logits: torch.Tensor, pred_boxes: torch.Tensor, target_sizes=None, threshold: float = 0.5) -> List[dict]:
    """Upstream's list of {"scores", "labels", "boxes"} per image for a whole batch (a sequence of frames) at once: one
    topk_detections launch and ONE read-back of the (B, 2) counts; the entries are device tensors, slices of the three
    outputs.  A NaN score is in no image's entries, as upstream's `score > threshold` excludes it.  What a script calls once
    per sequence in place of its per-frame loop."""
    _check_post_shapes(logits, pred_boxes, target_sizes)
    if not _post_kernel_takes(logits, pred_boxes):
        return post_process_torch(logits, pred_boxes, target_sizes, threshold)
    scores, labels, boxes, counts = topk_detections(logits, pred_boxes, target_sizes, threshold)
    out = []
    for b, (n_nan, n_keep) in enumerate(counts.cpu().tolist()):   # the call's one read-back
        out.append({"scores": scores[b, n_nan:n_nan + n_keep], "labels": labels[b, n_nan:n_nan + n_keep],
                    "boxes": boxes[b, n_nan:n_nan + n_keep]})
    return out


def post_process_object_detection(self, outputs, threshold: float = 0.5, target_sizes=None, use_focal_loss: bool = True):
    """Drop-in for RTDetrImageProcessor.post_process_object_detection
    (`RTDetrImageProcessor.post_process_object_detection = dfine.post_process_object_detection`).  `outputs`
    has `logits` and `pred_boxes` as attributes or as keys (the reference's trainers pass a dict).  Upstream's ValueError for a
    target_sizes of the wrong length is kept; use_focal_loss=False takes upstream's torch ops."""
    if isinstance(outputs, Mapping):
        logits, pred_boxes = outputs["logits"], outputs["pred_boxes"]
    else:
        logits, pred_boxes = outputs.logits, outputs.pred_boxes
    if not use_focal_loss:
        return post_process_torch(logits, pred_boxes, target_sizes, threshold, use_focal_loss=False)
    return post_process_detections(logits, pred_boxes, target_sizes, threshold)


# ---- image pre-processing (RTDetrImageProcessorPil.preprocess with its defaults, image_processing_pil_rt_detr.py:380-505) -------
# Every D-FINE script starts a sequence with processor(images=frames, return_tensors="pt")["pixel_values"].to(device): Pillow's
# 8-bit BILINEAR resize to a fixed size and a rescale, a frame at a time on the host, then an fp32 upload.  Here the raw frames go
# up once as bytes and csrc/dfine_preprocess.hip writes the model's input batch, bit for bit the processor's.
PRE_MAX_TAPS, PRE_MAX_W, PRE_MAX_H = DFINE_PRE_MAX_TAPS, DFINE_PRE_MAX_W, DFINE_PRE_MAX_H   # the limits of m355_dfine_preprocess
PRE_MAX_FRAMES = 65535
PRE_MAX_ASPECT = 64      # Pillow resizes very tall, thin images (in_h / in_w of 125 and more, measured) vertical pass first
PRE_PRECISION_BITS = 22  # Pillow's fixed point
preprocess_calls = {"kernel": 0, "original": 0}   # how many bound preprocess calls took which path (tests and tools read it)


@functools.lru_cache(maxsize=256)
def resize_tables(in_size: int, out_size: int):
    """Pillow's coefficients of one axis of an 8-bit BILINEAR resize (precompute_coeffs + normalize_coeffs_8bpc), float64 in its
    order of operations: (xmin (out,) int32, counts (out,) int32, coefficients (out, ksize) int32, zero behind a row's count).
    Output xx = clip((2^21 + sum_t coefficients[xx, t] * pixel[xmin[xx] + t]) >> 22, 0, 255).  Cached per (in, out); read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be >= 1")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs                                   # bilinear: support 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # C's (int): towards zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    counts = xmax - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    arg = np.abs(((taps + xmin[:, None]) - center[:, None] + 0.5) / fs)
    w = np.where((arg < 1.0) & (taps < counts[:, None]), 1.0 - arg, 0.0)
    total = np.zeros(out_size, np.float64)
    for t in range(ksize):                         # summed in tap order, as Pillow does
        total += w[:, t]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    coef = (w * float(1 << PRE_PRECISION_BITS) + 0.5).astype(np.int32)
    out = (xmin.astype(np.int32), counts.astype(np.int32), coef)
    for a in out:
        a.setflags(write=False)
    return out


def rescale_table(rescale_factor: float = 1 / 255) -> torch.Tensor:
    """the fp32 value of every byte: float32(float64(b) * rescale_factor), what the processor's numpy rescale gives"""
    return torch.from_numpy((np.arange(256, dtype=np.float64) * float(rescale_factor)).astype(np.float32))


def preprocess_in_domain(in_h: int, in_w: int, out_h: int, out_w: int) -> bool:
    """Whether preprocess_images takes a source of (in_h, in_w) for an output of (out_h, out_w): an aspect ratio within 64 : 1
    either way (the shapes whose pass order in Pillow is known to be horizontal-first), sizes and tap counts within the kernel's
    limits.  bind_processor sends everything else to the original processor ("falls back")."""
    if not (1 <= in_h <= PRE_MAX_H and 1 <= in_w <= PRE_MAX_W and 1 <= out_h <= PRE_MAX_H and 4 <= out_w <= PRE_MAX_W and out_w % 4 == 0):
        return False
    if in_h > PRE_MAX_ASPECT * in_w or in_w > PRE_MAX_ASPECT * in_h:
        return False
    return all(int(math.ceil(max(i / o, 1.0))) * 2 + 1 <= PRE_MAX_TAPS for i, o in ((in_h, out_h), (in_w, out_w)))


def _as_rgb_array(image):
    """uint8 (h, w, 3) ndarray of a PIL image in mode RGB or of such an ndarray, else None"""
    if isinstance(image, np.ndarray):
        return image if image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 else None
    if getattr(image, "mode", None) == "RGB" and hasattr(image, "resize") and hasattr(image, "size"):
        return np.asarray(image)
    return None


def _pre_size(size):
    out_h, out_w = (int(size["height"]), int(size["width"])) if isinstance(size, Mapping) else (int(size[0]), int(size[1]))
    return out_h, out_w


def _pre_arrays(images, out_h, out_w):
    if not isinstance(images, (list, tuple)):
        images = [images]
    arrays = [_as_rgb_array(im) for im in images]
    if not arrays or len(arrays) > PRE_MAX_FRAMES or any(a is None for a in arrays):
        raise ValueError("images: 1..65535 PIL images in mode RGB or uint8 (h, w, 3) arrays are expected")
    for a in arrays:
        if not preprocess_in_domain(a.shape[0], a.shape[1], out_h, out_w):
            raise ValueError(f"a {a.shape[0]} x {a.shape[1]} image to {out_h} x {out_w} is outside the kernel's domain "
                             "(aspect ratio within 64 : 1, sizes and tap counts within the limits of m355_dfine_preprocess)")
    return arrays


def _pass_torch(img: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    xmin, counts, coef = resize_tables(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    acc = np.full((out_size,) + src.shape[1:], 1 << (PRE_PRECISION_BITS - 1), np.int64)
    lift = (slice(None),) + (None,) * (src.ndim - 1)
    for t in range(coef.shape[1]):                 # a coefficient behind a row's count is 0: its clamped tap adds nothing
        acc += coef[:, t].astype(np.int64)[lift] * src[np.minimum(xmin.astype(np.int64) + t, in_size - 1)]
    return np.moveaxis(np.clip(acc >> PRE_PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def preprocess_images_torch(images, size=(640, 640), rescale_factor: float = 1 / 255) -> torch.Tensor:
    """preprocess_images on the host in numpy, from the same tables: (T, 3, H, W) fp32 on the CPU, the processor's bits.  The
    fallback where there is no device, and the tests' second opinion."""
    out_h, out_w = _pre_size(size)
    table = rescale_table(rescale_factor).numpy()
    frames = [table[_pass_torch(_pass_torch(a, out_w, 1), out_h, 0)].transpose(2, 0, 1) for a in _pre_arrays(images, out_h, out_w)]
    return torch.from_numpy(np.ascontiguousarray(np.stack(frames)))


class _PreBuffers:
    """pinned staging, its device copy and the uint8 scratch of preprocess_images on one device, kept and grown"""

    def __init__(self):
        self.host = self.dev = self.mid = None
        self.copied = self.done = None   # events: the last upload has left the staging buffer / the last kernels have read dev and mid

    def reserve(self, device, total: int, mid_bytes: int):
        grow_stage = self.host is None or self.host.numel() < total
        grow_mid = self.mid is None or self.mid.numel() < mid_bytes
        if (grow_stage or grow_mid) and self.done is not None:
            self.done.synchronize()              # nothing in flight reads the buffers that are let go
        if grow_stage:
            cap = (total + (1 << 22) - 1) >> 22 << 22
            self.host = torch.empty((cap,), dtype=torch.uint8, pin_memory=True)
            self.dev = torch.empty((cap,), dtype=torch.uint8, device=device)
            self.copied, self.done = torch.cuda.Event(), torch.cuda.Event()
        else:
            self.copied.synchronize()            # the previous upload has read the staging buffer
            torch.cuda.current_stream().wait_event(self.done)
        if grow_mid:
            self.mid = torch.empty(((max(mid_bytes, 1) + (1 << 22) - 1) >> 22 << 22,), dtype=torch.uint8, device=device)


_pre_buffers: dict = {}


def _align16(n: int) -> int:
    return (n + 15) & ~15


class _PrePlan:
    """The staging layout of one preprocess_images call: image table | axis table | int32 pool | rescale table | frames, each part
    and each frame at a multiple of 16 bytes.  One axis entry per distinct (in, out) pair, its xmin | counts | coefficients in the
    pool; a pass with in == out has no table (-1)."""

    def __init__(self, arrays, out_h: int, out_w: int):
        self.out_h, self.out_w, self.T = out_h, out_w, len(arrays)
        axis_of, axis_rows, parts, self.pool_len = {}, [], [], 0
        passes = []
        for a in arrays:
            tabs = []
            for key in ((a.shape[1], out_w), (a.shape[0], out_h)):
                if key[0] == key[1]:
                    tabs.append(-1)
                    continue
                if key not in axis_of:
                    xmin, counts, coef = resize_tables(*key)
                    axis_of[key] = len(axis_rows)
                    axis_rows.append(DfinePreAxis(key[0], key[1], coef.shape[1], self.pool_len))
                    parts.extend((xmin, counts, coef.reshape(-1)))
                    self.pool_len += key[1] * (2 + coef.shape[1])
                tabs.append(axis_of[key])
            passes.append(tabs)
        self.n_axes = len(axis_rows)
        self.axes = (DfinePreAxis * max(self.n_axes, 1))(*axis_rows)
        self.pool = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        self.images = (DfinePreImage * self.T)()
        self.o_images = 0
        self.o_axes = _align16(C.sizeof(self.images))
        self.o_pool = _align16(self.o_axes + C.sizeof(self.axes))
        self.o_rescale = _align16(self.o_pool + 4 * self.pool_len)
        self.o_frames = _align16(self.o_rescale + 1024)
        offset = mid_rows = 0
        for i, (a, (htab, vtab)) in enumerate(zip(arrays, passes)):
            self.images[i] = DfinePreImage(offset, a.shape[0], a.shape[1], htab, vtab, mid_rows if htab >= 0 else 0, 0)
            offset = _align16(offset + a.size)
            mid_rows += a.shape[0] if htab >= 0 else 0
        self.src_bytes = offset
        self.total = self.o_frames + offset
        self.mid_bytes = mid_rows * out_w * 3

    def fill(self, host: np.ndarray, arrays, rescale_factor: float):
        """write the tables and the frames into the uint8 staging array"""
        C.memmove(host.ctypes.data + self.o_images, self.images, C.sizeof(self.images))
        C.memmove(host.ctypes.data + self.o_axes, self.axes, C.sizeof(self.axes))
        host[self.o_pool:self.o_pool + 4 * self.pool_len].view(np.int32)[:] = self.pool
        host[self.o_rescale:self.o_rescale + 1024].view(np.float32)[:] = rescale_table(rescale_factor).numpy()
        for r, a in zip(self.images, arrays):
            at = self.o_frames + r.offset
            np.copyto(host[at:at + a.size].reshape(a.shape), a)

    def launch(self, host_ptr: int, dev_ptr: int, mid_ptr: int, mid_bytes: int, out_ptr: int, stream) -> int:
        """m355_dfine_preprocess on a staging buffer at host_ptr and its device copy at dev_ptr; returns the status"""
        at = lambda base, off, used=True: C.c_void_p(base + off) if used else None
        return lib.m355_dfine_preprocess(
            at(dev_ptr, self.o_frames), self.src_bytes, at(host_ptr, self.o_images), at(dev_ptr, self.o_images), self.T,
            at(host_ptr, self.o_axes, self.n_axes), at(dev_ptr, self.o_axes, self.n_axes), self.n_axes,
            at(host_ptr, self.o_pool, self.n_axes), at(dev_ptr, self.o_pool, self.n_axes), self.pool_len,
            at(dev_ptr, self.o_rescale), self.out_h, self.out_w, C.c_void_p(mid_ptr), mid_bytes, C.c_void_p(out_ptr), stream)


def preprocess_images(images, size=(640, 640), rescale_factor: float = 1 / 255, device=None) -> torch.Tensor:
    """RTDetrImageProcessorPil's pixel_values of a list of frames, on the device: (T, 3, H, W) fp32, bit for bit
    processor(images=images, return_tensors="pt")["pixel_values"] for resize-to-`size` (BILINEAR) + rescale, no normalise, no pad.
    images: PIL images in mode RGB or uint8 (h, w, 3) ndarrays of any mix of sizes inside `preprocess_in_domain` (ValueError
    otherwise); size (H, W) or {"height", "width"}.  The frames, the per-image table, one coefficient table per distinct
    (in, out) pair and the rescale table are packed into one pinned buffer and go up in one copy; then at most two launches
    (csrc/dfine_preprocess.hip), asynchronous on the current stream.  Staging, device copy and scratch are kept and grown."""
    out_h, out_w = _pre_size(size)
    arrays = _pre_arrays(images, out_h, out_w)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("preprocess_images runs on a CUDA device; preprocess_images_torch is the host path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    plan = _PrePlan(arrays, out_h, out_w)
    with torch.cuda.device(device):
        buf = _pre_buffers.setdefault(device, _PreBuffers())
        buf.reserve(device, plan.total, plan.mid_bytes)
        plan.fill(buf.host.numpy(), arrays, rescale_factor)
        buf.dev[:plan.total].copy_(buf.host[:plan.total], non_blocking=True)
        buf.copied.record()
        out = torch.empty((len(arrays), 3, out_h, out_w), dtype=torch.float32, device=device)
        check(plan.launch(buf.host.data_ptr(), buf.dev.data_ptr(), buf.mid.data_ptr(), buf.mid.numel(), out.data_ptr(), _stream()))
        buf.done.record()
    return out


def _processor_fast_path(processor, images, annotations, kwargs):
    """(frames, (H, W), rescale_factor) where bind_processor's preprocess takes the kernel path, else None"""
    known = {"do_resize", "size", "resample", "do_rescale", "rescale_factor", "do_normalize", "do_pad", "return_tensors",
             "image_mean", "image_std", "do_convert_annotations", "format", "pad_size"}
    if annotations is not None or not set(kwargs) <= known or not torch.cuda.is_available():
        return None
    opt = lambda name: kwargs[name] if name in kwargs else getattr(processor, name, None)   # upstream's setdefault from self
    if not opt("do_resize") or not opt("do_rescale") or opt("do_normalize") or opt("do_pad") or opt("return_tensors") != "pt":
        return None
    try:
        size = {k: v for k, v in dict(opt("size")).items() if v is not None}
        if set(size) != {"height", "width"} or int(opt("resample")) != 2:   # PIL.Image.BILINEAR
            return None
        out_h, out_w = int(size["height"]), int(size["width"])
        factor = float(opt("rescale_factor"))
    except (TypeError, ValueError):
        return None
    frames = list(images) if isinstance(images, (list, tuple)) else [images]
    arrays = [_as_rgb_array(im) for im in frames]
    if not arrays or len(arrays) > PRE_MAX_FRAMES or any(a is None for a in arrays):
        return None
    if not all(preprocess_in_domain(a.shape[0], a.shape[1], out_h, out_w) for a in arrays):
        return None
    return arrays, (out_h, out_w), factor


def processor_preprocess(self, images, annotations=None, return_segmentation_masks=None, masks_path=None, **kwargs):
    """RTDetrImageProcessorPil.preprocess of a processor bound by bind_processor: the kernel path where `_processor_fast_path`
    holds (pixel_values come back on the current CUDA device), upstream's own method with its result untouched otherwise."""
    fast = _processor_fast_path(self, images, annotations, kwargs)
    if fast is None:
        preprocess_calls["original"] += 1
        return self._m355_unbound.preprocess(self, images, annotations, return_segmentation_masks, masks_path, **kwargs)
    from transformers.image_processing_base import BatchFeature
    arrays, size, factor = fast
    preprocess_calls["kernel"] += 1
    return BatchFeature({"pixel_values": preprocess_images(arrays, size, factor)})


_bound_processor_classes: dict = {}


def bind_processor(processor):
    """Make processor(images=frames, return_tensors="pt") return a BatchFeature whose pixel_values is already on the GPU
    (INTEGRATION.md): the INSTANCE gets a subclass of its own class, under the same name, whose `preprocess` is
    `processor_preprocess`.  Its class, its attributes, its config (to_dict) and what save_pretrained writes stay as they are;
    every call outside the fast path runs upstream's method.  Returns the processor."""
    cls = type(processor)
    if cls in _bound_processor_classes.values():
        return processor
    if cls not in _bound_processor_classes:
        _bound_processor_classes[cls] = type(cls.__name__, (cls,), {
            "preprocess": processor_preprocess, "_m355_unbound": cls,   # class attributes: the instance's __dict__ is its config
            "__module__": cls.__module__, "__qualname__": cls.__qualname__, "__doc__": cls.__doc__})
    processor.__class__ = _bound_processor_classes[cls]
    return processor


# ---- temporal encoder layers (nn.TransformerEncoderLayer, post-norm, ReLU, head dim 32) between their GEMMs ---------------------
# The D-FINE trainers put nn.TransformerEncoder(nn.TransformerEncoderLayer(256, 8, 1024, 0.1, batch_first=True), 4) on the frozen
# decoder's last_hidden_state (T frames = batch, Q queries = sequence) and train nothing else.  The nn.Linear layers stay torch
# GEMMs (autograd yields their weight gradients); everything between them is csrc/dfine_encoder.hip.
SITE_ATTN, SITE_ATTN_OUT, SITE_FFN, SITE_FFN_OUT = 0, 1, 2, 3   # dropout sites of a layer: the mask is f(seed, site, element)
ENCODER_HEAD_DIM = 32
ADDLN_MAX_D = 1024
encoder_calls = {"kernel": 0, "torch": 0}   # how many encoder_layer_forward calls took which path (tests and tools read it)


def _draw_seed() -> int:
    """one 62-bit integer from torch.default_generator (a host generator: no device synchronisation); torch.manual_seed
    makes the sequence reproducible"""
    return int(torch.randint(0, 1 << 62, (), dtype=torch.int64))


def _dropout_args(dropout_p: float, seed):
    p = float(dropout_p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout_p must be in [0, 1), got {dropout_p}")
    if p == 0.0:
        return 0.0, 0
    seed = _draw_seed() if seed is None else int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit in 64 unsigned bits")
    return p, seed


def _f32c16(t: torch.Tensor, name: str) -> torch.Tensor:
    """contiguous fp32 CUDA, 16-byte aligned: a view that is not (a column slice, an odd storage offset) is copied once"""
    t = _f32c(t, name)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def dropout_keep_mask(seed: int, site: int, shape, p: float, device=None) -> torch.Tensor:
    """The bool keep-mask the encoder kernels use for a tensor of `shape` at dropout site `site`, computed on the device by
    the same device function (dropout_keep4): element e (flat, row-major) is kept when word e % 4 of
    Philox4x32-10(counter = (e // 4, site, 0), key = seed) is >= floor(float32(p) * 2^32).  Not torch's mask stream."""
    shape = tuple(int(s) for s in shape)
    dev = torch.device("cuda") if device is None else torch.device(device)
    out = torch.empty(shape, dtype=torch.uint8, device=dev)
    if out.numel():
        check(lib.m355_dfine_dropout_mask(out.numel(), float(p), int(seed), int(site), _ptr(out), _stream()))
    return out.bool()


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, n_heads, p, seed, site):
        x = _f32c16(qkv, "qkv")
        out, lse = _attn_forward(x, n_heads, p, seed, site, True)
        ctx.save_for_backward(x, out, lse)   # the packed projection, the output and per-row statistics: no probabilities, no mask
        ctx.meta = (n_heads, p, seed, site, qkv.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, lse = ctx.saved_tensors
        n_heads, p, seed, site, dtype = ctx.meta
        B, S, _ = x.shape
        g = _f32c16(grad_out, "grad_output")
        gx = torch.empty_like(x)
        check(lib.m355_dfine_attn_backward(_ptr(g), _ptr(x), _ptr(out), _ptr(lse), B, S, n_heads, ENCODER_HEAD_DIM, p, seed, site,
                                           _ptr(gx), _stream()))
        return gx.to(dtype), None, None, None, None


def _attn_forward(x, n_heads, p, seed, site, keep_stats: bool):
    B, S, _ = x.shape
    out = torch.empty((B, S, n_heads * ENCODER_HEAD_DIM), dtype=torch.float32, device=x.device)
    lse = torch.empty((B, n_heads, S, 2), dtype=torch.float32, device=x.device) if keep_stats else None   # (max, log2 sum)
    check(lib.m355_dfine_attn_forward(_ptr(x), B, S, n_heads, ENCODER_HEAD_DIM, p, seed, site, _ptr(out), _ptr(lse), _stream()))
    return out, lse


def self_attention(qkv: torch.Tensor, n_heads: int, dropout_p: float = 0.0, seed=None, site: int = SITE_ATTN) -> torch.Tensor:
    """The core of nn.MultiheadAttention for head dim 32: qkv (B, S, 3 D), D = 32 * n_heads, exactly what
    F.linear(x, in_proj_weight, in_proj_bias) leaves (head h's q, k, v at columns 32 h, D + 32 h, 2 D + 32 h, read through
    strides) -> softmax(q k^T / sqrt(32)) [dropout on the probabilities] v as (B, S, D), the layout out_proj reads.  ONE launch
    forward, one backward; the S x S scores never reach memory and only the per-row log-sum-exp (B, H, S, held as the pair
    maximum, log2 of the sum) and the output are kept for the backward.  A qkv that is not contiguous (or not 16-byte aligned) is copied first.  dropout_p > 0 with seed=None draws
    a seed from torch.default_generator on the host."""
    if qkv.dim() != 3 or n_heads < 1 or qkv.shape[-1] != 3 * ENCODER_HEAD_DIM * n_heads:
        raise ValueError(f"qkv must be (B, S, 3 * {ENCODER_HEAD_DIM} * n_heads): the kernel takes head dim {ENCODER_HEAD_DIM} only")
    if qkv.shape[0] < 1 or qkv.shape[1] < 1:
        raise ValueError("qkv must have at least one frame and one token")
    p, seed = _dropout_args(dropout_p, seed)
    if _wants_grad(qkv):
        return _SelfAttention.apply(qkv, int(n_heads), p, seed, int(site))
    return _attn_forward(_f32c16(qkv, "qkv"), int(n_heads), p, seed, int(site), False)[0]


class _RowForm(NamedTuple):
    """One form of the row LayerNorm (csrc/dfine_rowln.hip) as _RowLayerNorm needs it.  The C entries take
    forward(sources, weight, bias, M, D, eps, scalars, out, mean, rstd, stream) and
    backward(grad_out, sources, weight, mean, rstd, M, D, scalars, source grads, dweight, dbias, work, work bytes, stream)."""
    forward: object
    backward: object
    names: tuple        # the source tensors as the public function names and takes them; the first has the output's shape (..., D)
    order: object       # itemgetter: the sources, and their gradients, in the order the C entries take them
    always_sums: bool   # the backward leaves its partial column sums even when neither dweight nor dbias is asked for


_ADD_LN = _RowForm(lib.m355_dfine_addln_forward, lib.m355_dfine_addln_backward,                     # scalars: p, seed, site
                   ("x", "y"), itemgetter(0, 1), True)
_ADD_CLAMP_LN = _RowForm(lib.m355_dfine_addln_clamp_forward, lib.m355_dfine_addln_clamp_backward,   # scalars: lo, hi
                         ("x", "y"), itemgetter(0, 1), True)
_GATE_LN = _RowForm(lib.m355_dfine_gate_ln_forward, lib.m355_dfine_gate_ln_backward,                # no scalars; entries: gate, x1, x2
                    ("x1", "x2", "gate_logits"), itemgetter(2, 0, 1), False)


class _RowLayerNorm(torch.autograd.Function):
    """Keeps the sources, the weight and the per-row mean and rstd: no mask, no sigmoid, no normalised row."""

    @staticmethod
    def forward(ctx, form, scalars, eps, weight, bias, *srcs):
        ts = tuple(map(_f32c16, srcs, form.names))
        w, b = _f32c16(weight, "weight"), _f32c16(bias, "bias")
        out, mean, rstd = _rowln_forward(form.forward, form.order(ts), w, b, eps, scalars, ts[0])
        ctx.save_for_backward(*ts, w, mean, rstd)
        ctx.meta = (form, scalars, [(t.shape, t.dtype) for t in (weight, bias, *srcs)])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        *ts, w, mean, rstd = ctx.saved_tensors
        form, scalars, like = ctx.meta
        D = w.numel()
        M = mean.numel()
        need = ctx.needs_input_grad   # form, scalars, eps, weight, bias, *srcs
        g = _f32c16(grad_out, "grad_output")
        gs = tuple(map(_grad_like, need[5:], ts))
        gw = torch.empty_like(w) if need[3] else None
        gb = torch.empty_like(w) if need[4] else None
        wbytes = int(lib.m355_dfine_addln_workspace_bytes(M, D)) if form.always_sums or need[3] or need[4] else 0
        work = torch.empty(wbytes, dtype=torch.uint8, device=w.device) if wbytes else None
        check(form.backward(_ptr(g), *map(_ptr, form.order(ts)), _ptr(w), _ptr(mean), _ptr(rstd), M, D, *scalars,
                            *map(_ptr, form.order(gs)), _ptr(gw), _ptr(gb), _ptr(work), wbytes, _stream()))
        return (None, None, None) + tuple(_as_input(t, *sd) for t, sd in zip((gw, gb, *gs), like))


def _rowln_forward(entry, srcs, w, b, eps, scalars, like):
    """entry: a form's forward C entry; srcs, w, b: its tensors as _f32c16 leaves them, srcs in the entry's order; like: the source
    with the output's shape -> out, mean, rstd"""
    D = like.shape[-1]
    M = like.numel() // D
    out = torch.empty_like(like)
    mean, rstd = like.new_empty(M), like.new_empty(M)
    check(entry(*map(_ptr, srcs), _ptr(w), _ptr(b), M, D, float(eps), *scalars, _ptr(out), _ptr(mean), _ptr(rstd), _stream()))
    return out, mean, rstd


def add_layer_norm(x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, dropout_p: float = 0.0,
                   seed=None, site: int = SITE_ATTN_OUT, clamp=None) -> torch.Tensor:
    """LayerNorm(x + dropout(y)) over the last axis (D a multiple of 4, at most 1024) in one pass: the residual, the dropout of
    the branch and the normalisation that torch runs as separate launches.  Differentiable in x, y, weight and bias; the
    backward recomputes the mask and the normalised rows from x, y and the saved per-row mean and rstd, and sums dweight and
    dbias in a fixed order (two launches).
    clamp=(lo, hi): LayerNorm(clamp(x + y, lo, hi)), the decoder layer's final_layer_norm(hidden.clamp(-65504, 65504)); x and y get
    no gradient where the sum lies strictly outside [lo, hi] (torch's clamp backward).  Without dropout: dropout_p must be 0."""
    D = x.shape[-1] if x.dim() else 0
    if x.dim() < 1 or x.shape != y.shape or tuple(weight.shape) != (D,) or tuple(bias.shape) != (D,):
        raise ValueError("x and y must have one shape (..., D), weight and bias the shape (D,)")
    if D < 4 or D % 4 or D > ADDLN_MAX_D or x.numel() == 0:
        raise ValueError(f"add_layer_norm takes a non-empty x with D a multiple of 4 in [4, {ADDLN_MAX_D}]")
    if clamp is not None:
        lo, hi = (float(v) for v in clamp)
        if not lo <= hi or float(dropout_p) != 0.0:
            raise ValueError("clamp=(lo, hi) needs lo <= hi and dropout_p == 0")
        form, scalars = _ADD_CLAMP_LN, (lo, hi)
    else:
        p, seed = _dropout_args(dropout_p, seed)
        form, scalars = _ADD_LN, (p, seed, int(site))
    if _wants_grad(x, y, weight, bias):
        return _RowLayerNorm.apply(form, scalars, float(eps), weight, bias, x, y)
    xs = _f32c16(x, "x")
    return _rowln_forward(form.forward, (xs, _f32c16(y, "y")), _f32c16(weight, "weight"), _f32c16(bias, "bias"), eps, scalars, xs)[0]


class _ReluDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, p, seed, site):
        out = _relu_dropout_forward(_f32c16(h, "h"), p, seed, site)
        ctx.save_for_backward(out)
        ctx.meta = (p, seed, site, h.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (out,) = ctx.saved_tensors
        p, seed, site, dtype = ctx.meta
        g = _f32c16(grad_out, "grad_output")
        gh = torch.empty_like(out)
        check(lib.m355_dfine_relu_dropout_backward(_ptr(g), _ptr(out), out.numel(), p, seed, site, _ptr(gh), _stream()))
        return gh.to(dtype), None, None, None


def _relu_dropout_forward(hs, p, seed, site):
    out = torch.empty_like(hs)
    check(lib.m355_dfine_relu_dropout_forward(_ptr(hs), hs.numel(), p, seed, site, _ptr(out), _stream()))
    return out


def relu_dropout(h: torch.Tensor, dropout_p: float = 0.0, seed=None, site: int = SITE_FFN) -> torch.Tensor:
    """dropout(relu(h)) in one elementwise launch; the backward (one launch) recomputes the mask and reads the sign of the
    saved output, the only tensor kept."""
    if h.numel() == 0:
        raise ValueError("relu_dropout takes a non-empty tensor")
    p, seed = _dropout_args(dropout_p, seed)
    if _wants_grad(h):
        return _ReluDropout.apply(h, p, seed, int(site))
    return _relu_dropout_forward(_f32c16(h, "h"), p, seed, int(site))


def _layer_is_kernel_shaped(layer) -> bool:
    """the module's own settings: post-norm, ReLU, batch_first, one packed in-projection, head dim 32, affine LayerNorms"""
    F = torch.nn.functional
    attn, act = layer.self_attn, layer.activation
    if layer.norm_first or not (act is F.relu or isinstance(act, torch.nn.ReLU)) or not getattr(attn, "batch_first", False):
        return False
    if not attn._qkv_same_embed_dim or attn.in_proj_weight is None or attn.bias_k is not None or attn.add_zero_attn:
        return False
    D = attn.embed_dim
    if attn.head_dim != ENCODER_HEAD_DIM or D > ADDLN_MAX_D:
        return False
    return _affine_norm(layer.norm1, D) and _affine_norm(layer.norm2, D)


def _encoder_layer_takes(layer, src, src_mask, src_key_padding_mask, is_causal) -> bool:
    """True when the kernels cover this call of an nn.TransformerEncoderLayer; anything else goes to torch's forward"""
    if src_mask is not None or src_key_padding_mask is not None or is_causal:
        return False
    if src.is_nested or src.dim() != 3 or not src.is_cuda or src.dtype != torch.float32 or src.numel() == 0:
        return False
    if torch.is_autocast_enabled() or not _layer_is_kernel_shaped(layer) or src.shape[-1] != layer.self_attn.embed_dim:
        return False
    return _fp32_cuda_params(layer)


def encoder_layer_forward(self, src, src_mask=None, src_key_padding_mask=None, is_causal=False):
    """nn.TransformerEncoderLayer.forward for the post-norm ReLU layer with head dim 32 on fp32 CUDA tensors: the four nn.Linear
    products are torch GEMMs on the module's own parameters, everything between them is three kernel-backed ops,
        x = add_layer_norm(x, out_proj(self_attention(in_proj(x))), norm1)
        x = add_layer_norm(x, linear2(relu_dropout(linear1(x))), norm2)
    with dropout (the module's own probabilities, one host-drawn seed per op) only when self.training.  A mask or padding mask,
    is_causal, norm_first=True, another activation, batch_first=False, head dim != 32, non-fp32 or CPU tensors and autocast go
    to the class's own forward, untouched.  Bound per instance by bind_encoder."""
    if not _encoder_layer_takes(self, src, src_mask, src_key_padding_mask, is_causal):
        encoder_calls["torch"] += 1
        return type(self).forward(self, src, src_mask=src_mask, src_key_padding_mask=src_key_padding_mask, is_causal=is_causal)
    encoder_calls["kernel"] += 1
    F = torch.nn.functional
    attn = self.self_attn
    train = self.training
    qkv = F.linear(src, attn.in_proj_weight, attn.in_proj_bias)
    a = self_attention(qkv, attn.num_heads, attn.dropout if train else 0.0, site=SITE_ATTN)
    y = F.linear(a, attn.out_proj.weight, attn.out_proj.bias)
    x = add_layer_norm(src, y, self.norm1.weight, self.norm1.bias, self.norm1.eps, self.dropout1.p if train else 0.0,
                       site=SITE_ATTN_OUT)
    h = relu_dropout(F.linear(x, self.linear1.weight, self.linear1.bias), self.dropout.p if train else 0.0, site=SITE_FFN)
    y = F.linear(h, self.linear2.weight, self.linear2.bias)
    return add_layer_norm(x, y, self.norm2.weight, self.norm2.bias, self.norm2.eps, self.dropout2.p if train else 0.0,
                          site=SITE_FFN_OUT)


def bind_encoder(encoder):
    """Set encoder_layer_forward on every nn.TransformerEncoderLayer INSTANCE inside `encoder` (an nn.TransformerEncoder, a
    single layer, or any module that holds some); torch's class is never touched, parameters, buffers and the state dict stay as
    they are, so existing checkpoints load unchanged.  Returns `encoder`."""
    _bind_forward(encoder, {torch.nn.TransformerEncoderLayer: encoder_layer_forward})
    return encoder


# ---- the context GRU of the improved temporal trainer (nn.GRU(256, 256, batch_first, bidirectional) on ONE sequence of T * Q steps)
# The input projection stays one torch GEMM for all steps and both directions; the serial chain is csrc/dfine_gru.hip.
GRU_HIDDEN = 256
GRU_MAX_BATCH = 8
gru_calls = {"kernel": 0, "torch": 0}   # how many gru_forward calls took which path (tests and tools read it)
_gru_status_words = {}                  # device index -> the int32 word the kernels OR their give-up bit into


def _gru_status_word(device: torch.device) -> torch.Tensor:
    word = _gru_status_words.get(device.index)
    if word is None:
        # zeroed on the host and copied synchronously once, so that no stream can meet the word before its zero
        word = _gru_status_words[device.index] = torch.zeros(1, dtype=torch.int32).to(device)
        torch.cuda.synchronize(device)
    return word


def gru_status() -> int:
    """0, or the OR of the give-up bits the GRU kernels have set on any device since import (1: a forward workgroup, 2: a backward
    workgroup stopped waiting for its chain's other workgroups and wrote NaN to the rest of its outputs).  One synchronising
    read per device that ran the kernels, on demand; nothing else reads the word."""
    bits = 0
    for word in _gru_status_words.values():
        bits |= int(word[0].item())
    return bits


def _gru_work(B: int, S: int, D: int, device) -> torch.Tensor:
    return torch.empty(int(lib.m355_dfine_gru_workspace_bytes(B, S, GRU_HIDDEN, D)), dtype=torch.uint8, device=device)


def _gru_forward(gi, w_hh, b_hh, h0, keep: bool):
    """contiguous aligned fp32 CUDA tensors -> out, h_n and the workspace (the saved gates behind the exchange area when keep)"""
    B, S, _ = gi.shape
    D = w_hh.shape[0]
    out = torch.empty((B, S, D * GRU_HIDDEN), dtype=torch.float32, device=gi.device)
    h_n = torch.empty((D, B, GRU_HIDDEN), dtype=torch.float32, device=gi.device)
    work = _gru_work(B, S if keep else 0, D, gi.device)
    check(lib.m355_dfine_gru_forward(_ptr(gi), _ptr(w_hh), _ptr(b_hh), _ptr(h0), B, S, GRU_HIDDEN, D, _ptr(out), _ptr(h_n), _ptr(work),
                                     work.numel(), int(keep), _ptr(_gru_status_word(gi.device)), _stream()))
    return out, h_n, work


def _gru_h_prev(out, h0, B, S, D):
    """(B, S, D, H): the state each step started from, by time index (direction 1 reads the step after it)"""
    o = out.view(B, S, D, GRU_HIDDEN)
    hp = torch.empty_like(o)
    hp[:, 1:, 0] = o[:, :-1, 0]
    hp[:, 0, 0] = h0[0] if h0 is not None else 0.0
    if D == 2:
        hp[:, :-1, 1] = o[:, 1:, 1]
        hp[:, -1, 1] = h0[1] if h0 is not None else 0.0
    return hp


class _GruRecurrence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0):
        g, w, b = _f32c16(gi, "gi"), _f32c16(w_hh, "weight_hh"), _f32c16(b_hh, "bias_hh")
        h = None if h0 is None else _f32c16(h0, "h0")
        out, h_n, work = _gru_forward(g, w, b, h, True)
        ctx.save_for_backward(w, h, out, work)   # the gates live in work; gi itself is not kept
        ctx.meta = [(t.shape, t.dtype) if t is not None else None for t in (gi, w_hh, b_hh, h0)]
        ctx.set_materialize_grads(False)
        return out, h_n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, grad_h_n):
        w, h0, out, work = ctx.saved_tensors
        B, S, DH = out.shape
        H = GRU_HIDDEN
        D = DH // H
        need = ctx.needs_input_grad
        g = _f32c16(grad_out, "grad_output") if grad_out is not None else torch.zeros_like(out)
        gh = _f32c16(grad_h_n, "grad_h_n") if grad_h_n is not None else None
        ggi = torch.empty((B, S, D * 3 * H), dtype=torch.float32, device=out.device)
        gan = torch.empty((B, S, D * H), dtype=torch.float32, device=out.device)
        gh0 = torch.empty((D, B, H), dtype=torch.float32, device=out.device)
        check(lib.m355_dfine_gru_backward(_ptr(g), _ptr(gh), _ptr(w), _ptr(h0), _ptr(out), B, S, H, D, _ptr(ggi), _ptr(gan), _ptr(gh0),
                                          _ptr(work), work.numel(), _ptr(_gru_status_word(out.device)), _stream()))
        gw = gb = None
        if need[1] or need[2]:
            ga = ggi.view(B, S, D, 3 * H).clone()      # what W_hh saw: the n-part carries the reset gate
            ga[..., 2 * H:] = gan.view(B, S, D, H)
            if need[2]:
                gb = ga.sum(dim=(0, 1))
            if need[1]:
                hp = _gru_h_prev(out, h0, B, S, D)
                gw = torch.stack([ga[:, :, d].reshape(B * S, 3 * H).t() @ hp[:, :, d].reshape(B * S, H) for d in range(D)])
        grads = (ggi if need[0] else None, gw, gb, gh0 if need[3] else None)
        return tuple(_as_input(t, *sd) if sd is not None else None for t, sd in zip(grads, ctx.meta))


def gru_recurrence(gi: torch.Tensor, weight_hh: torch.Tensor, bias_hh: torch.Tensor, h0=None):
    """The serial part of torch's one-layer GRU with hidden size 256: gi (B, S, D * 768) = the input-side pre-activations of all
    steps (x @ cat(W_ih, W_ih_reverse).T + b_ih; gate order r, z, n; direction 1 in the second half of the last axis),
    weight_hh (D, 768, 256), bias_hh (D, 768), h0 (D, B, 256) or None -> out (B, S, D * 256), h_n (D, B, 256); D in {1, 2},
    B <= 8.  ONE launch forward and one backward for all chains; differentiable in all four inputs (grad_weight_hh and
    grad_bias_hh are one GEMM and one column sum over what the backward kernel stored).  With nothing to differentiate no gate
    is saved.  A gi that is not contiguous (or not 16-byte aligned) is copied first."""
    H = GRU_HIDDEN
    if weight_hh.dim() != 3 or weight_hh.shape[0] not in (1, 2) or tuple(weight_hh.shape[1:]) != (3 * H, H):
        raise ValueError(f"weight_hh must be (D, {3 * H}, {H}) with D in (1, 2): the kernel takes hidden size {H} only")
    D = weight_hh.shape[0]
    if tuple(bias_hh.shape) != (D, 3 * H):
        raise ValueError(f"bias_hh must be (D, {3 * H})")
    if gi.dim() != 3 or gi.shape[2] != D * 3 * H or gi.shape[1] < 1 or not 1 <= gi.shape[0] <= GRU_MAX_BATCH:
        raise ValueError(f"gi must be (B, S, D * {3 * H}) with 1 <= B <= {GRU_MAX_BATCH} and S >= 1")
    if h0 is not None and tuple(h0.shape) != (D, gi.shape[0], H):
        raise ValueError(f"h0 must be (D, B, {H})")
    if _wants_grad(gi, weight_hh, bias_hh, *(() if h0 is None else (h0,))):
        return _GruRecurrence.apply(gi, weight_hh, bias_hh, h0)
    out, h_n, _ = _gru_forward(_f32c16(gi, "gi"), _f32c16(weight_hh, "weight_hh"), _f32c16(bias_hh, "bias_hh"),
                               None if h0 is None else _f32c16(h0, "h0"), False)
    return out, h_n


def _gru_takes(gru, input, hx) -> bool:
    """True when the kernel covers this call of an nn.GRU; anything else goes to torch's forward"""
    if not torch.is_tensor(input) or input.dim() != 3 or not input.is_cuda or input.dtype != torch.float32:
        return False
    if gru.num_layers != 1 or not gru.batch_first or not gru.bias or gru.hidden_size != GRU_HIDDEN or getattr(gru, "proj_size", 0):
        return False
    if torch.is_autocast_enabled() or input.shape[2] != gru.input_size or input.shape[1] < 1 or not 1 <= input.shape[0] <= GRU_MAX_BATCH:
        return False
    D = 2 if gru.bidirectional else 1
    if hx is not None and not (torch.is_tensor(hx) and hx.is_cuda and hx.dtype == torch.float32
                               and tuple(hx.shape) == (D, input.shape[0], GRU_HIDDEN)):
        return False
    return _fp32_cuda_params(gru)


def gru_forward(self, input, hx=None):
    """nn.GRU.forward (same arguments, same (output, h_n)) for one layer, batch_first, hidden size 256, uni- or bidirectional, on a
    3-d fp32 CUDA input with B <= 8: one torch GEMM on the module's own weight_ih / bias_ih for all steps and both directions,
    then gru_recurrence.  num_layers > 1 (and its dropout), proj_size, bias=False, batch_first=False, a PackedSequence, a 2-d
    input, another hidden size, non-fp32 or CPU tensors and autocast go to the class's own forward, untouched.  Bound per
    instance by bind_gru."""
    if not _gru_takes(self, input, hx):
        gru_calls["torch"] += 1
        return type(self).forward(self, input, hx)
    gru_calls["kernel"] += 1
    sfx = ("", "_reverse") if self.bidirectional else ("",)
    par = lambda name: [getattr(self, f"{name}_l0{s}") for s in sfx]
    gi = torch.nn.functional.linear(input, torch.cat(par("weight_ih")), torch.cat(par("bias_ih")))
    return gru_recurrence(gi, torch.stack(par("weight_hh")), torch.stack(par("bias_hh")), hx)


def bind_gru(module):
    """Set gru_forward on every nn.GRU INSTANCE inside `module` (an nn.GRU or any module that holds some); torch's class is never
    touched, parameters and the state dict stay as they are, so existing checkpoints load unchanged.  Returns `module`."""
    _bind_forward(module, {torch.nn.GRU: gru_forward})
    return module


# ---- D-FINE decoder layers and their quality heads (transformers' DFineDecoderLayer / DFineLQE) between their GEMMs --------------
# Every trainer runs the six decoder layers forward and backward on every step.  The nn.Linear layers stay torch GEMMs on the
# modules' own parameters (autograd yields their weight gradients); between them: self_attention, add_layer_norm,
# deformable_attention, gate_layer_norm, relu_dropout, add_layer_norm(clamp=...) (csrc/dfine_rowln.hip) and lqe_statistics (csrc/dfine_decoder.hip).
LQE_MAX_BINS1 = 64
LQE_MAX_TOPK = 8
DECODER_CLAMP = (-65504.0, 65504.0)   # DFineDecoderLayer.forward: final_layer_norm(hidden_states.clamp(min=-65504, max=65504))
decoder_calls = {"kernel": 0, "torch": 0}   # decoder_layer_forward and lqe_forward calls by path (tests and tools read it)


def gate_layer_norm(x1: torch.Tensor, x2: torch.Tensor, gate_logits: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                    eps: float) -> torch.Tensor:
    """DFineGate.forward behind its nn.Linear: LayerNorm(sigmoid(g[..., :D]) * x1 + sigmoid(g[..., D:]) * x2) with
    g = gate(cat(x1, x2)) of shape (..., 2 D), D a multiple of 4 in [4, 1024], in ONE launch.  Differentiable in x1, x2,
    gate_logits, weight and bias; only the inputs and the per-row mean and rstd are kept, the backward (one launch, plus the
    ordered column sums of dweight and dbias when asked for) forms the sigmoids and the normalised row again."""
    D = x1.shape[-1] if x1.dim() else 0
    if x1.dim() < 1 or x1.shape != x2.shape or tuple(gate_logits.shape) != tuple(x1.shape[:-1]) + (2 * D,):
        raise ValueError("x1 and x2 must have one shape (..., D) and gate_logits the shape (..., 2 D)")
    if tuple(weight.shape) != (D,) or tuple(bias.shape) != (D,):
        raise ValueError("weight and bias must have the shape (D,)")
    if D < 4 or D % 4 or D > ADDLN_MAX_D or x1.numel() == 0:
        raise ValueError(f"gate_layer_norm takes a non-empty x1 with D a multiple of 4 in [4, {ADDLN_MAX_D}]")
    if _wants_grad(x1, x2, gate_logits, weight, bias):
        return _RowLayerNorm.apply(_GATE_LN, (), float(eps), weight, bias, x1, x2, gate_logits)
    a, b, g = _f32c16(x1, "x1"), _f32c16(x2, "x2"), _f32c16(gate_logits, "gate_logits")
    return _rowln_forward(_GATE_LN.forward, (g, a, b), _f32c16(weight, "weight"), _f32c16(bias, "bias"), eps, (), a)[0]


class _LqeStatistics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_corners, nb1, k):
        c = _f32c(pred_corners, "pred_corners")
        stat, idx = _lqe_forward(c, nb1, k, True)
        ctx.save_for_backward(c, idx)   # the logits and the chosen bins as bytes: no probabilities
        ctx.meta = (nb1, k, pred_corners.dtype)
        return stat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stat):
        c, idx = ctx.saved_tensors
        nb1, k, dtype = ctx.meta
        g = _f32c(grad_stat, "grad_output")
        gc = torch.empty_like(c)
        check(lib.m355_dfine_lqe_backward(_ptr(g), _ptr(c), _ptr(idx), c.numel() // (4 * nb1), nb1, k, _ptr(gc), _stream()))
        return gc.to(dtype), None, None


def _lqe_forward(c, nb1, k, keep_index: bool):
    M = c.numel() // (4 * nb1)
    stat = torch.empty(tuple(c.shape[:-1]) + (4 * (k + 1),), dtype=torch.float32, device=c.device)
    idx = torch.empty((M, 4, k), dtype=torch.uint8, device=c.device) if keep_index else None
    check(lib.m355_dfine_lqe_forward(_ptr(c), M, nb1, k, _ptr(stat), _ptr(idx), _stream()))
    return stat, idx


def lqe_statistics(pred_corners: torch.Tensor, max_num_bins: int, top_k: int) -> torch.Tensor:
    """DFineLQE.forward in front of its MLP: pred_corners (..., 4 * (max_num_bins + 1)) -> (..., 4 * (top_k + 1)), per box side the
    softmax over its max_num_bins + 1 logits, the top_k largest probabilities in descending order and then their mean (the layout
    reg_conf reads), in ONE launch.  Of bins with exactly equal probability the lowest bin counts as the larger one, which decides
    where the gradient of a tie goes (the values do not depend on it).  top_k in [1, 8], top_k <= max_num_bins + 1 <= 64.
    Differentiable; the backward (one launch) reads the logits and the chosen bins, kept as bytes."""
    nb1, k = int(max_num_bins) + 1, int(top_k)
    if not 1 <= k <= LQE_MAX_TOPK or not k <= nb1 <= LQE_MAX_BINS1:
        raise ValueError(f"lqe_statistics takes top_k in [1, {LQE_MAX_TOPK}] and top_k <= max_num_bins + 1 <= {LQE_MAX_BINS1}")
    if pred_corners.dim() < 1 or pred_corners.shape[-1] != 4 * nb1 or pred_corners.numel() == 0:
        raise ValueError("pred_corners must be a non-empty (..., 4 * (max_num_bins + 1)) tensor")
    if _wants_grad(pred_corners):
        return _LqeStatistics.apply(pred_corners, nb1, k)
    return _lqe_forward(_f32c(pred_corners, "pred_corners"), nb1, k, False)[0]


def _fp32_cuda(*tensors) -> bool:
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _affine_norm(norm, D: int) -> bool:
    return (isinstance(norm, torch.nn.LayerNorm) and tuple(norm.normalized_shape) == (D,) and norm.weight is not None
            and norm.bias is not None)


def _records_attentions(layer, kwargs) -> bool:
    """transformers collects attention weights through forward hooks on the two attention submodules"""
    if kwargs.get("output_attentions") or getattr(getattr(layer.self_attn, "config", None), "output_attentions", False):
        return True
    return any(len(m._forward_hooks) or len(m._forward_pre_hooks) for m in (layer.self_attn, layer.encoder_attn))


def _decoder_layer_takes(layer, hidden_states, position_embeddings, encoder_hidden_states, encoder_attention_mask, kwargs) -> bool:
    """True when the kernels cover this call of a DFineDecoderLayer; anything else goes to the class's own forward"""
    if encoder_attention_mask is not None or _records_attentions(layer, kwargs):
        return False
    sa = layer.self_attn
    if layer.training and (float(layer.dropout) > 0.0 or float(sa.attention_dropout) > 0.0):
        return False
    x = hidden_states
    if not _fp32_cuda(x, encoder_hidden_states) or x.dim() != 3 or x.numel() == 0 or torch.is_autocast_enabled():
        return False
    if position_embeddings is not None and not (_fp32_cuda(position_embeddings) and position_embeddings.shape == x.shape):
        return False
    D = x.shape[-1]
    if sa.head_dim != ENCODER_HEAD_DIM or D % ENCODER_HEAD_DIM or D != layer.hidden_size or D > ADDLN_MAX_D:
        return False
    if any(lin.bias is None for lin in (sa.q_proj, sa.k_proj, sa.v_proj, sa.o_proj)):
        return False
    mlp = layer.mlp
    if not isinstance(mlp.act, torch.nn.ReLU) or mlp.num_layers != 2 or len(mlp.layers) != 2:
        return False
    if not all(_affine_norm(n, D) for n in (layer.self_attn_layer_norm, layer.gateway.norm, layer.final_layer_norm)):
        return False
    return _fp32_cuda_params(layer)


def decoder_layer_forward(self, hidden_states, position_embeddings=None, reference_points=None, spatial_shapes=None,
                          spatial_shapes_list=None, encoder_hidden_states=None, encoder_attention_mask=None, **kwargs):
    """DFineDecoderLayer.forward (modeling_d_fine.py, transformers 5.15.0) on fp32 CUDA tensors, the nn.Linear products as torch
    GEMMs on the module's own parameters and everything between them on the kernels:
        x = add_layer_norm(x, o_proj(self_attention([q | k](x + pos), v(x))), self_attn_layer_norm)   # k without its bias
        c = deformable_attention(x + pos, ...)
        x = gate_layer_norm(x, c, gateway.gate(cat(x, c)), gateway.norm)
        x = add_layer_norm(x, mlp.layers[1](relu_dropout(mlp.layers[0](x))), final_layer_norm, clamp=(-65504, 65504))
    A call goes to the class's own forward, untouched, when encoder_attention_mask is given (the denoising groups), when the module
    trains with config.dropout or attention_dropout above 0, when tensors or parameters are not fp32 CUDA, under autocast, on an
    empty input, with a head dim other than 32 or D not a multiple of 4 in [4, 1024], with an activation other than ReLU, and when
    attention weights are recorded (output_attentions, or a forward hook on either attention submodule).  2-d reference points
    and the "discrete" method keep self.encoder_attn(...) for the cross-attention and the kernels for the rest.
    bind_decoder(attention=False) keeps self.self_attn(...) as well.  Bound per instance by bind_decoder."""
    if not _decoder_layer_takes(self, hidden_states, position_embeddings, encoder_hidden_states, encoder_attention_mask, kwargs):
        decoder_calls["torch"] += 1
        return type(self).forward(self, hidden_states, position_embeddings=position_embeddings, reference_points=reference_points,
                                  spatial_shapes=spatial_shapes, spatial_shapes_list=spatial_shapes_list,
                                  encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask, **kwargs)
    decoder_calls["kernel"] += 1
    F = torch.nn.functional
    x, pos, sa = hidden_states, position_embeddings, self.self_attn
    if getattr(self, "_m355_attention_kernel", False):
        qk_in = x if pos is None else x + pos
        # k_proj.bias adds the same q . b to every key's logit of a query, which the softmax cancels: the keys are formed without it
        # and its gradient is the exact 0 (times 0, so that it stays in the graph) instead of fp32 rounding noise around 0
        qk = F.linear(qk_in, torch.cat([sa.q_proj.weight, sa.k_proj.weight]), torch.cat([sa.q_proj.bias, sa.k_proj.bias * 0.0]))
        qkv = torch.cat([qk, F.linear(x, sa.v_proj.weight, sa.v_proj.bias)], dim=-1)
        y = F.linear(self_attention(qkv, x.shape[-1] // ENCODER_HEAD_DIM), sa.o_proj.weight, sa.o_proj.bias)
    else:
        y = sa(hidden_states=x, attention_mask=None, position_embeddings=pos, **kwargs)[0]
    n = self.self_attn_layer_norm
    x = add_layer_norm(x, y, n.weight, n.bias, n.eps)

    ca = self.encoder_attn
    q = x if pos is None else x + pos
    pts = [int(v) for v in ca.num_points_list]
    if (reference_points is not None and reference_points.shape[-1] == 4 and ca.decoder_method == "default" and sum(pts) <= 16
            and len(pts) <= 8 and spatial_shapes_list is not None and _fp32_cuda(reference_points)):
        c = deformable_attention(q, reference_points, encoder_hidden_states, spatial_shapes_list, ca.sampling_offsets,
                                 ca.attention_weights, pts, ca.n_heads, ca.offset_scale)
    else:
        c = ca(hidden_states=q, encoder_hidden_states=encoder_hidden_states, reference_points=reference_points,
               spatial_shapes=spatial_shapes, spatial_shapes_list=spatial_shapes_list)[0]

    gw = self.gateway
    g = F.linear(torch.cat([x, c], dim=-1), gw.gate.weight, gw.gate.bias)
    x = gate_layer_norm(x, c, g, gw.norm.weight, gw.norm.bias, gw.norm.eps)

    l0, l1 = self.mlp.layers
    y = F.linear(relu_dropout(F.linear(x, l0.weight, l0.bias), 0.0), l1.weight, l1.bias)
    n = self.final_layer_norm
    return add_layer_norm(x, y, n.weight, n.bias, n.eps, clamp=DECODER_CLAMP)


def lqe_forward(self, scores, pred_corners):
    """DFineLQE.forward: scores + self.reg_conf(lqe_statistics(pred_corners, self.max_num_bins, self.top_prob_values)); reg_conf
    stays the module's own MLP.  CPU or non-fp32 tensors, autocast, an empty input and bin or top-k counts outside the kernel's
    limits go to the class's own forward, untouched.  Bound per instance by bind_decoder."""
    nb1, k = int(self.max_num_bins) + 1, int(self.top_prob_values)
    if not (_fp32_cuda(scores, pred_corners) and pred_corners.dim() == 3 and pred_corners.numel() and not torch.is_autocast_enabled()
            and pred_corners.shape[-1] == 4 * nb1 and 1 <= k <= LQE_MAX_TOPK and k <= nb1 <= LQE_MAX_BINS1
            and _fp32_cuda_params(self)):
        decoder_calls["torch"] += 1
        return type(self).forward(self, scores, pred_corners)
    decoder_calls["kernel"] += 1
    return scores + self.reg_conf(lqe_statistics(pred_corners, self.max_num_bins, k))


def bind_decoder(module, attention: bool = False):
    """Set decoder_layer_forward on every DFineDecoderLayer INSTANCE and lqe_forward on every DFineLQE INSTANCE inside `module` (a
    DFineDecoder, a whole DFineForObjectDetection, a single layer, or any module that holds some); transformers' classes are never
    touched, parameters, buffers and the state dict stay as they are, so existing checkpoints load unchanged.  Returns `module`.
    attention=False keeps each layer's self.self_attn(...) as the class runs it and takes the other ops; attention=True runs the
    self-attention core on dfine.self_attention too.  The default is the arm that profiles/dfine_decoder_bench.json shows faster for
    a layer's training step (forward + backward) at (50, 300, 256): torch's scaled_dot_product_attention, 3.29 ms against 3.60 ms
    (the attention backward kernel runs on VALU FMAs); at (16, 300, 256) and below the two are within each other's spread."""
    from transformers.models.d_fine import modeling_d_fine as M   # lazily: the package does not need transformers otherwise
    for m in _bind_forward(module, {M.DFineDecoderLayer: decoder_layer_forward, M.DFineLQE: lqe_forward}):
        if isinstance(m, M.DFineDecoderLayer):
            m._m355_attention_kernel = bool(attention)   # a plain attribute: not a parameter, not a buffer, not in the state dict
    return module


# ---- the decoder's own loop around its layers (DFineDecoder.forward, modeling_d_fine.py:1184-1293) ------------------------------
# Six times per call, between the layers bind_decoder covers: query_pos_head, pre_bbox_head / bbox_embed[i], the corner accumulation,
# the integral and distance2bbox, and at layer 0 inverse_sigmoid + sigmoid.  The nn.Linear products stay torch GEMMs on the module's
# own parameters; between them query_pos_hidden, relu_dropout, refine_reference and refine_boxes (csrc/dfine_loop.hip).
QUERY_POS_MAX_H = 2048           # the limits of m355_dfine_query_pos_*; anything outside them takes query_pos_hidden_torch
loop_calls = {"kernel": 0, "torch": 0}   # decoder_forward calls by path (tests and tools read it)


def query_pos_hidden_torch(ref: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """query_pos_hidden in torch ops, any device and dtype"""
    return torch.relu(torch.nn.functional.linear(ref, weight, bias))


def _qp_forward(r, w, b) -> torch.Tensor:
    H = w.shape[0]
    out = torch.empty(tuple(r.shape[:-1]) + (H,), dtype=torch.float32, device=r.device)
    check(lib.m355_dfine_query_pos_forward(_ptr(r), _ptr(w), _ptr(b), r.numel() // 4, H, _ptr(out), _stream()))
    return out


class _QueryPosHidden(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref, weight, bias):
        r, w = _f32c16(ref, "ref"), _f32c16(weight, "weight")
        out = _qp_forward(r, w, _f32c16(bias, "bias"))
        ctx.save_for_backward(out, r, w)   # the mask is the sign of the output
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        out, r, w = ctx.saved_tensors
        N, H = r.numel() // 4, w.shape[0]
        g = _f32c16(grad_out, "grad_output")
        need = ctx.needs_input_grad
        gr, gw = _grad_like(need[0], r), _grad_like(need[1], w)
        gb = torch.empty(H, dtype=torch.float32, device=w.device) if need[2] else None
        work, nbytes = None, 0
        if need[1] or need[2]:   # the slabs' partial rows of dweight | dbias
            nbytes = int(lib.m355_dfine_query_pos_workspace_bytes(N, H))
            work = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        check(lib.m355_dfine_query_pos_backward(_ptr(g), _ptr(out), _ptr(r), _ptr(w), N, H, _ptr(gr), _ptr(gw), _ptr(gb), _ptr(work),
                                                nbytes, _stream()))
        return gr, gw, gb


def query_pos_hidden(ref: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """relu(ref @ weight.T + bias), the first Linear + ReLU of DFineDecoder.query_pos_head: ref (..., 4), weight (H, 4), bias (H,) ->
    (..., H) in ONE launch (N H floats written, 4 FMAs each).  Differentiable in all three; the backward reads the saved output for
    the mask (gradient 0 where the pre-activation is <= 0, as torch's ReLU), leaves per-slab partial rows of dweight | dbias and adds
    them in slab order (one launch + the ordered sum); dref is formed only where asked, a gradient not asked for is a null pointer.
    CPU or non-fp32 tensors, autocast, an empty ref and H outside the multiples of 4 in [4, 2048] take query_pos_hidden_torch."""
    H = weight.shape[0] if weight.dim() == 2 else -1
    if ref.dim() < 1 or ref.shape[-1] != 4 or weight.dim() != 2 or weight.shape[1] != 4 or tuple(bias.shape) != (H,):
        raise ValueError("ref must be (..., 4), weight (H, 4) and bias (H,)")
    if not (_fp32_cuda(ref, weight, bias) and not torch.is_autocast_enabled() and ref.numel() and H % 4 == 0
            and 4 <= H <= QUERY_POS_MAX_H):
        return query_pos_hidden_torch(ref, weight, bias)
    if _wants_grad(ref, weight, bias):
        return _QueryPosHidden.apply(ref, weight, bias)
    return _qp_forward(_f32c16(ref, "ref"), _f32c16(weight, "weight"), _f32c16(bias, "bias"))


def refine_reference_torch(delta: torch.Tensor, ref: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """refine_reference in torch ops: upstream's inverse_sigmoid (modeling_d_fine.py:1084-1088) operation for operation"""
    x = ref.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.sigmoid(delta + torch.log(x1 / x2))


def _refine_reference_forward(d, r, eps: float) -> torch.Tensor:
    out = torch.empty_like(d)
    check(lib.m355_dfine_refine_reference_forward(_ptr(d), _ptr(r), d.numel(), eps, _ptr(out), _stream()))
    return out


class _RefineReference(torch.autograd.Function):
    @staticmethod
    def forward(ctx, delta, ref, eps):
        out = _refine_reference_forward(_f32c(delta, "delta"), _f32c(ref, "ref"), eps)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (out,) = ctx.saved_tensors
        g = _f32c(grad_out, "grad_output")
        gd = torch.empty_like(out)
        check(lib.m355_dfine_refine_reference_backward(_ptr(g), _ptr(out), out.numel(), _ptr(gd), _stream()))
        return gd, None, None


def refine_reference(delta: torch.Tensor, ref: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """sigmoid(delta + inverse_sigmoid(ref, eps)), the reference points DFineDecoder.forward forms at layer 0, in ONE launch; delta
    and ref have one shape.  The gradient goes to delta only (one launch, from the saved output): a ref that requires grad, CPU or
    non-fp32 tensors, autocast and an empty input take refine_reference_torch."""
    if delta.shape != ref.shape:
        raise ValueError("delta and ref must have one shape")
    if not (_fp32_cuda(delta, ref) and not torch.is_autocast_enabled() and delta.numel() and float(eps) >= 0.0
            and not _wants_grad(ref)):
        return refine_reference_torch(delta, ref, eps)
    if _wants_grad(delta):
        return _RefineReference.apply(delta, ref, float(eps))
    return _refine_reference_forward(_f32c(delta, "delta"), _f32c(ref, "ref"), float(eps))


def refine_boxes_torch(delta_corners: torch.Tensor, prev_corners, project: torch.Tensor, points: torch.Tensor, reg_scale):
    """refine_boxes in torch ops: upstream's add, DFineIntegral.forward (softmax + linear) and distance2bbox"""
    pred = delta_corners if prev_corners is None else delta_corners + prev_corners
    nb1 = project.numel()
    p = torch.softmax(pred.reshape(-1, nb1), dim=1)
    d = torch.nn.functional.linear(p, project.to(p.device).reshape(1, -1)).reshape(tuple(pred.shape[:-1]) + (4,))
    return pred, distance2bbox(points, d, reg_scale)


def _refine_boxes_forward(d, pv, pr, pt, reg_scale: float):
    pred = torch.empty_like(d) if pv is not None else None
    boxes = torch.empty(tuple(d.shape[:-1]) + (4,), dtype=torch.float32, device=d.device)
    check(lib.m355_dfine_refine_boxes_forward(_ptr(d), _ptr(pv), _ptr(pr), _ptr(pt), boxes.numel() // 4, pr.numel(), reg_scale,
                                              _ptr(pred), _ptr(boxes), _stream()))
    return (d if pred is None else pred), boxes


class _RefineBoxes(torch.autograd.Function):
    """refine_boxes with m355_dfine_refine_boxes_backward behind it.  Without prev_corners the one output is boxes: pred_corners is
    delta_corners itself, and autograd adds what flows into it elsewhere."""

    @staticmethod
    def forward(ctx, delta, prev, project, points, reg_scale):
        d, pv = _f32c16(delta, "delta_corners"), None if prev is None else _f32c16(prev, "prev_corners")
        pr, pt = _f32c(project, "project"), _f32c16(points, "points")
        pred, boxes = _refine_boxes_forward(d, pv, pr, pt, reg_scale)
        ctx.save_for_backward(pred, pr, pt)
        ctx.meta = (reg_scale, prev is not None)
        ctx.set_materialize_grads(False)
        return (pred, boxes) if prev is not None else boxes

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        pred, pr, pt = ctx.saved_tensors
        reg_scale, has_prev = ctx.meta
        g_pred, g_boxes = grads if has_prev else (None, grads[0])
        gc = gp = None
        if g_boxes is None:
            gc = g_pred   # nothing came through the boxes
        else:
            gq = None if g_pred is None else _f32c16(g_pred, "grad_output")
            gb = _f32c16(g_boxes, "grad_output")
            gc, gp = torch.empty_like(pred), _grad_like(ctx.needs_input_grad[3], pt)
            check(lib.m355_dfine_refine_boxes_backward(_ptr(gq), _ptr(gb), _ptr(pred), _ptr(pr), _ptr(pt), gb.numel() // 4, pr.numel(),
                                                       reg_scale, _ptr(gc), _ptr(gp), _stream()))
        return (gc if ctx.needs_input_grad[0] else None, gc if has_prev and ctx.needs_input_grad[1] else None, None, gp, None)


def refine_boxes(delta_corners: torch.Tensor, prev_corners, project: torch.Tensor, points: torch.Tensor, reg_scale: float):
    """One layer's box refinement of DFineDecoder.forward in ONE launch: pred_corners = delta_corners + prev_corners (torch's bits)
    and boxes = distance2bbox(points, integral(pred_corners, project), reg_scale); returns (pred_corners, boxes).  At layer 0
    prev_corners is None and pred_corners is delta_corners itself.  delta_corners, prev_corners (..., 4 * (bins + 1)), points
    (..., 4).  The backward (one launch) writes the one gradient g_pred_corners + d boxes / d pred_corners . g_boxes, which serves
    both addends, and dpoints where asked.  project is a constant, as in decode_boxes.  CPU or non-fp32 tensors, autocast, an empty
    input, bins + 1 outside [2, 64] and reg_scale == 0 take refine_boxes_torch."""
    nb1 = project.numel()
    lead = delta_corners.shape[:-1]
    if delta_corners.dim() < 1 or delta_corners.shape[-1] != 4 * nb1 or tuple(points.shape) != tuple(lead) + (4,):
        raise ValueError("delta_corners must be (..., 4 * len(project)) and points (..., 4)")
    if prev_corners is not None and prev_corners.shape != delta_corners.shape:
        raise ValueError("prev_corners must have the shape of delta_corners")
    if torch.is_grad_enabled() and project.requires_grad:
        raise RuntimeError("refine_boxes treats project (the weighting function W(n)) as a constant: it has no gradient; "
                           "detach it, or use integral() + distance2bbox() to train reg_scale / up")
    tensors = (delta_corners, project, points) + (() if prev_corners is None else (prev_corners,))
    if not (_fp32_cuda(*tensors) and not torch.is_autocast_enabled() and delta_corners.numel() and 2 <= nb1 <= LQE_MAX_BINS1
            and not torch.is_tensor(reg_scale) and float(reg_scale) != 0.0):
        return refine_boxes_torch(delta_corners, prev_corners, project, points, reg_scale)
    if _wants_grad(*tensors):
        out = _RefineBoxes.apply(delta_corners, prev_corners, project, points, float(reg_scale))
        return out if prev_corners is not None else (delta_corners, out)
    d = _f32c16(delta_corners, "delta_corners")
    pred, boxes = _refine_boxes_forward(d, None if prev_corners is None else _f32c16(prev_corners, "prev_corners"),
                                        _f32c(project, "project"), _f32c16(points, "points"), float(reg_scale))
    return (delta_corners if prev_corners is None else pred), boxes


def _loop_project(decoder):
    """(project, reg_scale as a float) of a DFineDecoder, cached on the instance as a plain attribute (not a buffer) under the
    _version, device and dtype of `up` and `reg_scale`: weighting_function's own bits, rebuilt after either parameter changes"""
    up, rs = decoder.up, decoder.reg_scale
    key = (up._version, up.device, up.dtype, rs._version, rs.device, rs.dtype)
    cached = getattr(decoder, "_m355_project", None)
    if cached is None or cached[0] != key:
        with torch.no_grad():
            cached = (key, weighting_function(decoder.max_num_bins, up, rs), float(rs))
        decoder._m355_project = cached
    return cached[1], cached[2]


def _relu_mlp_shaped(mlp, in_features=None) -> bool:
    layers = list(getattr(mlp, "layers", ()))
    if not layers or not all(isinstance(l, torch.nn.Linear) and l.bias is not None for l in layers):
        return False
    if hasattr(mlp, "act") and not isinstance(mlp.act, torch.nn.ReLU):
        return False
    return getattr(mlp, "num_layers", len(layers)) == len(layers) and (in_features is None or layers[0].in_features == in_features)


def _relu_mlp(mlp, x: torch.Tensor) -> torch.Tensor:
    """DFineMLP.forward with ReLU: the Linears as torch GEMMs on the module's parameters, relu_dropout(., 0.0) between them"""
    last = len(mlp.layers) - 1
    for j, layer in enumerate(mlp.layers):
        x = torch.nn.functional.linear(x, layer.weight, layer.bias)
        if j < last:
            x = relu_dropout(x, 0.0)
    return x


def _decoder_loop_takes(dec, encoder_hidden_states, reference_points, inputs_embeds, kwargs) -> bool:
    """True when the kernels cover this call of a DFineDecoder; anything else goes to the class's own forward"""
    if dec.bbox_embed is None or dec.class_embed is None:
        return False
    cfg = getattr(dec, "config", None)
    if any(kwargs.get(k) or getattr(cfg, k, False) for k in ("output_hidden_states", "output_attentions")):
        return False
    if kwargs.get("return_dict") is False:
        return False
    x, ref = inputs_embeds, reference_points
    if not _fp32_cuda(x, ref, encoder_hidden_states) or torch.is_autocast_enabled() or x.dim() != 3 or x.numel() == 0:
        return False
    if ref.dim() != 3 or ref.shape[-1] != 4 or ref.shape[:2] != x.shape[:2]:
        return False
    qp = dec.query_pos_head
    if not _relu_mlp_shaped(qp, 4) or len(qp.layers) != 2:
        return False
    if not _relu_mlp_shaped(dec.pre_bbox_head) or not hasattr(dec.pre_bbox_head, "act"):
        return False
    if len(dec.bbox_embed) < len(dec.layers) or not all(_relu_mlp_shaped(m) and hasattr(m, "act") for m in dec.bbox_embed):
        return False
    nb1 = int(dec.max_num_bins) + 1
    if not 2 <= nb1 <= LQE_MAX_BINS1 or any(m.layers[-1].out_features != 4 * nb1 for m in dec.bbox_embed):
        return False
    if dec.up.requires_grad or dec.reg_scale.requires_grad:   # project is a constant of refine_boxes
        return False
    own = [dec.up, dec.reg_scale]
    for m in (qp, dec.pre_bbox_head, dec.bbox_embed, dec.class_embed):
        own.extend(m.parameters())
    return _fp32_cuda(*own)


def decoder_forward(self, encoder_hidden_states, reference_points, inputs_embeds, spatial_shapes, level_start_index=None,
                    spatial_shapes_list=None, encoder_attention_mask=None, memory_mask=None, **kwargs):
    """DFineDecoder.forward (modeling_d_fine.py:1184-1293, transformers 5.15.0) on fp32 CUDA tensors, in upstream's order and with its
    detach points; the nn.Linear products as torch GEMMs on the module's own parameters and between them
        pos = query_pos_head.layers[1](query_pos_hidden(ref, query_pos_head.layers[0])).clamp(-10, 10)
        new_ref = refine_reference(pre_bbox_head(x), ref)                            # layer 0; the inner ReLUs: relu_dropout(., 0.0)
        pred_corners, boxes = refine_boxes(bbox_embed[i](x + x_prev.detach()), pred_corners, project, new_ref.detach(), reg_scale)
    The layers and lqe_layers[i] are called as modules (bind_decoder composes), class_embed[i] runs where upstream runs it, the
    final stacks stay torch; every field of DFineDecoderOutput is filled as upstream.  project = weighting_function(...) and
    float(reg_scale) are cached on the instance (_loop_project), so a call rebuilds neither.
    A call goes to the class's own forward, untouched and with its decorators, when bbox_embed or class_embed is None, when tensors
    or the loop's parameters are not fp32 CUDA, under autocast, with reference points that are not (B, Q, 4), when query_pos_head is
    not a two-layer head of input width 4, an MLP's activation is not ReLU, `up` or `reg_scale` requires grad, recorded outputs are
    asked for (output_hidden_states / output_attentions in kwargs or config) and on an empty input.  A denoising mask does not force
    it: the layers decide for themselves.  Bound per instance by bind_decoder_loop."""
    if not _decoder_loop_takes(self, encoder_hidden_states, reference_points, inputs_embeds, kwargs):
        loop_calls["torch"] += 1
        return type(self).forward(self, encoder_hidden_states=encoder_hidden_states, reference_points=reference_points,
                                  inputs_embeds=inputs_embeds, spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                                  spatial_shapes_list=spatial_shapes_list, encoder_attention_mask=encoder_attention_mask,
                                  memory_mask=memory_mask, **kwargs)
    loop_calls["kernel"] += 1
    from transformers.models.d_fine.modeling_d_fine import DFineDecoderOutput
    F = torch.nn.functional
    project, reg_scale = _loop_project(self)
    q0, q1 = self.query_pos_head.layers
    hidden_states = inputs_embeds
    intermediate, intermediate_reference_points, intermediate_logits = (), (), ()
    intermediate_predicted_corners, initial_reference_points = (), ()
    output_detach = pred_corners_undetach = None
    ref_points_detach = torch.sigmoid(reference_points)

    for i, decoder_layer in enumerate(self.layers):
        ref_points_input = ref_points_detach.unsqueeze(2)
        query_pos_embed = F.linear(query_pos_hidden(ref_points_detach, q0.weight, q0.bias), q1.weight, q1.bias).clamp(min=-10, max=10)
        hidden_states = decoder_layer(hidden_states, position_embeddings=query_pos_embed, reference_points=ref_points_input,
                                      spatial_shapes=spatial_shapes, spatial_shapes_list=spatial_shapes_list,
                                      encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask,
                                      **kwargs)
        if i == 0:
            new_reference_points = refine_reference(_relu_mlp(self.pre_bbox_head, hidden_states), ref_points_detach)
            ref_points_initial = new_reference_points.detach()
        delta = _relu_mlp(self.bbox_embed[i], hidden_states if output_detach is None else hidden_states + output_detach)
        pred_corners, inter_ref_bbox = refine_boxes(delta, pred_corners_undetach, project, ref_points_initial, reg_scale)
        pred_corners_undetach = pred_corners
        ref_points_detach = inter_ref_bbox.detach()
        output_detach = hidden_states.detach()
        intermediate += (hidden_states,)

        if self.training or i == self.eval_idx:
            scores = self.class_embed[i](hidden_states)
            if i == 0:
                intermediate_logits += (scores,)
                intermediate_reference_points += (new_reference_points,)
            scores = self.lqe_layers[i](scores, pred_corners)
            intermediate_logits += (scores,)
            intermediate_reference_points += (inter_ref_bbox,)
            initial_reference_points += (ref_points_initial,)
            intermediate_predicted_corners += (pred_corners,)

    return DFineDecoderOutput(
        last_hidden_state=hidden_states,
        intermediate_hidden_states=torch.stack(intermediate),
        intermediate_logits=torch.stack(intermediate_logits, dim=1),
        intermediate_reference_points=torch.stack(intermediate_reference_points, dim=1),
        intermediate_predicted_corners=torch.stack(intermediate_predicted_corners, dim=1),
        initial_reference_points=torch.stack(initial_reference_points, dim=1),
    )


def bind_decoder_loop(module):
    """Set decoder_forward on every DFineDecoder INSTANCE inside `module` (a DFineDecoder, a whole DFineForObjectDetection, or any
    module that holds some); transformers' classes are never touched, parameters, buffers and the state dict stay as they are.
    Composes with bind_decoder and bind_model.  Returns `module`."""
    from transformers.models.d_fine import modeling_d_fine as M   # lazily: the package does not need transformers otherwise
    _bind_forward(module, {M.DFineDecoder: decoder_forward})
    return module


# ---- NCHW maps <-> token rows, the exact GELU and the AIFI layer of the hybrid encoder (DFineAIFILayer, DFineEncoderLayer) --------
# The trainers freeze only the backbone, so the AIFI layer runs forward and backward on every step.  Its nn.Linear products stay
# torch GEMMs; between them the kernels above (self_attention, add_layer_norm) and csrc/dfine_layout.hip: the map -> token transpose
# with x + pos from the same read, its adjoint, and the erf GELU.  The same transpose with a level table and valid_mask is the memory
# assembly of DFineModel.forward.
LAYOUT_MAX_LEVELS = 8            # the limits of m355_dfine_maps_to_tokens / _tokens_to_maps; anything outside them takes the *_torch form
LAYOUT_MAX_TOKENS = (1 << 31) - 1
layout_calls = {"kernel": 0, "torch": 0}   # maps_to_tokens and tokens_to_maps calls by path (tests and tools read it)
aifi_calls = {"kernel": 0, "torch": 0}     # aifi_forward calls by path


def _level_shapes(maps):
    if not isinstance(maps, (list, tuple)) or not maps or not all(torch.is_tensor(m) and m.dim() == 4 for m in maps):
        raise ValueError("maps must be a non-empty list of (B, D, h, w) tensors")
    B, D = maps[0].shape[:2]
    if any(m.shape[:2] != (B, D) or m.device != maps[0].device or m.dtype != maps[0].dtype for m in maps):
        raise ValueError("the maps must agree in batch size, channels, device and dtype")
    return [(int(m.shape[2]), int(m.shape[3])) for m in maps]


def _layout_takes(B: int, D: int, shapes, *tensors) -> bool:
    S = sum(h * w for h, w in shapes)
    return (_fp32_cuda(*tensors) and not torch.is_autocast_enabled() and B >= 1 and S >= 1 and all(h * w for h, w in shapes)
            and D % 4 == 0 and 4 <= D <= ADDLN_MAX_D and len(shapes) <= LAYOUT_MAX_LEVELS and S <= LAYOUT_MAX_TOKENS
            and len({t.device for t in tensors}) == 1)


def maps_to_tokens_torch(maps, pos=None, mask=None):
    """upstream's expressions: torch.cat([m.flatten(2).transpose(1, 2) for m in maps], 1), tokens + pos, mask * tokens"""
    tokens = torch.cat([m.flatten(2).transpose(1, 2) for m in maps], 1)
    if pos is not None:
        return tokens, tokens + pos
    if mask is not None:
        return tokens, mask.to(tokens.dtype).reshape(1, -1, 1) * tokens
    return tokens, None


def tokens_to_maps_torch(tokens, shapes):
    """upstream's expression per level: transpose(1, 2).reshape(B, D, h, w).contiguous()"""
    B, _, D = tokens.shape
    out, s = [], 0
    for h, w in shapes:
        out.append(tokens[:, s:s + h * w].transpose(1, 2).reshape(B, D, h, w).contiguous())
        s += h * w
    return out


def _shape_table(shapes):
    return (C.c_int32 * (2 * len(shapes)))(*[v for hw in shapes for v in hw])


def _maps_to_tokens_forward(maps, shapes, pos, mask):
    """maps, pos, mask as _f32c16 leaves them (mask: fp32 (S,)) -> tokens, extra or None"""
    B, D = maps[0].shape[:2]
    S = sum(h * w for h, w in shapes)
    tokens = torch.empty((B, S, D), dtype=torch.float32, device=maps[0].device)
    extra = torch.empty_like(tokens) if pos is not None or mask is not None else None
    ptrs = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    check(lib.m355_dfine_maps_to_tokens(ptrs, _shape_table(shapes), len(shapes), B, D, _ptr(pos), _ptr(mask), _ptr(tokens), _ptr(extra),
                                        _stream()))
    return tokens, extra


def _tokens_to_maps_forward(tokens, extra, mask, shapes, B, D):
    """tokens and extra (either may be None) as _f32c16 leaves them -> the maps of tokens (+ extra (* mask))"""
    dev = (tokens if tokens is not None else extra).device
    maps = [torch.empty((B, D, h, w), dtype=torch.float32, device=dev) for h, w in shapes]
    ptrs = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    check(lib.m355_dfine_tokens_to_maps(_ptr(tokens), _ptr(extra), _ptr(mask), _shape_table(shapes), len(shapes), B, D, ptrs, _stream()))
    return maps


class _MapsToTokens(torch.autograd.Function):
    """Saves nothing but the mask: the backward is tokens_to_maps of both gradients."""

    @staticmethod
    def forward(ctx, shapes, pos, mask, *maps):
        tokens, extra = _maps_to_tokens_forward([_f32c16(m, "maps") for m in maps], shapes, pos, mask)
        ctx.meta = (shapes, mask, maps[0].shape[0], maps[0].shape[1])
        ctx.set_materialize_grads(False)   # an unused output's gradient stays None: 0 + mask * g would turn a -0 into +0
        if extra is None:
            return tokens
        return tokens, extra

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_tokens, g_extra=None):
        shapes, mask, B, D = ctx.meta
        gt = _f32c16(g_tokens, "grad_tokens") if g_tokens is not None else None
        ge = _f32c16(g_extra, "grad_extra") if g_extra is not None else None
        if gt is None and ge is None:
            return (None, None, None) + (None,) * len(shapes)
        return (None, None, None) + tuple(_tokens_to_maps_forward(gt, ge, mask if ge is not None else None, shapes, B, D))


class _TokensToMaps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, shapes):
        B, _, D = tokens.shape
        ctx.meta = (shapes, tokens.shape)
        ctx.set_materialize_grads(False)   # backward fills the levels nobody used with zeros itself
        return tuple(_tokens_to_maps_forward(_f32c16(tokens, "tokens"), None, None, shapes, B, D))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_maps):
        shapes, (B, _, D) = ctx.meta
        like = next((g for g in g_maps if g is not None), None)
        if like is None:
            return None, None
        gs = [_f32c16(g, "grad_maps") if g is not None else like.new_zeros((B, D, h, w)) for g, (h, w) in zip(g_maps, shapes)]
        return _maps_to_tokens_forward(gs, shapes, None, None)[0], None


def maps_to_tokens(maps, pos=None, mask=None):
    """maps: a list of L <= 8 (B, D, h_l, w_l) feature maps -> (tokens, extra): tokens (B, S, D) = torch.cat([m.flatten(2)
    .transpose(1, 2) for m in maps], 1) in ONE launch for all levels (a tiled transpose through LDS), and from the same read of the
    maps extra = tokens + pos for pos (S, D) (the AIFI layer's q / k input) or mask * tokens for a mask of S elements (the 0 / 1
    valid_mask of DFineModel.forward, any dtype: a true multiply, 0 * inf is NaN); None without either.  pos and mask are constants
    and exclude each other.  Differentiable in the maps: the backward is tokens_to_maps of grad_tokens + grad_extra (* mask), one
    launch.  Maps that are not contiguous (channels-last) or not 16-byte aligned are copied once.  CPU or non-fp32 tensors,
    autocast, D not a multiple of 4 in [4, 1024], more than 8 levels and an empty level take maps_to_tokens_torch; layout_calls
    counts the path."""
    shapes = _level_shapes(maps)
    B, D = (int(v) for v in maps[0].shape[:2])
    S = sum(h * w for h, w in shapes)
    if pos is not None and mask is not None:
        raise ValueError("pos and mask exclude each other")
    if (pos is not None and pos.requires_grad) or (mask is not None and mask.requires_grad):
        raise ValueError("pos and mask are constants: neither may require grad")
    if pos is not None:
        if pos.numel() != S * D or pos.shape[-1] != D:
            raise ValueError("pos must be (S, D)")
        pos = pos.reshape(S, D)
    if mask is not None and mask.numel() != S:
        raise ValueError("mask must have S elements")
    extras = [t for t in (pos,) if t is not None]
    if not _layout_takes(B, D, shapes, *maps, *extras) or (mask is not None and mask.device != maps[0].device):
        layout_calls["torch"] += 1
        return maps_to_tokens_torch(maps, pos, mask)
    layout_calls["kernel"] += 1
    p = _f32c16(pos, "pos") if pos is not None else None
    m = mask.reshape(S).to(torch.float32).contiguous() if mask is not None else None
    if _wants_grad(*maps):
        out = _MapsToTokens.apply(shapes, p, m, *maps)
        return out if isinstance(out, tuple) else (out, None)
    return _maps_to_tokens_forward([_f32c16(t, "maps") for t in maps], shapes, p, m)


def tokens_to_maps(tokens, shapes):
    """tokens (B, S, D), shapes [(h_l, w_l)] with sum h_l w_l == S -> the list of contiguous (B, D, h_l, w_l) maps,
    map_l[b, c, y, x] = tokens[b, start_l + y w_l + x, c]: transpose(1, 2).reshape(B, D, h, w).contiguous() for every level in ONE
    launch; differentiable, the backward is maps_to_tokens.  The fallbacks of maps_to_tokens apply (tokens_to_maps_torch)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    if not torch.is_tensor(tokens) or tokens.dim() != 3 or sum(h * w for h, w in shapes) != tokens.shape[1]:
        raise ValueError("tokens must be (B, S, D) and the shapes must add up to S")
    B, _, D = (int(v) for v in tokens.shape)
    if not _layout_takes(B, D, shapes, tokens):
        layout_calls["torch"] += 1
        return tokens_to_maps_torch(tokens, shapes)
    layout_calls["kernel"] += 1
    if _wants_grad(tokens):
        return list(_TokensToMaps.apply(tokens, shapes))
    return _tokens_to_maps_forward(_f32c16(tokens, "tokens"), None, None, shapes, B, D)


def gelu_torch(h: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.gelu(h)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        hs = _f32c16(h, "h")
        ctx.save_for_backward(hs)   # the input alone: the backward recomputes Phi(h) and phi(h)
        return _gelu_forward(hs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (hs,) = ctx.saved_tensors
        g = _f32c16(grad_out, "grad_output")
        gh = torch.empty_like(hs)
        check(lib.m355_dfine_gelu_backward(_ptr(g), _ptr(hs), hs.numel(), _ptr(gh), _stream()))
        return gh


def _gelu_forward(hs):
    out = torch.empty_like(hs)
    check(lib.m355_dfine_gelu_forward(_ptr(hs), hs.numel(), _ptr(out), _stream()))
    return out


def gelu(h: torch.Tensor) -> torch.Tensor:
    """The exact GELU h * Phi(h) = h * 0.5 * (1 + erf(h / sqrt(2))), F.gelu with its default arguments, in one elementwise launch;
    the backward (one launch) is g * (Phi(h) + h * phi(h)) from the saved input, the only tensor kept.  CPU or non-fp32 tensors,
    autocast and an empty tensor take gelu_torch."""
    if not _fp32_cuda(h) or h.numel() == 0 or torch.is_autocast_enabled():
        return gelu_torch(h)
    if _wants_grad(h):
        return _Gelu.apply(h)
    return _gelu_forward(_f32c16(h, "h"))


def _is_exact_gelu(act) -> bool:
    """transformers' ACT2CLS["gelu"] (GELUActivation on F.gelu) or nn.GELU() with approximate="none" """
    F = torch.nn.functional
    if isinstance(act, torch.nn.GELU):
        return act.approximate == "none"
    return type(act).__name__ == "GELUActivation" and getattr(act, "act", None) is F.gelu


def _records_outputs(layer, kwargs) -> bool:
    """transformers collects hidden states and attention weights through forward hooks on the layers and their attention"""
    cfg = getattr(layer, "config", None)
    if any(kwargs.get(k) or getattr(cfg, k, False) for k in ("output_hidden_states", "output_attentions")):
        return True
    mods = [layer, *layer.layers, *(enc.self_attn for enc in layer.layers)]
    return any(len(m._forward_hooks) or len(m._forward_pre_hooks) for m in mods)


def _aifi_takes(layer, x, kwargs) -> bool:
    """True when the kernels cover this call of a DFineAIFILayer; anything else goes to the class's own forward"""
    if not _fp32_cuda(x) or x.dim() != 4 or x.numel() == 0 or torch.is_autocast_enabled():
        return False
    D = x.shape[1]
    if D != layer.encoder_hidden_dim or D % 4 or not 4 <= D <= ADDLN_MAX_D or len(layer.layers) < 1:
        return False
    if _records_outputs(layer, kwargs):
        return False
    for enc in layer.layers:
        sa, mlp = enc.self_attn, enc.mlp
        if enc.normalize_before or enc.hidden_size != D:
            return False
        if layer.training and (float(enc.dropout) > 0.0 or float(sa.attention_dropout) > 0.0):
            return False
        if not _is_exact_gelu(mlp.act) or mlp.num_layers != 2 or len(mlp.layers) != 2:
            return False
        if not (_affine_norm(enc.self_attn_layer_norm, D) and _affine_norm(enc.final_layer_norm, D)):
            return False
        if getattr(layer, "_m355_attention_kernel", False) and (
                sa.head_dim != ENCODER_HEAD_DIM or D % ENCODER_HEAD_DIM
                or any(lin.bias is None for lin in (sa.q_proj, sa.k_proj, sa.v_proj, sa.o_proj))):
            return False
    return _fp32_cuda_params(layer)


def aifi_forward(self, hidden_states, **kwargs):
    """DFineAIFILayer.forward with its DFineEncoderLayer(s) (modeling_d_fine.py:542-610, 699-753, transformers 5.15.0) on fp32 CUDA
    tensors, the nn.Linear products as torch GEMMs on the module's own parameters and everything between them on the kernels:
        x, xp = maps_to_tokens([map], pos=pos_embed)              # tokens and tokens + pos from one read of the map
        y = o_proj(self_attention([q | k](xp), v(x)))             # k without its bias; attention=False: self.self_attn(...)
        x = add_layer_norm(x, y, self_attn_layer_norm)
        x = add_layer_norm(x, mlp.layers[1](gelu(mlp.layers[0](x))), final_layer_norm)
        x = x.clamp(-max, max) when training                      # unconditional: no isfinite().all(), no synchronisation
        return tokens_to_maps(x, [(h, w)])[0]
    The clamp is the identity on finite values and on NaN and its backward passes every element it did not move, so it equals
    upstream's conditional one in value and gradient.  A call goes to the class's own forward, untouched, with normalize_before,
    when the module trains with config.dropout above 0, with an activation other than the exact GELU or an MLP that is not two
    layers, on non-fp32, CPU or empty tensors, under autocast, with D not a multiple of 4 in [4, 1024], when outputs are recorded
    (output_hidden_states / output_attentions, or a forward hook on the layer, its encoder layers or their self_attn) and, with
    attention=True, with a head dim other than 32 or a projection without bias.  Bound per instance by bind_aifi."""
    if not _aifi_takes(self, hidden_states, kwargs):
        aifi_calls["torch"] += 1
        return type(self).forward(self, hidden_states, **kwargs)
    aifi_calls["kernel"] += 1
    F = torch.nn.functional
    H, W = hidden_states.shape[2:]
    pos = None
    if self.training or self.eval_size is None:
        pos = self.position_embedding(width=W, height=H, device=hidden_states.device, dtype=hidden_states.dtype)   # (1, H W, D), cached
    attention = getattr(self, "_m355_attention_kernel", False)
    x, xp = maps_to_tokens([hidden_states], pos=pos[0] if attention and pos is not None else None)
    for i, enc in enumerate(self.layers):
        sa = enc.self_attn
        if attention:
            qk_in = x if pos is None else (xp if i == 0 else x + pos)
            # k_proj.bias shifts every logit of a query by the same q . b, which the softmax cancels (decoder_layer_forward)
            qk = F.linear(qk_in, torch.cat([sa.q_proj.weight, sa.k_proj.weight]), torch.cat([sa.q_proj.bias, sa.k_proj.bias * 0.0]))
            qkv = torch.cat([qk, F.linear(x, sa.v_proj.weight, sa.v_proj.bias)], dim=-1)
            y = F.linear(self_attention(qkv, x.shape[-1] // ENCODER_HEAD_DIM), sa.o_proj.weight, sa.o_proj.bias)
        else:
            y = sa(hidden_states=x, attention_mask=None, position_embeddings=pos, **kwargs)[0]
        n = enc.self_attn_layer_norm
        x = add_layer_norm(x, y, n.weight, n.bias, n.eps)
        l0, l1 = enc.mlp.layers
        y = F.linear(gelu(F.linear(x, l0.weight, l0.bias)), l1.weight, l1.bias)
        n = enc.final_layer_norm
        x = add_layer_norm(x, y, n.weight, n.bias, n.eps)
        if self.training:
            c = torch.finfo(x.dtype).max   # upstream's finfo.max - 1000 is finfo.max in fp32
            x = x.clamp(-c, c)
    return tokens_to_maps(x, [(int(H), int(W))])[0]


def bind_aifi(module, attention: bool = False):
    """Set aifi_forward on every DFineAIFILayer INSTANCE inside `module` (a DFineHybridEncoder, a whole DFineForObjectDetection, a
    single layer, or any module that holds some); transformers' classes are never touched, parameters, buffers and the state dict
    stay as they are.  Returns `module`.  attention=False keeps each encoder layer's self.self_attn(...) as the class runs it;
    attention=True runs the attention core on dfine.self_attention with the packed [q | k](x + pos), v(x) projection.  The default
    is the arm that profiles/dfine_aifi_bench.json shows faster for the layer's training step (forward + backward) at
    (50, 256, 20, 20): 3.60 ms against 3.72 ms (the unbound layer: 3.92 ms); at (1, 256, 20, 20) attention=False is SLOWER than the
    unbound layer (1.32 against 1.15 ms, host-bound) and attention=True faster (0.98 ms)."""
    from transformers.models.d_fine import modeling_d_fine as M   # lazily: the package does not need transformers otherwise
    for m in _bind_forward(module, {M.DFineAIFILayer: aifi_forward}):
        m._m355_attention_kernel = bool(attention)   # a plain attribute: not a parameter, not a buffer, not in the state dict
    return module


# ---- encoder query selection (DFineModel.forward, modeling_d_fine.py:1804-1828) ----------------------------------------------------
# Between the hybrid encoder's heads and the decoder every call of a D-FINE model picks its num_queries tokens: row max of the class
# logits, top-k, three gathers and a sigmoid.  csrc/dfine_select.hip does it in two launches forward (row max on all CUs; one block
# per image for the top-k of csrc/topk_select.h and the gathers) and one backward, with a stated order among equal scores.
SELECT_MAX_QUERIES = 2048        # the limits of m355_dfine_select_forward; anything outside them takes select_queries_torch
SELECT_MAX_TOKENS = 1 << 24      # S stays below it
model_calls = {"kernel": 0, "torch": 0}   # query selections by path (tests and tools read it)


class QuerySelection(NamedTuple):
    indices: torch.Tensor                  # (B, K) int64, in output order
    reference_points_unact: torch.Tensor   # (B, K, 4) rows of coord_logits
    boxes: torch.Tensor                    # (B, K, 4) their sigmoid
    logits: torch.Tensor                   # (B, K, C) rows of class_logits
    target: torch.Tensor | None            # (B, K, D) rows of memory, or None without one


def _check_select_shapes(class_logits, coord_logits, memory):
    if class_logits.dim() != 3 or tuple(coord_logits.shape) != tuple(class_logits.shape[:2]) + (4,):
        raise ValueError("class_logits (B, S, C) and coord_logits (B, S, 4) are expected")
    if memory is not None and (memory.dim() != 3 or tuple(memory.shape[:2]) != tuple(class_logits.shape[:2])):
        raise ValueError("memory (B, S, D) must have the tokens of class_logits")


def _select_kernel_takes(class_logits, coord_logits, memory, K: int) -> bool:
    B, S, Cn = class_logits.shape
    tensors = (class_logits, coord_logits) if memory is None else (class_logits, coord_logits, memory)
    return (_fp32_cuda(*tensors) and not torch.is_autocast_enabled() and B >= 1 and Cn >= 1 and (memory is None or memory.shape[-1] >= 1)
            and 1 <= K <= min(S, SELECT_MAX_QUERIES) and S < SELECT_MAX_TOKENS and B * S < 1 << 31)


def select_queries_torch(class_logits: torch.Tensor, coord_logits: torch.Tensor, memory=None, num_queries: int = 300) -> QuerySelection:
    """select_queries in torch ops, on whatever device and dtype the tensors have, with the kernel's order rule: a stable descending
    sort of the row maxima, so NaN scores come first and an exact tie goes to the lowest token (torch.topk promises no order among
    equal scores; where the scores are distinct the two agree).  What select_queries falls back to and the baseline of the tests.
    A num_queries above S raises as torch.topk does."""
    _check_select_shapes(class_logits, coord_logits, memory)
    K = int(num_queries)
    scores = class_logits.detach().max(-1).values
    if not 0 <= K <= scores.shape[1]:
        torch.topk(scores, K, dim=1)   # raises torch.topk's own error
    model_calls["torch"] += 1
    ind = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :K]
    rows = lambda t: t.gather(1, ind.unsqueeze(-1).expand(-1, -1, t.shape[-1]))
    ref = rows(coord_logits)
    return QuerySelection(ind, ref, torch.sigmoid(ref), rows(class_logits), None if memory is None else rows(memory))


def _select_forward(cl, co, mem, K: int, keep_inverse: bool):
    """contiguous fp32 CUDA tensors -> indices, ref, boxes, logits, target or None, inverse map or None"""
    B, S, Cn = cl.shape
    D = mem.shape[-1] if mem is not None else 0
    dev = cl.device
    work = torch.empty((B, S), dtype=torch.float32, device=dev)   # the token scores
    ind = torch.empty((B, K), dtype=torch.int64, device=dev)
    ref = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    boxes = torch.empty_like(ref)
    logits = torch.empty((B, K, Cn), dtype=torch.float32, device=dev)
    target = torch.empty((B, K, D), dtype=torch.float32, device=dev) if mem is not None else None
    inv = torch.empty((B, S), dtype=torch.int32, device=dev) if keep_inverse else None
    check(lib.m355_dfine_select_forward(_ptr(cl), _ptr(co), _ptr(mem), B, S, Cn, D, K, _ptr(work), work.numel() * 4, _ptr(ind), _ptr(ref),
                                        _ptr(boxes), _ptr(logits), _ptr(target), _ptr(inv), _stream()))
    return ind, ref, boxes, logits, target, inv


class _SelectQueries(torch.autograd.Function):
    """indices, ref, boxes, logits, target = select(class_logits, coord_logits, memory); saves the boxes and the inverse map."""

    @staticmethod
    def forward(ctx, class_logits, coord_logits, memory, K):
        cl, co = class_logits.contiguous(), coord_logits.contiguous()
        mem = memory.contiguous() if memory is not None else None
        ind, ref, boxes, logits, target, inv = _select_forward(cl, co, mem, K, True)
        ctx.save_for_backward(boxes, inv)
        ctx.meta = (tuple(cl.shape), mem.shape[-1] if mem is not None else 0, K)
        ctx.mark_non_differentiable(ind)
        ctx.set_materialize_grads(False)   # an output nobody differentiates arrives as None, not as a tensor of zeros
        return ind, ref, boxes, logits, target

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _g_ind, g_ref, g_boxes, g_logits, g_target):
        boxes, inv = ctx.saved_tensors
        (B, S, Cn), D, K = ctx.meta
        dev = inv.device
        need_cl, need_co, need_mem = ctx.needs_input_grad[:3]
        g = [None if t is None else _f32c(t, "grad_output") for t in (g_ref, g_boxes, g_logits, g_target)]
        d_cl = torch.empty((B, S, Cn), dtype=torch.float32, device=dev) if need_cl else None
        d_co = torch.empty((B, S, 4), dtype=torch.float32, device=dev) if need_co else None
        d_mem = torch.empty((B, S, D), dtype=torch.float32, device=dev) if need_mem else None
        check(lib.m355_dfine_select_backward(_ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(g[3]), _ptr(boxes), _ptr(inv), B, S, Cn, max(D, 1), K,
                                             _ptr(d_cl), _ptr(d_co), _ptr(d_mem), _stream()))
        return d_cl, d_co, d_mem, None


def select_queries(class_logits: torch.Tensor, coord_logits: torch.Tensor, memory=None, num_queries: int = 300) -> QuerySelection:
    """The query selection of DFineModel.forward: class_logits (B, S, C) = enc_score_head's output, coord_logits (B, S, 4) =
    enc_bbox_head's output + anchors, memory (B, S, D) = enc_output's output or None.  Per image the num_queries tokens with the
    greatest score (score = max over C) -> QuerySelection(indices (B, K) int64, reference_points_unact (B, K, 4), boxes =
    sigmoid of those, logits (B, K, C), target (B, K, D) or None); the gathered rows are copies, bit for bit.

    Order: a NaN score first (torch.topk's order; a row that holds a NaN scores NaN, as torch.max gives), then descending score,
    -0 == +0, an exact tie to the lowest token.  Bitwise reproducible, and an image's rows do not depend on its batch.  Two launches
    forward and one backward (no memset, no atomics: the gradients of the three inputs are written in full through an inverse
    map), no device-to-host transfer and no synchronisation; with nothing to differentiate no inverse map is kept.  indices carry no
    gradient.  CPU or non-fp32 tensors, autocast and shapes beyond the kernel's limits (num_queries > 2048, S >= 2^24,
    B * S >= 2^31) take select_queries_torch, the same outputs from torch ops; model_calls counts the calls by path."""
    _check_select_shapes(class_logits, coord_logits, memory)
    K = int(num_queries)
    if not _select_kernel_takes(class_logits, coord_logits, memory, K):
        return select_queries_torch(class_logits, coord_logits, memory, K)
    model_calls["kernel"] += 1
    if _wants_grad(class_logits, coord_logits) or (memory is not None and _wants_grad(memory)):
        return QuerySelection(*_SelectQueries.apply(class_logits, coord_logits, memory, K))
    cl, co = class_logits.detach().contiguous(), coord_logits.detach().contiguous()
    mem = memory.detach().contiguous() if memory is not None else None
    return QuerySelection(*_select_forward(cl, co, mem, K, False)[:5])


def _mask_is_all_ones(model, valid_mask) -> bool:
    """Whether this valid_mask tensor is all ones, found once (one synchronisation, as _loop_project's float(reg_scale)) and cached
    on the instance by the tensor's identity and version; the cache holds the tensor, so its id cannot be reused while it counts"""
    cached = getattr(model, "_m355_valid_mask_ones", None)
    if cached is not None and cached[0] is valid_mask and cached[1] == valid_mask._version:
        return cached[2]
    ones = bool(valid_mask.all())
    model._m355_valid_mask_ones = (valid_mask, valid_mask._version, ones)
    return ones


def model_forward(self, pixel_values=None, pixel_mask=None, encoder_outputs=None, inputs_embeds=None, labels=None, **kwargs):
    """DFineModel.forward (modeling_d_fine.py:1666-1861, transformers 5.15.0) with its query selection (:1804-1828: row max, top-k,
    three gathers, sigmoid) on select_queries.  The module's own sub-modules run everything else, in upstream's order: backbone,
    projections, encoder, enc_output, the score and box heads, anchors, the denoising group and the decoder.  The decoder's
    inputs_embeds and init_reference_points are detached as upstream; with config.learn_initial_query the queries are
    weight_embedding and no memory rows are gathered.  This body always runs; only the selection switches between the kernels and
    select_queries_torch (CPU or non-fp32 tensors, autocast, shapes beyond the limits), and model_calls counts it.  Every field of
    DFineModelOutput is filled as upstream; return_dict=False gives its tuple.  Among equal scores upstream's torch.topk promises
    no order; this one has select_queries' rule.  With bind_model(assembly=True) the memory assembly (:1750-1797: three
    flatten(2).transpose(1, 2) views materialised by torch.cat, then valid_mask * source_flatten) is one maps_to_tokens call:
    source_flatten is its tokens and memory its masked second output, or the tokens themselves for a valid_mask that is all ones
    (found once per mask tensor, _mask_is_all_ones).  Bound per instance by bind_model."""
    from transformers.modeling_outputs import BaseModelOutput
    from transformers.models.d_fine import modeling_d_fine as M   # lazily: the package does not need transformers otherwise
    return_dict = kwargs.pop("return_dict", None)
    if return_dict is None:
        return_dict = getattr(self.config, "return_dict", True)
    if pixel_values is None and inputs_embeds is None:
        raise ValueError("You have to specify either pixel_values or inputs_embeds")
    if inputs_embeds is None:
        batch_size, _, height, width = pixel_values.shape
        device = pixel_values.device
        if pixel_mask is None:
            pixel_mask = torch.ones((batch_size, height, width), device=device)
        features = self.backbone(pixel_values, pixel_mask)
        proj_feats = [self.encoder_input_proj[level](source) for level, (source, mask) in enumerate(features)]
    else:
        device = inputs_embeds.device
        proj_feats = inputs_embeds
    if encoder_outputs is None:
        encoder_outputs = self.encoder(proj_feats, **kwargs)
    elif not isinstance(encoder_outputs, BaseModelOutput):
        encoder_outputs = BaseModelOutput(last_hidden_state=encoder_outputs[0],
                                          hidden_states=encoder_outputs[1] if len(encoder_outputs) > 1 else None,
                                          attentions=encoder_outputs[2] if len(encoder_outputs) > 2 else None)

    sources = [self.decoder_input_proj[level](source) for level, source in enumerate(encoder_outputs.last_hidden_state)]
    if self.config.num_feature_levels > len(sources):   # lowest resolutions: 3x3 stride 2 convolutions on the final stage
        for i in range(len(sources), self.config.num_feature_levels):
            sources.append(self.decoder_input_proj[i](encoder_outputs.last_hidden_state[-1]))

    assembly = getattr(self, "_m355_assembly", False)
    source_flatten, spatial_shapes_list = [], []
    spatial_shapes = torch.empty((len(sources), 2), device=device, dtype=torch.long)
    for level, source in enumerate(sources):
        height, width = source.shape[-2:]
        spatial_shapes[level, 0] = height
        spatial_shapes[level, 1] = width
        spatial_shapes_list.append((height, width))
        if not assembly:
            source_flatten.append(source.flatten(2).transpose(1, 2))
    if not assembly:
        source_flatten = torch.cat(source_flatten, 1)
    level_start_index = torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1]))

    if self.training and self.config.num_denoising > 0 and labels is not None:
        denoising_class, denoising_bbox_unact, attention_mask, denoising_meta_values = M.get_contrastive_denoising_training_group(
            targets=labels, num_classes=self.config.num_labels, num_queries=self.config.num_queries,
            class_embed=self.denoising_class_embed, num_denoising_queries=self.config.num_denoising,
            label_noise_ratio=self.config.label_noise_ratio, box_noise_scale=self.config.box_noise_scale)
    else:
        denoising_class, denoising_bbox_unact, attention_mask, denoising_meta_values = None, None, None, None

    like = sources[0] if assembly else source_flatten
    batch_size, device, dtype = len(like), like.device, like.dtype
    if self.training or self.config.anchor_image_size is None:
        anchors, valid_mask = self.generate_anchors(tuple(spatial_shapes_list), device=device, dtype=dtype)   # hashable: lru_cache
        mask_key = valid_mask
    else:
        anchors, valid_mask, mask_key = self.anchors.to(device, dtype), self.valid_mask.to(device, dtype), self.valid_mask
    if assembly:   # one launch: the levels' tokens and valid_mask * tokens from one read of the maps
        if _mask_is_all_ones(self, mask_key):
            source_flatten, _ = maps_to_tokens(sources)
            memory = source_flatten   # 1.0 * x is x, bit for bit
        else:
            source_flatten, memory = maps_to_tokens(sources, mask=valid_mask)
    else:
        memory = valid_mask.to(source_flatten.dtype) * source_flatten
    output_memory = self.enc_output(memory)
    enc_outputs_class = self.enc_score_head(output_memory)
    enc_outputs_coord_logits = self.enc_bbox_head(output_memory) + anchors

    # ---- the selection: upstream's topk / gather / sigmoid chain
    learn = bool(self.config.learn_initial_query)
    picked = select_queries(enc_outputs_class, enc_outputs_coord_logits, None if learn else output_memory.detach(),
                            self.config.num_queries)
    reference_points_unact, enc_topk_bboxes, enc_topk_logits = picked.reference_points_unact, picked.boxes, picked.logits
    if denoising_bbox_unact is not None:
        reference_points_unact = torch.concat([denoising_bbox_unact, reference_points_unact], 1)
    target = self.weight_embedding.tile([batch_size, 1, 1]) if learn else picked.target.detach()
    if denoising_class is not None:
        target = torch.concat([denoising_class, target], 1)
    init_reference_points = reference_points_unact.detach()

    decoder_outputs = self.decoder(inputs_embeds=target, encoder_hidden_states=source_flatten, encoder_attention_mask=attention_mask,
                                   reference_points=init_reference_points, spatial_shapes=spatial_shapes,
                                   spatial_shapes_list=spatial_shapes_list, level_start_index=level_start_index, **kwargs)
    out = M.DFineModelOutput(
        last_hidden_state=decoder_outputs.last_hidden_state,
        intermediate_hidden_states=decoder_outputs.intermediate_hidden_states,
        intermediate_logits=decoder_outputs.intermediate_logits,
        intermediate_reference_points=decoder_outputs.intermediate_reference_points,
        intermediate_predicted_corners=decoder_outputs.intermediate_predicted_corners,
        initial_reference_points=decoder_outputs.initial_reference_points,
        decoder_hidden_states=decoder_outputs.hidden_states,
        decoder_attentions=decoder_outputs.attentions,
        cross_attentions=decoder_outputs.cross_attentions,
        encoder_last_hidden_state=encoder_outputs.last_hidden_state,
        encoder_hidden_states=encoder_outputs.hidden_states,
        encoder_attentions=encoder_outputs.attentions,
        init_reference_points=init_reference_points,
        enc_topk_logits=enc_topk_logits,
        enc_topk_bboxes=enc_topk_bboxes,
        enc_outputs_class=enc_outputs_class,
        enc_outputs_coord_logits=enc_outputs_coord_logits,
        denoising_meta_values=denoising_meta_values,
    )
    return out if return_dict else out.to_tuple()


def bind_model(module, assembly: bool = True):
    """Set model_forward on every DFineModel INSTANCE inside `module` (a DFineForObjectDetection, a DFineModel, or any module that
    holds some); transformers' classes are never touched, parameters, buffers and the state dict stay as they are, so existing
    checkpoints load unchanged.  Returns `module`.  Composes with bind_decoder (different classes): bind_decoder(bind_model(m)).
    What it buys is the selection's order rule (a bound model's queries do not depend on torch.topk's tie-break) and fewer launches;
    measured (profiles/dfine_select_bench.json, ms per call, median of 7 blocks): the selection alone at (50, 8400, C = 80, D = 256,
    K = 300) forward 0.092 against 0.299 for upstream's torch ops (2 against 30 device activities), forward + backward 0.146 against
    0.366; at (16, ...) and (1, ...) with C = 80 forward + backward is host-bound and the bound median is SLOWER (0.223 against
    0.197, 0.205 against 0.181, spreads overlapping); model.model(pixel_values) at 2 x 256 x 256 does not move: eval 18.9 against
    18.8, training 61.8 against 64.8, inside the spread.
    assembly=True also runs the memory assembly (cat of the flattened levels, valid_mask * source_flatten) as one maps_to_tokens
    launch; assembly=False keeps the torch lines.  The default is the arm profiles/dfine_aifi_bench.json shows faster at
    (50, 8400, 256) with the generated mask: forward + backward 0.51 against 2.26 ms; at 2 x 256 x 256 the model's step does not move
    (training 53.5 against 52.7, the bound median SLOWER inside the spread)."""
    from transformers.models.d_fine import modeling_d_fine as M   # lazily: the package does not need transformers otherwise
    for m in _bind_forward(module, {M.DFineModel: model_forward}):
        m._m355_assembly = bool(assembly)   # a plain attribute: not a parameter, not a buffer, not in the state dict
    return module


def bind_all(module, attention: bool = False):
    """bind_model, bind_decoder, bind_decoder_loop, bind_aifi, bind_encoder and bind_gru on whatever `module` holds (each binds the
    instances of its own classes and leaves everything else alone); `attention` goes to bind_decoder and bind_aifi.  Returns
    `module`: one line for a trainer in place of six."""
    bind_model(module)
    bind_decoder(module, attention=attention)
    bind_decoder_loop(module)
    bind_aifi(module, attention=attention)
    bind_encoder(module)
    bind_gru(module)
    return module


# ---- The temporal head of the trainers: between temporal_encoder / context_aggregator and the loss or the post-processing -------
# Every trainer guards its class logits and its box decode with clamp / nan_to_num; the improved trainer also fuses the frames with a
# softmax over the frame axis, adds anomaly scores to the class columns and adds a frame-to-frame consistency loss; every trainer
# takes a per-frame cross-entropy against "no object" on frames without ground truth.  csrc/dfine_temporal.hip runs each as one
# launch forward and one backward (the consistency loss: two forward), the guarded decode is decode_boxes(guard=True).
TEMPORAL_MAX_T = 1024            # the limits of m355_dfine_temporal_fuse_*; anything outside them takes temporal_fuse_torch
TEMPORAL_MAX_D = 1024
TEMPORAL_MAX_Q = 1 << 20
NOOBJECT_MAX_Q = 2048            # the limits of m355_dfine_noobject_loss_*
NOOBJECT_MAX_C = 1024
CONSISTENCY_MAX_N = 1 << 27      # Q * C of m355_dfine_consistency_loss_*; T * Q * C stays below 2^31
temporal_calls = {"kernel": 0, "torch": 0}   # calls of the temporal-head ops by path (tests and tools read it)


def _temporal_takes(*tensors) -> bool:
    return _fp32_cuda(*tensors) and not torch.is_autocast_enabled() and all(t.numel() > 0 for t in tensors)


def _check_fuse_shapes(fused, scores, context):
    if fused.dim() != 3 or tuple(scores.shape) not in (tuple(fused.shape[:2]), tuple(fused.shape[:2]) + (1,)):
        raise ValueError("fused (T, Q, D) and scores (T, Q, 1) or (T, Q) are expected")
    if context is not None and context.shape != fused.shape:
        raise ValueError("context must have the shape of fused")


def temporal_fuse_torch(fused: torch.Tensor, scores: torch.Tensor, context=None) -> torch.Tensor:
    """temporal_fuse in torch ops on whatever device and dtype the tensors have: what it falls back to."""
    _check_fuse_shapes(fused, scores, context)
    temporal_calls["torch"] += 1
    out = fused * torch.softmax(scores.reshape(tuple(fused.shape[:2]) + (1,)), dim=0)
    return out if context is None else out + context


def _fuse_forward(f, s, c, keep_stats: bool):
    T, Q, D = f.shape
    out = torch.empty_like(f)
    stats = torch.empty((2, Q), dtype=torch.float32, device=f.device) if keep_stats else None
    check(lib.m355_dfine_temporal_fuse_forward(_ptr(f), _ptr(s), _ptr(c), T, Q, D, _ptr(out), _ptr(stats), _stream()))
    return out, stats


class _TemporalFuse(torch.autograd.Function):
    """out = fused * softmax_t(scores) (+ context); saves the scores, the (max, log-sum) of every column and, for the gradient of the
    scores, fused: no weights, no product."""

    @staticmethod
    def forward(ctx, fused, scores, context):
        f, s = fused.contiguous(), scores.contiguous()
        c = context.contiguous() if context is not None else None
        out, stats = _fuse_forward(f, s, c, True)
        ctx.save_for_backward(s, stats, f if ctx.needs_input_grad[1] else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        s, stats, f = ctx.saved_tensors
        need_f, need_s, need_c = ctx.needs_input_grad
        g = _f32c(grad_out, "grad_output")
        T, Q, D = g.shape
        d_f = torch.empty_like(g) if need_f else None
        d_s = torch.empty_like(s) if need_s else None
        if need_f or need_s:
            check(lib.m355_dfine_temporal_fuse_backward(_ptr(g), _ptr(f), _ptr(s), _ptr(stats), T, Q, D, _ptr(d_f), _ptr(d_s), _stream()))
        return d_f, d_s, (g if need_c else None)


def temporal_fuse(fused: torch.Tensor, scores: torch.Tensor, context=None) -> torch.Tensor:
    """The improved trainer's frame fusion (temp_dfine_over_improved.py:220, 227): fused (T, Q, D), scores (T, Q, 1) or (T, Q) = the
    temporal_attention head's output, context (T, Q, D) or None -> fused * softmax(scores, dim=0) (+ context), ONE launch.
    Differentiable in all three; the backward is one launch in which one block owns a query column (the sum over T in a fixed order,
    no workspace), the gradient of context is the incoming gradient itself.  Kept for it: the scores, the per-column max and
    log-sum, and fused only when the scores need a gradient; nothing under no_grad.  A query column does not depend on the other
    columns of the call; bitwise reproducible.  D that is no multiple of 4 (or a view that is not 16-byte aligned) is handled in
    the kernel by 4-byte accesses.  CPU or non-fp32 tensors, autocast, T > 1024, D > 1024 or Q > 2^20 take temporal_fuse_torch;
    temporal_calls counts the calls by path."""
    _check_fuse_shapes(fused, scores, context)
    tensors = (fused, scores) if context is None else (fused, scores, context)
    T, Q, D = fused.shape
    if not (_temporal_takes(*tensors) and T <= TEMPORAL_MAX_T and D <= TEMPORAL_MAX_D and Q <= TEMPORAL_MAX_Q):
        return temporal_fuse_torch(fused, scores, context)
    temporal_calls["kernel"] += 1
    if _wants_grad(*tensors):
        return _TemporalFuse.apply(fused, scores, context)
    c = context.detach().contiguous() if context is not None else None
    return _fuse_forward(fused.detach().contiguous(), scores.detach().contiguous(), c, False)[0]


def _check_guard_shapes(cls_logits, anomaly):
    if cls_logits.dim() < 1 or (anomaly is not None and (cls_logits.shape[-1] < 2 or tuple(anomaly.shape) != tuple(
            cls_logits.shape[:-1]) + (cls_logits.shape[-1] - 1,))):
        raise ValueError("cls_logits (..., C1) and anomaly (..., C1 - 1) are expected")


def guard_logits_torch(cls_logits: torch.Tensor, anomaly=None, bound: float = 20.0) -> torch.Tensor:
    """guard_logits in torch ops (the trainers' lines) on whatever device and dtype the tensors have: what it falls back to."""
    _check_guard_shapes(cls_logits, anomaly)
    temporal_calls["torch"] += 1
    v = cls_logits if anomaly is None else torch.cat([cls_logits[..., :-1] + anomaly, cls_logits[..., -1:]], dim=-1)
    return torch.nan_to_num(v.clamp(-bound, bound), nan=0.0, posinf=bound, neginf=-bound)


class _GuardLogits(torch.autograd.Function):
    """guard_logits; saves its inputs (no copy of a contiguous input) and forms the mask again in the backward."""

    @staticmethod
    def forward(ctx, cls_logits, anomaly, bound):
        c = cls_logits.contiguous()
        a = anomaly.contiguous() if anomaly is not None else None
        ctx.save_for_backward(c, a)
        ctx.bound = bound
        return _guard_forward(c, a, bound)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        c, a = ctx.saved_tensors
        g = _f32c(grad_out, "grad_output")
        d_c = torch.empty_like(c) if ctx.needs_input_grad[0] else None
        d_a = torch.empty_like(a) if a is not None and ctx.needs_input_grad[1] else None
        check(lib.m355_dfine_guard_logits_backward(_ptr(g), _ptr(c), _ptr(a), c.numel() // c.shape[-1], c.shape[-1], ctx.bound, _ptr(d_c),
                                                   _ptr(d_a), _stream()))
        return d_c, d_a, None


def _guard_forward(c, a, bound: float) -> torch.Tensor:
    out = torch.empty_like(c)
    check(lib.m355_dfine_guard_logits_forward(_ptr(c), _ptr(a), c.numel() // c.shape[-1], c.shape[-1], bound, _ptr(out), _stream()))
    return out


def guard_logits(cls_logits: torch.Tensor, anomaly=None, bound: float = 20.0) -> torch.Tensor:
    """The trainers' guarded class logits (temp_dfine_over.py:189-195; with anomaly scores temp_dfine_over_improved.py:237-247):
    cls_logits (..., C1), anomaly (..., C1 - 1) or None -> nan_to_num((cls_logits, with anomaly added to all but the last column)
    .clamp(-bound, bound), nan=0, posinf=bound, neginf=-bound) in ONE launch, without the slice and the cat.  One rounding per
    element: torch's fp32 bits, forward and backward.  The gradient (one launch for both inputs) passes where -bound <= v <= bound
    and is 0 for NaN, +-inf and clamped values, as torch's clamp and nan_to_num give.  CPU or non-fp32 tensors and autocast take
    guard_logits_torch; temporal_calls counts the calls by path."""
    _check_guard_shapes(cls_logits, anomaly)
    bound = float(bound)
    tensors = (cls_logits,) if anomaly is None else (cls_logits, anomaly)
    if not (_temporal_takes(*tensors) and bound >= 0.0 and cls_logits.numel() <= 1 << 40):
        return guard_logits_torch(cls_logits, anomaly, bound)
    temporal_calls["kernel"] += 1
    if _wants_grad(*tensors):
        return _GuardLogits.apply(cls_logits, anomaly, bound)
    return _guard_forward(cls_logits.detach().contiguous(), anomaly.detach().contiguous() if anomaly is not None else None, bound)


def decode_boxes_torch(pred_corners: torch.Tensor, project: torch.Tensor, points: torch.Tensor, reg_scale: float,
                       clamp01: bool = False, guard: bool = False) -> torch.Tensor:
    """decode_boxes in torch ops (DFineIntegral.forward, distance2bbox and, with guard, the trainers' nan_to_num lines) on whatever
    device and dtype the tensors have: what decode_boxes(guard=True) falls back to."""
    temporal_calls["torch"] += 1
    nb1 = project.numel()
    c = torch.nan_to_num(pred_corners, nan=0.0, posinf=1.0, neginf=0.0) if guard else pred_corners
    p = torch.softmax(c.reshape(-1, nb1), dim=1)
    d = torch.nn.functional.linear(p, project.to(p.device).reshape(1, -1)).reshape(tuple(pred_corners.shape[:-1]) + (4,))
    if guard:
        d = torch.nan_to_num(d, nan=0.0, posinf=1.0, neginf=0.0)
    boxes = distance2bbox(points, d, reg_scale)
    if clamp01:
        boxes = boxes.clamp(0, 1)
    return torch.nan_to_num(boxes, nan=0.5, posinf=1.0, neginf=0.0) if guard else boxes


def _noobject_class(cls_logits, class_index) -> int:
    if cls_logits.dim() != 3:
        raise ValueError("cls_logits (T, Q, C1) is expected")
    C1 = cls_logits.shape[-1]
    c = int(class_index)
    if not -C1 <= c < C1:
        raise IndexError(f"class_index {c} is out of range for {C1} classes")
    return c % C1


def noobject_loss_torch(cls_logits: torch.Tensor, class_index: int = -1) -> torch.Tensor:
    """noobject_loss in torch ops: F.cross_entropy of every frame against the one class; what it falls back to."""
    c = _noobject_class(cls_logits, class_index)
    temporal_calls["torch"] += 1
    T, Q, _ = cls_logits.shape
    target = torch.full((Q,), c, dtype=torch.long, device=cls_logits.device)
    return torch.stack([torch.nn.functional.cross_entropy(cls_logits[t], target) for t in range(T)]) if T else cls_logits.new_zeros((0,))


class _NoObjectLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls_logits, c):
        x = cls_logits.contiguous()
        ctx.save_for_backward(x)   # the input alone: the backward forms the softmax again
        ctx.c = c
        return _noobject_forward(x, c)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        T, Q, C1 = x.shape
        g = _f32c(grad_out, "grad_output")
        dx = torch.empty_like(x)
        check(lib.m355_dfine_noobject_loss_backward(_ptr(g), _ptr(x), T, Q, C1, ctx.c, _ptr(dx), _stream()))
        return dx, None


def _noobject_forward(x, c: int) -> torch.Tensor:
    T, Q, C1 = x.shape
    out = torch.empty((T,), dtype=torch.float32, device=x.device)
    check(lib.m355_dfine_noobject_loss_forward(_ptr(x), T, Q, C1, c, _ptr(out), _stream()))
    return out


def noobject_loss(cls_logits: torch.Tensor, class_index: int = -1) -> torch.Tensor:
    """The trainers' loss of a frame without ground truth (temp_dfine_over.py:278-281), for every frame at once: cls_logits
    (T, Q, C1) -> (T,), entry t = F.cross_entropy(cls_logits[t], full((Q,), class_index)).  The loss loop indexes it where it now
    calls cross_entropy; an entry nobody uses receives a zero gradient, so its frame's logits do too.  ONE launch (a block per
    frame, fixed order) and one backward, g[t] / Q * (softmax - onehot), which reads the logits alone.  CPU or non-fp32 tensors,
    autocast, Q > 2048 or C1 > 1024 take noobject_loss_torch; temporal_calls counts the calls by path."""
    c = _noobject_class(cls_logits, class_index)
    T, Q, C1 = cls_logits.shape
    if not (_temporal_takes(cls_logits) and Q <= NOOBJECT_MAX_Q and C1 <= NOOBJECT_MAX_C):
        return noobject_loss_torch(cls_logits, c)
    temporal_calls["kernel"] += 1
    if _wants_grad(cls_logits):
        return _NoObjectLoss.apply(cls_logits, c)
    return _noobject_forward(cls_logits.detach().contiguous(), c)


def consistency_loss_torch(a: torch.Tensor) -> torch.Tensor:
    """consistency_loss as the improved trainer's loop of mse_loss calls (temp_dfine_over_improved.py:291-299): what it falls back to."""
    if a.dim() != 3:
        raise ValueError("a (T, Q, C) is expected")
    temporal_calls["torch"] += 1
    T = a.shape[0]
    if T <= 1:
        return a.new_zeros(())
    loss = 0.0
    for t in range(1, T):
        loss = loss + torch.nn.functional.mse_loss(a[t], a[t - 1])
    return loss / (T - 1)


class _ConsistencyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        x = a.contiguous()
        ctx.save_for_backward(x)
        return _consistency_forward(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        g = _f32c(grad_out, "grad_output")
        dx = torch.empty_like(x)
        check(lib.m355_dfine_consistency_loss_backward(_ptr(g), _ptr(x), x.shape[0], x[0].numel(), _ptr(dx), _stream()))
        return dx


def _consistency_forward(x) -> torch.Tensor:
    T, N = x.shape[0], x[0].numel()
    work = torch.empty(int(lib.m355_dfine_consistency_workspace_bytes(T, N)), dtype=torch.uint8, device=x.device)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    check(lib.m355_dfine_consistency_loss_forward(_ptr(x), T, N, _ptr(work), work.numel(), _ptr(out), _stream()))
    return out


def consistency_loss(a: torch.Tensor) -> torch.Tensor:
    """The improved trainer's anomaly consistency loss (temp_dfine_over_improved.py:291-299) without its Python loop: a (T, Q, C) ->
    a scalar, (1 / (T - 1)) sum_{t >= 1} mean((a[t] - a[t - 1]) ** 2); T = 1 gives a zero tensor.  Two launches forward (per-frame
    partial sums into a workspace, then a fixed-order sum) and one backward,
    g * 2 / ((T - 1) Q C) * ((a[t] - a[t - 1]) [t >= 1] - (a[t + 1] - a[t]) [t < T - 1]), instead of T - 1 small graphs.  CPU or
    non-fp32 tensors, autocast, Q * C > 2^27 or T * Q * C >= 2^31 take consistency_loss_torch; temporal_calls counts the calls."""
    if a.dim() != 3:
        raise ValueError("a (T, Q, C) is expected")
    T, N = a.shape[0], a.shape[1] * a.shape[2]
    if not (_temporal_takes(a) and N <= CONSISTENCY_MAX_N and T * N < 1 << 31):
        return consistency_loss_torch(a)
    temporal_calls["kernel"] += 1
    if T == 1:
        return a.new_zeros(())
    if _wants_grad(a):
        return _ConsistencyLoss.apply(a)
    return _consistency_forward(a.detach().contiguous())


def temporal_head(fused: torch.Tensor, init_ref: torch.Tensor, class_head, bbox_head, project: torch.Tensor, reg_scale: float, *,
                  scores=None, context=None, anomaly_head=None, bound: float = 20.0):
    """What the three trainers and their eval / predict scripts run between the temporal encoder and the loss or the
    post-processing, from the ops above: [temporal_fuse(fused, scores, context)] -> class_head, bbox_head and anomaly_head (the
    callers' nn.Modules, torch GEMMs, with their own parameters) -> guard_logits(cls, anomaly, bound) ->
    decode_boxes(bbox_dist, project, init_ref, reg_scale, clamp01=True, guard=True).
    fused (T, Q, D); init_ref (T, Q, 4); project (bins + 1,): the trainers' Wn, a constant here; scores (T, Q, 1) or (T, Q) with
    an optional context (T, Q, D): the improved trainer's attention scores and GRU context; anomaly_head: its anomaly_detector.
    Returns (cls_logits (T, Q, C1), bbox_pred (T, Q, 4), anomaly_scores (T, Q, C1 - 1) or None)."""
    if scores is None and context is not None:
        raise ValueError("context comes with scores: the fusion is fused * softmax(scores) + context")
    x = fused if scores is None else temporal_fuse(fused, scores, context)
    anomaly = anomaly_head(x) if anomaly_head is not None else None
    cls_logits = guard_logits(class_head(x), anomaly, bound)
    bbox_pred = decode_boxes(bbox_head(x), project, init_ref, reg_scale, clamp01=True, guard=True)
    return cls_logits, bbox_pred, anomaly


# ---- the end of the trainers' step: clip_grad_norm_ and the Adam / AdamW update (csrc/dfine_optim.hip) ----

OPTIM_CHUNK = DFINE_OPTIM_CHUNK                # elements of a tensor that one block takes
OPTIM_MAX_TENSORS = DFINE_OPTIM_MAX_TENSORS    # rows of one table; a longer list takes torch's own function
OPTIM_RING = 4                                 # pinned tables in flight before a step waits for the oldest copy
optim_calls = {"kernel": 0, "torch": 0}        # clip_grad_norm_ calls and bound steps by path (tests and tools read it)
_OPTIM_ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("chunk0", "<i4"), ("lr", "<f4"),
                       ("weight_decay", "<f4"), ("beta1", "<f4"), ("beta2", "<f4"), ("eps", "<f4"), ("step_size", "<f4"),
                       ("bc2_sqrt", "<f4"), ("one_minus_beta1", "<f4"), ("one_minus_beta2", "<f4"), ("decay", "<f4"),
                       ("reserved", "<i4", (3,))])
assert _OPTIM_ROW.itemsize == C.sizeof(DfineOptimRow) == 96


class _OptimTables:
    """The tables of one caller on one device: a ring of pinned buffers, each with its device copy and the event after the
    launches that read it, and the partial sums of the norm.  A pinned buffer is rewritten only after its event has passed."""

    def __init__(self, device):
        self.device = device
        self.slots = [None] * OPTIM_RING   # [host tensor, rows (numpy view of it), device tensor, event]
        self.turn = 0
        self.partials = None

    def take(self, n: int):
        """the next slot with room for n rows, its earlier upload and launches behind it"""
        if self.slots[0] is None or self.slots[0][1].shape[0] < n:   # all slots at once: no pinned allocation in a later step
            cap = max(64, 1 << (n - 1).bit_length())
            for i in range(OPTIM_RING):
                host = torch.empty((cap * _OPTIM_ROW.itemsize,), dtype=torch.uint8, pin_memory=True)
                self.slots[i] = [host, host.numpy().view(_OPTIM_ROW), torch.empty_like(host, device=self.device, pin_memory=False),
                                 torch.cuda.Event()]
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % OPTIM_RING
        if not slot[3].query():
            slot[3].synchronize()          # the GPU is OPTIM_RING steps behind: wait for the oldest
        return slot

    def reserve_partials(self, chunks: int) -> torch.Tensor:
        if self.partials is None or self.partials.numel() < chunks:
            self.partials = torch.empty((max(1024, 1 << (chunks - 1).bit_length()),), dtype=torch.float32, device=self.device)
        return self.partials


def _optim_upload(slot, n: int):
    """rows [0, n) of the slot's pinned table to its device copy, one asynchronous copy; -> (host pointer, device pointer)"""
    nbytes = n * _OPTIM_ROW.itemsize
    slot[2][:nbytes].copy_(slot[0][:nbytes], non_blocking=True)
    return C.c_void_p(slot[0].data_ptr()), C.c_void_p(slot[2].data_ptr())


def _optim_chunks(numel: np.ndarray, rows: np.ndarray) -> int:
    """write numel and the chunk prefix of the rows; -> the number of chunks (the grid)"""
    chunks = (numel + (OPTIM_CHUNK - 1)) // OPTIM_CHUNK
    ends = np.cumsum(chunks)
    total = int(ends[-1])
    if total > 0x7fffffff:
        raise ValueError("the tensors have more chunks than one launch can index")
    rows["numel"] = numel
    rows["chunk0"] = ends - chunks
    return total


_clip_tables: dict = {}


def _clip_takes(grads, norm_type, error_if_nonfinite) -> bool:
    if not grads or len(grads) > OPTIM_MAX_TENSORS or error_if_nonfinite:
        return False
    try:
        if float(norm_type) != 2.0:
            return False
    except (TypeError, ValueError):
        return False
    dev = grads[0].device
    return dev.type == "cuda" and all(g.device == dev and g.dtype is torch.float32 and g.layout is torch.strided and
                                      g.is_contiguous() for g in grads)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ for contiguous fp32 CUDA gradients and the 2-norm, three launches and one table upload
    whatever the number of tensors: the squared sums of all chunks, their sum in a fixed order with the norm and the coefficient
    c = min(1, max_norm / (norm + 1e-6)) in double, and g = g c in place, rounded once (c == 1 gives every bit back).  Returns
    the total norm as a 0-d device tensor and does not synchronise; bitwise reproducible.  Non-finite gradients behave as with
    error_if_nonfinite=False.  Any other norm_type, error_if_nonfinite=True, CPU, non-fp32, sparse or non-contiguous gradients
    and lists over OPTIM_MAX_TENSORS take torch's function; `foreach` only matters there."""
    parameters = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not _clip_takes(grads, norm_type, error_if_nonfinite):
        optim_calls["torch"] += 1
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    dev = grads[0].device
    grads = [g for g in grads if g.numel() > 0]
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    if not grads:
        return out.zero_()[0]
    n = len(grads)
    with torch.cuda.device(dev):
        tables = _clip_tables.get(dev)
        if tables is None:
            tables = _clip_tables[dev] = _OptimTables(dev)
        slot = tables.take(n)
        rows = slot[1][:n]
        rows["g"] = [g.data_ptr() for g in grads]
        chunks = _optim_chunks(np.array([g.numel() for g in grads], np.int64), rows)
        partials = tables.reserve_partials(chunks)
        h, d = _optim_upload(slot, n)
        stream = _stream()
        check(lib.m355_dfine_grad_sumsq_launch(h, d, n, _ptr(partials), partials.numel(), stream))
        check(lib.m355_dfine_clip_scale_launch(h, d, n, _ptr(partials), partials.numel(), float(max_norm), _ptr(out), stream))
        slot[3].record()
    optim_calls["kernel"] += 1
    return out[0]


def _optim_group_takes(group) -> bool:
    """the default flags of torch.optim.Adam / AdamW, python-number hyper-parameters"""
    if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable") or group.get("fused"):
        return False
    betas = group["betas"]
    return not any(isinstance(x, torch.Tensor) for x in (group["lr"], group["weight_decay"], group["eps"], betas[0], betas[1]))


def _optim_tensor_takes(t, device) -> bool:
    return (isinstance(t, torch.Tensor) and t.device == device and t.dtype is torch.float32 and t.layout is torch.strided and
            t.is_contiguous())


class _OptimEntry:
    """a parameter of a bound optimizer as its step last saw it: the state tensors it has checked, their pointers, and the
    parameter's slot in the host buffer of step counts.  Compared by identity."""
    __slots__ = ("ptr", "m", "v", "step", "m_ptr", "v_ptr", "numel", "slot")


class _BoundAdam:
    """What a bound optimizer keeps between steps: its tables, one entry per parameter that has had a gradient, and the rows of
    the last step that do not change while the same parameters have gradients (p, m, v, numel, the chunk prefix).
    The `step` tensors of the optimizer's state are 0-d views of ONE host buffer: torch keeps a 0-d fp32 host tensor per
    parameter and adds 1 to each, which for some hundred tensors costs more than the whole update on the device; as views they
    are incremented and read with one numpy operation.  To torch, to state_dict() and to a checkpoint each is the 0-d tensor it
    always was; a `step` that came in through load_state_dict() is copied into the buffer and replaced by its view."""

    def __init__(self, device, max_norm, n_params: int):
        self.device = device
        self.max_norm = None if max_norm is None else float(max_norm)
        self.tables = _OptimTables(device)
        self.entries = {}
        self.slot_of = {}
        self.steps = torch.zeros((max(64, n_params),), dtype=torch.float64 if torch.get_default_dtype() is torch.float64 else torch.float32)
        self.steps_np = self.steps.numpy()
        self.cached = None

    def _step_view(self, optimizer, p, value: float) -> int:
        """the slot of p in the buffer of step counts, holding `value`"""
        i = self.slot_of.get(p)
        if i is None:
            i = self.slot_of[p] = len(self.slot_of)
            if i >= self.steps.numel():              # parameters added after the binding: a larger buffer, every view moved
                old = self.steps
                self.steps = torch.zeros((2 * (i + 1),), dtype=old.dtype)
                self.steps[:old.numel()] = old
                self.steps_np = self.steps.numpy()
                for q, e in self.entries.items():
                    if optimizer.state[q].get("step") is e.step:
                        e.step = optimizer.state[q]["step"] = self.steps[e.slot]
        self.steps_np[i] = value
        return i

    def entry(self, optimizer, p):
        """the checked entry of a parameter that has a gradient, its state created as torch creates it; None: outside the domain"""
        st = optimizer.state[p]
        e = self.entries.get(p)
        if len(st) == 0:
            i = self._step_view(optimizer, p, 0.0)
            st["step"] = self.steps[i]
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            e = None
        ptr = p.data_ptr()
        m, v, step = st.get("exp_avg"), st.get("exp_avg_sq"), st.get("step")
        if e is not None and e.ptr == ptr and e.m is m and e.v is v and e.step is step:
            return e
        if not (_optim_tensor_takes(p, self.device) and _optim_tensor_takes(m, self.device) and _optim_tensor_takes(v, self.device) and
                m.shape == p.shape and v.shape == p.shape and isinstance(step, torch.Tensor) and step.device.type == "cpu" and
                step.numel() == 1 and step.dtype in (torch.float32, torch.float64)):
            return None
        e = self.entries[p] = _OptimEntry()
        e.ptr, e.m, e.v, e.m_ptr, e.v_ptr, e.numel = ptr, m, v, m.data_ptr(), v.data_ptr(), p.numel()
        e.slot = self._step_view(optimizer, p, float(step))
        e.step = st["step"] = self.steps[e.slot]
        return e

    def collect(self, optimizer):
        """-> (entries, gradients, group index of each, mode, entries without elements) of the parameters that have a gradient,
        or None when this step is outside the kernels' domain; parameters without elements get no row (torch updates nothing of
        them but `step`)"""
        if getattr(optimizer, "grad_scale", None) is not None or getattr(optimizer, "found_inf", None) is not None:
            return None
        ents, grads, gidx, empty = [], [], [], []
        mode = None
        for gi, group in enumerate(optimizer.param_groups):
            if not _optim_group_takes(group):
                return None
            m = DFINE_OPTIM_ADAMW if group.get("decoupled_weight_decay") else DFINE_OPTIM_ADAM
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.layout is not torch.strided or not g.is_contiguous():
                    return None
                e = self.entry(optimizer, p)
                if e is None or (mode is not None and mode != m):
                    return None
                mode = m
                if e.numel == 0:
                    empty.append(e)
                    continue
                ents.append(e)
                grads.append(g)
                gidx.append(gi)
        if len(ents) > OPTIM_MAX_TENSORS:
            return None
        return ents, grads, gidx, mode, empty

    def static_rows(self, ents, gidx):
        """-> (rows with p, m, v, numel and chunk0 filled, chunks, group index array, step slot array), kept while the same
        entries come in the same order"""
        c = self.cached
        if c is None or c[0] != ents or c[1] != gidx:
            rows = np.zeros((len(ents),), _OPTIM_ROW)
            rows["p"] = [e.ptr for e in ents]
            rows["m"] = [e.m_ptr for e in ents]
            rows["v"] = [e.v_ptr for e in ents]
            chunks = _optim_chunks(np.array([e.numel for e in ents], np.int64), rows)
            c = self.cached = (ents, gidx, rows, chunks, np.asarray(gidx, np.intp), np.array([e.slot for e in ents], np.intp))
        return c[2:]

    def bump(self, slots) -> np.ndarray:
        """add 1 to the step counts in `slots`; -> the new counts in double"""
        self.steps_np[slots] += 1
        return self.steps_np[slots].astype(np.float64)


def _optimizer_step(self, closure=None):
    """`step` of an optimizer bound by bind_optimizer"""
    bound = self._m355_optim
    loss = None
    if closure is not None:
        with torch.enable_grad():
            loss = closure()
    with torch.no_grad():
        plan = bound.collect(self)
        if plan is None:
            # torch's own clip and step on the same state, without a second round of the step hooks (this call runs inside them)
            optim_calls["torch"] += 1
            self.last_grad_norm = None
            if bound.max_norm is not None:
                self.last_grad_norm = torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g["params"]],
                                                                     bound.max_norm)
            torch_step = type(self).step
            getattr(torch_step, "__wrapped__", torch_step)(self)
            return loss
        ents, grads, gidx, mode, empty = plan
        self.last_grad_norm = None
        if empty:
            bound.bump(np.array([e.slot for e in empty], np.intp))
        n = len(ents)
        if n == 0:
            return loss
        static, chunks, gidx, slots = bound.static_rows(ents, gidx)
        t = bound.bump(slots)
        hyper = np.array([(g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"]) for g in self.param_groups], np.float64)
        lr, wd, beta1, beta2, eps = hyper[gidx].T
        with torch.cuda.device(bound.device):
            slot = bound.tables.take(n)
            rows = slot[1][:n]
            rows[:] = static
            rows["g"] = [g.data_ptr() for g in grads]
            rows["lr"], rows["weight_decay"], rows["beta1"], rows["beta2"], rows["eps"] = lr, wd, beta1, beta2, eps
            rows["step_size"] = lr / (1.0 - beta1 ** t)            # in double, each tensor with its own step count
            rows["bc2_sqrt"] = np.sqrt(1.0 - beta2 ** t)
            rows["one_minus_beta1"], rows["one_minus_beta2"], rows["decay"] = 1.0 - beta1, 1.0 - beta2, 1.0 - lr * wd
            h, d = _optim_upload(slot, n)
            stream = _stream()
            if bound.max_norm is None:
                check(lib.m355_dfine_adam_launch(h, d, n, mode, None, 0, 0.0, None, stream))
            else:
                partials = bound.tables.reserve_partials(chunks)
                norm = torch.empty((4,), dtype=torch.float32, device=bound.device)
                check(lib.m355_dfine_grad_sumsq_launch(h, d, n, _ptr(partials), partials.numel(), stream))
                check(lib.m355_dfine_adam_launch(h, d, n, mode, _ptr(partials), partials.numel(), bound.max_norm, _ptr(norm), stream))
                self.last_grad_norm = norm[0]
            slot[3].record()
        optim_calls["kernel"] += 1
    return loss


def _hooked_optimizer_step(self, closure=None):
    self._opt_called = True              # what an lr_scheduler's wrapper of `step` sets: its call-order check reads it
    return _optimizer_step_with_hooks(self, closure)


_optimizer_step_with_hooks = torch.optim.Optimizer.profile_hook_step(_optimizer_step)   # torch's step pre- and post-hooks
_hooked_optimizer_step._wrapped_by_lr_sched = True   # a scheduler constructed later finds `step` wrapped and leaves it alone


def bind_optimizer(optimizer, max_norm=None):
    """Give THIS optimizer instance a `step` that runs the update of all its parameters as one launch (csrc/dfine_optim.hip);
    returns its argument.  Bound: torch.optim.Adam and torch.optim.AdamW with their default flags (no amsgrad, maximize,
    capturable, differentiable, fused) whose parameters are all contiguous fp32 tensors on one CUDA device; anything else comes
    back untouched and runs torch's step.  The state is torch's own (`step` a 0-d tensor on the host, exp_avg, exp_avg_sq,
    created lazily; the `step` tensors of one bound optimizer are views of one host buffer, so that all of them are incremented at
    once), so state_dict() / load_state_dict() and checkpoints interchange with an unbound optimizer; parameters without a gradient are
    skipped, the groups' hyper-parameters are read on every call (schedulers work, bound before or after their construction),
    and the step does not synchronise: the table goes up as one asynchronous copy from a ring of pinned buffers.
    max_norm: fold torch.nn.utils.clip_grad_norm_(all parameters, max_norm) into the step: one launch for the squared norm, and
    the coefficient applied inside the update.  The trainer drops its clip line; `.grad` stays as backward left it (it is not
    scaled in place, unlike clip_grad_norm_) and `optimizer.last_grad_norm` is the total norm as a 0-d device tensor.
    A step that meets something outside the domain (a non-contiguous gradient, a flag switched on later) runs torch's
    clip_grad_norm_ and step for that call."""
    import types
    if type(optimizer) not in (torch.optim.Adam, torch.optim.AdamW) or not all(_optim_group_takes(g) for g in optimizer.param_groups):
        return optimizer
    params = [p for g in optimizer.param_groups for p in g["params"]]
    if not params or params[0].device.type != "cuda" or not all(_optim_tensor_takes(p, params[0].device) for p in params):
        return optimizer
    optimizer._m355_optim = _BoundAdam(params[0].device, max_norm, len(params))
    optimizer.last_grad_norm = None
    optimizer.step = types.MethodType(_hooked_optimizer_step, optimizer)
    return optimizer
