"""Restatements for the decoder-loop tests (dfine.query_pos_hidden / refine_reference / refine_boxes / decoder_forward).

torch expressions of the three ops and of transformers' DFineDecoder.forward (modeling_d_fine.py:1184-1293, no mask, no dropout) on
the decoder's own state dict; the layers and the LQE heads are those of tests/dfine_decoder_ref.py.  They run in any dtype on any
device: float64 on the CPU is the reference of every numeric test, fp32 on the GPU is the baseline the kernels' error is measured
against.
"""
import torch

import dfine_decoder_ref as layer_ref

F = torch.nn.functional
FIELDS = ("last_hidden_state", "intermediate_hidden_states", "intermediate_logits", "intermediate_reference_points",
          "intermediate_predicted_corners", "initial_reference_points")


# ---- the three ops ---------------------------------------------------------------------------------------------------------------
def query_pos_hidden(ref, weight, bias):
    """the first Linear + ReLU of query_pos_head: ref (..., 4), weight (H, 4), bias (H,)"""
    return torch.relu(F.linear(ref, weight, bias))


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


def refine_reference(delta, ref, eps=1e-5):
    return torch.sigmoid(delta + inverse_sigmoid(ref, eps))


def weighting_function(max_num_bins, up, reg_scale):
    upper_bound1 = abs(up[0]) * abs(reg_scale)
    upper_bound2 = abs(up[0]) * abs(reg_scale) * 2
    step = (upper_bound1 + 1) ** (2 / (max_num_bins - 2))
    left = [-((step) ** i) + 1 for i in range(max_num_bins // 2 - 1, 0, -1)]
    right = [(step) ** i - 1 for i in range(1, max_num_bins // 2)]
    return torch.cat([-upper_bound2] + left + [torch.zeros_like(up[0][None])] + right + [upper_bound2], 0)


def integral(pred_corners, project):
    nb1 = project.numel()
    p = torch.softmax(pred_corners.reshape(-1, nb1), dim=1)
    return F.linear(p, project.reshape(1, -1)).reshape(tuple(pred_corners.shape[:-1]) + (4,))


def distance2bbox(points, distance, reg_scale):
    reg_scale = abs(reg_scale)
    x0 = points[..., 0] - (0.5 * reg_scale + distance[..., 0]) * (points[..., 2] / reg_scale)
    y0 = points[..., 1] - (0.5 * reg_scale + distance[..., 1]) * (points[..., 3] / reg_scale)
    x1 = points[..., 0] + (0.5 * reg_scale + distance[..., 2]) * (points[..., 2] / reg_scale)
    y1 = points[..., 1] + (0.5 * reg_scale + distance[..., 3]) * (points[..., 3] / reg_scale)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1)


def refine_boxes(delta_corners, prev_corners, project, points, reg_scale):
    """(pred_corners, boxes); prev_corners None: pred_corners is delta_corners"""
    pred = delta_corners if prev_corners is None else delta_corners + prev_corners
    return pred, distance2bbox(points, integral(pred, project), reg_scale)


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def _sub(P, prefix):
    return {k[len(prefix) + 1:]: v for k, v in P.items() if k.startswith(prefix + ".")}


def relu_mlp(x, P, prefix):
    """DFineMLP / DFineMLPPredictionHead with ReLU on "<prefix>.layers.<j>.weight" / ".bias\""""
    n = len(_sub(P, prefix)) // 2
    for j in range(n):
        x = F.linear(x, P[f"{prefix}.layers.{j}.weight"], P[f"{prefix}.layers.{j}.bias"])
        if j < n - 1:
            x = torch.relu(x)
    return x


def decoder_loop(P, enc, reference_points, x, shapes, *, training, eval_idx, n_heads, num_points_list, offset_scale, eps, max_num_bins,
                 top_k):
    """DFineDecoder.forward on the decoder's state dict P ("layers.<i>...", "query_pos_head...", "pre_bbox_head...",
    "bbox_embed.<i>...", "class_embed.<i>...", "lqe_layers.<i>...", "up", "reg_scale"), in upstream's order and with its detach
    points; returns the six fields of DFineDecoderOutput as a dict"""
    n_layers = len({k.split(".")[1] for k in P if k.startswith("layers.")})
    project = weighting_function(max_num_bins, P["up"], P["reg_scale"])
    inter, inter_ref, inter_logits, inter_corners, initial_ref = [], [], [], [], []
    output_detach = pred_corners_undetach = 0
    ref_detach = torch.sigmoid(reference_points)
    for i in range(n_layers):
        pos = relu_mlp(ref_detach, P, "query_pos_head").clamp(min=-10, max=10)
        x = layer_ref.decoder_layer(x, pos, ref_detach, enc, shapes, _sub(P, f"layers.{i}"), n_heads, num_points_list, offset_scale, eps)
        if i == 0:
            new_ref = refine_reference(relu_mlp(x, P, "pre_bbox_head"), ref_detach)
            ref_initial = new_ref.detach()
        pred_corners = relu_mlp(x + output_detach, P, f"bbox_embed.{i}") + pred_corners_undetach
        boxes = distance2bbox(ref_initial, integral(pred_corners, project), P["reg_scale"])
        pred_corners_undetach = pred_corners
        ref_detach = boxes.detach()
        output_detach = x.detach()
        inter.append(x)
        if training or i == eval_idx:
            scores = F.linear(x, P[f"class_embed.{i}.weight"], P[f"class_embed.{i}.bias"])
            if i == 0:
                inter_logits.append(scores)
                inter_ref.append(new_ref)
            inter_logits.append(layer_ref.lqe(scores, pred_corners, _sub(P, f"lqe_layers.{i}"), max_num_bins, top_k))
            inter_ref.append(boxes)
            initial_ref.append(ref_initial)
            inter_corners.append(pred_corners)
    return {"last_hidden_state": x, "intermediate_hidden_states": torch.stack(inter),
            "intermediate_logits": torch.stack(inter_logits, dim=1), "intermediate_reference_points": torch.stack(inter_ref, dim=1),
            "intermediate_predicted_corners": torch.stack(inter_corners, dim=1),
            "initial_reference_points": torch.stack(initial_ref, dim=1)}
