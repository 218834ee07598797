"""Restatements for the decoder-layer tests (dfine.gate_layer_norm / add_layer_norm(clamp=...) / lqe_statistics /
decoder_layer_forward / lqe_forward).

torch expressions of the three ops, of transformers' DFineDecoderLayer.forward (no mask, no dropout) and of DFineLQE.forward on
dicts of the modules' own parameters; they run in any dtype on any device: float64 on the CPU is the reference of every numeric
test, fp32 on the GPU is the baseline the kernels' error is measured against.  The cross-attention is tests/msda_grad_ref.py.
"""
import math

import torch

import msda_grad_ref

HEAD_DIM = 32
CLAMP = (-65504.0, 65504.0)
F = torch.nn.functional


# ---- the three ops ---------------------------------------------------------------------------------------------------------------
def gate_layer_norm(x1, x2, gate_logits, weight, bias, eps):
    """DFineGate.forward behind its nn.Linear; gate_logits (..., 2 D)"""
    g1, g2 = torch.sigmoid(gate_logits).chunk(2, dim=-1)
    return F.layer_norm(g1 * x1 + g2 * x2, (x1.shape[-1],), weight, bias, eps)


def add_clamp_layer_norm(x, y, weight, bias, eps, lo=CLAMP[0], hi=CLAMP[1]):
    return F.layer_norm((x + y).clamp(min=lo, max=hi), (x.shape[-1],), weight, bias, eps)


def lqe_topk(prob, k):
    """the k largest of the last axis in descending order, an exact tie to the lowest index first: (values, indices)"""
    values, idx = torch.sort(prob, dim=-1, descending=True, stable=True)
    return values[..., :k], idx[..., :k]


def lqe_statistics(pred_corners, max_num_bins, top_k):
    """pred_corners (..., 4 * (max_num_bins + 1)) -> (..., 4 * (top_k + 1)): per side the top_k probabilities, then their mean"""
    lead = pred_corners.shape[:-1]
    prob = torch.softmax(pred_corners.reshape(*lead, 4, max_num_bins + 1), dim=-1)
    top, _ = lqe_topk(prob, top_k)
    return torch.cat([top, top.mean(dim=-1, keepdim=True)], dim=-1).reshape(*lead, 4 * (top_k + 1))


# ---- the layer and the quality head ------------------------------------------------------------------------------------------------
LAYER_PARAM_NAMES = tuple(f"{m}.{p}" for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                                               "self_attn_layer_norm", "encoder_attn.sampling_offsets",
                                               "encoder_attn.attention_weights", "gateway.gate", "gateway.norm", "mlp.layers.0",
                                               "mlp.layers.1", "final_layer_norm") for p in ("weight", "bias"))


def layer_params(layer):
    """the 24 parameters of a DFineDecoderLayer as a dict under their state-dict names"""
    named = dict(layer.named_parameters())
    assert set(named) == set(LAYER_PARAM_NAMES), sorted(set(named) ^ set(LAYER_PARAM_NAMES))
    return {n: named[n] for n in LAYER_PARAM_NAMES}


def self_attention(x, pos, P, n_heads):
    """DFineSelfAttention: position embeddings on q and k only"""
    B, Q, D = x.shape
    qk_in = x if pos is None else x + pos
    lin = lambda t, name: F.linear(t, P[f"self_attn.{name}.weight"], P[f"self_attn.{name}.bias"])  # noqa: E731
    q, k, v = (t.reshape(B, Q, n_heads, D // n_heads).transpose(1, 2) for t in (lin(qk_in, "q_proj"), lin(qk_in, "k_proj"),
                                                                                lin(x, "v_proj")))
    prob = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // n_heads), dim=-1)
    return lin((prob @ v).transpose(1, 2).reshape(B, Q, D), "o_proj")


def cross_attention(q, ref_points, enc, shapes, P, n_heads, num_points_list, offset_scale):
    """DFineMultiscaleDeformableAttention.forward for 4-d reference points (B, Q, 4), method "default": the two nn.Linear layers,
    the softmax over the points, the sampling locations from the reference boxes (on q's device, unlike
    msda_grad_ref.module_locations), then msda_grad_ref.msda"""
    B, Q, D = q.shape
    n = sum(num_points_list)
    off = F.linear(q, P["encoder_attn.sampling_offsets.weight"], P["encoder_attn.sampling_offsets.bias"]).reshape(B, Q, n_heads, n, 2)
    logit = F.linear(q, P["encoder_attn.attention_weights.weight"], P["encoder_attn.attention_weights.bias"]).reshape(B, Q, n_heads, n)
    nscale = torch.tensor([1.0 / m for m in num_points_list for _ in range(m)], dtype=q.dtype, device=q.device).reshape(1, 1, 1, -1, 1)
    loc = ref_points[:, :, None, None, :2] + off * nscale * ref_points[:, :, None, None, 2:] * offset_scale
    return msda_grad_ref.msda(enc.reshape(B, -1, n_heads, D // n_heads), shapes, loc, torch.softmax(logit, dim=-1), num_points_list)


def decoder_layer(x, pos, ref_points, enc, shapes, P, n_heads, num_points_list, offset_scale, eps=1e-5):
    """DFineDecoderLayer.forward without mask and dropout; ref_points (B, Q, 4) or (B, Q, 1, 4), enc (B, S, D)"""
    B, Q, D = x.shape
    x = F.layer_norm(x + self_attention(x, pos, P, n_heads), (D,), P["self_attn_layer_norm.weight"], P["self_attn_layer_norm.bias"], eps)
    q = x if pos is None else x + pos
    c = cross_attention(q, ref_points.reshape(B, Q, 4), enc, shapes, P, n_heads, list(num_points_list), offset_scale)
    g = F.linear(torch.cat([x, c], dim=-1), P["gateway.gate.weight"], P["gateway.gate.bias"])
    x = gate_layer_norm(x, c, g, P["gateway.norm.weight"], P["gateway.norm.bias"], eps)
    h = torch.relu(F.linear(x, P["mlp.layers.0.weight"], P["mlp.layers.0.bias"]))
    y = F.linear(h, P["mlp.layers.1.weight"], P["mlp.layers.1.bias"])
    return add_clamp_layer_norm(x, y, P["final_layer_norm.weight"], P["final_layer_norm.bias"], eps)


def lqe(scores, pred_corners, P, max_num_bins, top_k):
    """DFineLQE.forward on the parameters of its reg_conf MLP (ReLU between the layers), "reg_conf.layers.<i>.weight" / ".bias\""""
    h = lqe_statistics(pred_corners, max_num_bins, top_k)
    n = len(P) // 2
    for i in range(n):
        h = F.linear(h, P[f"reg_conf.layers.{i}.weight"], P[f"reg_conf.layers.{i}.bias"])
        if i < n - 1:
            h = torch.relu(h)
    return scores + h
