"""Generates tests/golden/dfine_decoder_golden.npz: inputs, parameters and outputs of transformers' own DFineGate, DFineLQE and
DFineDecoderLayer (transformers 5.15.0, models/d_fine/modeling_d_fine.py) at a tiny config, on the CPU in fp32 with seeded random
parameters and inputs.  Run in the build container only (`python tests/golden/make_dfine_decoder_golden.py`); the .npz is data."""
import os

import numpy as np
import torch
import transformers
from transformers.models.d_fine import modeling_d_fine as M
from transformers.models.d_fine.configuration_d_fine import DFineConfig

torch.manual_seed(0)
cfg = DFineConfig(d_model=64, decoder_attention_heads=2, decoder_ffn_dim=128, decoder_n_points=[3, 6, 3])
B, Q = 2, 17
shapes = [(8, 8), (4, 4), (2, 2)]
S = sum(h * w for h, w in shapes)
out = {"transformers_version": np.array(transformers.__version__), "shapes": np.array(shapes, np.int32),
       "heads": np.array(cfg.decoder_attention_heads, np.int32), "points": np.array(cfg.decoder_n_points, np.int32),
       "offset_scale": np.array(cfg.decoder_offset_scale, np.float32), "eps": np.array(cfg.layer_norm_eps, np.float32),
       "max_num_bins": np.array(cfg.max_num_bins, np.int32), "top_k": np.array(cfg.top_prob_values, np.int32)}


def randomise_norms(module):   # LayerNorm starts at weight 1, bias 0, which would hide a swapped or dropped affine term
    for m in module.modules():
        if isinstance(m, torch.nn.LayerNorm):
            with torch.no_grad():
                m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                m.bias.copy_(0.2 * torch.randn_like(m.bias))


def put(prefix, module):
    for n, p in module.named_parameters():
        out[f"{prefix}.{n}"] = p.detach().numpy().copy()


with torch.no_grad():
    gate = M.DFineGate(cfg.d_model).eval()
    randomise_norms(gate)
    x1, x2 = torch.randn(B, Q, cfg.d_model), torch.randn(B, Q, cfg.d_model)
    out["gate_x1"], out["gate_x2"], out["gate_out"] = x1.numpy(), x2.numpy(), gate(x1, x2).numpy()
    put("gate", gate)

    lqe = M.DFineLQE(cfg).eval()
    scores = torch.randn(B, Q, 3)
    corners = 3.0 * torch.randn(B, Q, 4 * (cfg.max_num_bins + 1))
    out["lqe_scores"], out["lqe_corners"], out["lqe_out"] = scores.numpy(), corners.numpy(), lqe(scores, corners).numpy()
    put("lqe", lqe)

    layer = M.DFineDecoderLayer(cfg).eval()
    randomise_norms(layer)
    hidden, pos = torch.randn(B, Q, cfg.d_model), torch.randn(B, Q, cfg.d_model).clamp(-10, 10)
    ref = torch.rand(B, Q, 1, 4) * torch.tensor([1.0, 1.0, 0.4, 0.4]) + torch.tensor([0.0, 0.0, 0.02, 0.02])
    enc = torch.randn(B, S, cfg.d_model)
    y = layer(hidden, position_embeddings=pos, reference_points=ref, spatial_shapes=torch.tensor(shapes), spatial_shapes_list=shapes,
              encoder_hidden_states=enc)
    out["layer_hidden"], out["layer_pos"], out["layer_ref"], out["layer_enc"] = hidden.numpy(), pos.numpy(), ref.numpy(), enc.numpy()
    out["layer_out"] = y.numpy()
    put("layer", layer)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dfine_decoder_golden.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
