"""Generates tests/golden/dfine_loop_golden_<case>.npz: inputs, the decoder's state dict and all six output fields of transformers'
own DFineDecoder.forward (transformers 5.15.0, models/d_fine/modeling_d_fine.py:1184-1293) at a tiny config, on the CPU in fp32 with
seeded random parameters and inputs.  The decoder is DFineForObjectDetection(cfg).model.decoder, which carries the model's class_embed
and bbox_embed.  Cases: "train" (training mode, every layer's heads), "eval" (eval mode, eval_idx = the last layer), "eval_idx1"
(eval mode, three decoder layers with eval_idx = 1; upstream then builds a fourth layer but three bbox_embed heads and its loop
raises IndexError, so this case appends one more head for the loop to run).
Run in the build container only (`python tests/golden/make_dfine_loop_golden.py`); the .npz files are data."""
import os

import numpy as np
import torch
import transformers
from transformers import DFineConfig, DFineForObjectDetection
from transformers.models.d_fine import modeling_d_fine as M

B, Q = 2, 11
shapes = [(8, 8), (4, 4), (2, 2)]
S = sum(h * w for h, w in shapes)
here = os.path.dirname(os.path.abspath(__file__))


def randomise(decoder):
    """LayerNorms start at weight 1, bias 0 and the last layer of every LQE and bbox_embed head at 0, which would hide a dropped term"""
    with torch.no_grad():
        for m in decoder.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                m.bias.copy_(0.2 * torch.randn_like(m.bias))
        for head in decoder.lqe_layers:
            head.reg_conf.layers[-1].weight.normal_(0.0, 0.1)
        for head in decoder.bbox_embed:   # starts at 0 too: every distribution would be flat
            head.layers[-1].weight.normal_(0.0, 0.5)
            head.layers[-1].bias.normal_(0.0, 0.5)


for case, training, layers, eval_idx in (("train", True, 2, -1), ("eval", False, 2, -1), ("eval_idx1", False, 3, 1)):
    torch.manual_seed(7)
    cfg = DFineConfig(d_model=32, decoder_attention_heads=2, decoder_ffn_dim=64, decoder_n_points=[3, 6, 3], decoder_layers=layers,
                      eval_idx=eval_idx, num_queries=Q, num_denoising=0, dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)
    decoder = DFineForObjectDetection(cfg).model.decoder
    while len(decoder.bbox_embed) < len(decoder.layers):
        decoder.bbox_embed.append(M.DFineMLP(cfg.hidden_size, cfg.hidden_size, 4 * (cfg.max_num_bins + 1), 3))
    randomise(decoder)
    decoder.train(training)
    enc, ref, x = torch.randn(B, S, cfg.d_model), torch.randn(B, Q, 4), torch.randn(B, Q, cfg.d_model)
    with torch.no_grad():
        y = decoder(encoder_hidden_states=enc, reference_points=ref, inputs_embeds=x, spatial_shapes=torch.tensor(shapes),
                    spatial_shapes_list=shapes)
    out = {"transformers_version": np.array(transformers.__version__), "shapes": np.array(shapes, np.int32),
           "training": np.array(training), "eval_idx": np.array(decoder.eval_idx, np.int32),
           "heads": np.array(cfg.decoder_attention_heads, np.int32), "points": np.array(cfg.decoder_n_points, np.int32),
           "offset_scale": np.array(cfg.decoder_offset_scale, np.float32), "eps": np.array(cfg.layer_norm_eps, np.float32),
           "max_num_bins": np.array(cfg.max_num_bins, np.int32), "top_k": np.array(cfg.top_prob_values, np.int32),
           "in_enc": enc.numpy(), "in_ref": ref.numpy(), "in_x": x.numpy()}
    for n, p in decoder.state_dict().items():
        out[f"param.{n}"] = p.detach().numpy().copy()
    for field in ("last_hidden_state", "intermediate_hidden_states", "intermediate_logits", "intermediate_reference_points",
                  "intermediate_predicted_corners", "initial_reference_points"):
        out[f"out_{field}"] = getattr(y, field).numpy()
    path = os.path.join(here, f"dfine_loop_golden_{case}.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items() if k.startswith("out_")})
