"""Records tests/golden/dfine_select_golden.npz from transformers' own DFineModel.forward on the CPU: the inputs and outputs of its
query selection (modeling_d_fine.py:1804-1828).  Run from the repository root:  python tests/golden/make_dfine_select_golden.py

The model is driven with encoder_outputs=([f0, f1, f2],) of random feature maps (the inputs_embeds route is broken upstream, and
a randomly initialised backbone gives two distinct scores among all tokens) and enc_score_head.weight.normal_(0, 0.5); the maker
asserts that every case's top K + 1 scores are pairwise distinct, so torch.topk's order is the only one.  output_memory is not
stored: the memory gather is a row copy like the other two."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dfine_select_ref as ref  # noqa: E402


def drive(model, feats, pixel_values, seed, **kwargs):
    """what the tests repeat: the same seed before each call, random features as the encoder's output"""
    torch.manual_seed(seed)
    return model(pixel_values, encoder_outputs=([f.clone() for f in feats],), **kwargs)


def build(case, seed):
    from transformers import DFineConfig
    from transformers.models.d_fine.modeling_d_fine import DFineModel
    B, levels, C, K = case
    torch.manual_seed(seed)
    config = DFineConfig(num_labels=C, num_queries=K, anchor_image_size=None, dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)
    model = DFineModel(config).eval()
    with torch.no_grad():
        model.enc_score_head.weight.normal_(0.0, 0.5)
    g = torch.Generator().manual_seed(seed + 1)
    feats = [torch.randn(B, config.encoder_hidden_dim, h, h, generator=g) for h in levels]
    pixel_values = torch.randn(B, 3, 64, 64, generator=g)   # the backbone runs on it and its features are dropped
    return model, feats, pixel_values


def record(case, seed):
    B, levels, C, K = case
    model, feats, pixel_values = build(case, seed)
    with torch.no_grad():
        out = drive(model, feats, pixel_values, seed)
    cls, coord = out.enc_outputs_class.numpy(), out.enc_outputs_coord_logits.numpy()
    init = out.init_reference_points.numpy()
    assert cls.shape == (B, sum(h * h for h in levels), C) and init.shape == (B, K, 4)
    gap = ref.top_gap(ref.token_scores(cls), K)
    assert gap > 0.0, (ref.case_name(case), gap)   # pairwise distinct: no tie for torch.topk to break
    ind = np.empty((B, K), np.int64)
    for b in range(B):
        for r in range(K):   # the token whose coordinate row is this output row
            hit = np.flatnonzero((coord[b].view(np.uint32) == init[b, r].view(np.uint32)).all(-1))
            assert len(hit) == 1, (b, r, hit)
            ind[b, r] = hit[0]
    got = {"enc_outputs_class": cls, "enc_outputs_coord_logits": coord, "indices": ind, "init_reference_points": init,
           "enc_topk_logits": out.enc_topk_logits.numpy(), "enc_topk_bboxes": out.enc_topk_bboxes.numpy()}
    print(f"{ref.case_name(case)}: smallest gap among the top {K + 1} scores {gap:.3e}")
    return {f"{ref.case_name(case)}/{k}": v for k, v in got.items()}


def main():
    arrays = {}
    for n, case in enumerate(ref.CASES):
        arrays.update(record(case, 100 + n))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), ref.GOLDEN)
    np.savez(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
