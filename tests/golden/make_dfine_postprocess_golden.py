"""Generates tests/golden/dfine_postprocess_golden.npz: inputs of the D-FINE detection post-processing and what transformers'
own RTDetrImageProcessorPil.post_process_object_detection (5.15.0, the method the torchvision-backed RTDetrImageProcessor shares
line for line) returns for them on CPU fp32 tensors, at the reference trainers' threshold 0.3 and at threshold -1 (all Q rows).

Random logits do not make safe goldens: fp32 sigmoids of normal logits tie exactly often enough that torch.topk's order among
the ties would be recorded.  Every image is therefore built by construction (tests/dfine_postprocess_ref.ladder_logits), and this
script asserts per image that the top Q + 1 float64 scores are pairwise at least 1e-4 apart and none lies within 1e-4 of the
threshold; a seed that misses either condition is skipped and the next one taken (the seed used is recorded).  Run in the
build container only (`python tests/golden/make_dfine_postprocess_golden.py`); the .npz is data: inputs and expected outputs."""
import os
import sys
import types

import numpy as np
import torch
import transformers
from transformers import RTDetrImageProcessorPil

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dfine_postprocess_ref as ref  # noqa: E402

MIN_GAP = 1e-4


def build_case(shape, seed):
    B, Q, C = shape
    rng = np.random.default_rng(seed)
    logits = np.stack([ref.ladder_logits(rng, Q, C) for _ in range(B)])
    return logits, ref.random_boxes(rng, B, Q)


def main():
    processor = RTDetrImageProcessorPil()
    out = {"transformers_version": np.array(transformers.__version__), "torch_version": np.array(torch.__version__),
           "threshold": np.array(ref.GOLDEN_THRESHOLD)}
    for shape, sizes in ref.CASES:
        B, Q, C = shape
        name = ref.case_name(shape)
        for seed in range(64):
            logits, boxes = build_case(shape, seed)
            cond = [ref.ladder_conditions(logits[b], ref.GOLDEN_THRESHOLD) for b in range(B)]
            if all(g >= MIN_GAP and d >= MIN_GAP for g, d in cond):
                break
        else:
            raise AssertionError(f"{name}: no seed below 64 meets the gap conditions")
        outputs = types.SimpleNamespace(logits=torch.from_numpy(logits), pred_boxes=torch.from_numpy(boxes))
        kept = processor.post_process_object_detection(outputs, threshold=ref.GOLDEN_THRESHOLD, target_sizes=sizes)
        full = processor.post_process_object_detection(outputs, threshold=-1.0, target_sizes=sizes)
        assert len(kept) == B and all(len(f["scores"]) == Q for f in full)
        out[name + "/logits"], out[name + "/boxes"], out[name + "/seed"] = logits, boxes, np.array(seed)
        if sizes is not None:
            out[name + "/sizes"] = np.array(sizes, np.int64)
        out[name + "/kept_counts"] = np.array([len(k["scores"]) for k in kept], np.int64)
        for key, dtype in (("scores", np.float32), ("labels", np.int64), ("boxes", np.float32)):
            out[f"{name}/kept_{key}"] = np.concatenate([k[key].numpy() for k in kept]).astype(dtype)
            out[f"{name}/full_{key}"] = np.stack([f[key].numpy() for f in full]).astype(dtype)
        print(name, "seed", seed, "gaps", ["%.3g" % g for g, _ in cond], "to threshold", ["%.3g" % d for _, d in cond],
              "kept", out[name + "/kept_counts"].tolist())
    path = os.path.join(HERE, ref.GOLDEN)
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
