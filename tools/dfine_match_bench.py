"""Times the D-FINE loss's Hungarian matcher: transformers' RTDetrHungarianMatcher.forward on device tensors (its ~25 torch
launches, the cost matrix's .cpu() and scipy included) against the same module with `forward = dfine.matcher_forward` (one HIP
launch).  Same process, alternating blocks, median of the blocks' per-call wall times (each block ends synchronised).

    python tools/dfine_match_bench.py [--calls 50] [--rounds 7] [--out profiles/dfine_match_bench.json]

Three shapes: (B 1, Q 300, n 3) the reference trainers' per-frame call; (B 16, Q 300, n 6..10) a batch of config 5;
(B 4, Q 300, n 64).  `launches` counts the device activities (kernels and copies) of one call under torch.profiler.
The kernel's own share of a bound call comes from `rocprofv3 --kernel-trace --stats -- python tools/dfine_match_bench.py`
(DESIGN.md section 9)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("frame_b1_n3", 300, [3]), ("batch_b16_n8", 300, [6, 7, 8, 9, 10, 8, 7, 9] * 2), ("b4_n64", 300, [64] * 4)]


def make_inputs(Q, sizes, C, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    logits = 2 * torch.randn(B, Q, C, generator=g)
    boxes = torch.sigmoid(torch.randn(B, Q, 4, generator=g))
    boxes[..., 2:] = boxes[..., 2:] * 0.5 + 0.01
    targets = []
    for n in sizes:
        tb = torch.rand(n, 4, generator=g)
        tb[:, 2:] = tb[:, 2:] * 0.4 + 0.02
        targets.append({"class_labels": torch.randint(0, C, (n,), generator=g).to(dev), "boxes": tb.to(dev)})
    return {"logits": logits.to(dev), "pred_boxes": boxes.to(dev)}, targets


def block(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_match_bench.json"))
    args = ap.parse_args()
    from transformers import DFineConfig
    from transformers.loss.loss_rt_detr import RTDetrHungarianMatcher
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)
    stock_forward = RTDetrHungarianMatcher.forward
    matcher = RTDetrHungarianMatcher(DFineConfig())
    result = {"device": torch.cuda.get_device_name(0), "calls_per_block": args.calls, "blocks": args.rounds, "unit": "us per call (wall)",
              "shapes": {}}
    for name, Q, sizes in SHAPES:
        outputs, targets = make_inputs(Q, sizes, 80, dev)
        variants = {
            "unbound": lambda: stock_forward(matcher, outputs, targets),
            "bound": lambda: dfine.matcher_forward(matcher, outputs, targets),
            "bound_check_false": lambda: dfine.hungarian_match(outputs["logits"], outputs["pred_boxes"], targets, check=False),
        }
        want = variants["unbound"]()
        got = variants["bound"]()
        same = all(torch.equal(a, c.cpu()) and torch.equal(b, d.cpu()) for (a, b), (c, d) in zip(want, got))
        for fn in variants.values():
            block(fn, 5)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(block(fn, args.calls))
        entry = {"B": len(sizes), "Q": Q, "targets_per_image": sizes, "same_indices": same}
        for k, fn in variants.items():
            entry[k] = {"median_us": round(statistics.median(times[k]), 1), "min_us": round(min(times[k]), 1),
                        "device_activities_per_call": device_activities(fn)}
        entry["speedup_bound_vs_unbound"] = round(entry["unbound"]["median_us"] / entry["bound"]["median_us"], 2)
        result["shapes"][name] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
