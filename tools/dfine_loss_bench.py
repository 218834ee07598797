"""Times the D-FINE criterion, forward + backward: transformers' DFineLoss(DFineConfig()) with RTDetrLoss.forward as it ships
(per decoder output: dozens of tiny torch ops for loss_labels_vfl, loss_boxes, loss_local, several synchronising checks, and
autograd's mirror of all of them) against the same module with `forward = dfine.criterion_forward` (per output: two HIP launches
forward, one backward).  The matcher is bound to dfine.matcher_forward in BOTH arms, so the difference is the loss terms alone.
Same process, alternating blocks, median of the blocks' per-call wall times (each block ends synchronised).

    python tools/dfine_loss_bench.py [--calls 20] [--rounds 7] [--out profiles/dfine_loss_bench.json]

Two shapes: (B 1, Q 300, n 3), one output without the local group: the reference trainers' per-frame call; (B 16, Q 300,
n 6..10) with the 13 outputs of DFineConfig() (main, 5 auxiliary layers with corners, the encoder output, 6 denoising outputs of
200 queries with corners), synthetic tensors of the right shapes.  `device_activities_per_call` counts kernels and copies of one
forward + backward under torch.profiler.  A shape is `accepted` when the slowest bound block is faster than the fastest unbound
block.  The kernels' own share comes from `rocprofv3 --kernel-trace --stats -- python tools/dfine_loss_bench.py` (DESIGN.md
section 9)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("frame_b1_n3_one_output", 300, [3], False), ("batch_b16_n8_13_outputs", 300, [6, 7, 8, 9, 10, 8, 7, 9] * 2, True)]


def make_inputs(config, Q, sizes, full, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, C, nb1 = len(sizes), config.num_labels, config.max_num_bins + 1
    leaves = []

    def leaf(t):
        t = t.to(dev).requires_grad_(True)
        leaves.append(t)
        return t

    def boxes(*lead):
        return torch.cat([torch.rand(*lead, 2, generator=g) * 0.6 + 0.2, torch.rand(*lead, 2, generator=g) * 0.3 + 0.05], -1)

    def output(q, corners, teacher=None):
        out = {"logits": leaf(2 * torch.randn(B, q, C, generator=g)), "pred_boxes": leaf(boxes(B, q))}
        if corners:
            out.update(pred_corners=leaf(torch.randn(B, q, 4 * nb1, generator=g)), ref_points=boxes(B, q).to(dev),
                       teacher_corners=teacher[0], teacher_logits=teacher[1])
        return out

    targets = [{"class_labels": torch.randint(0, C, (n,), generator=g).to(dev), "boxes": boxes(n).to(dev)} for n in sizes]
    outputs = output(Q, False)
    if full:
        def teacher(q):
            return torch.randn(B, q, 4 * nb1, generator=g).to(dev), torch.randn(B, q, C, generator=g).to(dev)
        groups = config.num_denoising // max(sizes)
        q_dn = 2 * groups * max(sizes)
        t_main, t_dn = teacher(Q), teacher(q_dn)
        outputs["auxiliary_outputs"] = [output(Q, True, t_main) for _ in range(config.decoder_layers - 1)] + [output(Q, False)]
        outputs["dn_auxiliary_outputs"] = [output(q_dn, True, t_dn) for _ in range(config.decoder_layers)]
        positive = [torch.cat([torch.arange(n) + 2 * max(sizes) * k for k in range(groups)]).to(dev) for n in sizes]
        outputs["denoising_meta_values"] = {"dn_positive_idx": positive, "dn_num_group": groups}
    return outputs, targets, leaves


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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_loss_bench.json"))
    args = ap.parse_args()
    from transformers import DFineConfig
    from transformers.loss.loss_d_fine import DFineLoss
    from transformers.loss.loss_rt_detr import RTDetrHungarianMatcher, RTDetrLoss
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)
    config = DFineConfig()
    criterion = DFineLoss(config).to(dev)
    stock_forward = RTDetrLoss.forward
    RTDetrHungarianMatcher.forward = dfine.matcher_forward   # both arms
    result = {"device": torch.cuda.get_device_name(0), "calls_per_block": args.calls, "blocks": args.rounds,
              "unit": "us per criterion call, forward + backward (wall)", "shapes": {}}
    for name, Q, sizes, full in SHAPES:
        outputs, targets, leaves = make_inputs(config, Q, sizes, full, dev)
        last = {}

        def step(forward, key):
            for t in leaves:
                t.grad = None
            losses = forward(criterion, outputs, targets)
            total = sum(losses.values())
            total.backward()
            last[key] = (total.detach(), len(losses))

        variants = {"unbound": lambda: step(stock_forward, "unbound"), "bound": lambda: step(dfine.criterion_forward, "bound")}
        for fn in variants.values():
            block(fn, 3)
        calls0 = dict(dfine.loss_calls)
        variants["bound"]()
        kernel_calls = dfine.loss_calls["kernel"] - calls0["kernel"]
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(block(fn, args.calls))
        entry = {"B": len(sizes), "Q": Q, "targets_per_image": sizes, "outputs": 13 if full else 1, "loss_keys": last["bound"][1],
                 "detection_loss_kernel_calls_per_criterion_call": kernel_calls,
                 "total_loss_unbound": float(last["unbound"][0]), "total_loss_bound": float(last["bound"][0])}
        for k, fn in variants.items():
            entry[k] = {"median_us": round(statistics.median(times[k]), 1), "min_us": round(min(times[k]), 1),
                        "max_us": round(max(times[k]), 1), "device_activities_per_call": device_activities(fn)}
        entry["speedup_bound_vs_unbound"] = round(entry["unbound"]["median_us"] / entry["bound"]["median_us"], 2)
        entry["accepted"] = entry["bound"]["max_us"] < entry["unbound"]["min_us"]
        result["shapes"][name] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
