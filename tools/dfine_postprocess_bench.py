"""Times the D-FINE inference tail: transformers' RTDetrImageProcessor.post_process_object_detection on device tensors (its
~15 torch launches and the three synchronising boolean-mask indexings per image) against the same call with
`post_process_object_detection = dfine.post_process_object_detection` bound (one HIP launch, one read-back of the counts).
Same process, alternating blocks, median / min / max of the blocks' per-call wall times (each block ends synchronised).

    python tools/dfine_postprocess_bench.py [--calls 50] [--rounds 7] [--out profiles/dfine_postprocess_bench.json]

Three points: (B 1, Q 300, C 3) the reference trainers' per-frame call; a 50-frame sequence, 50 unbound per-frame calls against
ONE dfine.post_process_detections call of B = 50 (a "call" is the whole sequence); (B 16, Q 300, C 80) one call each.
`device_activities_per_call` counts the kernels and copies of one call under torch.profiler.  The kernel's own time comes from
`rocprofv3 --kernel-trace --stats -- python tools/dfine_postprocess_bench.py`."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLD = 0.3
FRAME_SIZE = (480, 640)


def make_inputs(B, Q, C, dev, seed=0):
    """detector-like logits: most candidates far below the threshold, a few dozen above it"""
    g = torch.Generator().manual_seed(seed)
    logits = 2 * torch.randn(B, Q, C, generator=g) - 4
    boxes = torch.sigmoid(torch.randn(B, Q, 4, generator=g))
    boxes[..., 2:] = boxes[..., 2:] * 0.5 + 0.01
    return logits.to(dev), boxes.to(dev)


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


def same_results(want, got):
    """kept counts equal and, where no two kept scores of an image tie, labels equal and boxes bit-equal"""
    if len(want) != len(got):
        return False
    for w, g in zip(want, got):
        if w["scores"].shape != g["scores"].shape:
            return False
        if w["scores"].unique().numel() == w["scores"].numel() and not (torch.equal(w["labels"], g["labels"]) and torch.equal(w["boxes"], g["boxes"])):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_postprocess_bench.json"))
    args = ap.parse_args()
    import transformers
    from defectdetection_viaobjectdetection_amd import dfine
    cls = transformers.RTDetrImageProcessor   # the PIL-backed class where torchvision is absent: the method is the same
    stock = cls.post_process_object_detection
    processor = cls()
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "processor": cls.__name__, "threshold": THRESHOLD, "blocks": args.rounds,
              "unit": "us per call (wall)", "shapes": {}}

    def per_frame(method, wrap, logits, boxes):
        """the loop of the reference's temporal model (temporal_dfine.py:183-193)"""
        out = []
        for i in range(logits.shape[0]):
            out.append(method(processor, wrap({"logits": logits[i:i + 1], "pred_boxes": boxes[i:i + 1]}),
                              target_sizes=torch.tensor([FRAME_SIZE]), threshold=THRESHOLD)[0])
        return out

    ns = lambda d: types.SimpleNamespace(**d)   # upstream reads attributes
    points = []
    lg, bx = make_inputs(1, 300, 3, dev)
    points.append(("frame_b1_q300_c3", (1, 300, 3), args.calls, {
        "unbound": lambda lg=lg, bx=bx: per_frame(stock, ns, lg, bx),
        "bound": lambda lg=lg, bx=bx: per_frame(dfine.post_process_object_detection, dict, lg, bx)}))
    lg, bx = make_inputs(50, 300, 3, dev, seed=1)
    points.append(("sequence_50_frames_q300_c3", (50, 300, 3), max(args.calls // 10, 2), {
        "unbound": lambda lg=lg, bx=bx: per_frame(stock, ns, lg, bx),
        "bound": lambda lg=lg, bx=bx: dfine.post_process_detections(lg, bx, [FRAME_SIZE] * 50, THRESHOLD),
        "bound_per_frame_loop": lambda lg=lg, bx=bx: per_frame(dfine.post_process_object_detection, dict, lg, bx)}))
    lg, bx = make_inputs(16, 300, 80, dev, seed=2)
    sizes16 = [FRAME_SIZE] * 16
    points.append(("batch_b16_q300_c80", (16, 300, 80), args.calls, {
        "unbound": lambda lg=lg, bx=bx: stock(processor, ns({"logits": lg, "pred_boxes": bx}), target_sizes=sizes16, threshold=THRESHOLD),
        "bound": lambda lg=lg, bx=bx: dfine.post_process_object_detection(processor, {"logits": lg, "pred_boxes": bx},
                                                                        target_sizes=sizes16, threshold=THRESHOLD)}))
    for name, shape, calls, variants in points:
        same = same_results(variants["unbound"](), variants["bound"]())
        for fn in variants.values():
            block(fn, 3)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(block(fn, calls))
        entry = {"B": shape[0], "Q": shape[1], "C": shape[2], "calls_per_block": calls, "same_results": same}
        for k, fn in variants.items():
            entry[k] = {"median_us": round(statistics.median(times[k]), 1), "min_us": round(min(times[k]), 1),
                        "max_us": round(max(times[k]), 1), "device_activities_per_call": device_activities(fn)}
        entry["speedup_bound_vs_unbound"] = round(entry["unbound"]["median_us"] / entry["bound"]["median_us"], 2)
        entry["slowest_bound_block_faster_than_fastest_unbound_block"] = entry["bound"]["max_us"] < entry["unbound"]["min_us"]
        result["shapes"][name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
