"""Times the first stage of every D-FINE script: processor(images=frames, return_tensors="pt")["pixel_values"].to(device) with the
installed RTDetrImageProcessorPil (Pillow resize + numpy rescale per frame on the host, then an fp32 upload) against the same call
on a processor bound by `dfine.bind_processor` (one uint8 upload, two HIP launches).  Same process, alternating blocks, median /
min / max of the blocks' per-call wall times (each block ends synchronised).

    python tools/dfine_preprocess_bench.py [--calls 2] [--rounds 7] [--out profiles/dfine_preprocess_bench.json]

Points: a 50-frame sequence from sources of 480 x 700, 1080 x 1920 and 640 x 640 (no resize: the rescale alone), and one frame of
480 x 700; output 640 x 640.  The frames are PIL images, as the scripts pass them; `bound_ndarray_frames` is the bound processor on
the same frames as uint8 arrays, which leaves Pillow's unpacking of its 4-byte pixels out.  `device_activities_per_call` counts the
kernels and copies of one call under torch.profiler.  `kernels` is the device time of the two launches alone (torch.profiler,
median of 9 calls) beside a plain fill of the same output bytes measured in the same run: their ratio is the distance to the
write floor."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT_SIZE = (640, 640)


def make_frames(T, h, w, seed=0):
    """B-scan-like frames: smooth structure plus noise, so neighbouring bytes differ as in a decoded image"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    frames = []
    for t in range(T):
        base = 110 + 60 * np.sin(xx / 37.0 + t) * np.cos(yy / 23.0) + rng.normal(0, 12, (h, w))
        rgb = np.stack([base, base * 0.9 + 10, base * 0.8 + 25], axis=2)
        frames.append(Image.fromarray(np.clip(rgb, 0, 255).astype(np.uint8)))
    return frames


def block(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def device_time_us(fn, match, repeats=9):
    """median over `repeats` calls of the summed device time of the events whose name contains `match`"""
    fn()
    times = []
    for _ in range(repeats):
        times.append(sum(e.device_time for e in device_events(fn) if match in e.name))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_preprocess_bench.json"))
    args = ap.parse_args()
    import transformers
    from defectdetection_viaobjectdetection_amd import dfine
    cls = transformers.RTDetrImageProcessorPil
    dev = torch.device("cuda", 0)
    plain, bound = cls(), dfine.bind_processor(cls())
    result = {"device": torch.cuda.get_device_name(0), "processor": cls.__name__, "output": list(OUT_SIZE), "blocks": args.rounds,
              "unit": "ms per call (wall); kernels: us (device)", "points": {}}
    points = [("sequence_50_frames_480x700", 50, 480, 700, args.calls), ("sequence_50_frames_1080x1920", 50, 1080, 1920, args.calls),
              ("sequence_50_frames_640x640", 50, 640, 640, args.calls), ("frame_1_480x700", 1, 480, 700, 10 * args.calls)]
    for name, T, h, w, calls in points:
        frames = make_frames(T, h, w)
        arrays = [np.asarray(f) for f in frames]
        variants = {"unbound": lambda: plain(images=frames, return_tensors="pt")["pixel_values"].to(dev),
                    "bound": lambda: bound(images=frames, return_tensors="pt")["pixel_values"].to(dev),
                    "bound_ndarray_frames": lambda: bound(images=arrays, return_tensors="pt")["pixel_values"].to(dev)}
        want, got, got_nd = variants["unbound"](), variants["bound"](), variants["bound_ndarray_frames"]()
        same = bool(torch.equal(want, got) and torch.equal(want, got_nd))
        del want, got, got_nd
        for fn in variants.values():
            block(fn, 1)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(block(fn, calls))
        entry = {"T": T, "source": [h, w], "calls_per_block": calls, "bit_identical": same,
                 "upload_bytes": {"unbound": T * 3 * OUT_SIZE[0] * OUT_SIZE[1] * 4, "bound": T * 3 * h * w}}
        for k, fn in variants.items():
            entry[k] = {"median_ms": round(statistics.median(times[k]), 3), "min_ms": round(min(times[k]), 3),
                        "max_ms": round(max(times[k]), 3), "device_activities_per_call": len(device_events(fn))}
        entry["speedup_bound_vs_unbound"] = round(entry["unbound"]["median_ms"] / entry["bound"]["median_ms"], 2)
        entry["bound_slower"] = entry["bound"]["median_ms"] > entry["unbound"]["median_ms"]
        # the launches alone against the write floor: a fill of the same output bytes, same run
        filled = torch.empty((T, 3) + OUT_SIZE, dtype=torch.float32, device=dev)
        fill_us = device_time_us(lambda: filled.fill_(0.5), "")
        entry["kernels"] = {
            "horizontal_us": round(device_time_us(lambda: dfine.preprocess_images(arrays, OUT_SIZE), "dfine_pre_h_kernel"), 1),
            "vertical_us": round(device_time_us(lambda: dfine.preprocess_images(arrays, OUT_SIZE), "dfine_pre_v_kernel"), 1),
            "fill_same_bytes_us": round(fill_us, 1), "output_bytes": filled.numel() * 4}
        entry["kernels"]["both_over_fill"] = round((entry["kernels"]["horizontal_us"] + entry["kernels"]["vertical_us"]) / max(fill_us, 1e-9), 2)
        result["points"][name] = entry
        del filled
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
