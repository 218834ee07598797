"""The two augmentation gathers at the training shape (batch 64 of 640x640 over a 256-image cache): microseconds per call of
(a) m355_augment on the default plan, (b) m355_augment_ex with neutral parameters (the same plans), (c) m355_augment_ex with
every option on (two mosaic layers, rotation / shear / perspective, flipud, a full paste list of 32 hexagons per layer), each
beside its bytes-moved floor (3 B out plus at most 12 B in per pixel and layer, at HBM_GBS).  Times are device events round
alternating blocks of calls of the C entries on prebuilt tables; an _ex call includes its three small table copies.  Kernel
time proper: run under `rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/augment_bench.py` and read augment_kernel /
augment_ex_kernel.
Usage: timeout 300 python tools/augment_bench.py [batch] [imgsz] [calls per block] [json out] [train step ms]"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from defectdetection_viaobjectdetection_amd._capi import AUG_MAX_PASTE, check, lib  # noqa: E402
from defectdetection_viaobjectdetection_amd.augment import Augmenter  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 640
CALLS = int(sys.argv[3]) if len(sys.argv) > 3 else 50
OUT = sys.argv[4] if len(sys.argv) > 4 else None
HBM_GBS = 8000.0            # MI355X peak HBM bandwidth (data sheet), GB/s: the floor is bytes over this constant
# the training step the launch times are set against: a constant handed in, NOT measured by this tool.  Default: the 24 ms of
# tools/train_bench.py for YOLOv8s-seg at batch 64; pass the figure of the same box as 5th argument.
TRAIN_STEP_MS = float(sys.argv[5]) if len(sys.argv) > 5 else 24.0
N_CACHE = 256


class Cache:
    """What Augmenter needs of a SegDataset: images, imgsz, labels, a length."""
    def __init__(self, n, size, seed=0):
        rng = np.random.default_rng(seed)
        self.images = rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)
        self.imgsz = (size, size)
        self.labels = [[(0, _hexagon(rng.uniform(0.2, 0.8) * size, rng.uniform(0.2, 0.8) * size, 0.08 * size, 0.06 * size))
                        for _ in range(2)] for _ in range(n)]

    def __len__(self):
        return len(self.images)


def _hexagon(cx, cy, rx, ry):
    return np.array([(cx + rx * math.cos(t), cy + ry * math.sin(t)) for t in np.linspace(0, 2 * math.pi, 7)[:-1]])


def full_plans(aug, rng):
    """Everything on: the Augmenter's own random plans under all six options, every layer's paste list filled to the cap."""
    plans = aug.plan(list(range(B)), mosaic_on=True)
    for p in plans:
        for lay in (p, p["layer1"]):
            cw = 2 * S
            lay["paste"] = [_hexagon(rng.uniform(0.1, 0.9) * cw, rng.uniform(0.1, 0.9) * cw, 0.04 * cw, 0.03 * cw)
                            for _ in range(AUG_MAX_PASTE)]
    return plans


def old_entry(aug, plans):
    """A closure that calls m355_augment on prebuilt parameters (the host work of Augmenter.render is not timed)."""
    out = aug.render(plans)
    raw = out._keepalive
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: check(lib.m355_augment(C.c_void_p(aug.cache.data_ptr()), C.c_void_p(raw.data_ptr()), C.c_void_p(out.data_ptr()),
                                          B, S, S, st))


def ex_entry(aug, plans):
    """The same for m355_augment_ex: prebuilt host tables; the call copies them to the device and launches."""
    out = aug.render_ex(plans)
    arr, parr, varr = aug._host
    n_polys = sum(L.poly_count for p in arr for L in p.layer[:p.n_layers])
    work = aug._work
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = varr.ctypes.data_as(C.POINTER(C.c_float)) if len(varr) else None
    return lambda: check(lib.m355_augment_ex(C.c_void_p(aug.cache.data_ptr()), len(aug.ds), arr, parr if n_polys else None, n_polys,
                                             vp, len(varr), C.c_void_p(work.data_ptr()), work.numel(), C.c_void_p(out.data_ptr()),
                                             B, S, S, st))


def main():
    assert torch.cuda.is_available(), "augment_bench needs the GPU"
    dev = torch.device("cuda", 0)
    ds = Cache(N_CACHE, S)
    base = Augmenter(ds, dev, seed=0)
    full = Augmenter(ds, dev, seed=0, degrees=10.0, shear=2.0, perspective=0.0005, flipud=0.5, mixup=1.0, copy_paste=0.5)
    full.cache = base.cache
    default_plans = base.plan(list(range(B)), mosaic_on=True)
    all_on = full_plans(full, np.random.default_rng(1))
    assert all(p["layer1"] is not None and p["layer1"]["mosaic"] and p["mosaic"] for p in all_on)
    runs = {"m355_augment, default plan": (old_entry(base, default_plans), 1),
            "m355_augment_ex, neutral": (ex_entry(base, default_plans), 1),
            "m355_augment_ex, all options on": (ex_entry(full, all_on), 2)}
    for fn, _ in runs.values():                      # warm up every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for rep in range(5):                             # alternate the three, five blocks each
        for name, (fn, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    parent = float(np.median(samples["m355_augment, default plan"]))
    result = dict(train_step_ms_given=TRAIN_STEP_MS, batch=B, imgsz=S, cache_images=N_CACHE, calls_per_block=CALLS, blocks=5, hbm_gbs=HBM_GBS, rows=[])
    print(f"batch {B}, {S}x{S}, {CALLS} calls per block, 5 blocks each; floor = (3 + 12 * layers) B per pixel at {HBM_GBS:.0f} GB/s")
    for name, (_, layers) in runs.items():
        us = float(np.median(samples[name]))
        floor = B * S * S * (3 + 12 * layers) / (HBM_GBS * 1e9) * 1e6
        row = dict(name=name, us_per_call=round(us, 1), min_us=round(min(samples[name]), 1), max_us=round(max(samples[name]), 1),
                   floor_us=round(floor, 1), over_floor=round(us / floor, 2), vs_parent=round(us / parent, 2),
                   share_of_train_step=round(us / (TRAIN_STEP_MS * 1e3), 4))
        result["rows"].append(row)
        print(f"{name:34s} {us:8.1f} us/call (min {row['min_us']}, max {row['max_us']})  floor {floor:6.1f} us  x{row['over_floor']:.2f} of floor"
              f"  x{row['vs_parent']:.2f} of m355_augment  {100 * row['share_of_train_step']:.2f} % of a {TRAIN_STEP_MS:.1f} ms step (step time given, not measured here)")
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        json.dump(result, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
