"""Native-resolution masks (predict(retina_masks=True)): kernel time and predict throughput.
  python tools/retina_bench.py [out.json]
      (a) b32 of 320 x 320 originals at net 320, (b) b32 of 1920 x 1080 originals at the 640 x 384 rect net, ~20 detections
      per image: m355_proto_masks_native timed by device events, mask bytes written, bytes / time against the 6.29 TB/s
      copy bandwidth, and the device-to-host copy of the masks on its own; then predict() images/s with retina_masks on and
      off for (a)
  python tools/retina_bench.py --kernels [reps=20]
      the kernel alone on (a) and (b) -- for a rocprofv3 --kernel-trace --stats run of its own"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from defectdetection_viaobjectdetection_amd import _capi  # noqa: E402

COPY_BW = 6.29e12      # measured device copy bandwidth, bytes / s
CASES = {"a_320_at_320": ((80, 80), (320, 320)), "b_1920x1080_at_640x384": ((96, 160), (1080, 1920))}


def make_case(name, B=32, n=20, max_det=300, seed=0):
    """Device tensors of one case: dets (B,max_det,38) with fp32 coefficients, counts, fp16 protos, boxes in original
    pixels sized like real detections (5-35 % of each side), the host shape and offset tables and the output buffer."""
    (mh, mw), (h0, w0) = CASES[name]
    rng = np.random.default_rng(seed)
    dets = np.zeros((B, max_det, 38), np.float32)
    dets[:, :n, 6:] = rng.standard_normal((B, n, 32)) * 0.5
    wh = rng.uniform(0.05, 0.35, (B, n, 2)) * np.array([w0, h0])
    c = rng.uniform(0, 1, (B, n, 2)) * np.array([w0, h0])
    boxes = np.zeros((B, max_det, 4), np.float32)
    boxes[:, :n] = np.concatenate((c - wh / 2, c + wh / 2), -1).clip(0, [w0, h0, w0, h0])
    hw = np.tile(np.array([[h0, w0]], np.int32), (B, 1))
    off = np.arange(B + 1, dtype=np.int64) * n * h0 * w0
    dev = torch.device("cuda", 0)
    t = dict(dets=torch.from_numpy(dets).to(dev), counts=torch.full((B,), n, dtype=torch.int32, device=dev),
             protos=torch.from_numpy(rng.standard_normal((B, mh, mw, 32)).astype(np.float16)).to(dev),
             boxes=torch.from_numpy(boxes).to(dev), out=torch.empty((int(off[-1]),), dtype=torch.uint8, device=dev))
    return t, hw, off, (B, max_det, mh, mw)


def launch(t, hw, off, dims):
    B, max_det, mh, mw = dims
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib.m355_proto_masks_native(P(t["dets"]), P(t["counts"]), P(t["protos"]), B, max_det, mh, mw,
                                                  hw.ctypes.data_as(ctypes.c_void_p), P(t["boxes"]),
                                                  off.ctypes.data_as(ctypes.c_void_p), P(t["out"]), st))


def kernel_times(reps=50):
    out = {}
    for name in CASES:
        t, hw, off, dims = make_case(name)
        for _ in range(5):
            launch(t, hw, off, dims)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for _ in range(reps):
            ev[0].record()
            launch(t, hw, off, dims)
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        nbytes = int(off[-1])
        med = float(np.median(ms))
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        d2h = []
        for _ in range(5):
            ev[0].record()
            host.copy_(t["out"], non_blocking=True)
            ev[1].record()
            ev[1].synchronize()
            d2h.append(ev[0].elapsed_time(ev[1]))
        out[name] = dict(mask_bytes=nbytes, kernel_ms_median=med, kernel_ms_min=float(min(ms)),
                         tb_per_s=nbytes / med / 1e9, floor_ms=nbytes / COPY_BW * 1e3,
                         ratio_to_floor=med / (nbytes / COPY_BW * 1e3), d2h_pinned_ms_median=float(np.median(d2h)))
        print(f"{name}: {nbytes / 1e6:.1f} MB of masks, kernel {med * 1e3:.1f} us (min {min(ms) * 1e3:.1f}) = "
              f"{nbytes / med / 1e9:.2f} TB/s, floor {nbytes / COPY_BW * 1e6:.1f} us -> {out[name]['ratio_to_floor']:.2f}x; "
              f"D2H (pinned) {np.median(d2h):.2f} ms")
        del t
    return out


def predict_rate(steps=5):
    from ultralytics import YOLO
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    from defectdetection_viaobjectdetection_amd.synthetic import synthetic_bscans
    m = YOLO("yolov8n-seg.yaml")
    m.set_classes(1, {0: "defect"})
    m.load_state_dict(synthetic_state_dict("n", 1, seed=0, cls_bias=-2.0))
    imgs = [np.ascontiguousarray(a) for a in synthetic_bscans(32, 320, 320, seed=5)]
    out = {}
    for retina in (False, True, False, True):
        m.predict(imgs, imgsz=320, retina_masks=retina, verbose=False)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = m.predict(imgs, imgsz=320, retina_masks=retina, verbose=False)
        dt = time.perf_counter() - t0
        n = sum(len(r) for r in res) / len(res)
        key = "retina" if retina else "letterboxed"
        out.setdefault(key, []).append(steps * len(imgs) / dt)
        print(f"predict b32 320^2 retina_masks={retina}: {steps * len(imgs) / dt:.0f} images/s ({n:.1f} detections / image, "
              f"masks {tuple(res[0].masks.data.shape) if res[0].masks is not None else None})")
    return {k: max(v) for k, v in out.items()}


def main():
    torch.cuda.init()
    if "--kernels" in sys.argv:
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        for name in CASES:
            t, hw, off, dims = make_case(name)
            for _ in range(reps):
                launch(t, hw, off, dims)
            torch.cuda.synchronize()
            print(f"{name}: {reps} launches, {int(off[-1]) / 1e6:.1f} MB each")
        return
    res = {"kernel": kernel_times(), "predict_images_per_s_a": predict_rate()}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
