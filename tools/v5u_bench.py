"""Detection throughput and its per-launch split (DESIGN.md sections on YOLOv5u and on YOLOv8 detect; any detect scale tag: 5s, 8n, ...).
  python tools/v5u_bench.py [scale=5s] [batch=32] [imgsz=640] [steps=30] [out.json]
      images/s of forward + NMS (keep_raw off: the predict path), then the op table (HIP events per launch)
  python tools/v5u_bench.py --stem-only [batch=32] [imgsz=640] [C0=32] [reps=20]
      the stem kernel alone through m355_stem6_fwd (for a rocprofv3 --kernel-trace --stats run of its own)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from defectdetection_viaobjectdetection_amd import _capi  # noqa: E402
from defectdetection_viaobjectdetection_amd.engine import SegEngine  # noqa: E402
from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict  # noqa: E402


def stem_only(B, S, c0, reps):
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 255, (B, S, S, 3), dtype=np.uint8)).cuda()
    w = torch.rand((c0, 3, 6, 6)) * 0.1 - 0.05
    b = torch.zeros(c0)
    y = torch.empty((B, S // 2, S // 2, c0), dtype=torch.float16, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(reps):
        _capi.check(_capi.lib.m355_stem6_fwd(ctypes.c_void_p(x.data_ptr()), B, S, S, ctypes.c_void_p(w.data_ptr()),
                                             ctypes.c_void_p(b.data_ptr()), c0, ctypes.c_void_p(y.data_ptr()), st))
    torch.cuda.synchronize()
    mb = (B * S * S * 3 + B * (S // 2) ** 2 * c0 * 2) / 1e6
    print(f"stem6 B={B} {S}x{S} C0={c0}: {reps} launches, {mb:.0f} MB each (read + write)")


def main(argv):
    if argv and argv[0] == "--stem-only":
        a = [int(v) for v in argv[1:]] + [32, 640, 32, 20][len(argv) - 1:]
        return stem_only(*a[:4])
    scale = argv[0] if len(argv) > 0 else "5s"
    B = int(argv[1]) if len(argv) > 1 else 32
    S = int(argv[2]) if len(argv) > 2 else 640
    steps = int(argv[3]) if len(argv) > 3 else 30
    out = argv[4] if len(argv) > 4 else None
    eng = SegEngine(scale, 1, (S, S), max_batch=B, keep_raw=False)
    eng.load_state_dict(synthetic_state_dict(scale, 1, seed=0))
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 255, (B, S, S, 3), dtype=np.uint8)).cuda()
    for _ in range(5):
        p, _ = eng.forward(x)
        eng.postprocess(p, None, 0.25, 0.7, 300)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        p, _ = eng.forward(x)
        eng.postprocess(p, None, 0.25, 0.7, 300)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    ips = B / dt
    print(f"{'yolov5' + scale[1] + 'u' if scale[0] == '5' else 'yolov8' + scale[1] if scale[0] == '8' else scale} b={B} {S}x{S}: {dt * 1e3:.3f} ms per batch (forward + NMS), {ips:.0f} images/s, "
          f"{eng.flops_per_image / 1e9:.2f} GFLOP per image")
    eng.set_profiling(True)
    for _ in range(10):
        eng.forward(x)
    torch.cuda.synchronize()
    ms, cnt = eng.collect_op_times()
    rows, tot = [], 0.0
    for oi, m, c in zip(eng.op_infos(), ms, cnt):
        if c == 0:
            continue
        us = m / c * 1e3
        tot += us
        rows.append(dict(kernel=oi["kernel"], layer=oi["layer"], us=round(us, 2),
                         tflops=round(oi["flops"] * B / (us * 1e-6) / 1e12, 2), gbs=round(oi["bytes"] * B / (us * 1e-6) / 1e9, 1)))
        print(f"{oi['kernel'][:34]:34s} {oi['layer'][:40]:40s} {us:8.1f} us {rows[-1]['tflops']:7.1f} TF/s {rows[-1]['gbs']:7.0f} GB/s")
    print(f"op table total {tot:.1f} us over {len(rows)} launches")
    if out:
        with open(out, "w") as f:
            json.dump(dict(scale=scale, batch=B, imgsz=S, ms_per_batch=dt * 1e3, images_per_s=ips, op_table_us=tot,
                           launches=len(rows), ops=rows), f, indent=1)
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1:])
