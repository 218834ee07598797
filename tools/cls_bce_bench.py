"""The class-BCE kernel of the detection loss (m355_cls_bce_launch) against what it replaces: torch's BCE-with-logits over the class
columns of the raw rows + autograd back to the rows, as loss_core runs the class term.  Device events around alternating blocks of
launches; bytes from the shapes (logits read + targets read + gradient written) over the kernel's time against HBM bandwidth.
  python tools/cls_bce_bench.py [batch=64] [anchors=8400] [reps=30] [out.json]"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from defectdetection_viaobjectdetection_amd.loss import cls_bce_device  # noqa: E402

HBM_TBS = 8.0      # MI355X peak HBM bandwidth, TB/s


def torch_form(raw, t, denom, mul, nc):
    r = raw.detach().requires_grad_(True)
    logits_cls = r.split((64, nc), 2)[1]
    loss = F.binary_cross_entropy_with_logits(logits_cls, t, reduction="sum") / denom
    (loss * mul).backward()
    return loss, r.grad


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3      # us


def main(argv):
    B = int(argv[0]) if len(argv) > 0 else 64
    A = int(argv[1]) if len(argv) > 1 else 8400
    reps = int(argv[2]) if len(argv) > 2 else 30
    out = argv[3] if len(argv) > 3 else None
    dev = torch.device("cuda", 0)
    rows = []
    for nc in (1, 80):
        g = torch.Generator().manual_seed(nc)
        raw = (torch.randn((B, A, 64 + nc), generator=g) * 2 - 3).to(dev)
        t = torch.zeros(B * A * nc)
        k = max(1, t.numel() // 100)
        t[torch.randperm(t.numel(), generator=g)[:k]] = torch.rand(k, generator=g)
        t = t.view(B, A, nc).to(dev)
        denom = t.sum().clamp_min(1.0)
        mul = 0.5 * B * 128.0
        s = mul / denom
        d_raw = torch.zeros_like(raw)
        kern = lambda: cls_bce_device(raw, t, s, d_raw)            # noqa: E731
        base = lambda: torch_form(raw, t, denom, mul, nc)          # noqa: E731
        for _ in range(3):
            kern(); base()
        torch.cuda.synchronize()
        # same values first (the gradient of the torch form has zeros in the box columns, as d_raw here)
        l_t, g_t = base()
        l_k = kern() / denom
        torch.cuda.synchronize()
        err_l = abs(float(l_k) - float(l_t)) / abs(float(l_t))
        err_g = float((d_raw - g_t).abs().max())
        tk, tb = [], []
        for _ in range(5):                                          # alternating blocks: other work shares the machine
            tk.append(timed(kern, reps))
            tb.append(timed(base, reps))
        n = B * A * nc
        us_k, us_b = sorted(tk)[len(tk) // 2], sorted(tb)[len(tb) // 2]
        gbs = 3 * n * 4 / (us_k * 1e-6) / 1e9
        rows.append(dict(batch=B, anchors=A, nc=nc, elements=n, kernel_us=round(us_k, 1), kernel_us_all=[round(v, 1) for v in tk],
                         torch_us=round(us_b, 1), torch_us_all=[round(v, 1) for v in tb], bytes_moved=3 * n * 4, gb_per_s=round(gbs, 1),
                         share_of_hbm_peak=round(gbs / (HBM_TBS * 1e3), 3), loss_rel_diff=err_l, grad_max_abs_diff=err_g))
        print(f"cls_bce b{B} A{A} nc{nc}: kernel (2 launches) {us_k:.1f} us, torch BCE + autograd {us_b:.1f} us ({us_b / us_k:.2f}x); "
              f"{3 * n * 4 / 1e6:.1f} MB -> {gbs:.0f} GB/s = {gbs / (HBM_TBS * 1e3):.1%} of {HBM_TBS} TB/s; loss rel diff {err_l:.1e}, grad max diff {err_g:.1e}")
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
