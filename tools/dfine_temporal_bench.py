"""Times the temporal-head ops of dfine (csrc/dfine_temporal.hip and the guarded decode: temporal_fuse, guard_logits,
decode_boxes(guard=True), noobject_loss, consistency_loss) and their composition temporal_head against the literal torch expressions
of the D-FINE trainers on the same device, fp32.  The method of tools/dfine_select_bench.py: same process, alternating blocks, HIP
events around each block, median / min / max of the blocks' per-call times; `device_activities_per_call` counts the kernels and
copies of one call under torch.profiler.

    python tools/dfine_temporal_bench.py [--calls 40] [--rounds 7] [--out profiles/dfine_temporal_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/dfine_temporal_bench.py --loop
        (25 forward + backward calls of every op at (50, 300, 256), C1 = 3, 33 bins, and nothing else: the kernels' times;
        profiles/dfine_temporal_bench_kernel_stats.csv is such a run's t_kernel_stats.csv, the library's kernels only)

Shapes: (T, Q, D) = (50, 300, 256) and (1, 300, 256), C1 = 3 classes (two defects + no object), 33 bins.  Each op forward under
no_grad, and forward + backward with every floating input under autograd."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q, D, C1, NB1, REG_SCALE = 300, 256, 3, 33, 4.0


def block(fn, calls):
    """ms per call between two events on the current stream"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def compare(variants, calls, rounds):
    for fn in variants.values():
        block(fn, 2)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(block(fn, calls))
    out = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
               "device_activities_per_call": device_activities(variants[k])} for k, v in times.items()}
    out["speedup_kernel_vs_torch"] = round(out["torch"]["median_ms"] / out["kernel"]["median_ms"], 3)
    return out


# ---- the trainers' expressions in torch ops ------------------------------------------------------------------------------------------
def torch_fuse(fused, scores, context):
    return fused * F.softmax(scores, dim=0) + context


def torch_guard(cls_logits, anomaly):
    cls_logits = torch.cat([cls_logits[:, :, :-1] + anomaly, cls_logits[:, :, -1:]], dim=-1).clamp(-20, 20)
    return torch.nan_to_num(cls_logits, nan=0.0, posinf=20.0, neginf=-20.0)


def torch_guard_plain(cls_logits):
    return torch.nan_to_num(cls_logits.clamp(-20, 20), nan=0.0, posinf=20.0, neginf=-20.0)


def torch_decode(project):
    def run(bbox_dist, init_ref):
        bbox_dist = torch.nan_to_num(bbox_dist, nan=0.0, posinf=1.0, neginf=0.0)
        p = F.softmax(bbox_dist.reshape(-1, NB1), dim=1)
        distances = F.linear(p, project.reshape(1, -1)).reshape(bbox_dist.shape[0], bbox_dist.shape[1], 4)
        distances = torch.nan_to_num(distances, nan=0.0, posinf=1.0, neginf=0.0)
        x0 = init_ref[..., 0] - (0.5 * REG_SCALE + distances[..., 0]) * (init_ref[..., 2] / REG_SCALE)
        y0 = init_ref[..., 1] - (0.5 * REG_SCALE + distances[..., 1]) * (init_ref[..., 3] / REG_SCALE)
        x1 = init_ref[..., 0] + (0.5 * REG_SCALE + distances[..., 2]) * (init_ref[..., 2] / REG_SCALE)
        y1 = init_ref[..., 1] + (0.5 * REG_SCALE + distances[..., 3]) * (init_ref[..., 3] / REG_SCALE)
        boxes = torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1).clamp(0, 1)
        return torch.nan_to_num(boxes, nan=0.5, posinf=1.0, neginf=0.0)
    return run


def torch_noobject(cls_logits):
    target = torch.full((cls_logits.shape[1],), cls_logits.shape[2] - 1, dtype=torch.long, device=cls_logits.device)
    return torch.stack([F.cross_entropy(cls_logits[t], target) for t in range(cls_logits.shape[0])])


def torch_consistency(a):
    if a.shape[0] == 1:
        return a.new_zeros(())
    loss = 0.0
    for t in range(1, a.shape[0]):
        loss = loss + F.mse_loss(a[t], a[t - 1])
    return loss / (a.shape[0] - 1)


class Heads(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.class_head, self.bbox_head, self.anomaly_detector = torch.nn.Linear(D, C1), torch.nn.Linear(D, 4 * NB1), torch.nn.Linear(D, C1 - 1)


def cases(dfine, dev, T):
    """name -> (kernel fn, torch fn, inputs under autograd, other inputs): fn(*inputs, *others) -> a tensor or a tuple of tensors"""
    g = torch.Generator(device=dev).manual_seed(T)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    project = dfine.weighting_function(NB1 - 1, torch.tensor([0.5], device=dev), REG_SCALE).float()
    init_ref = 0.2 + 0.4 * torch.rand(T, Q, 4, device=dev, generator=g)
    heads = Heads().to(dev)
    kernel_decode = lambda c, r: dfine.decode_boxes(c, project, r, REG_SCALE, clamp01=True, guard=True)   # noqa: E731

    def kernel_head(f, s, c):
        return dfine.temporal_head(f, init_ref, heads.class_head, heads.bbox_head, project, REG_SCALE, scores=s, context=c,
                                   anomaly_head=heads.anomaly_detector)

    def torch_head(f, s, c):
        x = torch_fuse(f, s, c)
        anomaly = heads.anomaly_detector(x)
        return torch_guard(heads.class_head(x), anomaly), torch_decode(project)(heads.bbox_head(x), init_ref), anomaly

    res = {
        "temporal_fuse": (dfine.temporal_fuse, torch_fuse, [rn(T, Q, D), rn(T, Q, 1), rn(T, Q, D)], []),
        "guard_logits_anomaly": (dfine.guard_logits, torch_guard, [8 * rn(T, Q, C1), rn(T, Q, C1 - 1)], []),
        "guard_logits": (dfine.guard_logits, torch_guard_plain, [8 * rn(T, Q, C1)], []),
        "decode_boxes_guard": (kernel_decode, torch_decode(project), [2 * rn(T, Q, 4 * NB1), init_ref.clone()], []),
        "noobject_loss": (dfine.noobject_loss, torch_noobject, [8 * rn(T, Q, C1)], []),
        "consistency_loss": (dfine.consistency_loss, torch_consistency, [rn(T, Q, C1 - 1)], []),
        "temporal_head": (kernel_head, torch_head, [rn(T, Q, D), rn(T, Q, 1), rn(T, Q, D)], list(heads.parameters())),
    }
    if T == 1:
        del res["consistency_loss"]   # one frame: a constant zero on both sides, nothing to time
    return res


def runners(fn, leaves, params, dev):
    def no_grad():
        with torch.no_grad():
            return fn(*leaves)

    ts = [t.clone().requires_grad_() for t in leaves]
    outs = fn(*ts)
    outs = outs if isinstance(outs, tuple) else (outs,)
    g = torch.Generator(device=dev).manual_seed(1)
    ups = [torch.randn(o.shape, device=dev, generator=g) for o in outs]

    def fwd_bwd():
        for t in ts + params:
            t.grad = None
        o = fn(*ts)
        torch.autograd.backward(o if isinstance(o, tuple) else (o,), ups)
    return no_grad, fwd_bwd


def bench(dfine, dev, calls, rounds):
    res = {}
    for T in (50, 1):
        entry = {}
        for name, (kfn, tfn, leaves, params) in cases(dfine, dev, T).items():
            before = dict(dfine.temporal_calls)
            k_ng, k_fb = runners(kfn, leaves, params, dev)
            t_ng, t_fb = runners(tfn, leaves, params, dev)
            entry[name] = {"forward_no_grad": compare({"torch": t_ng, "kernel": k_ng}, calls, rounds),
                           "forward_backward": compare({"torch": t_fb, "kernel": k_fb}, calls, rounds)}
            assert dfine.temporal_calls["torch"] == before["torch"], f"{name} fell back to torch"
        res[f"T={T},Q={Q},D={D},C1={C1},bins+1={NB1}"] = entry
    return res


def loop(dfine, dev, calls=25):
    """the workload of a kernel-trace run: forward + backward of every op at the trainers' shape"""
    for name, (kfn, _, leaves, params) in cases(dfine, dev, 50).items():
        if name == "temporal_head":
            continue   # its kernels are the ops' own
        fwd_bwd = runners(kfn, leaves, params, dev)[1]
        for _ in range(calls):
            fwd_bwd()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", action="store_true", help="run the kernel-trace workload and exit")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_temporal_bench.json"))
    args = ap.parse_args()
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)   # no GPU: this fails, there is nothing to measure
    if args.loop:
        return loop(dfine, dev)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "float32", "blocks": args.rounds,
              "calls_per_block": args.calls, "unit": "ms per call (HIP events)"}
    result["temporal"] = bench(dfine, dev, args.calls, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
