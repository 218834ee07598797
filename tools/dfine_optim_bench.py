"""Times the end of the D-FINE trainers' step, gradient clipping + Adam / AdamW, in four arms on the same parameters and gradients:

    torch          torch.nn.utils.clip_grad_norm_(params, 1.0) + optimizer.step()   (what the trainers run: the comparator)
    torch_fused    the same with fused=True
    bound          dfine.clip_grad_norm_(params, 1.0) + the step of dfine.bind_optimizer(optimizer)
    bound_clip     the step of dfine.bind_optimizer(optimizer, max_norm=1.0) alone, the clip folded into the update

    python tools/dfine_optim_bench.py [--calls 20] [--rounds 7] [--out profiles/dfine_optim_bench.json]

The method of the other D-FINE tools: same process, alternating blocks, wall time around each block with a synchronise at its end,
median (min - max) of the blocks' per-call times; `device_activities_per_call` counts the kernels and copies of one call under
torch.profiler.  Points: (a) the improved trainer's set, the non-backbone parameters of DFineForObjectDetection(DFineConfig()) plus
its temporal encoder, attention and anomaly heads, context GRU and projector, in three groups, AdamW(weight_decay=0.01);
(b) the temporal encoder alone, Adam(lr=1e-5).  The gradients are random and stay in place between calls (every arm gets its own
copy; the arms that scale .grad in place see it shrink to the clip norm after the first call, which changes no timing: every
pass of every arm runs whatever the coefficient is).
Also recorded per point: the time of the bound arms' kernels from HIP events around the launches alone (tables uploaded before),
a plain fill of the same number of bytes as the update moves (28 B per element) in the same run as the bandwidth yardstick, and
the host time the bound step spends before its first launch (collecting pointers and building the table)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def event_block(fn, calls):
    """us per call between two events on the current stream"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls * 1e3


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def summary(values, digits=1):
    return {"median_us": round(statistics.median(values), digits), "min_us": round(min(values), digits), "max_us": round(max(values), digits)}


def temporal_modules(d_model=256, num_defect_classes=4):
    """the modules the improved trainer adds to the detector (the names decide its parameter groups)"""
    nn = torch.nn
    m = nn.Module()
    layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=8, dim_feedforward=1024, dropout=0.1, batch_first=True)
    m.temporal_encoder = nn.TransformerEncoder(layer, num_layers=4)
    m.temporal_attention = nn.Sequential(nn.Linear(d_model, 256), nn.ReLU(), nn.Linear(256, 1))
    m.anomaly_detector = nn.Sequential(nn.Linear(d_model, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
                                       nn.Linear(128, num_defect_classes))
    m.context_aggregator = nn.GRU(d_model, d_model, batch_first=True, bidirectional=True)
    m.context_projector = nn.Linear(d_model * 2, d_model)
    return m


def improved_trainer_groups(dev):
    from transformers import DFineConfig, DFineForObjectDetection
    model = torch.nn.Module()
    model.dfine = DFineForObjectDetection(DFineConfig())
    for n, p in temporal_modules().named_parameters():
        model.register_parameter(n.replace(".", "_"), p)
    model.to(dev)
    groups = {"backbone": [], "temporal": [], "classifier": []}
    for name, p in model.named_parameters():
        if "dfine.model.backbone" in name:
            continue                                   # frozen in the trainer
        if "temporal" in name or "anomaly" in name or "context" in name:
            groups["temporal"].append(p)
        elif "class" in name:
            groups["classifier"].append(p)
        else:
            groups["backbone"].append(p)
    lrs = {"backbone": 1e-5, "temporal": 5e-4, "classifier": 1e-4}
    return [dict(params=ps, lr=lrs[k]) for k, ps in groups.items()], lambda gs, **kw: torch.optim.AdamW(gs, weight_decay=0.01, **kw)


def temporal_encoder_groups(dev):
    enc = temporal_modules().temporal_encoder.to(dev)
    return [dict(params=list(enc.parameters()))], lambda gs, **kw: torch.optim.Adam(gs, lr=1e-5, **kw)


def clone_groups(groups, grads):
    """fresh leaves with the same values, and their own copy of the gradients"""
    out = []
    for g in groups:
        ps = [torch.nn.Parameter(p.detach().clone()) for p in g["params"]]
        for p, q in zip(ps, g["params"]):
            p.grad = grads[q].clone()
        out.append({**g, "params": ps})
    return out


def measure(name, groups, make, dfine, args):
    torch.manual_seed(0)
    base = [p for g in groups for p in g["params"]]
    grads = {p: torch.randn_like(p) * 0.01 for p in base}
    arms, params = {}, {}
    for arm in ("torch", "torch_fused", "bound", "bound_clip"):
        gs = clone_groups(groups, grads)
        params[arm] = [p for g in gs for p in g["params"]]
        arms[arm] = make(gs, **({"fused": True} if arm == "torch_fused" else {}))
    dfine.bind_optimizer(arms["bound"])
    dfine.bind_optimizer(arms["bound_clip"], max_norm=1.0)
    assert "step" in vars(arms["bound"]) and "step" in vars(arms["bound_clip"])

    def torch_arm(arm):
        def fn():
            torch.nn.utils.clip_grad_norm_(params[arm], 1.0)
            arms[arm].step()
        return fn

    def bound_arm():
        dfine.clip_grad_norm_(params["bound"], 1.0)
        arms["bound"].step()

    variants = {"torch": torch_arm("torch"), "torch_fused": torch_arm("torch_fused"), "bound": bound_arm,
                "bound_clip": arms["bound_clip"].step}
    for fn in variants.values():
        block(fn, 3)
    calls0 = dict(dfine.optim_calls)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(block(fn, args.calls))
    assert dfine.optim_calls["torch"] == calls0["torch"], "a bound arm fell back to torch"
    numel = sum(p.numel() for p in base)
    entry = {"tensors": len(base), "elements": numel, "tensors_up_to_256_elements": sum(p.numel() <= 256 for p in base),
             "chunks": sum(-(-p.numel() // dfine.OPTIM_CHUNK) for p in base),
             "update_bytes": 28 * numel, "norm_bytes": 4 * numel}
    for k, fn in variants.items():
        entry[k] = {**summary(times[k]), "device_activities_per_call": device_activities(fn)}
    for k in ("torch_fused", "bound", "bound_clip"):
        entry[f"speedup_{k}_vs_torch"] = round(entry["torch"]["median_us"] / entry[k]["median_us"], 2)

    # the kernels alone: the launches of one fused-clip step, replayed on a table that is already on the device
    from defectdetection_viaobjectdetection_amd._capi import lib
    bound = arms["bound_clip"]._m355_optim
    slot = bound.tables.slots[(bound.tables.turn - 1) % dfine.OPTIM_RING]
    n, chunks = len(base), entry["chunks"]
    h, d = dfine.C.c_void_p(slot[0].data_ptr()), dfine.C.c_void_p(slot[2].data_ptr())
    partials = bound.tables.partials
    norm = torch.empty((4,), dtype=torch.float32, device=partials.device)
    mode = 1 if arms["bound_clip"].param_groups[0].get("decoupled_weight_decay") else 0
    stream = dfine._stream()

    def sumsq():
        dfine.check(lib.m355_dfine_grad_sumsq_launch(h, d, n, dfine._ptr(partials), partials.numel(), stream))

    def adam_clip():
        dfine.check(lib.m355_dfine_adam_launch(h, d, n, mode, dfine._ptr(partials), partials.numel(), 1.0, dfine._ptr(norm), stream))

    def adam_plain():
        dfine.check(lib.m355_dfine_adam_launch(h, d, n, mode, None, 0, 0.0, None, stream))

    def clip_scale():
        dfine.check(lib.m355_dfine_clip_scale_launch(h, d, n, dfine._ptr(partials), partials.numel(), 1.0, dfine._ptr(norm), stream))

    fill = torch.empty((28 * numel,), dtype=torch.uint8, device=partials.device)
    kernels = {"grad_sumsq": sumsq, "norm_and_adam": adam_clip, "adam": adam_plain, "norm_and_clip_scale": clip_scale,
               "fill_of_update_bytes": lambda: fill.fill_(1)}
    for fn in kernels.values():
        event_block(fn, 3)
    ktimes = {k: [] for k in kernels}
    for _ in range(args.rounds):
        for k, fn in kernels.items():
            ktimes[k].append(event_block(fn, args.calls))
    entry["kernels_hip_events"] = {k: summary(v, 2) for k, v in ktimes.items()}
    ad = entry["kernels_hip_events"]["adam"]["median_us"]
    entry["adam_GBps"] = round(28 * numel / ad / 1e3, 1)
    entry["fill_GBps"] = round(28 * numel / entry["kernels_hip_events"]["fill_of_update_bytes"]["median_us"] / 1e3, 1)

    # the host side of one bound step up to its first launch: collecting the pointers and writing the table
    opt = arms["bound_clip"]
    host = []
    for _ in range(args.rounds * 3):
        t0 = time.perf_counter()
        with torch.no_grad():
            bound.collect(opt)
        host.append((time.perf_counter() - t0) * 1e6)
    entry["host_collect_us"] = summary(host)
    torch.cuda.synchronize()
    # no launch: the whole step against an empty queue minus its kernels bounds the rest of the host work
    entry["bound_clip_step_enqueue_us"] = summary([_enqueue_us(opt.step) for _ in range(args.rounds * 3)])
    return entry


def _enqueue_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    t = (time.perf_counter() - t0) * 1e6
    torch.cuda.synchronize()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_optim_bench.json"))
    args = ap.parse_args()
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "calls_per_block": args.calls, "blocks": args.rounds,
              "unit": "us per call: clip (max_norm 1.0) + step (wall, synchronise per block)", "chunk_elements": dfine.OPTIM_CHUNK,
              "points": {}}
    for name, build in (("improved_trainer_adamw_3_groups", improved_trainer_groups), ("temporal_encoder_adam", temporal_encoder_groups)):
        groups, make = build(dev)
        result["points"][name] = measure(name, groups, make, dfine, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
