"""Times the temporal encoder of the D-FINE trainers, nn.TransformerEncoder(nn.TransformerEncoderLayer(256, 8, 1024, 0.1,
batch_first=True), 4) in fp32, bound (dfine.bind_encoder: torch GEMMs + the HIP ops of csrc/dfine_encoder.hip) against unbound
(torch's own module on the same device).  Same process, alternating blocks, HIP events around each block, median / min / max of
the blocks' per-call times.

    python tools/dfine_encoder_bench.py [--calls 10] [--rounds 7] [--out profiles/dfine_encoder_bench.json]

Shapes (50, 300, 256), the trainers' 50-frame sequence, and (1, 300, 256); per shape: the eval forward under no_grad and the
training forward + backward at p = 0.1 (and at p = 0, which separates the cost of the mask generator).  The two paths draw
different dropout masks (the bound path's stream is not torch's), so the training outputs are not compared here; the eval outputs
are.  `device_activities_per_call` counts the kernels and copies of one call under torch.profiler.  `ops` times the three HIP ops
alone at the larger shape, forward and forward + backward."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    out = {}
    for k, fn in variants.items():
        out[k] = {"median_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                  "max_ms": round(max(times[k]), 4), "device_activities_per_call": device_activities(fn)}
    return out


def make_encoder(p, dev):
    torch.manual_seed(0)
    layer = torch.nn.TransformerEncoderLayer(d_model=256, nhead=8, dim_feedforward=1024, dropout=p, batch_first=True)
    return torch.nn.TransformerEncoder(layer, num_layers=4).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_encoder_bench.json"))
    args = ap.parse_args()
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "layers": 4, "d_model": 256, "heads": 8,
              "dim_feedforward": 1024, "dtype": "float32", "blocks": args.rounds, "calls_per_block": args.calls,
              "unit": "ms per call (HIP events)", "shapes": {}}

    def train_step(enc, x):
        def fn():
            for p in enc.parameters():
                p.grad = None
            enc(x).square().mean().backward()
        return fn

    def eval_step(enc, x):
        def fn():
            with torch.no_grad():
                return enc(x)
        return fn

    for shape in ((50, 300, 256), (1, 300, 256)):
        x = torch.randn(shape, device=dev)
        entry = {}
        for p in (0.1, 0.0):
            unbound = make_encoder(p, dev)
            bound = dfine.bind_encoder(copy.deepcopy(unbound))
            if p == 0.1:
                unbound.eval()
                bound.eval()
                a, b = eval_step(bound, x)(), eval_step(unbound, x)()
                entry["eval_max_abs_difference"] = float((a - b).abs().max())
                entry["eval_forward_no_grad"] = compare({"unbound": eval_step(unbound, x), "bound": eval_step(bound, x)}, args.calls,
                                                        args.rounds)
            unbound.train()
            bound.train()
            before = dict(dfine.encoder_calls)
            key = f"train_forward_backward_p{p:g}"
            entry[key] = compare({"unbound": train_step(unbound, x), "bound": train_step(bound, x)}, args.calls, args.rounds)
            assert dfine.encoder_calls["torch"] == before["torch"], "the bound encoder fell back to torch"
        for key, val in entry.items():
            if isinstance(val, dict):
                val["speedup_bound_vs_unbound"] = round(val["unbound"]["median_ms"] / val["bound"]["median_ms"], 3)
        result["shapes"]["x".join(str(s) for s in shape)] = entry

    # the three ops alone at (50, 300, 256)
    B, S, D, H = 50, 300, 256, 8
    qkv = torch.randn(B, S, 3 * D, device=dev, requires_grad=True)
    xs, ys = torch.randn(B, S, D, device=dev, requires_grad=True), torch.randn(B, S, D, device=dev, requires_grad=True)
    w, bias = torch.ones(D, device=dev, requires_grad=True), torch.zeros(D, device=dev, requires_grad=True)
    hid = torch.randn(B, S, 1024, device=dev, requires_grad=True)
    go, gh = torch.randn(B, S, D, device=dev), torch.randn(B, S, 1024, device=dev)

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def fwd_bwd(fn, leaves, g):
        def run():
            torch.autograd.grad(fn(), leaves, g)
        return run

    ops = {}
    for p in (0.0, 0.1):
        tag = f"p{p:g}"
        attn = lambda p=p: dfine.self_attention(qkv, H, p, 1)
        ln = lambda p=p: dfine.add_layer_norm(xs, ys, w, bias, 1e-5, p, 1)
        relu = lambda p=p: dfine.relu_dropout(hid, p, 1)
        ops[f"self_attention_{tag}"] = compare({"forward": fwd(attn), "forward_backward": fwd_bwd(attn, [qkv], go)}, args.calls, args.rounds)
        ops[f"add_layer_norm_{tag}"] = compare({"forward": fwd(ln), "forward_backward": fwd_bwd(ln, [xs, ys, w, bias], go)}, args.calls,
                                               args.rounds)
        ops[f"relu_dropout_{tag}"] = compare({"forward": fwd(relu), "forward_backward": fwd_bwd(relu, [hid], gh)}, args.calls, args.rounds)
    F = torch.nn.functional

    def torch_attn(p):
        def fn():
            q, k, v = (t.reshape(B, S, H, 32).transpose(1, 2) for t in qkv.split(D, dim=-1))
            prob = F.dropout(torch.softmax(q @ k.transpose(-1, -2) / 32 ** 0.5, dim=-1), p, True)
            return (prob @ v).transpose(1, 2).reshape(B, S, D)
        return fn

    for p in (0.0, 0.1):
        ops[f"torch_attention_math_p{p:g}"] = compare({"forward": fwd(torch_attn(p)), "forward_backward": fwd_bwd(torch_attn(p), [qkv], go)},
                                                      args.calls, args.rounds)
    result["ops_50x300x256"] = ops
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
