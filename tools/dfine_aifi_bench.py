"""Times the AIFI layer of the hybrid encoder (dfine.bind_aifi), the map / token layout ops and the GELU of csrc/dfine_layout.hip and
the memory assembly of dfine.bind_model against the torch lines they replace on the same device, fp32.  The method of
tools/dfine_temporal_bench.py: same process, alternating blocks, HIP events around each block, median / min / max of the blocks'
per-call times; `device_activities_per_call` counts the kernels and copies of one call under torch.profiler.

    python tools/dfine_aifi_bench.py [--calls 20] [--rounds 7] [--out profiles/dfine_aifi_bench.json]

Points: the AIFI layer at (50, 256, 20, 20) and (1, 256, 20, 20), eval forward and training forward + backward, for the unbound
transformers module, bind_aifi(attention=False) and bind_aifi(attention=True); maps_to_tokens with the generated valid_mask at
(50, 256, [80 x 80, 40 x 40, 20 x 20]) against torch.cat + valid_mask * source_flatten; gelu at (20000, 1024) against F.gelu; the layout
kernels against a plain clone() of the same bytes in the same run (the floor of a copy); model.model(pixel_values) at 2 x 256 x 256 with
the assembly on and off and the AIFI layer bound and unbound."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS = [(80, 80), (40, 40), (20, 20)]


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


def compare(variants, calls, rounds, base="torch"):
    for fn in variants.values():
        block(fn, 2)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(block(fn, calls))
    out = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
               "device_activities_per_call": device_activities(variants[k])} for k, v in times.items()}
    for k in variants:
        if k != base:
            out[f"speedup_{k}_vs_{base}"] = round(out[base]["median_ms"] / out[k]["median_ms"], 3)
    return out


def runners(fn, leaves, params, dev):
    """fn(*leaves) -> a tensor or a tuple (None entries allowed): the no_grad call and the forward + backward call"""
    def no_grad():
        with torch.no_grad():
            return fn(*leaves)

    ts = [t.clone().requires_grad_() for t in leaves]
    flat = lambda o: [t for t in (o if isinstance(o, (tuple, list)) else (o,)) if t is not None]   # noqa: E731
    g = torch.Generator(device=dev).manual_seed(1)
    ups = [torch.randn(o.shape, device=dev, generator=g) for o in flat(fn(*ts))]

    def fwd_bwd():
        for t in ts + params:
            t.grad = None
        torch.autograd.backward(flat(fn(*ts)), ups)
    return no_grad, fwd_bwd


def bench_aifi(dfine, dev, calls, rounds):
    from transformers import DFineConfig
    from transformers.models.d_fine import modeling_d_fine as M
    torch.manual_seed(0)
    layer = M.DFineAIFILayer(DFineConfig()).to(dev)   # 256 channels, 8 heads, ffn 1024, GELU, dropout 0
    arms = {"torch": layer, "kernel": dfine.bind_aifi(copy.deepcopy(layer), attention=False),
            "kernel_attention": dfine.bind_aifi(copy.deepcopy(layer), attention=True)}
    res = {}
    for B in (50, 1):
        x = torch.randn(B, 256, 20, 20, device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        fwd, step = {}, {}
        for name, m in arms.items():
            fwd[name] = runners(m.eval(), [x], [], dev)[0]
        entry = {"eval_forward": compare(fwd, calls, rounds)}
        for name, m in arms.items():
            step[name] = runners(m.train(), [x], list(m.parameters()), dev)[1]
        before = dict(dfine.aifi_calls)
        entry["train_forward_backward"] = compare(step, calls, rounds)
        assert dfine.aifi_calls["torch"] == before["torch"], "a bound layer fell back to torch"
        res[f"B={B},D=256,20x20"] = entry
    return res


def bench_layout(dfine, dev, calls, rounds):
    from transformers.models.d_fine import modeling_d_fine as M
    B, D = 50, 256
    g = torch.Generator(device=dev).manual_seed(2)
    maps = [torch.randn(B, D, h, w, device=dev, generator=g) for h, w in LEVELS]
    valid_mask = M.DFineModel._cached_generate_anchors(tuple(LEVELS), 0.05, dev, torch.float32)[1]
    assert not bool(valid_mask.all())

    def torch_assembly(*ms):
        source_flatten = torch.cat([m.flatten(2).transpose(1, 2) for m in ms], 1)
        return source_flatten, valid_mask.to(source_flatten.dtype) * source_flatten

    def torch_tokens(*ms):
        return torch.cat([m.flatten(2).transpose(1, 2) for m in ms], 1)

    kernel_assembly = lambda *ms: dfine.maps_to_tokens(list(ms), mask=valid_mask)   # noqa: E731
    kernel_tokens = lambda *ms: dfine.maps_to_tokens(list(ms))[0]                   # noqa: E731
    res = {}
    for name, kfn, tfn in (("maps_to_tokens_mask", kernel_assembly, torch_assembly), ("maps_to_tokens_plain", kernel_tokens, torch_tokens)):
        k_ng, k_fb = runners(kfn, maps, [], dev)
        t_ng, t_fb = runners(tfn, maps, [], dev)
        res[name] = {"forward_no_grad": compare({"torch": t_ng, "kernel": k_ng}, calls, rounds),
                     "forward_backward": compare({"torch": t_fb, "kernel": k_fb}, calls, rounds)}
    # the floor: a plain copy of the same bytes in the same run
    tokens = kernel_tokens(*maps)
    shapes = [(h, w) for h, w in LEVELS]
    floor = {"clone": lambda: tokens.clone(), "maps_to_tokens": lambda: kernel_tokens(*maps),
             "tokens_to_maps": lambda: dfine.tokens_to_maps(tokens, shapes)}
    with torch.no_grad():
        res["against_clone_of_the_same_bytes"] = compare(floor, calls, rounds, base="clone")
    x = torch.randn(50, 256, 20, 20, device=dev, generator=g)
    t1 = dfine.maps_to_tokens([x])[0]
    floor1 = {"clone": lambda: t1.clone(), "maps_to_tokens": lambda: dfine.maps_to_tokens([x])[0],
              "tokens_to_maps": lambda: dfine.tokens_to_maps(t1, [(20, 20)])}
    with torch.no_grad():
        res["against_clone_of_the_same_bytes_50x256x20x20"] = compare(floor1, calls, rounds, base="clone")
    res["bytes_read_or_written_each_way"] = {"three_levels": tokens.numel() * 4, "20x20": t1.numel() * 4}
    return {f"B={B},D={D},levels=80x80+40x40+20x20": res}


def bench_gelu(dfine, dev, calls, rounds):
    h = 3 * torch.randn(20000, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    k_ng, k_fb = runners(dfine.gelu, [h], [], dev)
    t_ng, t_fb = runners(F.gelu, [h], [], dev)
    return {"20000x1024": {"forward_no_grad": compare({"torch": t_ng, "kernel": k_ng}, calls, rounds),
                           "forward_backward": compare({"torch": t_fb, "kernel": k_fb}, calls, rounds)}}


def bench_model(dfine, dev, calls, rounds):
    from transformers import DFineConfig, DFineForObjectDetection
    torch.manual_seed(0)
    model = DFineForObjectDetection(DFineConfig(dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)).to(dev)
    x = torch.randn(2, 3, 256, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    arms = {"torch": dfine.bind_model(copy.deepcopy(model), assembly=False),
            "assembly": dfine.bind_model(copy.deepcopy(model), assembly=True),
            "aifi": dfine.bind_aifi(dfine.bind_model(copy.deepcopy(model), assembly=False)),
            "assembly_aifi": dfine.bind_aifi(dfine.bind_model(copy.deepcopy(model), assembly=True))}

    def forward(m):
        def run():
            with torch.no_grad():
                return m.model(pixel_values=x)
        return run

    def step(m):
        params = [p for p in m.parameters() if p.requires_grad]

        def run():
            for p in params:
                p.grad = None
            m.model(pixel_values=x).last_hidden_state.square().mean().backward()
        return run

    res = {"note": "2 x 256 x 256: widths 32, 16, 8 give a valid_mask of ones, so the assembly writes no second output here"}
    for m in arms.values():
        m.eval()
    res["eval_forward"] = compare({k: forward(m) for k, m in arms.items()}, calls, rounds)
    for m in arms.values():
        m.train()
    res["train_forward_backward"] = compare({k: step(m) for k, m in arms.items()}, calls, rounds)
    return {"2x3x256x256": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_aifi_bench.json"))
    args = ap.parse_args()
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)   # no GPU: this fails, there is nothing to measure
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "float32", "blocks": args.rounds,
              "calls_per_block": args.calls, "unit": "ms per call (HIP events)"}
    result["aifi_layer"] = bench_aifi(dfine, dev, args.calls, args.rounds)
    result["layout"] = bench_layout(dfine, dev, args.calls, args.rounds)
    result["gelu"] = bench_gelu(dfine, dev, args.calls, args.rounds)
    result["model"] = bench_model(dfine, dev, max(args.calls // 4, 3), args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
