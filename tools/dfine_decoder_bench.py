"""Times the D-FINE decoder path bound with dfine.bind_decoder (torch GEMMs + the kernels of csrc/dfine_decoder.hip,
csrc/dfine_encoder.hip and the fused deformable attention) against transformers' own modules on the same device, fp32.
The method of tools/dfine_gru_bench.py: same process, alternating blocks, HIP events around each block, median / min / max of the
blocks' per-call times; `device_activities_per_call` counts the kernels and copies of one call under torch.profiler.

    python tools/dfine_decoder_bench.py [--calls 5] [--rounds 7] [--out profiles/dfine_decoder_bench.json]

* ops: gate + LayerNorm, add + clamp + LayerNorm and the LQE statistics alone at M = 15 000 and 4 800 rows, forward and forward +
  backward, against the torch expressions of transformers' modules.
* layer: one DFineDecoderLayer (256 wide, 8 heads, 12 points, levels 32^2 + 16^2 + 8^2) at (50, 300, 256), (16, 300, 256) and
  (1, 300, 256): eval forward under no_grad and training forward + backward, unbound, bound with attention=True and with
  attention=False (the unbound layer and the attention=False arm run torch's scaled_dot_product_attention, as in a whole model).
* model: DFineForObjectDetection(DFineConfig(dropout=0)).model(pixel_values) at 2 x 256 x 256, eval forward and training forward +
  backward, unbound and bound with either setting."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAPS = [(32, 32), (16, 16), (8, 8)]


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
    for k in variants:
        if k != "unbound":
            out[f"speedup_{k}_vs_unbound"] = round(out["unbound"]["median_ms"] / out[k]["median_ms"], 3)
    return out


def fwd_bwd(fn, leaves):
    def run():
        for t in leaves:
            t.grad = None
        fn().square().mean().backward()
    return run


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def bench_ops(dfine, dev, calls, rounds):
    F = torch.nn.functional
    res = {}
    for M in (15000, 4800):
        D = 256
        x1, x2, g = (torch.randn(M, d, device=dev, requires_grad=True) for d in (D, D, 2 * D))
        w, b = torch.ones(D, device=dev, requires_grad=True), torch.zeros(D, device=dev, requires_grad=True)
        c = torch.randn(M, 4 * 33, device=dev, requires_grad=True)

        def gate_torch():
            g1, g2 = torch.sigmoid(g).chunk(2, dim=-1)
            return F.layer_norm(g1 * x1 + g2 * x2, (D,), w, b, 1e-5)

        def lqe_torch():
            top, _ = F.softmax(c.reshape(M, 4, 33), dim=-1).topk(4, dim=-1)
            return torch.cat([top, top.mean(dim=-1, keepdim=True)], dim=-1).reshape(M, 20)

        pairs = {
            "gate_layer_norm": (gate_torch, lambda: dfine.gate_layer_norm(x1, x2, g, w, b, 1e-5), [x1, x2, g, w, b]),
            "add_clamp_layer_norm": (lambda: F.layer_norm((x1 + x2).clamp(min=-65504, max=65504), (D,), w, b, 1e-5),
                                     lambda: dfine.add_layer_norm(x1, x2, w, b, 1e-5, clamp=dfine.DECODER_CLAMP), [x1, x2, w, b]),
            "lqe_statistics": (lqe_torch, lambda: dfine.lqe_statistics(c, 32, 4), [c]),
        }
        entry = {}
        for name, (t_fn, k_fn, leaves) in pairs.items():
            entry[name] = {"forward_no_grad": compare({"unbound": no_grad(t_fn), "bound": no_grad(k_fn)}, calls, rounds),
                           "forward_backward": compare({"unbound": fwd_bwd(t_fn, leaves), "bound": fwd_bwd(k_fn, leaves)}, calls, rounds)}
        res[f"M={M}"] = entry
    return res


def bench_layer(dfine, M, cfg, dev, calls, rounds):
    torch.manual_seed(0)
    cfg = copy.deepcopy(cfg)
    cfg._attn_implementation = "sdpa"   # what a whole model dispatches to; a layer built alone would fall to the eager attention
    unbound = M.DFineDecoderLayer(cfg).to(dev)
    arms = {"unbound": unbound, "bound_attention": dfine.bind_decoder(copy.deepcopy(unbound), attention=True),
            "bound_no_attention": dfine.bind_decoder(copy.deepcopy(unbound), attention=False)}
    S = sum(h * w for h, w in MAPS)
    res = {}
    for B in (50, 16, 1):
        x, pos, enc = (torch.randn(B, n, 256, device=dev) for n in (300, 300, S))
        rp = torch.rand(B, 300, 1, 4, device=dev) * torch.tensor([1.0, 1.0, 0.4, 0.4], device=dev) + 0.02
        kw = dict(position_embeddings=pos.clamp(-10, 10), reference_points=rp, spatial_shapes=torch.tensor(MAPS, device=dev),
                  spatial_shapes_list=MAPS, encoder_hidden_states=enc)
        xg = x.clone().requires_grad_()   # the layer below feeds a gradient in a real step
        before = dict(dfine.decoder_calls)
        entry = {"eval_forward_no_grad": compare({k: no_grad(lambda m=m: m.eval()(x, **kw)) for k, m in arms.items()}, calls, rounds),
                 "train_forward_backward": compare({k: fwd_bwd(lambda m=m: m.train()(xg, **kw), [xg] + list(m.parameters()))
                                                    for k, m in arms.items()}, calls, rounds)}
        assert dfine.decoder_calls["torch"] == before["torch"], "a bound layer fell back to torch"
        res[f"{B}x300x256"] = entry
    return res


def bench_model(dfine, cfg, dev, calls, rounds):
    from transformers import DFineForObjectDetection
    torch.manual_seed(0)
    unbound = DFineForObjectDetection(cfg).to(dev)
    arms = {"unbound": unbound, "bound_attention": dfine.bind_decoder(copy.deepcopy(unbound), attention=True),
            "bound_no_attention": dfine.bind_decoder(copy.deepcopy(unbound), attention=False)}
    x = torch.rand(2, 3, 256, 256, device=dev)

    def train_step(m):
        def run():
            m.train().zero_grad(set_to_none=True)
            out = m.model(pixel_values=x)
            (out.last_hidden_state.square().mean() + out.intermediate_logits.square().mean()).backward()
        return run

    before = dict(dfine.decoder_calls)
    res = {"input": "2x3x256x256",
           "eval_forward_no_grad": compare({k: no_grad(lambda m=m: m.eval().model(pixel_values=x)) for k, m in arms.items()}, calls,
                                           rounds),
           "train_forward_backward": compare({k: train_step(m) for k, m in arms.items()}, calls, rounds)}
    assert dfine.decoder_calls["torch"] == before["torch"], "the bound model fell back to torch"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_decoder_bench.json"))
    args = ap.parse_args()
    import transformers
    from transformers import DFineConfig
    from transformers.models.d_fine import modeling_d_fine as M
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)
    cfg = DFineConfig(dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "transformers": transformers.__version__,
              "dtype": "float32", "blocks": args.rounds, "calls_per_block": args.calls, "unit": "ms per call (HIP events)",
              "bind_decoder_default_attention": dfine.bind_decoder.__defaults__[0]}
    result["ops"] = bench_ops(dfine, dev, args.calls, args.rounds)
    result["layer"] = bench_layer(dfine, M, cfg, dev, args.calls, args.rounds)
    result["model"] = bench_model(dfine, cfg, dev, args.calls, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
