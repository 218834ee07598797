"""Times dfine.select_queries (csrc/dfine_select.hip: two launches forward, one backward) against the torch expression of
DFineModel.forward's query selection (transformers 5.15.0 modeling_d_fine.py:1804-1828: max, topk, three gathers with repeated
int64 indices, sigmoid) on the same device, fp32.  The method of tools/dfine_decoder_bench.py: same process, alternating blocks,
HIP events around each block, median / min / max of the blocks' per-call times; `device_activities_per_call` counts the kernels
and copies of one call under torch.profiler.

    python tools/dfine_select_bench.py [--calls 40] [--rounds 7] [--out profiles/dfine_select_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/dfine_select_bench.py --loop
        (25 forward + backward calls at (50, 8400, C = 80, D = 256, K = 300), memory detached, and nothing else: the three kernels'
        times; profiles/dfine_select_bench_kernel_stats.csv is such a run's t_kernel_stats.csv, the library's kernels only)

* select: (B, 8400, C, D = 256, K = 300) for B = 50, 16, 1 and C = 2, 80: forward under no_grad, and forward + backward with the
  class and coordinate logits under autograd and the memory detached (what the model does) and with the memory under autograd too.
* model: DFineForObjectDetection(DFineConfig(dropout=0)).model(pixel_values) at 2 x 256 x 256, eval forward and training forward +
  backward, unbound against dfine.bind_model."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, D, K = 8400, 256, 300


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
    out["speedup_bound_vs_unbound"] = round(out["unbound"]["median_ms"] / out["bound"]["median_ms"], 3)
    return out


def torch_select(cl, co, mem):
    """upstream's expression: reference_points_unact, enc_topk_bboxes, enc_topk_logits, target"""
    _, ind = torch.topk(cl.max(-1).values, K, dim=1)
    ref = co.gather(dim=1, index=ind.unsqueeze(-1).repeat(1, 1, co.shape[-1]))
    return (ref, torch.sigmoid(ref), cl.gather(dim=1, index=ind.unsqueeze(-1).repeat(1, 1, cl.shape[-1])),
            mem.gather(dim=1, index=ind.unsqueeze(-1).repeat(1, 1, mem.shape[-1])))


def bench_select(dfine, dev, calls, rounds):
    res = {}
    for B in (50, 16, 1):
        for C in (2, 80):
            g = torch.Generator(device=dev).manual_seed(B + C)
            cl, co, mem = (torch.randn(B, S, n, device=dev, generator=g) for n in (C, 4, D))
            ups = [torch.randn(B, K, n, device=dev, generator=g) for n in (4, 4, C, D)]
            kernel_select = lambda a, b, c: dfine.select_queries(a, b, c, K)[1:]

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn(cl, co, mem)
                return run

            def fwd_bwd(fn, with_memory):
                leaves = [cl.clone().requires_grad_(), co.clone().requires_grad_(), mem.clone().requires_grad_(with_memory)]
                n = 4 if with_memory else 3

                def run():
                    for t in leaves:
                        t.grad = None
                    outs = fn(*leaves)
                    torch.autograd.backward(outs[:n], ups[:n])
                return run

            before = dict(dfine.model_calls)
            entry = {"forward_no_grad": compare({"unbound": no_grad(torch_select), "bound": no_grad(kernel_select)}, calls, rounds),
                     "forward_backward_logits": compare({"unbound": fwd_bwd(torch_select, False), "bound": fwd_bwd(kernel_select, False)},
                                                        calls, rounds),
                     "forward_backward_logits_and_memory": compare({"unbound": fwd_bwd(torch_select, True),
                                                                    "bound": fwd_bwd(kernel_select, True)}, calls, rounds)}
            assert dfine.model_calls["torch"] == before["torch"], "select_queries fell back to torch"
            res[f"B={B},S={S},C={C},D={D},K={K}"] = entry
    return res


def bench_model(dfine, dev, calls, rounds):
    from transformers import DFineConfig, DFineForObjectDetection
    torch.manual_seed(0)
    unbound = DFineForObjectDetection(DFineConfig(dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)).to(dev)
    arms = {"unbound": unbound, "bound": dfine.bind_model(copy.deepcopy(unbound))}
    x = torch.rand(2, 3, 256, 256, device=dev)

    def eval_forward(m):
        def run():
            with torch.no_grad():
                return m.eval().model(pixel_values=x)
        return run

    def train_step(m):
        def run():
            m.train().zero_grad(set_to_none=True)
            out = m.model(pixel_values=x)
            (out.last_hidden_state.square().mean() + out.intermediate_logits.square().mean() + out.enc_topk_logits.square().mean()
             + out.enc_topk_bboxes.square().mean()).backward()
        return run

    before = dict(dfine.model_calls)
    res = {"input": "2x3x256x256",
           "eval_forward_no_grad": compare({k: eval_forward(m) for k, m in arms.items()}, calls, rounds),
           "train_forward_backward": compare({k: train_step(m) for k, m in arms.items()}, calls, rounds)}
    assert dfine.model_calls["torch"] == before["torch"], "the bound model fell back to torch"
    return res


def loop(dfine, dev, calls=25):
    """the workload of a kernel-trace run: forward + backward as the model makes them, at the trainers' shape"""
    g = torch.Generator(device=dev).manual_seed(0)
    cl, co, mem = (torch.randn(50, S, n, device=dev, generator=g) for n in (80, 4, D))
    ups = [torch.randn(50, K, n, device=dev, generator=g) for n in (4, 4, 80)]
    cl.requires_grad_()
    co.requires_grad_()
    for _ in range(calls):
        cl.grad = co.grad = None
        torch.autograd.backward(dfine.select_queries(cl, co, mem, K)[1:4], ups)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", action="store_true", help="run the kernel-trace workload and exit")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--model-calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_select_bench.json"))
    args = ap.parse_args()
    import transformers
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)   # no GPU: this fails, there is nothing to measure
    if args.loop:
        return loop(dfine, dev)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "transformers": transformers.__version__,
              "dtype": "float32", "blocks": args.rounds, "calls_per_block": {"select": args.calls, "model": args.model_calls},
              "unit": "ms per call (HIP events)"}
    result["select"] = bench_select(dfine, dev, args.calls, args.rounds)
    result["model"] = bench_model(dfine, dev, args.model_calls, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
