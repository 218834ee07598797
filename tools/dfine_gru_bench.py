"""Times the context GRU of the improved temporal D-FINE trainer, nn.GRU(256, 256, batch_first=True, bidirectional=True) in fp32,
bound (dfine.bind_gru: one torch GEMM + the persistent recurrence kernels of csrc/dfine_gru.hip) against unbound (torch's own
module on the same device).  The method of tools/dfine_encoder_bench.py: same process, alternating blocks, HIP events around
each block, median / min / max of the blocks' per-call times; fewer calls per block, since one call is a chain of up to 15 000
serial steps.

    python tools/dfine_gru_bench.py [--calls 2] [--rounds 7] [--out profiles/dfine_gru_bench.json]

Points: (1, 15 000, 256), the trainer's 50 frames x 300 queries as one sequence, and (1, 300, 256); per point the eval forward
under no_grad and the training forward + backward.  The (1, 15 000) forward of both paths is also held to nn.GRU in float64 on the
CPU by the tests' parity rule, max |kernel - ref64| <= 2 max |torch fp32 - ref64| + 1e-6 max |ref64|; the tool writes its JSON
and then exits non-zero when that forward misses the rule or dfine.gru_status() is not 0."""
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


def compare(variants, calls, rounds):
    for fn in variants.values():
        block(fn, 1)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(block(fn, calls))
    out = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
           for k, v in times.items()}
    out["speedup_bound_vs_unbound"] = round(out["unbound"]["median_ms"] / out["bound"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfine_gru_bench.json"))
    args = ap.parse_args()
    from defectdetection_viaobjectdetection_amd import dfine
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    unbound = torch.nn.GRU(256, 256, batch_first=True, bidirectional=True).to(dev)
    bound = dfine.bind_gru(copy.deepcopy(unbound))
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "module": "GRU(256, 256, batch_first, bidirectional)",
              "dtype": "float32", "blocks": args.rounds, "calls_per_block": args.calls, "unit": "ms per call (HIP events)", "shapes": {}}

    def train_step(gru, x):
        def fn():
            for p in gru.parameters():
                p.grad = None
            gru(x)[0].square().mean().backward()
        return fn

    def eval_step(gru, x):
        def fn():
            with torch.no_grad():
                return gru(x)[0]
        return fn

    for shape in ((1, 15000, 256), (1, 300, 256)):
        x = torch.randn(shape, device=dev)
        entry = {}
        before = dict(dfine.gru_calls)
        if shape[1] == 15000:
            ref = copy.deepcopy(unbound).cpu().double()
            with torch.no_grad():
                want = ref(x.cpu().double())[0]
            e_k = float((eval_step(bound, x)().double().cpu() - want).abs().max())
            e_t = float((eval_step(unbound, x)().double().cpu() - want).abs().max())
            scale = float(want.abs().max())
            entry["forward_vs_float64"] = {"kernel_max_abs_error": e_k, "torch_fp32_max_abs_error": e_t, "max_abs_ref": scale,
                                           "within_parity_rule": bool(e_k <= 2 * e_t + 1e-6 * scale)}
        entry["eval_forward_no_grad"] = compare({"unbound": eval_step(unbound, x), "bound": eval_step(bound, x)}, args.calls, args.rounds)
        entry["train_forward_backward"] = compare({"unbound": train_step(unbound, x), "bound": train_step(bound, x)}, args.calls,
                                                  args.rounds)
        assert dfine.gru_calls["torch"] == before["torch"], "the bound GRU fell back to torch"
        result["shapes"]["x".join(str(s) for s in shape)] = entry
    result["gru_status"] = dfine.gru_status()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    parity = result["shapes"]["1x15000x256"]["forward_vs_float64"]
    if not parity["within_parity_rule"] or result["gru_status"]:
        sys.exit(f"FAILED: (1, 15000) forward outside the parity rule or a give-up bit set: {parity}, status {result['gru_status']}")


if __name__ == "__main__":
    main()
