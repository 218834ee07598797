"""dfine.select_queries on the GPU: the query selection of DFineModel.forward (row max, top-k, three gathers, sigmoid) in two
launches forward and one backward.

Indices and gathered rows are held exactly to what transformers' own DFineModel.forward recorded in
tests/golden/dfine_select_golden.npz (every case's top K + 1 scores pairwise distinct) and, where ties, non-finite scores or the
kernel's seams are the point, to the numpy restatement of tests/dfine_select_ref.py, whose order rule is the kernel's.  Boxes are
held to  max |kernel - float64| <= 2 * max |torch fp32 sigmoid on this device - float64| + 6e-8  (6e-8: one fp32 ulp below 1), the
bound of tests/test_dfine_postprocess_gpu.py.  The coordinate gradient is held to twice torch's fp32 error against float64; every
other gradient element is a copy or a zero and is held exactly."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import dfine_select_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ref.GOLDEN)
IDS = [ref.case_name(c) for c in ref.CASES]


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {ref.case_name(c): ref.load_case(z, c) for c in ref.CASES}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_box_bound(what, kernel_boxes, rows, want):
    """kernel sigmoid against float64, bounded by torch's own fp32 sigmoid of the same rows on the same device"""
    t = torch.sigmoid(rows).cpu().numpy().astype(np.float64)
    k = kernel_boxes.cpu().numpy().astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(k), nan), what
    err_kernel, err_torch = float(np.abs(k - want)[~nan].max(initial=0.0)), float(np.abs(t - want)[~nan].max(initial=0.0))
    print(f"{what}: box error vs float64: kernel {err_kernel:.3e}, torch fp32 {err_torch:.3e}")
    assert err_kernel <= 2 * err_torch + 6e-8, (what, err_kernel, err_torch)


def _assert_equals_restatement(what, dfine, cl, co, mem, K, expect_path="kernel"):
    before = dict(dfine.model_calls)
    out = dfine.select_queries(cl, co, mem, K)
    other = "torch" if expect_path == "kernel" else "kernel"
    assert dfine.model_calls[expect_path] == before[expect_path] + 1 and dfine.model_calls[other] == before[other], what
    B, S, C = cl.shape
    ind, rows, boxes, logits, target = ref.select(cl.cpu().numpy(), co.cpu().numpy(), None if mem is None else mem.cpu().numpy(), K)
    assert out.indices.dtype == torch.int64 and out.indices.shape == (B, K) and out.indices.is_cuda
    assert np.array_equal(out.indices.cpu().numpy(), ind), what
    assert out.reference_points_unact.shape == (B, K, 4) and out.boxes.shape == (B, K, 4) and out.logits.shape == (B, K, C)
    assert np.array_equal(_bits(out.reference_points_unact.cpu().numpy()), _bits(rows)), what
    assert np.array_equal(_bits(out.logits.cpu().numpy()), _bits(logits)), what
    if mem is None:
        assert out.target is None
    else:
        assert out.target.shape == (B, K, mem.shape[-1]) and np.array_equal(_bits(out.target.cpu().numpy()), _bits(target)), what
    _assert_box_bound(what, out.boxes, out.reference_points_unact, boxes)
    return out


def _random(seed, B, S, C, D, device):
    g = np.random.default_rng(seed)
    cl = torch.from_numpy(g.normal(size=(B, S, C)).astype(np.float32)).to(device)
    co = torch.from_numpy(g.normal(scale=3.0, size=(B, S, 4)).astype(np.float32)).to(device)
    mem = None if D is None else torch.from_numpy(g.normal(size=(B, S, D)).astype(np.float32)).to(device)
    return cl, co, mem


def _raw(cl, co, mem, K, inverse=True):
    """the C entry on outputs poisoned with NaN / -7"""
    from defectdetection_viaobjectdetection_amd import _capi
    B, S, C = cl.shape
    D = mem.shape[-1] if mem is not None else 0
    dev = cl.device
    work = torch.empty((B, S), device=dev)
    ind = torch.full((B, K), -7, dtype=torch.int64, device=dev)
    rows = torch.full((B, K, 4), float("nan"), device=dev)
    boxes = torch.full((B, K, 4), float("nan"), device=dev)
    logits = torch.full((B, K, C), float("nan"), device=dev)
    target = torch.full((B, K, D), float("nan"), device=dev) if mem is not None else None
    inv = torch.full((B, S), -7, dtype=torch.int32, device=dev) if inverse else None
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = _capi.lib.m355_dfine_select_forward(ptr(cl), ptr(co), ptr(mem), B, S, C, D, K, ptr(work), work.numel() * 4, ptr(ind), ptr(rows),
                                             ptr(boxes), ptr(logits), ptr(target), ptr(inv),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _capi.lib.m355_last_error(None)
    torch.cuda.synchronize()
    return [t for t in (ind, rows, boxes, logits, target, inv) if t is not None]


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_golden_cases(cuda_device, golden, case):
    from defectdetection_viaobjectdetection_amd import dfine
    B, levels, C, K = case
    g = golden[ref.case_name(case)]
    cl, co = torch.from_numpy(g["enc_outputs_class"]).to(cuda_device), torch.from_numpy(g["enc_outputs_coord_logits"]).to(cuda_device)
    out = _assert_equals_restatement(ref.case_name(case), dfine, cl, co, None, K)
    assert np.array_equal(out.indices.cpu().numpy(), g["indices"])
    assert np.array_equal(_bits(out.reference_points_unact.cpu().numpy()), _bits(g["init_reference_points"]))
    assert np.array_equal(_bits(out.logits.cpu().numpy()), _bits(g["enc_topk_logits"]))
    want = 1.0 / (1.0 + np.exp(-g["init_reference_points"].astype(np.float64)))
    _assert_box_bound(ref.case_name(case) + " (golden rows)", out.boxes, torch.from_numpy(g["init_reference_points"]).to(cuda_device), want)


# (B, S, K, C, D): S around the wave (64), the sort's capacity (2048: at most that many go to the sort directly, more go through
# the radix select) and two unrolled passes of the block (4096); K = 1, 2, S, the model's 300 and the limit 2048; C with and
# without 16-byte rows (1, 3, 5, 81 against 4, 80); D likewise; with and without a memory
EDGES = [(1, 1, 1, 1, 1), (3, 63, 2, 3, 36), (1, 64, 64, 4, 256), (3, 65, 65, 5, 1), (1, 2048, 300, 80, 36), (3, 2048, 2048, 81, 1),
         (1, 2049, 2048, 4, 256), (3, 2049, 1, 1, 36), (1, 2049, 2, 80, 256), (1, 4097, 300, 5, 256), (3, 4097, 2048, 3, None)]


@pytest.mark.parametrize("shape", EDGES, ids=["b%d_s%d_k%d_c%d_d%s" % s for s in EDGES])
def test_edge_shapes(cuda_device, shape):
    from defectdetection_viaobjectdetection_amd import dfine
    B, S, K, C, D = shape
    cl, co, mem = _random(sum(v or 0 for v in shape), B, S, C, D, cuda_device)
    _assert_equals_restatement(str(shape), dfine, cl, co, mem, K)


def _straddle_ties(S):
    return [S - 1, 63, 64, S // 2, 5, 128, S - 2, 191, 192, 65, 0, S // 2 + 1]


def _tie_scores(kind, S):
    g = np.random.default_rng(7)
    if kind == "all_equal":
        return np.full((2, S), 0.25, np.float32)
    if kind == "straddle":                 # two clear winners, then twelve equal tokens across the block for seven places (K = 9)
        x = np.full((1, S), -2.0, np.float32)
        x[0, [S - 3, 7]] = [3.0, 2.5]
        x[0, _straddle_ties(S)] = 1.0
        return x
    if kind == "signed_zeros":             # -0 ties with +0
        x = np.where(g.uniform(size=(2, S)) < 0.5, -0.0, 0.0).astype(np.float32)
        x[:, ::7] = -1.0
        return x
    if kind == "two_values":               # the two scores a randomly initialised model produces, repeated in blocks
        x = np.where((np.arange(S) // 37) % 2 == 0, 0.0123, 0.0119).astype(np.float32)
        return np.stack([x, x[::-1].copy()])
    raise KeyError(kind)


TIES = [(k, S) for k in ("all_equal", "straddle", "signed_zeros", "two_values") for S in (300, 2500)]


@pytest.mark.parametrize("kind,S", TIES, ids=[f"{k}-s{S}" for k, S in TIES])
def test_exact_ties(cuda_device, kind, S):
    """an exact tie goes to the lowest token: sorted directly (S = 300) and through the radix selection (S = 2500)"""
    from defectdetection_viaobjectdetection_amd import dfine
    scores = _tie_scores(kind, S)
    B, C, K = scores.shape[0], 3, 9 if kind == "straddle" else 100
    g = np.random.default_rng(8)
    x = np.minimum(g.normal(size=(B, S, C)).astype(np.float32) - 9.0, scores[..., None])   # below the score
    x[..., 1] = scores                                                                       # which one class holds
    _, co, mem = _random(9, B, S, C, 4, cuda_device)
    out = _assert_equals_restatement(f"{kind} S {S}", dfine, torch.from_numpy(x).to(cuda_device), co, mem, K)
    if kind == "all_equal":
        assert out.indices.cpu().tolist() == [list(range(K))] * 2
    if kind == "straddle":                 # S - 3, 7, then the lowest seven of the twelve
        assert out.indices.cpu().tolist() == [[S - 3, 7] + sorted(_straddle_ties(S))[:7]]


@pytest.mark.parametrize("S", [50, 2350])
def test_non_finite_scores(cuda_device, S):
    """a row that holds a NaN scores NaN and leads (torch.max, torch.topk's order); +inf next; -inf last"""
    from defectdetection_viaobjectdetection_amd import dfine
    cl, co, mem = _random(11, 2, S, 7, 4, cuda_device)
    cl[0, [0, 5, 9], [0, 6, 3]] = float("nan")
    cl[0, 5, 2] = float("inf")             # NaN wins inside the row
    cl[0, 13, 4] = float("inf")
    cl[0, 17] = float("-inf")
    cl[1, [S - 2, S - 1], 1] = float("nan")
    cl[1, 1:4] = float("-inf")
    K = min(S, 2048)                       # S = 50: every token, the -inf rows included
    out = _assert_equals_restatement("non-finite", dfine, cl, co, mem, K)
    assert out.indices[0, :4].cpu().tolist() == [0, 5, 9, 13] and out.indices[1, :2].cpu().tolist() == [S - 2, S - 1]
    if K == S:
        assert out.indices[0, -1].item() == 17 and out.indices[1, -3:].cpu().tolist() == [1, 2, 3]
    cl[0], cl[1] = float("nan"), float("-inf")
    out = _assert_equals_restatement("all NaN / all -inf", dfine, cl, co, mem, 30)
    assert out.indices.cpu().tolist() == [list(range(30))] * 2
    co[0, 3] = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0])
    out = dfine.select_queries(cl, co, mem, 30)
    b = out.boxes[0, 3].cpu()
    assert torch.isnan(b[0]) and b[1:].tolist() == [1.0, 0.0, 0.5]


def test_batch_invariance_reproducibility_and_full_overwrite(cuda_device):
    """an image alone and inside a batch of 3 give equal bits; two runs give equal bits; every poisoned output element is written"""
    B, S, C, D, K = 3, 2500, 6, 20, 300
    cl, co, mem = _random(21, B, S, C, D, cuda_device)
    run1, run2 = _raw(cl, co, mem, K), _raw(cl, co, mem, K)
    ind, rows, boxes, logits, target, inv = run1
    assert (ind >= 0).all() and not any(torch.isnan(t).any() for t in (rows, boxes, logits, target))
    assert ((inv >= -1) & (inv < K)).all() and ((inv >= 0).sum(1) == K).all()
    assert torch.equal(inv.gather(1, ind).cpu(), torch.arange(K, dtype=torch.int32).expand(B, K))
    for x, y in zip(run1, run2):
        assert torch.equal(x, y)
    for b in range(B):
        alone = _raw(cl[b:b + 1].contiguous(), co[b:b + 1].contiguous(), mem[b:b + 1].contiguous(), K)
        for x, y in zip(run1, alone):
            assert torch.equal(x[b:b + 1], y), b
    plain = _raw(cl, co, None, K, inverse=False)   # no memory, no inverse map
    for x, y in zip(plain, (ind, rows, boxes, logits)):
        assert torch.equal(x, y)
    small = _raw(cl[:, :40].contiguous(), co[:, :40].contiguous(), mem[:, :40].contiguous(), 40)   # K = S through the entry
    assert torch.equal(small[0].sort(1).values.cpu(), torch.arange(40).expand(B, 40)) and (small[5] >= 0).all()


def test_input_layouts(cuda_device):
    """views whose storage starts 1 float off a 16-byte boundary (the 4-byte paths), and non-contiguous inputs"""
    from defectdetection_viaobjectdetection_amd import dfine
    B, S, C, D, K = 2, 2100, 8, 16, 300
    cl, co, mem = _random(31, B, S, C, D, cuda_device)

    def off_by_one(t):
        buf = torch.empty(t.numel() + 1, device=t.device)
        buf[1:] = t.reshape(-1)
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    aligned = _assert_equals_restatement("aligned", dfine, cl, co, mem, K)
    shifted = _assert_equals_restatement("offset 1 float", dfine, off_by_one(cl), off_by_one(co), off_by_one(mem), K)
    for x, y in zip(aligned, shifted):
        assert torch.equal(x, y)
    view_c, view_m = cl[..., :-1], mem.transpose(0, 1).contiguous().transpose(0, 1)   # C = 7 with row stride 8; batch-strided memory
    assert not view_c.is_contiguous() and not view_m.is_contiguous()
    _assert_equals_restatement("non-contiguous", dfine, view_c, co.transpose(0, 1).contiguous().transpose(0, 1), view_m, K)
    for i in range(B):
        one = _assert_equals_restatement(f"slice {i}", dfine, cl[i:i + 1], co[i:i + 1], mem[i:i + 1], K)
        for x, y in zip(aligned, one):
            assert torch.equal(x[i:i + 1], y), i
    wide = _random(32, 1, 700, 91, 5, cuda_device)   # the widest class count of the limits; D not a multiple of 4
    _assert_equals_restatement("C 91", dfine, *wide, 300)


SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(range(4), n)]   # of (g_ref, g_boxes, g_logits, g_target)


@pytest.mark.parametrize("shape", [(2, 525, 300, 80, 256), (3, 2049, 2048, 5, 36)], ids=["model", "edge"])
def test_backward_for_every_subset_of_upstream_gradients(cuda_device, shape):
    """the three input gradients against torch's gather / sigmoid backward at the kernel's own indices: copies and zeros exactly,
    the coordinate term g_ref + g_boxes * b * (1 - b) within twice torch's fp32 error of float64; two runs give equal bits"""
    from defectdetection_viaobjectdetection_amd import dfine
    B, S, K, C, D = shape
    base = _random(41, B, S, C, D, cuda_device)
    gen = torch.Generator(device="cpu").manual_seed(42)
    ups = [torch.randn(s, generator=gen).to(cuda_device) for s in ((B, K, 4), (B, K, 4), (B, K, C), (B, K, D))]
    ind = dfine.select_queries(*base, K).indices
    rows = lambda t: t.gather(1, ind.unsqueeze(-1).repeat(1, 1, t.shape[-1]))

    def grads(fn, subset):
        cl, co, mem = (t.clone().requires_grad_(True) for t in base)
        outs = fn(cl, co, mem)
        got = torch.autograd.grad([outs[i] for i in subset], [cl, co, mem], [ups[i] for i in subset], allow_unused=True)
        return [torch.zeros_like(t) if g is None else g for g, t in zip(got, base)]

    def torch_expr(cl, co, mem):
        r = rows(co)
        return r, torch.sigmoid(r), rows(cl), rows(mem)

    b64 = torch.sigmoid(rows(base[1]).double())
    for subset in SUBSETS:
        before = dfine.model_calls["kernel"]
        ours = grads(lambda cl, co, mem: dfine.select_queries(cl, co, mem, K)[1:], subset)
        assert dfine.model_calls["kernel"] == before + 1
        again = grads(lambda cl, co, mem: dfine.select_queries(cl, co, mem, K)[1:], subset)
        want = grads(torch_expr, subset)
        for a, b in zip(ours, again):
            assert torch.equal(a, b), subset
        assert all(g.dtype == torch.float32 and g.shape == t.shape for g, t in zip(ours, base))
        assert torch.equal(ours[0], want[0]) and torch.equal(ours[2], want[2]), subset
        if 1 not in subset:                # no sigmoid term: copies of g_ref, or zeros
            assert torch.equal(ours[1], want[1]), subset
            continue
        g64 = ups[1].double() * b64 * (1 - b64) + (ups[0].double() if 0 in subset else 0.0)
        want64 = torch.zeros(B, S, 4, dtype=torch.float64, device=cuda_device).scatter(1, ind.unsqueeze(-1).repeat(1, 1, 4), g64)
        err_kernel, err_torch = float((ours[1].double() - want64).abs().max()), float((want[1].double() - want64).abs().max())
        print(f"{shape} {subset}: coordinate gradient error vs float64: kernel {err_kernel:.3e}, torch fp32 {err_torch:.3e}")
        assert err_kernel <= 2 * err_torch, (subset, err_kernel, err_torch)
        unselected = torch.ones(B, S, dtype=torch.bool, device=cuda_device).scatter(1, ind, False)
        assert (ours[1][unselected] == 0).all(), subset


def test_without_gradients_no_inverse_map_and_detached_inputs(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    cl, co, mem = _random(51, 2, 700, 4, 8, cuda_device)
    plain = dfine.select_queries(cl, co, mem, 50)
    assert not any(t.requires_grad for t in plain)
    with torch.no_grad():
        off = dfine.select_queries(cl.requires_grad_(True), co, mem, 50)
    assert not any(t.requires_grad for t in off)
    on = dfine.select_queries(cl, co, mem.detach(), 50)   # memory without a gradient: as model_forward passes it
    assert on.logits.requires_grad and not on.indices.requires_grad
    for x, y in zip(plain, on):
        assert torch.equal(x, y)
    (on.logits.sum() + on.boxes.sum()).backward()
    assert cl.grad is not None and int((cl.grad != 0).sum()) == 2 * 50 * 4


def test_beyond_the_limits_takes_the_torch_path(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    cl, co, mem = _random(61, 1, 2100, 3, 4, cuda_device)
    _assert_equals_restatement("K 2049", dfine, cl, co, mem, 2049, expect_path="torch")
    before = dict(dfine.model_calls)
    out = dfine.select_queries(cl.double(), co.double(), None, 300)
    assert dfine.model_calls == {"kernel": before["kernel"], "torch": before["torch"] + 1}
    assert out.boxes.dtype == torch.float64 and out.boxes.is_cuda
    assert np.array_equal(out.indices.cpu().numpy(), ref.select(cl.cpu().numpy(), co.cpu().numpy(), None, 300)[0])
    with torch.autocast("cuda", dtype=torch.float16):
        dfine.select_queries(cl, co, mem, 300)
    assert dfine.model_calls["torch"] == before["torch"] + 2
    with pytest.raises(RuntimeError):
        dfine.select_queries(cl, co, mem, 2101)   # K above S: torch.topk's error


def test_select_queries_does_not_synchronise(cuda_device, golden):
    from defectdetection_viaobjectdetection_amd import dfine
    g = golden["b2_s1344_c5_k300"]
    cl, co = torch.from_numpy(g["enc_outputs_class"]).to(cuda_device), torch.from_numpy(g["enc_outputs_coord_logits"]).to(cuda_device)
    mem = torch.randn(2, 1344, 32, device=cuda_device)
    view = torch.cat([cl, cl], -1)[..., :5]
    ups = torch.randn(2, 300, 4, device=cuda_device)
    want = dfine.select_queries(cl, co, mem, 300)        # first calls: code object load
    clg, cog = cl.clone().requires_grad_(True), co.clone().requires_grad_(True)
    dfine.select_queries(clg, cog, mem, 300).boxes.backward(ups)
    clg.grad = cog.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [dfine.select_queries(cl, co, mem, 300), dfine.select_queries(view, co, mem, 300)]
        tracked = dfine.select_queries(clg, cog, mem, 300)
        (tracked.boxes * ups).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for out in outs + [tracked]:
        for x, y in zip(want, out):
            assert torch.equal(x, y)
    assert cog.grad is not None and clg.grad is not None and not clg.grad.any()
    # the same through the profiler, should this build of torch not honour the debug mode: no device-to-host copy
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        (dfine.select_queries(clg, cog, mem, 300).boxes * ups).sum().backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    for kernel in ("dfine_token_scores_kernel", "dfine_select_gather_kernel", "dfine_select_backward_kernel"):
        assert any(kernel in n for n in names), sorted(set(names))
    assert not any("dtoh" in n.lower().replace(" ", "").replace("_", "") for n in names), sorted(set(names))
