"""dfine.topk_detections / post_process_detections / post_process_object_detection on the GPU: the D-FINE inference tail
(sigmoid, top-K, labels, scaled boxes, threshold) in one kernel launch.

Labels, counts and box bits are held exactly to what transformers' own post_process_object_detection recorded in
tests/golden/dfine_postprocess_golden.npz (every image built so that its top scores are at least 1e-4 apart) and, where ties or
non-finite logits are the point, to the float64 restatement of tests/dfine_postprocess_ref.py, whose order rule is the kernel's.
Scores are held to  max |kernel - float64| <= 2 * max |torch fp32 on this device - float64| + 6e-8  (6e-8: one fp32 ulp below 1)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import dfine_postprocess_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ref.GOLDEN)
IDS = [ref.case_name(s) for s, _ in ref.CASES]


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {shape: ref.load_case(z, shape) for shape, _ in ref.CASES}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _score_errors(kernel_scores, torch_scores, want):
    """(kernel error, torch fp32 error) against the float64 scores; NaN must sit where NaN is wanted"""
    k, t = np.asarray(kernel_scores, np.float64), np.asarray(torch_scores, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(k), nan)
    return float(np.abs(k - want)[~nan].max(initial=0.0)), float(np.abs(t - want)[~nan].max(initial=0.0))


def _assert_score_bound(what, kernel_scores, torch_scores, want):
    err_kernel, err_torch = _score_errors(kernel_scores, torch_scores, want)
    print(f"{what}: score error vs float64: kernel {err_kernel:.3e}, torch fp32 {err_torch:.3e}")
    assert err_kernel <= 2 * err_torch + 6e-8, (what, err_kernel, err_torch)


def _torch_rows(logits, boxes, sizes, index):
    """torch fp32 on the device of `logits`, taken at the restatement's flat candidates: scores (B, K), boxes (B, K, 4)"""
    B, Q, C = logits.shape
    idx = torch.from_numpy(index).to(logits.device)
    scores = torch.sigmoid(logits).flatten(1).gather(1, idx)
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    if sizes is not None:
        s = torch.as_tensor(sizes).to(logits.device)
        xyxy = xyxy * torch.stack([s[:, 1], s[:, 0], s[:, 1], s[:, 0]], 1)[:, None, :]
    return scores.cpu().numpy(), xyxy.gather(1, (idx // C).unsqueeze(-1).repeat(1, 1, 4)).cpu().numpy()


def _assert_equals_restatement(what, dfine, logits, boxes, sizes, threshold):
    """the four outputs of topk_detections against the restatement: labels and counts exact, boxes torch's fp32 bits, scores bound"""
    scores, labels, out_boxes, counts = dfine.topk_detections(logits, boxes, sizes, threshold)
    want_scores, want_labels, _, want_counts, index = ref.post_process(logits.cpu().numpy(), boxes.cpu().numpy(), sizes, threshold)
    assert np.array_equal(labels.cpu().numpy(), want_labels), what
    assert np.array_equal(counts.cpu().numpy(), want_counts), (what, counts.cpu().tolist(), want_counts.tolist())
    torch_scores, torch_boxes = _torch_rows(logits, boxes, sizes, index)
    assert np.array_equal(_bits(out_boxes.cpu().numpy()), _bits(torch_boxes)), what
    _assert_score_bound(what, scores.cpu().numpy(), torch_scores, want_scores)
    return scores, labels, out_boxes, counts


def _assert_dicts_equal_torch(what, dfine, logits, boxes, sizes, threshold):
    """post_process_detections against post_process_torch on the same device: structure, labels and box bits exact, scores bound"""
    got = dfine.post_process_detections(logits, boxes, sizes, threshold)
    want = dfine.post_process_torch(logits, boxes, sizes, threshold)
    f64_scores, _, _, f64_counts, _ = ref.post_process(logits.cpu().numpy(), boxes.cpu().numpy(), sizes, threshold)
    assert len(got) == len(want) == logits.shape[0]
    for b, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w) == ["boxes", "labels", "scores"]
        for k in g:
            assert g[k].dtype == w[k].dtype and g[k].device == w[k].device and g[k].shape == w[k].shape, (what, b, k)
        assert not torch.isnan(g["scores"]).any()
        assert torch.equal(g["labels"], w["labels"]), (what, b)
        assert np.array_equal(_bits(g["boxes"].cpu().numpy()), _bits(w["boxes"].cpu().numpy())), (what, b)
        n_nan, n_keep = (int(v) for v in f64_counts[b])
        _assert_score_bound(f"{what} image {b}", g["scores"].cpu().numpy(), w["scores"].cpu().numpy(), f64_scores[b, n_nan:n_nan + n_keep])
    return got


def _ladder(seed, B, Q, C, threshold=ref.GOLDEN_THRESHOLD):
    rng = np.random.default_rng(seed)
    logits = np.stack([ref.ladder_logits(rng, Q, C) for _ in range(B)])
    for b in range(B):
        gap, dist = ref.ladder_conditions(logits[b], threshold)
        assert (gap >= 1e-4 or Q * C == 1) and dist >= 1e-4, (seed, b, gap, dist)
    return logits, ref.random_boxes(rng, B, Q)


def _raw(logits, boxes, sizes, threshold):
    """the C entry on outputs poisoned with NaN / -1"""
    from defectdetection_viaobjectdetection_amd import _capi
    B, Q, C = logits.shape
    dev = logits.device
    scores = torch.full((B, Q), float("nan"), device=dev)
    labels = torch.full((B, Q), -1, dtype=torch.int64, device=dev)
    out_boxes = torch.full((B, Q, 4), float("nan"), device=dev)
    counts = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = _capi.lib.m355_dfine_postprocess(ptr(logits), ptr(boxes), B, Q, C, ptr(sizes), threshold, ptr(scores), ptr(labels),
                                          ptr(out_boxes), ptr(counts), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _capi.lib.m355_last_error(None)
    torch.cuda.synchronize()
    return scores, labels, out_boxes, counts


@pytest.mark.parametrize("shape,sizes", ref.CASES, ids=IDS)
def test_golden_cases(cuda_device, golden, shape, sizes):
    from defectdetection_viaobjectdetection_amd import dfine
    case = golden[shape]
    B, Q, C = shape
    logits, boxes = torch.from_numpy(case["logits"]).to(cuda_device), torch.from_numpy(case["boxes"]).to(cuda_device)
    before = dict(dfine.post_calls)
    scores, labels, out_boxes, counts = _assert_equals_restatement(ref.case_name(shape), dfine, logits, boxes, sizes, ref.GOLDEN_THRESHOLD)
    assert dfine.post_calls["kernel"] == before["kernel"] + 1 and dfine.post_calls["torch"] == before["torch"]
    assert all(t.is_cuda for t in (scores, labels, out_boxes, counts))
    assert (scores.dtype, labels.dtype, out_boxes.dtype, counts.dtype) == (torch.float32, torch.int64, torch.float32, torch.int32)
    assert (scores.shape, labels.shape, out_boxes.shape, counts.shape) == ((B, Q), (B, Q), (B, Q, 4), (B, 2))
    assert counts.cpu().tolist() == [[0, len(case["kept"][b][0])] for b in range(B)]
    for b in range(B):
        g_scores, g_labels, g_boxes = case["full"][b]
        assert np.array_equal(labels[b].cpu().numpy(), g_labels), b
        assert np.array_equal(_bits(out_boxes[b].cpu().numpy()), _bits(g_boxes)), b
    dicts = dfine.post_process_detections(logits, boxes, sizes, ref.GOLDEN_THRESHOLD)
    assert isinstance(dicts, list) and len(dicts) == B
    for b, d in enumerate(dicts):
        k_scores, k_labels, k_boxes = case["kept"][b]
        assert sorted(d) == ["boxes", "labels", "scores"] and all(v.is_cuda for v in d.values())
        assert (d["scores"].dtype, d["labels"].dtype, d["boxes"].dtype) == (torch.float32, torch.int64, torch.float32)
        assert d["scores"].shape == k_scores.shape and d["boxes"].shape == k_boxes.shape
        assert np.array_equal(d["labels"].cpu().numpy(), k_labels)
        assert np.array_equal(_bits(d["boxes"].cpu().numpy()), _bits(k_boxes))


def test_batch_invariance_reproducibility_and_full_overwrite(cuda_device, golden):
    """image b of a batch gives the bits of the same image alone; two runs give equal bits; every poisoned output is written"""
    case = golden[(2, 300, 80)]
    logits, boxes = torch.from_numpy(case["logits"]).to(cuda_device), torch.from_numpy(case["boxes"]).to(cuda_device)
    sizes = torch.tensor(case["sizes"], dtype=torch.float32, device=cuda_device)
    run1, run2 = _raw(logits, boxes, sizes, 0.3), _raw(logits, boxes, sizes, 0.3)
    assert not torch.isnan(run1[0]).any() and not torch.isnan(run1[2]).any() and (run1[1] >= 0).all() and (run1[3] >= 0).all()
    for x, y in zip(run1, run2):
        assert torch.equal(x, y)
    for b in range(2):
        alone = _raw(logits[b:b + 1].contiguous(), boxes[b:b + 1].contiguous(), sizes[b:b + 1].contiguous(), 0.3)
        for x, y in zip(run1, alone):
            assert torch.equal(x[b:b + 1], y), b
    no_sizes = _raw(logits, boxes, None, 0.3)
    assert not torch.isnan(no_sizes[2]).any() and torch.equal(no_sizes[1], run1[1])


def _tie_logits(kind, C):
    g = np.random.default_rng(7)
    if kind == "straddle_q5_c4":          # two clear winners, then six equal candidates for three places
        x = np.full((1, 5, 4), -2.0, np.float32)
        x.reshape(-1)[[17, 2]] = [3.0, 2.5]
        x.reshape(-1)[[19, 4, 11, 6, 13, 0]] = 1.0
        return x
    if kind == "straddle_selected":       # the same across the waves' runs of a selection: 2 winners, 10 candidates for 6 places
        x = np.full((1, 8, 300), -2.0, np.float32)
        x.reshape(-1)[[2100, 7]] = [3.0, 2.5]
        x.reshape(-1)[[2399, 63, 64, 1300, 5, 640, 2000, 319, 320, 1999]] = 1.0
        return x
    Q = 70                                # C 5: 350 candidates, sorted directly; C 31: 2 170, through the radix selection
    if kind == "rows_repeated":
        return np.repeat(g.normal(size=(2, 1, C)).astype(np.float32), Q, 1)
    if kind == "all_equal":
        return np.full((2, Q, C), 0.25, np.float32)
    if kind == "saturated":               # a third of the candidates at +30: score exactly 1.0
        x = g.normal(size=(2, Q, C)).astype(np.float32)
        x[g.uniform(size=x.shape) < 1 / 3] = 30.0
        return x
    if kind == "signed_zeros":            # -0 ties with +0
        x = np.where(g.uniform(size=(2, Q, C)) < 0.5, -0.0, 0.0).astype(np.float32)
        x[:, ::7, 1] = -1.0
        return x
    raise KeyError(kind)


TIE_CASES = [("straddle_q5_c4", 4), ("straddle_selected", 300)] + [(k, C) for k in ("rows_repeated", "all_equal", "saturated", "signed_zeros")
                                                                   for C in (5, 31)]


@pytest.mark.parametrize("kind,C", TIE_CASES, ids=[f"{k}-c{C}" for k, C in TIE_CASES])
def test_exact_ties(cuda_device, kind, C):
    """an exact tie goes to the lowest flat index: the output equals the restatement, and the score sequence is torch.topk's"""
    from defectdetection_viaobjectdetection_amd import dfine
    x = _tie_logits(kind, C)
    B, Q, C = x.shape
    logits = torch.from_numpy(x).to(cuda_device)
    boxes = torch.from_numpy(ref.random_boxes(np.random.default_rng(8), B, Q)).to(cuda_device)
    sizes = [(480, 640)] * B
    what = f"{kind} C {C}"
    scores, labels, _, counts = _assert_equals_restatement(what, dfine, logits, boxes, sizes, 0.5)
    if kind == "straddle_q5_c4":
        assert labels.cpu().tolist() == [[17 % 4, 2 % 4, 0, 0, 6 % 4]]   # flat 17, 2, then the lowest three of the six: 0, 4, 6
    if kind == "straddle_selected":
        assert labels.cpu().tolist() == [[i % 300 for i in (2100, 7, 5, 63, 64, 319, 320, 640)]]
    want = ref.post_process(x, boxes.cpu().numpy(), sizes, 0.5)[0]
    top = torch.topk(torch.sigmoid(logits).flatten(1), Q, dim=-1).values
    _assert_score_bound(what + " (torch.topk values)", scores.cpu().numpy(), top.cpu().numpy(), want)


@pytest.mark.parametrize("C", [7, 47])   # 350 candidates (sorted directly) and 2 350 (through the radix selection)
def test_non_finite_logits(cuda_device, C):
    """NaN rows lead (torch.topk's order) and are in no dict; +inf scores 1, -inf scores 0"""
    from defectdetection_viaobjectdetection_amd import dfine
    x, bx = _ladder(11, 2, 50, C)
    flat = x.reshape(2, -1)
    flat[0, [0, 5, 9]] = np.nan
    flat[0, 13], flat[0, [17, 21]] = np.inf, -np.inf
    flat[1, [348, 349]] = np.nan
    flat[1, [1, 2, 3]] = -np.inf
    logits, boxes = torch.from_numpy(x).to(cuda_device), torch.from_numpy(bx).to(cuda_device)
    sizes = [(375, 500), (640, 640)]
    scores, labels, _, counts = _assert_equals_restatement("non-finite", dfine, logits, boxes, sizes, 0.3)
    assert counts[:, 0].cpu().tolist() == [3, 2]
    assert torch.isnan(scores[0, :3]).all() and labels[0, :3].cpu().tolist() == [0, 5, 9 % C] and float(scores[0, 3]) == 1.0
    dicts = _assert_dicts_equal_torch("non-finite", dfine, logits, boxes, sizes, 0.3)
    assert float(dicts[0]["scores"][0]) == 1.0 and int(dicts[0]["labels"][0]) == 13 % C
    # every logit of an image NaN, or -inf: K NaN rows by ascending index, or K zero scores
    logits[0], logits[1] = float("nan"), float("-inf")
    scores, labels, _, counts = _assert_equals_restatement("all NaN / all -inf", dfine, logits, boxes, sizes, 0.0)
    assert counts.cpu().tolist() == [[50, 0], [0, 0]] and torch.isnan(scores[0]).all() and (scores[1] == 0).all()
    assert [len(d["scores"]) for d in dfine.post_process_detections(logits, boxes, sizes, 0.0)] == [0, 0]


@pytest.mark.parametrize("threshold", [0.0, 1.0, -1.0, 0.3])
def test_threshold_values(cuda_device, threshold):
    """Q * C == K (a full sort) with a zero score and a score of exactly 1: `>` is strict at both ends"""
    from defectdetection_viaobjectdetection_amd import dfine
    x, bx = _ladder(12, 2, 37, 1)
    x[0, 3, 0], x[0, 10, 0], x[1, 36, 0] = -np.inf, 30.0, -np.inf
    logits, boxes = torch.from_numpy(x).to(cuda_device), torch.from_numpy(bx).to(cuda_device)
    _, _, _, counts = _assert_equals_restatement(f"threshold {threshold}", dfine, logits, boxes, None, threshold)
    if threshold in (0.0, 1.0, -1.0):
        assert counts.cpu().tolist() == {0.0: [[0, 36], [0, 36]], 1.0: [[0, 0], [0, 0]], -1.0: [[0, 37], [0, 37]]}[threshold]
    _assert_dicts_equal_torch(f"threshold {threshold}", dfine, logits, boxes, None, threshold)


def test_target_sizes_forms(cuda_device, golden):
    from defectdetection_viaobjectdetection_amd import dfine
    case = golden[(3, 300, 2)]
    logits, boxes = torch.from_numpy(case["logits"]).to(cuda_device), torch.from_numpy(case["boxes"]).to(cuda_device)
    as_list = dfine.topk_detections(logits, boxes, case["sizes"], 0.3)
    forms = {"tuple list": [tuple(s) for s in case["sizes"]],
             "int64 device": torch.tensor(case["sizes"], dtype=torch.int64, device=cuda_device),
             "float32 device": torch.tensor(case["sizes"], dtype=torch.float32, device=cuda_device),
             "int32 host": torch.tensor(case["sizes"], dtype=torch.int32),
             "float64 host": torch.tensor(case["sizes"], dtype=torch.float64)}
    for name, sizes in forms.items():
        for x, y in zip(as_list, dfine.topk_detections(logits, boxes, sizes, 0.3)):
            assert torch.equal(x, y), name
    for b in range(3):
        assert np.array_equal(_bits(as_list[2][b].cpu().numpy()), _bits(case["full"][b][2]))
    plain = dfine.topk_detections(logits, boxes, None, 0.3)
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    idx = torch.from_numpy(ref.post_process(case["logits"], case["boxes"], None, 0.3)[4]).to(cuda_device) // 2
    assert torch.equal(plain[2], xyxy.gather(1, idx.unsqueeze(-1).repeat(1, 1, 4))) and torch.equal(plain[1], as_list[1])
    with pytest.raises(ValueError, match="as many target sizes as the batch dimension"):
        dfine.topk_detections(logits, boxes, case["sizes"][:2], 0.3)


def test_input_layouts(cuda_device):
    """a non-contiguous logits view, a batch slice, C not a power of two, Q * C not a multiple of 64"""
    from defectdetection_viaobjectdetection_amd import dfine
    x, bx = _ladder(13, 3, 50, 8)
    wide, boxes = torch.from_numpy(x).to(cuda_device), torch.from_numpy(bx).to(cuda_device)
    view = wide[..., :-1]                 # C = 7, row stride 8
    assert not view.is_contiguous() and (50 * 7) % 64 != 0
    sizes = [(480, 640), (375, 500), (333, 777)]
    whole = _assert_equals_restatement("view", dfine, view, boxes, sizes, 0.3)
    for i in range(3):
        one = _assert_equals_restatement(f"slice {i}", dfine, view[i:i + 1], boxes[i:i + 1], sizes[i:i + 1], 0.3)
        for a, b in zip(whole, one):
            assert torch.equal(a[i:i + 1], b), i
    for Q, C in ((33, 3), (33, 5), (33, 91), (683, 3)):   # 683 * 3 = 2 049: the smallest size that goes through the selection
        y, by = _ladder(14 + C + Q, 1, Q, C)
        _assert_equals_restatement(f"Q {Q} C {C}", dfine, torch.from_numpy(y).to(cuda_device), torch.from_numpy(by).to(cuda_device), [(32, 48)], 0.3)


def test_beyond_the_limits_takes_the_fallback(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    x, bx = _ladder(20, 1, 2049, 1)
    logits, boxes = torch.from_numpy(x).to(cuda_device), torch.from_numpy(bx).to(cuda_device)
    before = dict(dfine.post_calls)
    scores, labels, out_boxes, counts = dfine.topk_detections(logits, boxes, [(480, 640)], 0.3)
    assert dfine.post_calls["kernel"] == before["kernel"] and dfine.post_calls["torch"] == before["torch"] + 1
    want_scores, want_labels, _, want_counts, index = ref.post_process(x, bx, [(480, 640)], 0.3)
    assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert counts.dtype == torch.int32 and np.abs(scores.cpu().numpy() - want_scores).max() <= 2e-7
    assert np.array_equal(_bits(out_boxes.cpu().numpy()), _bits(_torch_rows(logits, boxes, [(480, 640)], index)[1]))
    dicts = dfine.post_process_detections(logits, boxes, [(480, 640)], 0.3)
    assert len(dicts) == 1 and len(dicts[0]["scores"]) == int(want_counts[0, 1])
    # inputs under autograd take the torch expression too, and stay differentiable
    small = logits[:, :40].clone().requires_grad_(True)
    got = dfine.post_process_detections(small, boxes[:, :40], None, 0.3)
    assert got[0]["scores"].requires_grad and dfine.post_calls["kernel"] == before["kernel"]


def test_topk_detections_does_not_synchronise(cuda_device, golden):
    from defectdetection_viaobjectdetection_amd import dfine
    case = golden[(1, 300, 3)]
    logits, boxes = torch.from_numpy(case["logits"]).to(cuda_device), torch.from_numpy(case["boxes"]).to(cuda_device)
    dev_sizes = torch.tensor(case["sizes"], dtype=torch.int64, device=cuda_device)
    view = torch.cat([logits, logits], -1)[..., :3]
    want = dfine.topk_detections(logits, boxes, case["sizes"], 0.3)   # first call: code object load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [dfine.topk_detections(logits, boxes, case["sizes"], 0.3), dfine.topk_detections(logits, boxes, dev_sizes, 0.3),
                dfine.topk_detections(view, boxes, torch.tensor(case["sizes"]), 0.3), dfine.topk_detections(logits, boxes, None, 0.3)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for out in outs[:3]:
        for x, y in zip(want, out):
            assert torch.equal(x, y)
    assert torch.equal(outs[3][0], want[0]) and torch.equal(outs[3][1], want[1])
    # the same through the profiler, should this build of torch not honour the debug mode: no device-to-host copy
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        dfine.topk_detections(logits, boxes, case["sizes"], 0.3)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert any("dfine_postprocess_kernel" in n for n in names), sorted(set(names))
    assert not any("dtoh" in n.lower().replace(" ", "").replace("_", "") for n in names), sorted(set(names))


def _processor_classes():
    import transformers
    found = []
    for name in ("RTDetrImageProcessor", "RTDetrImageProcessorPil", "RTDetrImageProcessorFast"):
        try:
            cls = getattr(transformers, name)
            cls.post_process_object_detection
        except Exception:
            continue
        if cls not in found:
            found.append(cls)
    return found


def test_bound_processor_runs_the_reference_frame_loop(cuda_device):
    """the per-frame loop of the reference's temporal model on 5 frames, the processor's method bound and unbound"""
    from defectdetection_viaobjectdetection_amd import dfine
    classes = _processor_classes()
    assert classes, "no RT-DETR image processor class imports"
    stock = [cls.post_process_object_detection for cls in classes]
    processor = classes[0]()
    x, bx = _ladder(16, 5, 300, 3)
    cls_logits, bbox_pred = torch.from_numpy(x).to(cuda_device), torch.from_numpy(bx).to(cuda_device)
    frame_sizes = [(480, 640), (480, 640), (375, 500), (1080, 1920), (333, 777)]

    def frame_loop(wrap):
        results = []
        for i, sz in enumerate(frame_sizes):
            results.append(processor.post_process_object_detection(
                wrap({"logits": cls_logits[i:i + 1], "pred_boxes": bbox_pred[i:i + 1]}), target_sizes=torch.tensor([sz]),
                threshold=0.3)[0])
        return results

    unbound = frame_loop(lambda d: types.SimpleNamespace(**d))   # upstream reads attributes
    before = dfine.post_calls["kernel"]
    try:
        for cls in classes:
            cls.post_process_object_detection = dfine.post_process_object_detection
        bound = frame_loop(dict) + frame_loop(lambda d: types.SimpleNamespace(**d))
        with pytest.raises(ValueError, match="as many target sizes as the batch dimension"):
            processor.post_process_object_detection({"logits": cls_logits, "pred_boxes": bbox_pred}, target_sizes=[(4, 4)])
    finally:
        for cls, fn in zip(classes, stock):
            cls.post_process_object_detection = fn
    assert dfine.post_calls["kernel"] == before + 10
    assert all(cls.post_process_object_detection is fn for cls, fn in zip(classes, stock))
    want = ref.post_process(x, bx, frame_sizes, 0.3)
    for i, u in enumerate(unbound):
        n = int(want[3][i, 1])
        for g in (bound[i], bound[5 + i]):
            assert sorted(g) == sorted(u) and all(g[k].dtype == u[k].dtype and g[k].device == u[k].device for k in u)
            assert torch.equal(g["labels"], u["labels"]) and len(g["labels"]) == n, i
            assert np.array_equal(_bits(g["boxes"].cpu().numpy()), _bits(u["boxes"].cpu().numpy())), i
            _assert_score_bound(f"frame {i}", g["scores"].cpu().numpy(), u["scores"].cpu().numpy(), want[0][i, :n])
    # the same five frames as one call for the sequence
    seq = dfine.post_process_detections(cls_logits, bbox_pred, frame_sizes, 0.3)
    for s, g in zip(seq, bound):
        assert all(torch.equal(s[k], g[k]) for k in g)
