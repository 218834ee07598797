"""D-FINE detection post-processing, the parts that need no GPU: the float64 restatement (tests/dfine_postprocess_ref.py) and
dfine.post_process_torch on CPU reproduce every golden case (recorded from transformers' own post_process_object_detection,
tests/golden/make_dfine_postprocess_golden.py), and m355_dfine_postprocess rejects bad arguments on the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dfine_postprocess_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ref.GOLDEN)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_cases_cover_the_issue_and_keep_their_gaps(golden):
    assert [s for s, _ in ref.CASES] == [(1, 300, 3), (2, 300, 80), (3, 300, 2), (2, 37, 1), (2, 20, 91), (2, 1024, 4), (2, 2048, 1),
                                         (1, 1, 1)]
    assert sum(sz is None for _, sz in ref.CASES) == 1 and any(h != w for _, sz in ref.CASES if sz for h, w in sz)
    assert float(golden["threshold"]) == ref.GOLDEN_THRESHOLD
    for shape, sizes in ref.CASES:
        case = ref.load_case(golden, shape)
        assert case["logits"].shape == shape and case["logits"].dtype == np.float32 and case["logits"].nbytes < 200 * 1024
        assert case["sizes"] == sizes
        for b in range(shape[0]):
            gap, dist = ref.ladder_conditions(case["logits"][b], ref.GOLDEN_THRESHOLD)
            assert gap >= 1e-4 and dist >= 1e-4, (shape, b, gap, dist)


@pytest.mark.parametrize("shape,sizes", ref.CASES, ids=[ref.case_name(s) for s, _ in ref.CASES])
def test_restatement_reproduces_the_golden_case(golden, shape, sizes):
    case = ref.load_case(golden, shape)
    scores, labels, boxes, counts, _ = ref.post_process(case["logits"], case["boxes"], sizes, ref.GOLDEN_THRESHOLD)
    for b in range(shape[0]):
        g_scores, g_labels, g_boxes = case["full"][b]
        assert np.array_equal(labels[b], g_labels), (shape, b)
        assert np.abs(scores[b] - g_scores).max() <= 1e-6
        assert np.all(np.abs(boxes[b] - g_boxes) <= 1e-6 * np.maximum(np.abs(boxes[b]), 1.0))
        k_scores, k_labels, k_boxes = case["kept"][b]
        n_nan, n_keep = counts[b]
        assert n_nan == 0 and n_keep == len(k_scores), (shape, b)
        assert np.array_equal(labels[b, :n_keep], k_labels)
        assert np.abs(scores[b, :n_keep] - k_scores).max(initial=0.0) <= 1e-6
        assert np.all(np.abs(boxes[b, :n_keep] - k_boxes) <= 1e-6 * np.maximum(np.abs(boxes[b, :n_keep]), 1.0))


@pytest.mark.parametrize("shape,sizes", ref.CASES, ids=[ref.case_name(s) for s, _ in ref.CASES])
def test_post_process_torch_on_cpu_equals_the_golden_case(golden, shape, sizes):
    from defectdetection_viaobjectdetection_amd import dfine
    case = ref.load_case(golden, shape)
    logits, boxes = torch.from_numpy(case["logits"]), torch.from_numpy(case["boxes"])
    for threshold, key in ((ref.GOLDEN_THRESHOLD, "kept"), (-1.0, "full")):
        got = dfine.post_process_torch(logits, boxes, sizes, threshold)
        assert len(got) == shape[0]
        for b, d in enumerate(got):
            g_scores, g_labels, g_boxes = case[key][b]
            assert sorted(d) == ["boxes", "labels", "scores"]
            assert d["labels"].dtype == torch.int64 and np.array_equal(d["labels"].numpy(), g_labels), (shape, b)
            assert d["boxes"].dtype == torch.float32 and np.array_equal(d["boxes"].numpy().view(np.uint32), g_boxes.view(np.uint32))
            s = d["scores"].numpy()
            assert s.dtype == np.float32 and s.shape == g_scores.shape
            assert np.all(np.abs(s - g_scores) <= np.spacing(np.maximum(s, g_scores))), (shape, b)   # 1 ulp
    # the functions that take the kernel on a GPU fall back to the same expression on CPU tensors
    full = dfine.post_process_detections(logits, boxes, sizes, -1.0)
    assert all(np.array_equal(d["labels"].numpy(), case["full"][b][1]) for b, d in enumerate(full))
    scores, labels, out_boxes, counts = dfine.topk_detections(logits, boxes, sizes, ref.GOLDEN_THRESHOLD)
    assert counts.dtype == torch.int32 and counts.tolist() == [[0, len(case["kept"][b][0])] for b in range(shape[0])]
    assert np.array_equal(labels.numpy(), np.stack([f[1] for f in case["full"]]))


def test_length_check_and_mapping_outputs_without_a_gpu():
    from defectdetection_viaobjectdetection_amd import dfine
    logits, boxes = torch.zeros(2, 5, 3), torch.full((2, 5, 4), 0.5)
    with pytest.raises(ValueError, match="as many target sizes as the batch dimension"):
        dfine.post_process_object_detection(None, {"logits": logits, "pred_boxes": boxes}, target_sizes=[(4, 4)])
    out = dfine.post_process_object_detection(None, {"logits": logits, "pred_boxes": boxes}, threshold=0.4, target_sizes=[(4, 8)] * 2)
    assert len(out) == 2 and out[0]["boxes"].shape == (5, 4) and out[0]["boxes"][0].tolist() == [2.0, 1.0, 6.0, 3.0]
    soft = dfine.post_process_object_detection(None, {"logits": logits, "pred_boxes": boxes}, threshold=0.4, use_focal_loss=False)
    assert len(soft) == 2 and soft[0]["scores"].numel() == 0   # softmax of equal logits: 1/3 each, below the threshold


def test_postprocess_entry_rejects_bad_arguments_without_a_gpu():
    """m355_dfine_postprocess validates every argument on the host before any HIP call: -1 (M355_ERR_INVALID) with a message,
    on fake device pointers that are never dereferenced."""
    from defectdetection_viaobjectdetection_amd import _capi
    fake = ctypes.c_void_p(0x1000)
    f, err = _capi.lib.m355_dfine_postprocess, lambda: _capi.lib.m355_last_error(None)

    def call(B=2, Q=300, C=3, **ptrs):
        p = dict(logits=fake, boxes=fake, sizes=fake, scores=fake, labels=fake, out_boxes=fake, counts=fake)
        p.update(ptrs)
        return f(p["logits"], p["boxes"], B, Q, C, p["sizes"], 0.5, p["scores"], p["labels"], p["out_boxes"], p["counts"], None)

    for name in ("logits", "boxes", "scores", "labels", "out_boxes", "counts"):
        assert call(**{name: None}) == -1, name
        assert b"dfine_postprocess: null pointer" in err()
    for kw in (dict(B=0), dict(B=-1), dict(Q=0), dict(Q=2049), dict(Q=-1), dict(C=0), dict(C=-3), dict(Q=2048, C=8192),
               dict(Q=1024, C=16384), dict(Q=2048, C=1 << 30)):
        assert call(**kw) == -1, kw
        assert b"Q in [1, 2048]" in err() and b"Q * C < 2^24" in err()
