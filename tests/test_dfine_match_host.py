"""Hungarian matcher of the D-FINE loss, the parts that need no GPU: the float64 restatement of the cost expression
(tests/dfine_match_ref.py) plus scipy reproduces every golden case (indices recorded from transformers'
RTDetrHungarianMatcher, tests/golden/make_dfine_match_golden.py), and m355_dfine_match rejects bad arguments on the host."""
import ctypes
import os

import numpy as np
import pytest

import dfine_match_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ref.GOLDEN)


def test_golden_cases_cover_the_issue_and_keep_their_gap():
    z = np.load(GOLDEN)
    names = ref.case_names(z)
    assert len(names) == 7 and sum(not ref.load_case(z, n)["focal"] for n in names) == 1
    assert any(max(ref.load_case(z, n)["sizes"]) > ref.load_case(z, n)["logits"].shape[1] for n in names)   # more targets than queries
    for n in names:
        case = ref.load_case(z, n)
        assert all(g >= 1e-3 for g in case["gap"]), (n, case["gap"])


def test_restatement_plus_scipy_reproduces_every_golden_case():
    linear_sum_assignment = pytest.importorskip("scipy.optimize").linear_sum_assignment
    z = np.load(GOLDEN)
    for name in ref.case_names(z):
        case = ref.load_case(z, name)
        for b, n in enumerate(case["sizes"]):
            cost = ref.cost_matrix(case["logits"][b], case["boxes"][b], case["labels"][b], case["tboxes"][b],
                                   use_focal_loss=case["focal"])
            assert cost.shape == (case["logits"].shape[1], n) and cost.dtype == np.float64
            rows, cols = linear_sum_assignment(cost)
            assert np.array_equal(rows, case["rows"][b]) and np.array_equal(cols, case["cols"][b]), (name, b)
            assert len(rows) == min(cost.shape)
            assert abs(cost[rows, cols].sum() - case["optimum"][b]) <= 1e-12 * max(1.0, abs(case["optimum"][b])), (name, b)


def test_match_entry_rejects_bad_arguments_without_a_gpu():
    """m355_dfine_match validates every argument on the host before any HIP call: -1 (M355_ERR_INVALID) with a message, on
    fake device pointers that are never dereferenced."""
    from defectdetection_viaobjectdetection_amd import _capi
    fake = ctypes.c_void_p(0x1000)
    f, err = _capi.lib.m355_dfine_match, lambda: _capi.lib.m355_last_error(None)

    def call(B=2, Q=300, C=3, counts=(3, 5), ptrs=None, work=None, work_bytes=0, kmax=None, cost=None):
        p = dict(logits=fake, boxes=fake, labels=fake, tboxes=fake, offsets=fake, rows=fake, cols=fake, flags=fake, counts=True)
        p.update(ptrs or {})
        h = (ctypes.c_int32 * max(len(counts), 1))(*counts) if p["counts"] else None
        k = min(Q, max(counts, default=0)) if kmax is None else kmax
        return f(p["logits"], p["boxes"], B, Q, C, p["labels"], p["tboxes"], p["offsets"], h, 2.0, 5.0, 2.0, 0.25, 2.0, 1,
                 work, work_bytes, cost, p["rows"], p["cols"], k, p["flags"], None)

    for name in ("logits", "boxes", "labels", "tboxes", "offsets", "rows", "cols", "flags"):
        assert call(ptrs={name: None}) == -1, name
        assert b"null pointer" in err()
    assert call(ptrs={"counts": False}) == -1
    for q in (0, 2049, -1):
        assert call(Q=q) == -1, q
        assert b"Q in [1, 2048]" in err()
    assert call(B=0, counts=()) == -1
    assert call(C=0) == -1
    for counts in ((3, 513), (-1, 5)):
        assert call(counts=counts) == -1, counts
        assert b"[0, 512]" in err()
    assert call(kmax=4) == -1 and b"kmax" in err()
    # 2048 queries x 512 targets do not fit in LDS: a workspace is required, and must be large enough
    ws = _capi.lib.m355_dfine_match_workspace_bytes
    need = ws(2, 2048, 512)
    assert need == 2 * 2048 * 512 * 4 and ws(2, 300, 5) == 0 and ws(4, 300, 64) == 0
    assert call(Q=2048, counts=(512, 1)) == -1 and b"workspace" in err()
    assert call(Q=2048, counts=(512, 1), work=fake, work_bytes=need - 1) == -1 and b"workspace" in err()
