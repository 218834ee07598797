"""D-FINE loss terms, the parts that need no GPU: the float64 restatement (tests/dfine_loss_ref.py) reproduces what transformers'
DFineLoss recorded (tests/golden/make_dfine_loss_golden.py), dfine.detection_loss's torch path agrees with it,
dfine.criterion_forward bound into DFineLoss returns upstream's keys and values, and m355_dfine_loss_forward / _backward reject
bad arguments on the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dfine_loss_ref as ref
from defectdetection_viaobjectdetection_amd import dfine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ref.GOLDEN)
GRADS = ("grad_logits", "grad_pred_boxes", "grad_pred_corners")


@pytest.fixture(scope="module")
def cases():
    z = np.load(GOLDEN)
    return {n: ref.load_case(z, n) for n in ref.case_names(z)}


def ref64(case):
    """values and weighted gradients of a case by the restatement, all float64"""
    outputs, targets, indices, kw = ref.tensors(case)
    values = ref.terms(outputs, targets, indices, float(case["num_boxes"]), **kw)
    grads = ref.weighted_grads(values, outputs)
    return ({k: float(v.detach()) for k, v in values.items()},
            {k: (torch.zeros_like(outputs[k[5:]]) if g is None else g).numpy() for k, g in grads.items()})


def test_golden_holds_the_nine_cases_of_the_issue(cases):
    assert len(cases) == 9
    shapes = {n[0]: tuple(c["logits"].shape) + (tuple(int(v) for v in c["sizes"]),) for n, c in cases.items()}
    assert shapes == {"a": (1, 300, 3, (3,)), "b": (2, 37, 1, (0, 5)), "c": (3, 20, 80, (30, 2, 0)), "d": (2, 5, 3, (1, 0)),
                      "e": (2, 20, 2, (0, 0)), "f": (1, 4, 2, (6,)), "g": (1, 300, 3, (3,)), "h": (2, 12, 3, (2, 2)),
                      "i": (1, 8, 2, (2,))}
    by = {n[0]: c for n, c in cases.items()}
    assert "pred_corners" not in by["d"] and all("pred_corners" in by[k] for k in "abcefghi")
    assert int(by["c"]["lens"][0]) == 20 and int(by["f"]["lens"][0]) == 4                     # every query matched
    assert np.array_equal(by["g"]["teacher_corners"], by["g"]["pred_corners"]) and float(by["g"]["loss_ddf"]) == 0.0
    assert list(by["h"]["lens"]) == [6, 6] and float(by["h"]["num_boxes"]) == 12.0            # 3 groups over 2 targets
    assert float(by["e"]["loss_bbox"]) == 0.0 and float(by["e"]["loss_fgl"]) == 0.0 and float(by["e"]["loss_ddf"]) > 0.0


def test_restatement_reproduces_every_golden_case(cases):
    """<= 1e-9 relative where upstream ran in float64; 2e-6 on what its loss_local forced to fp32 (the generator says where),
    given the same fp32 ref_points / target boxes upstream was given"""
    for name, case in cases.items():
        outputs, targets, indices, kw = ref.tensors(case)
        values = ref.terms(outputs, targets, indices, float(case["num_boxes"]), as_recorded=True, **kw)
        grads = ref.weighted_grads(values, outputs)
        fp32 = set(case["fp32_terms"].tolist())
        for k, v in values.items():
            tol = 2e-6 if k in fp32 else 1e-9
            assert abs(float(v.detach()) - float(case[k])) <= tol * max(1.0, abs(float(case[k]))), (name, k, float(v.detach()), float(case[k]))
        for k, g in grads.items():
            g = np.zeros_like(case[k]) if g is None else g.numpy()
            tol = 2e-6 if k in fp32 else 1e-9
            assert np.abs(g - case[k]).max() <= tol * max(np.abs(case[k]).max(), 1e-30), (name, k)


def test_detection_loss_on_cpu_tensors_agrees_with_the_restatement(cases):
    """CPU tensors take detection_loss_torch.  In float64 it is the restatement to 1e-9 (the same expressions; log q by
    log_softmax instead of log(softmax)); in fp32 each term is a sum of at most B * Q * 4 * 33 < 2^17 products of O(1) factors, each
    with a few roundings of 2^-24: the error of the sum is far below 2^17 * 2^-24 < 1e-2 relative in the worst case and grows as
    the square root of the count in practice; 1e-4 of scale is asserted."""
    before = dict(dfine.loss_calls)
    for name, case in cases.items():
        want, want_grads = ref64(case)
        for dtype, tol in ((torch.float64, 1e-9), (torch.float32, 1e-4)):
            outputs, targets, indices, kw = ref.tensors(case, dtype=dtype)
            local = {k: outputs[k] for k in ("pred_corners", "ref_points", "teacher_corners", "teacher_logits") if k in outputs}
            got = dfine.detection_loss(outputs["logits"], outputs["pred_boxes"], targets, indices, float(case["num_boxes"]),
                                       **local, **kw)
            assert list(got) == [k for k in ref.TERMS if k in want]
            for k, v in got.items():
                assert v.dim() == 0 and abs(float(v) - want[k]) <= tol * max(1.0, abs(want[k])), (name, dtype, k, float(v), want[k])
            for k, g in ref.weighted_grads(got, outputs).items():
                g = np.zeros_like(want_grads[k]) if g is None else g.double().numpy()
                assert np.abs(g - want_grads[k]).max() <= tol * max(np.abs(want_grads[k]).max(), 1e-30), (name, dtype, k)
    assert dfine.loss_calls["torch"] == before["torch"] + 2 * len(cases) and dfine.loss_calls["kernel"] == before["kernel"]


def test_detection_loss_refuses_a_partial_local_group(cases):
    case = cases["a_q300"]
    outputs, targets, indices, kw = ref.tensors(case, dtype=torch.float32, requires_grad=False)
    with pytest.raises(ValueError, match="go together"):
        dfine.detection_loss(outputs["logits"], outputs["pred_boxes"], targets, indices, 3.0, alpha=0.75, gamma=2.0,
                             pred_corners=outputs["pred_corners"])
    with pytest.raises(ValueError, match="one target dict"):
        dfine.detection_loss(outputs["logits"], outputs["pred_boxes"], targets, indices + indices, 3.0, alpha=0.75, gamma=2.0)


def synthetic_criterion_inputs(config, B=2, Q=12, sizes=(2, 3), groups=2, seed=0, device="cpu"):
    """an `outputs` dict of the form DFineForObjectDetectionLoss builds: the main output, two auxiliary outputs (one with
    corners, one without) and a denoising group with its meta values"""
    g = torch.Generator().manual_seed(seed)
    C, nb1 = config.num_labels, config.max_num_bins + 1

    def boxes(*lead):
        return torch.cat([torch.rand(*lead, 2, generator=g) * 0.6 + 0.2, torch.rand(*lead, 2, generator=g) * 0.3 + 0.05], -1)

    def output(q, corners):
        out = {"logits": torch.randn(B, q, C, generator=g), "pred_boxes": boxes(B, q)}
        if corners:
            out.update(pred_corners=torch.randn(B, q, 4 * nb1, generator=g), ref_points=boxes(B, q),
                       teacher_corners=torch.randn(B, q, 4 * nb1, generator=g), teacher_logits=torch.randn(B, q, C, generator=g))
        return out

    targets = [{"class_labels": torch.randint(0, C, (n,), generator=g), "boxes": boxes(n)} for n in sizes]
    q_dn = 2 * groups * max(sizes)
    outputs = output(Q, False)
    outputs["auxiliary_outputs"] = [output(Q, True), output(Q, False)]
    outputs["dn_auxiliary_outputs"] = [output(q_dn, True)]
    positive = [torch.cat([torch.arange(n) + 2 * max(sizes) * k for k in range(groups)]) for n in sizes]
    outputs["denoising_meta_values"] = {"dn_positive_idx": positive, "dn_num_group": groups}

    def to(v):
        if torch.is_tensor(v):
            return v.to(device)
        if isinstance(v, dict):
            return {k: to(x) for k, x in v.items()}
        if isinstance(v, list):
            return [to(x) for x in v]
        return v
    return to(outputs), to(targets)


def test_criterion_forward_bound_into_dfine_loss_returns_upstreams_keys_and_values(monkeypatch):
    """fp32 on both sides, the same expressions in another order of operations: 1e-4 of scale, as above"""
    pytest.importorskip("scipy")
    from transformers import DFineConfig
    from transformers.loss.loss_d_fine import DFineLoss
    from transformers.loss.loss_rt_detr import RTDetrLoss
    config = DFineConfig()
    criterion = DFineLoss(config)
    outputs, targets = synthetic_criterion_inputs(config)
    want = criterion(outputs, targets)
    monkeypatch.setattr(RTDetrLoss, "forward", dfine.criterion_forward)
    before = dict(dfine.loss_calls)
    got = criterion(outputs, targets)
    assert dfine.loss_calls["torch"] == before["torch"] + 4
    assert list(got) == list(want)
    assert {k for k in got if "fgl" in k or "ddf" in k} == {"loss_fgl_aux_0", "loss_ddf_aux_0", "loss_fgl_dn_0", "loss_ddf_dn_0"}
    for k in want:
        assert got[k].dim() == 0 and abs(float(got[k]) - float(want[k])) <= 1e-4 * max(1.0, abs(float(want[k]))), (k, got[k], want[k])


def test_loss_entries_reject_bad_arguments_without_a_gpu():
    """Every argument check of m355_dfine_loss_forward / _backward comes before any HIP call: -1 (M355_ERR_INVALID) with a
    message, on fake device pointers that are never dereferenced."""
    from defectdetection_viaobjectdetection_amd import _capi
    fake = ctypes.c_void_p(0x1000)
    err = lambda: _capi.lib.m355_last_error(None)   # noqa: E731
    need = _capi.lib.m355_dfine_loss_workspace_bytes(2, 300)
    assert need == 2 * 75 * 8 * 4 and _capi.lib.m355_dfine_loss_workspace_bytes(1, 5) == 2 * 8 * 4
    names = ("logits", "boxes", "mq", "mt", "offs", "labels", "tboxes", "corners", "ref", "tcorners", "tlogits", "project", "work",
             "out", "saved", "gterms", "gl", "gb", "gc")

    def call(backward=False, B=2, Q=300, C=3, M=4, T=5, num_boxes=5.0, nb1=33, reg_scale=4.0, temp=5.0, work_bytes=need, **null):
        p = {n: (None if null.get(n) is None and n in null else fake) for n in names}
        head = (p["logits"], p["boxes"], B, Q, C, p["mq"], p["mt"], M, p["offs"], p["labels"], p["tboxes"], T, num_boxes, 0.75, 2.0,
                p["corners"], p["ref"], p["tcorners"], p["tlogits"], p["project"], nb1, reg_scale, temp)
        if backward:
            return _capi.lib.m355_dfine_loss_backward(p["gterms"], *head, p["saved"], p["gl"], p["gb"], p["gc"], None)
        return _capi.lib.m355_dfine_loss_forward(*head, p["work"], work_bytes, p["out"], None)

    no_local = dict(corners=None, ref=None, tcorners=None, tlogits=None, project=None)
    for backward in (False, True):
        for kw in (dict(B=0), dict(Q=0), dict(C=0), dict(B=65536, Q=65536)):
            assert call(backward, **kw) == -1 and b"B, Q, C >= 1" in err(), kw
        assert call(backward, M=-1) == -1 and b"M >= 0" in err()
        for name in ("logits", "boxes"):
            assert call(backward, **{name: None}) == -1 and b"null pointer" in err(), name
        assert call(backward, num_boxes=0.0) == -1 and b"num_boxes" in err()
        for name in ("mq", "mt", "offs", "labels", "tboxes"):
            assert call(backward, **{name: None}) == -1 and b"match list or the targets" in err(), name
        for name in no_local:
            assert call(backward, **{name: None}) == -1 and b"all or none" in err(), name
        for kw in (dict(nb1=65), dict(nb1=1), dict(reg_scale=0.0), dict(temp=0.0)):
            assert call(backward, **kw) == -1 and b"bins + 1 <= 64" in err(), kw
    assert call(out=None) == -1 and b"null pointer" in err()
    assert call(work=None) == -1 and b"workspace" in err()
    assert call(work_bytes=need - 1) == -1 and b"workspace" in err()
    assert call(True, saved=None) == -1 and b"null pointer" in err()
    assert call(True, gterms=None) == -1 and b"grad_terms" in err()
    assert call(True, **no_local) == -1 and b"without the local group" in err()
    # nothing asked of the backward, and an empty match list with NULL match pointers, pass the checks without a launch
    assert call(True, gl=None, gb=None, gc=None) == 0
    assert call(True, M=0, mq=None, mt=None, offs=None, gl=None, gb=None, gc=None) == 0
