"""The optimizer step of the D-FINE trainers without a GPU: the float64 restatement (tests/dfine_optim_ref.py) against torch's
own CPU Adam / AdamW + clip_grad_norm_, and the host validation of the three C entries."""
import ctypes
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import dfine_optim_ref as ref

STEPS, T_MAX = 5, 8
GROUPS = [dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8),
          dict(lr=3e-4, weight_decay=0.05, betas=(0.8, 0.99), eps=1e-6),
          dict(lr=2e-4, weight_decay=0.0, betas=(0.4, 0.95), eps=1e-7)]
SHAPES = [(5,), (3, 4), (17,), (2, 3, 2), (9,), (1,), (6,)]
GROUP_OF = [0, 1, 2, 0, 1, 2, 0]
ALTERNATING = (1, 4)      # gradient None on odd steps
FROZEN = 6                # requires_grad=False: never a gradient


def _gradient(i, k, rng):
    if i == FROZEN or (i in ALTERNATING and k % 2 == 1):
        return None
    return (rng.standard_normal(SHAPES[i]) * 0.7).astype(np.float32)


@pytest.mark.parametrize("adamw", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["plain", "clip"])
def test_float64_restatement_matches_torch_cpu(adamw, max_norm):
    rng = np.random.default_rng(11)
    values = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    params = [torch.nn.Parameter(torch.from_numpy(v.copy()), requires_grad=i != FROZEN) for i, v in enumerate(values)]
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls([dict(params=[p for p, g in zip(params, GROUP_OF) if g == j], **h) for j, h in enumerate(GROUPS)])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_MAX)
    model = ref.AdamRef(values, GROUP_OF, GROUPS, adamw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for k in range(STEPS):
            grads = [_gradient(i, k, rng) for i in range(len(SHAPES))]
            for p, g in zip(params, grads):
                p.grad = None if g is None else torch.from_numpy(g.copy())
            for j, h in enumerate(GROUPS):
                model.groups[j]["lr"] = ref.cosine_lr(h["lr"], k, T_MAX)
                assert math.isclose(opt.param_groups[j]["lr"], model.groups[j]["lr"], rel_tol=1e-12)
            want_norm = model.step(grads, max_norm)
            if max_norm is not None:
                got_norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
                assert math.isclose(float(got_norm), want_norm, rel_tol=1e-5)
            opt.step()
            sched.step()
    for i, p in enumerate(params):
        st = opt.state.get(p, {})
        assert (int(st["step"]) if st else 0) == model.t[i], i
        np.testing.assert_allclose(p.detach().numpy(), model.p[i], rtol=1e-5, atol=0, err_msg=f"p {i}")
        if st:
            np.testing.assert_allclose(st["exp_avg"].numpy(), model.m[i], rtol=1e-5, atol=1e-12, err_msg=f"m {i}")
            np.testing.assert_allclose(st["exp_avg_sq"].numpy(), model.v[i], rtol=1e-5, atol=0, err_msg=f"v {i}")
        else:
            assert not model.m[i].any() and not model.v[i].any() and np.array_equal(model.p[i], values[i].astype(np.float64))
    assert model.t == [5, 3, 5, 5, 3, 5, 0]


def test_clip_coefficient_keeps_nan_and_zeroes_on_inf():
    assert ref.clip_coefficient(0.5, 1.0) == 1.0
    assert ref.clip_coefficient(math.inf, 1.0) == 0.0
    assert math.isnan(ref.clip_coefficient(math.nan, 1.0))
    assert ref.total_norm([np.array([3.0], np.float32), None, np.array([[4.0]], np.float32)]) == 5.0


def _table(rows):
    from defectdetection_viaobjectdetection_amd import _capi
    t = (_capi.DfineOptimRow * len(rows))()
    chunk0 = 0
    for r, (numel, ptrs) in zip(t, rows):
        r.p, r.g, r.m, r.v = ptrs
        r.numel, r.chunk0 = numel, min(chunk0, 2 ** 31 - 1)
        r.lr, r.beta1, r.beta2, r.eps, r.step_size, r.bc2_sqrt = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.03
        r.one_minus_beta1, r.one_minus_beta2, r.decay = 0.1, 0.001, 1.0
        chunk0 += (max(numel, 0) + _capi.DFINE_OPTIM_CHUNK - 1) // _capi.DFINE_OPTIM_CHUNK
    return t


def test_optimizer_entries_reject_bad_arguments_without_a_gpu():
    """The three entries validate on the host before any HIP call: -1 (M355_ERR_INVALID) and a message; the device pointers are
    fakes that are never dereferenced."""
    from defectdetection_viaobjectdetection_amd import _capi
    lib, fake = _capi.lib, ctypes.c_void_p(0x10000)
    good = (0x20000, 0x30000, 0x40000, 0x50000)

    def calls(table, count, h=True, d=True, only=None):
        """the status of every entry (or of those in `only`) for this table.  Every call made here must be one the entry refuses:
        an accepted call would launch on these fake pointers where there is a GPU."""
        hp = ctypes.cast(table, ctypes.c_void_p) if h else None
        dp = fake if d else None
        entries = {"grad_sumsq": lambda: lib.m355_dfine_grad_sumsq_launch(hp, dp, count, fake, 1 << 40, None),
                   "clip_scale": lambda: lib.m355_dfine_clip_scale_launch(hp, dp, count, fake, 1 << 40, 1.0, fake, None),
                   "adam": lambda: lib.m355_dfine_adam_launch(hp, dp, count, _capi.DFINE_OPTIM_ADAMW, fake, 1 << 40, 1.0, fake, None)}
        return {name: call() for name, call in entries.items() if only is None or name in only}

    def refused(rcs, text):
        for name, rc in rcs.items():
            assert rc == -1, (name, rc, text)
        msg = lib.m355_last_error(None)
        assert text in msg, (msg, text)

    ok = _table([(5, good), (4097, good)])
    refused(calls(ok, 2, h=False), b"null table")
    refused(calls(ok, 2, d=False), b"null table")
    for count in (0, -1, _capi.DFINE_OPTIM_MAX_TENSORS + 1):
        refused(calls(ok, count), b"tensor count")
    refused(calls(_table([(5, good), (-1, good)]), 2), b"negative numel")
    for role in range(4):
        for off in (1, 2, 3):
            ptrs = list(good)
            ptrs[role] += off
            refused(calls(_table([(5, tuple(ptrs))]), 1), b"4-byte aligned")
    refused(calls(_table([(5, (good[0], None, good[2], good[3]))]), 1), b"null pointer")
    # p, m, v are the update's alone: the other two entries take such a row, so only the update is called with it
    for role in (0, 2, 3):
        ptrs = list(good)
        ptrs[role] = None
        refused(calls(_table([(5, tuple(ptrs))]), 1, only=("adam",)), b"null pointer")
    # 2^31 chunks: one more than a launch can index, as one tensor and as the sum of two
    cap = (2 ** 31 - 1) * _capi.DFINE_OPTIM_CHUNK
    refused(calls(_table([(cap + 1, good)]), 1), b"more chunks")
    refused(calls(_table([(cap, good), (1, good)]), 2), b"more chunks")
    refused(calls(_table([(2 ** 62, good)]), 1), b"more chunks")
    bad_prefix = _table([(5, good), (5, good)])
    bad_prefix[1].chunk0 = 0
    refused(calls(bad_prefix, 2), b"chunk0")
    refused(calls(_table([(0, good)]), 1), b"no elements")
    # the arguments beside the table
    hp = ctypes.cast(ok, ctypes.c_void_p)
    assert lib.m355_dfine_grad_sumsq_launch(hp, fake, 2, None, 3, None) == -1 and b"partials" in lib.m355_last_error(None)
    assert lib.m355_dfine_grad_sumsq_launch(hp, fake, 2, fake, 2, None) == -1 and b"partials" in lib.m355_last_error(None)
    assert lib.m355_dfine_clip_scale_launch(hp, fake, 2, fake, 3, 1.0, None, None) == -1 and b"norm" in lib.m355_last_error(None)
    assert lib.m355_dfine_adam_launch(hp, fake, 2, 2, None, 0, 0.0, None, None) == -1 and b"mode" in lib.m355_last_error(None)
    assert lib.m355_dfine_adam_launch(hp, fake, 2, 1, fake, 3, 1.0, None, None) == -1 and b"together" in lib.m355_last_error(None)
    assert lib.m355_dfine_adam_launch(hp, fake, 2, 1, fake, 2, 1.0, fake, None) == -1 and b"partials" in lib.m355_last_error(None)
    assert lib.m355_dfine_adam_launch(hp, fake, 2, 1, ctypes.c_void_p(0x10002), 3, 1.0, fake, None) == -1
    assert b"4-byte aligned" in lib.m355_last_error(None)
    assert lib.m355_dfine_adam_launch(hp, fake, 2, 1, fake, 3, 1.0, ctypes.c_void_p(0x10004), None) == -1
    assert b"8-byte aligned" in lib.m355_last_error(None)


def test_row_layout_is_the_header_one():
    from defectdetection_viaobjectdetection_amd import _capi, dfine
    assert ctypes.sizeof(_capi.DfineOptimRow) == dfine._OPTIM_ROW.itemsize == 96
    for name, _ in _capi.DfineOptimRow._fields_:
        assert getattr(_capi.DfineOptimRow, name).offset == dfine._OPTIM_ROW.fields[name][1], name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355yolo.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"#define M355_(DFINE_OPTIM_\w+) (\d+)", header)}
    assert macros == {"DFINE_OPTIM_CHUNK": _capi.DFINE_OPTIM_CHUNK, "DFINE_OPTIM_MAX_TENSORS": _capi.DFINE_OPTIM_MAX_TENSORS,
                      "DFINE_OPTIM_ADAM": _capi.DFINE_OPTIM_ADAM, "DFINE_OPTIM_ADAMW": _capi.DFINE_OPTIM_ADAMW}


def test_unbindable_optimizers_come_back_untouched_on_the_host():
    from defectdetection_viaobjectdetection_amd import dfine
    p = torch.nn.Parameter(torch.zeros(3))
    for opt in (torch.optim.AdamW([p]), torch.optim.Adam([p]), torch.optim.SGD([p], lr=0.1)):
        assert dfine.bind_optimizer(opt, max_norm=1.0) is opt
        assert "step" not in vars(opt) and not hasattr(opt, "_m355_optim")
