"""The temporal-head ops without a GPU: the torch restatements of tests/dfine_temporal_ref.py against transformers' own functions
and against the guard table, the C entries' refusals before any device work, and the CPU fallbacks of the Python layer."""
import ctypes as C

import pytest
import torch

import dfine_temporal_ref as ref

NAN, INF = float("nan"), float("inf")


def _randn(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


@pytest.mark.parametrize("clamp01", [False, True])
def test_refs_equal_the_chain_of_transformers_functions(clamp01):
    """float64 on the CPU: the restated integral, distance2bbox and the guarded chain against DFineIntegral, distance2bbox and
    weighting_function of transformers, on inputs with planted non-finite logits and a NaN reference point"""
    M = pytest.importorskip("transformers.models.d_fine.modeling_d_fine")
    from transformers import DFineConfig
    bins, reg_scale = 32, 4.0
    project = M.weighting_function(bins, torch.tensor([0.5], dtype=torch.float64), torch.tensor([reg_scale], dtype=torch.float64))
    corners, points = _randn((2, 7, 4 * (bins + 1)), 1), torch.rand(2, 7, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    upstream_integral = M.DFineIntegral(DFineConfig(max_num_bins=bins))
    assert torch.equal(ref.integral(corners, project), upstream_integral(corners, project))
    assert torch.equal(ref.distance2bbox(points, ref.integral(corners, project), reg_scale),
                       M.distance2bbox(points, upstream_integral(corners, project), reg_scale))
    corners[0, 0, 3], corners[0, 1, 40], corners[1, 2, 70], points[1, 3, 0] = NAN, INF, -INF, NAN
    for guard in (False, True):
        mine = ref.decode_boxes(corners, project, points, reg_scale, clamp01, guard)
        theirs = ref.decode_boxes(corners, project, points, reg_scale, clamp01, guard, upstream_integral, M.distance2bbox)
        assert torch.equal(torch.nan_to_num(mine, nan=-7.0), torch.nan_to_num(theirs, nan=-7.0))
        assert guard == bool(torch.isfinite(mine).all())


def test_refs_reproduce_the_guard_table():
    x = torch.tensor(ref.LOGIT_TABLE[0], requires_grad=True)
    out = ref.guard_logits(x)
    out.sum().backward()
    assert torch.equal(out.detach(), torch.tensor(ref.LOGIT_TABLE[1])) and torch.equal(x.grad, torch.tensor(ref.LOGIT_TABLE[2]))
    b = torch.tensor(ref.BOX_TABLE[0], requires_grad=True)
    out = ref.guard_boxes(b)
    out.sum().backward()
    assert torch.equal(out.detach(), torch.tensor(ref.BOX_TABLE[1])) and torch.equal(b.grad, torch.tensor(ref.BOX_TABLE[2]))
    # the anomaly scores reach all but the last column, and receive the gradient of their columns
    cls = torch.tensor([[19.0, NAN, 1.0], [-19.5, 2.0, 19.0]], requires_grad=True)
    an = torch.tensor([[2.0, 1.0], [-0.5, INF]], requires_grad=True)
    out = ref.guard_logits(cls, an)
    out.sum().backward()
    assert torch.equal(out.detach(), torch.tensor([[20.0, 0.0, 1.0], [-20.0, 20.0, 19.0]]))
    assert torch.equal(cls.grad, torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0]])) and torch.equal(an.grad, cls.grad[:, :2])


def test_guarded_decode_reference_sends_exact_zeros_into_replaced_logits():
    project = torch.linspace(-2, 2, 5, dtype=torch.float64)
    corners, points = _randn((3, 20), 3).requires_grad_(), (torch.rand(3, 4, dtype=torch.float64) * 0.4 + 0.2)
    with torch.no_grad():
        corners[0, 1], corners[1, 7], corners[2, 19] = NAN, INF, -INF
    ref.decode_boxes(corners, project, points, 4.0, True, True).sum().backward()
    for i, k in ((0, 1), (1, 7), (2, 19)):
        assert float(corners.grad[i, k]) == 0.0
    assert torch.isfinite(corners.grad).all() and int((corners.grad == 0).sum()) < corners.numel() // 2


def test_reference_losses_against_closed_forms():
    a = _randn((4, 3, 2), 5)
    want = ((a[1:] - a[:-1]) ** 2).mean(dim=(1, 2)).sum() / 3
    assert abs(float(ref.consistency_loss(a) - want)) < 1e-14 and float(ref.consistency_loss(a[:1])) == 0.0
    x = _randn((2, 5, 3), 6)
    want = (torch.logsumexp(x, -1) - x[..., 2]).mean(-1)
    assert float((ref.noobject_loss(x) - want).abs().max()) < 1e-14


def test_entries_refuse_bad_arguments_before_any_device_work():
    """null pointers, T, Q or D <= 0 and limits exceeded come back as M355_ERR_INVALID (-1); the pointers are fake and never read"""
    from defectdetection_viaobjectdetection_amd import _capi
    lib, fake = _capi.lib, C.c_void_p(0x1000)
    fuse_f = lambda T=50, Q=300, D=256, f=fake, s=fake, o=fake: lib.m355_dfine_temporal_fuse_forward(f, s, None, T, Q, D, o, None, None)  # noqa: E731
    fuse_b = lambda T=50, Q=300, D=256, g=fake, f=fake, st=fake, ds=fake: lib.m355_dfine_temporal_fuse_backward(  # noqa: E731
        g, f, fake, st, T, Q, D, fake, ds, None)
    for call in (fuse_f, fuse_b):
        assert call(T=0) == -1 and call(Q=0) == -1 and call(D=0) == -1 and call(T=-3) == -1
        assert call(T=1025) == -1 and call(D=1025) == -1 and call(Q=(1 << 20) + 1) == -1
        assert b"temporal_fuse" in lib.m355_last_error(None)
    assert fuse_f(f=None) == -1 and fuse_f(s=None) == -1 and fuse_f(o=None) == -1
    assert fuse_b(g=None) == -1 and fuse_b(st=None) == -1 and fuse_b(f=None) == -1   # grad_scores needs fused

    guard_f = lambda rows=10, C1=3, c=fake, a=None, b=20.0, o=fake: lib.m355_dfine_guard_logits_forward(c, a, rows, C1, b, o, None)  # noqa: E731
    guard_b = lambda rows=10, C1=3, g=fake, c=fake, a=None, da=None: lib.m355_dfine_guard_logits_backward(  # noqa: E731
        g, c, a, rows, C1, 20.0, fake, da, None)
    assert guard_f(rows=0) == -1 and guard_f(C1=0) == -1 and guard_f(rows=(1 << 40) // 3 + 1) == -1 and guard_f(b=-1.0) == -1
    assert guard_f(c=None) == -1 and guard_f(o=None) == -1 and guard_f(C1=1, a=fake) == -1 and guard_f(b=NAN) == -1
    assert guard_b(rows=0) == -1 and guard_b(g=None) == -1 and guard_b(c=None) == -1 and guard_b(da=fake) == -1   # grad_anomaly alone

    noobj_f = lambda T=5, Q=300, C1=3, c=2, x=fake, o=fake: lib.m355_dfine_noobject_loss_forward(x, T, Q, C1, c, o, None)  # noqa: E731
    noobj_b = lambda T=5, Q=300, C1=3, c=2, g=fake, x=fake, d=fake: lib.m355_dfine_noobject_loss_backward(g, x, T, Q, C1, c, d, None)  # noqa: E731
    for call in (noobj_f, noobj_b):
        assert call(T=0) == -1 and call(Q=0) == -1 and call(C1=0) == -1 and call(Q=2049) == -1 and call(C1=1025) == -1
        assert call(c=3) == -1 and call(c=-1) == -1 and call(x=None) == -1
    assert noobj_f(o=None) == -1 and noobj_b(g=None) == -1 and noobj_b(d=None) == -1

    cons_f = lambda T=50, N=600, a=fake, w=fake, nbytes=1 << 20, o=fake: lib.m355_dfine_consistency_loss_forward(a, T, N, w, nbytes, o, None)  # noqa: E731
    cons_b = lambda T=50, N=600, g=fake, a=fake, d=fake: lib.m355_dfine_consistency_loss_backward(g, a, T, N, d, None)  # noqa: E731
    for call in (cons_f, cons_b):
        assert call(T=1) == -1 and call(T=0) == -1 and call(N=0) == -1 and call(N=(1 << 27) + 1) == -1 and call(T=1 << 12, N=1 << 20) == -1
        assert call(a=None) == -1
    assert cons_f(o=None) == -1 and cons_f(w=None) == -1 and cons_f(nbytes=49 * 4 - 1) == -1 and cons_b(g=None) == -1 and cons_b(d=None) == -1
    assert lib.m355_dfine_consistency_workspace_bytes(50, 600) == 49 * 4 and lib.m355_dfine_consistency_workspace_bytes(50, 4097) == 49 * 8
    assert lib.m355_dfine_consistency_workspace_bytes(1, 600) == 0

    dec_f = lambda n=4, nb1=33, rs=4.0, d=fake: lib.m355_dfine_decode_guarded(d, fake, fake, fake, n, nb1, rs, 1, None)  # noqa: E731
    dec_b = lambda n=4, nb1=33, rs=4.0, d=fake: lib.m355_dfine_decode_guarded_backward(fake, d, fake, fake, fake, None, n, nb1, rs, 1, None)  # noqa: E731
    for call in (dec_f, dec_b):
        assert call(n=-1) == -1 and call(nb1=1) == -1 and call(rs=0.0) == -1 and call(n=1 << 40) == -1 and call(d=None) == -1


def test_cpu_tensors_take_the_torch_expressions_and_the_counter_says_so():
    from defectdetection_viaobjectdetection_amd import dfine
    before = dict(dfine.temporal_calls)
    f, s, c = _randn((5, 3, 6), 10, torch.float32), _randn((5, 3, 1), 11, torch.float32), _randn((5, 3, 6), 12, torch.float32)
    assert torch.equal(dfine.temporal_fuse(f, s, c), ref.temporal_fuse(f, s, c))
    assert torch.equal(dfine.temporal_fuse(f, s[..., 0]), ref.temporal_fuse(f, s))
    cls, an = torch.tensor([ref.LOGIT_TABLE[0]]), _randn((1, 7), 13, torch.float32)
    assert torch.equal(dfine.guard_logits(cls), torch.tensor([ref.LOGIT_TABLE[1]]))
    assert torch.equal(dfine.guard_logits(cls, an), ref.guard_logits(cls, an))
    project = torch.linspace(-2, 2, 5)
    corners, points = _randn((2, 3, 20), 14, torch.float32), torch.rand(2, 3, 4)
    corners[0, 0, 0], points[1, 1, 1] = NAN, NAN
    assert torch.equal(dfine.decode_boxes(corners, project, points, 4.0, clamp01=True, guard=True),
                       ref.decode_boxes(corners, project, points, 4.0, True, True))
    x = _randn((3, 4, 5), 15, torch.float32)
    assert torch.equal(dfine.noobject_loss(x), ref.noobject_loss(x)) and torch.equal(dfine.noobject_loss(x, 0), ref.noobject_loss(x, 0))
    assert torch.equal(dfine.consistency_loss(x), ref.consistency_loss(x)) and float(dfine.consistency_loss(x[:1])) == 0.0
    heads = [torch.nn.Linear(6, n) for n in (3, 20, 2)]
    got = dfine.temporal_head(f, torch.rand(5, 3, 4), heads[0], heads[1], project, 4.0, scores=s, context=c, anomaly_head=heads[2])
    assert got[0].shape == (5, 3, 3) and got[1].shape == (5, 3, 4) and got[2].shape == (5, 3, 2)
    after = dfine.temporal_calls
    assert after["kernel"] == before["kernel"] and after["torch"] == before["torch"] + 12   # 9 calls above, 3 inside temporal_head
    with pytest.raises(ValueError):
        dfine.temporal_fuse(f, s[:4])
    with pytest.raises(ValueError):
        dfine.guard_logits(cls, an[:, :3])
    with pytest.raises(IndexError):
        dfine.noobject_loss(x, 5)
    with pytest.raises(ValueError):
        dfine.temporal_head(f, torch.rand(5, 3, 4), heads[0], heads[1], project, 4.0, context=c)
    with pytest.raises(RuntimeError, match="CUDA"):   # guard=False keeps the old behaviour: no CPU path
        dfine.decode_boxes(corners, project, points, 4.0)
