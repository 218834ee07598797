"""The temporal-head ops on the GPU (csrc/dfine_temporal.hip and the guarded instances of the decode kernels): dfine.temporal_fuse,
guard_logits, decode_boxes(guard=True), noobject_loss, consistency_loss, temporal_head and their gradients.

Every output and gradient tensor is held to the float64 restatement of tests/dfine_temporal_ref.py on the CPU by the project's
standing rule: max |kernel - ref64| <= 2 * max |torch fp32 on this device - ref64| + 1e-6 * max |ref64|, where "torch fp32" is the
same restatement in fp32 on the GPU and the float64 inputs are the fp32 inputs widened.  Where one rounding per element decides the
result (guard_logits, an idle guard of the decode) the comparison is of bits."""
import copy
import itertools

import pytest
import torch

import dfine_temporal_ref as ref

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def _judge(name, kernel, torch32, want, failures):
    w = want.detach().double().cpu()
    e_k = float((kernel.detach().double().cpu() - w).abs().max())
    e_t = float((torch32.detach().double().cpu() - w).abs().max())
    scale = float(w.abs().max())
    print(f"{name}: max error vs float64: kernel {e_k:.3e}, torch fp32 {e_t:.3e} (max |ref| {scale:.4g})")
    assert tuple(kernel.shape) == tuple(w.shape), name
    if not e_k <= 2 * e_t + 1e-6 * scale:
        failures.append((name, e_k, e_t, scale))


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _three_ways(fn_kernel, fn_ref, inputs, gw, dev, leaves=None):
    """(out, grads of `leaves` (indices into inputs; default all)) of the kernel, of torch fp32 on the device, of float64 on the CPU;
    an input that is None stays None"""
    res = []
    for kind in ("kernel", "torch", "ref64"):
        to = (lambda t: t.double()) if kind == "ref64" else (lambda t: t.to(dev))
        ts = [None if t is None else to(t) for t in inputs]
        want = [i for i in range(len(ts)) if ts[i] is not None] if leaves is None else list(leaves)
        for i in want:
            ts[i].requires_grad_()
        out = (fn_kernel if kind == "kernel" else fn_ref)(*ts)
        grads = torch.autograd.grad((out * gw.to(out.device, out.dtype)).sum(), [ts[i] for i in want]) if want else ()
        res.append((out,) + tuple(grads))
    return res


def _check_three_ways(tag, names, res):
    failures = []
    for name, k, t, w in zip(names, *res):
        assert k.is_cuda and k.dtype == torch.float32 and torch.isfinite(k).all(), name
        _judge(f"{tag} {name}", k, t, w, failures)
    assert not failures, failures


def _packs(fn):
    """how many tensors autograd saved while fn ran"""
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(1) or t, lambda t: t):
        out = fn()
    return len(saved), out


# ---- temporal_fuse ---------------------------------------------------------------------------------------------------------------
FUSE_NAMES = ("dfused", "dscores", "dcontext")


def _fuse_inputs(T, Q, D, with_context):
    return [_randn((T, Q, D), T + Q + D), 2.0 * _randn((T, Q, 1), T + Q + D + 1), _randn((T, Q, D), T + Q + D + 2) if with_context else None]


# one frame; a 16-byte path of two frames; the trainers' T and D with a last chunk of 2 frames; more frames than a backward pass of
# the block holds and D = 260 (two trips of the lanes, the second partial); D % 4 != 0: the 4-byte instance
@pytest.mark.parametrize("with_context", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 4), (2, 3, 256), (50, 7, 256), (65, 2, 260), (5, 3, 6)])
def test_temporal_fuse(cuda_device, shape, with_context):
    from defectdetection_viaobjectdetection_amd import dfine
    inputs, gw = _fuse_inputs(*shape, with_context), _randn(shape, 9)
    before = dict(dfine.temporal_calls)
    n = 3 if with_context else 2
    subsets = [s for r in range(1, n + 1) for s in itertools.combinations(range(n), r)]
    for leaves in subsets:
        res = _three_ways(dfine.temporal_fuse, ref.temporal_fuse, inputs, gw, cuda_device, leaves)
        _check_three_ways(f"temporal_fuse {shape} context={with_context} leaves={leaves}", ("out",) + tuple(FUSE_NAMES[i] for i in leaves), res)
    assert dfine.temporal_calls["torch"] == before["torch"] and dfine.temporal_calls["kernel"] == before["kernel"] + len(subsets)
    # scores as (T, Q) give the bits of (T, Q, 1), and the gradient takes their shape
    f, s = inputs[0].to(cuda_device), inputs[1].to(cuda_device)
    s2 = s[..., 0].clone().requires_grad_()
    out = dfine.temporal_fuse(f, s2)
    assert _bits(out, dfine.temporal_fuse(f, s))
    assert torch.autograd.grad(out.sum(), s2)[0].shape == s2.shape


def test_temporal_fuse_underflowing_weights(cuda_device):
    """a column whose scores spread over 200: most of its weights underflow to 0 and one frame carries the column"""
    from defectdetection_viaobjectdetection_amd import dfine
    T, Q, D = 50, 7, 256
    inputs, gw = _fuse_inputs(T, Q, D, True), _randn((T, Q, D), 9)
    inputs[1][:, 2, 0] = torch.linspace(-100.0, 100.0, T)[torch.randperm(T, generator=torch.Generator().manual_seed(1))]
    res = _three_ways(dfine.temporal_fuse, ref.temporal_fuse, inputs, gw, cuda_device)
    _check_three_ways("temporal_fuse spread 200", ("out",) + FUSE_NAMES, res)
    assert int((res[0][0][:, 2] == inputs[2].to(cuda_device)[:, 2]).all(dim=-1).sum()) >= T // 3   # weight 0: the context alone


def test_temporal_fuse_one_frame_has_no_score_gradient(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    f, s, c = (t.to(cuda_device).requires_grad_() for t in _fuse_inputs(1, 5, 256, True))
    out = dfine.temporal_fuse(f, s, c)
    d_f, d_s = torch.autograd.grad((out * _randn((1, 5, 256), 3).to(cuda_device)).sum(), [f, s])
    assert _bits(out, f + c) and int((d_s != 0).sum()) == 0 and d_f.abs().max() > 0


def test_temporal_fuse_column_alone_and_twice(cuda_device):
    """column q of a (50, 7, 256) call and the same column as a call of its own give equal bits, outputs and gradients; so do two
    runs of the whole call"""
    from defectdetection_viaobjectdetection_amd import dfine
    T, Q, D = 50, 7, 256
    inputs, gw = [t.to(cuda_device) for t in _fuse_inputs(T, Q, D, True)], _randn((T, Q, D), 9).to(cuda_device)

    def run(f, s, c, g):
        f, s, c = (t.clone().contiguous().requires_grad_() for t in (f, s, c))
        out = dfine.temporal_fuse(f, s, c)
        return (out,) + torch.autograd.grad((out * g).sum(), [f, s, c])

    whole, again = run(*inputs, gw), run(*inputs, gw)
    for a, b in zip(whole, again):
        assert _bits(a, b)
    for q in (0, 3, 6):
        alone = run(*(t[:, q:q + 1] for t in inputs), gw[:, q:q + 1])
        for name, a, b in zip(("out",) + FUSE_NAMES, whole, alone):
            assert _bits(a[:, q:q + 1], b), (q, name)


def test_temporal_fuse_saves_nothing_without_a_gradient(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    f, s, c = (t.to(cuda_device) for t in _fuse_inputs(5, 3, 8, True))
    n, plain = _packs(lambda: dfine.temporal_fuse(f, s, c))
    assert n == 0 and plain.grad_fn is None
    with torch.no_grad():
        n, off = _packs(lambda: dfine.temporal_fuse(f.clone().requires_grad_(), s, c))
    assert n == 0 and off.grad_fn is None and _bits(off, plain)
    n, on = _packs(lambda: dfine.temporal_fuse(f.clone().requires_grad_(), s, c))
    assert n == 2 and on.grad_fn is not None and _bits(on.detach(), plain)   # the scores and the column statistics, not fused
    assert _packs(lambda: dfine.temporal_fuse(f, s.clone().requires_grad_(), c))[0] == 3


# ---- guard_logits ----------------------------------------------------------------------------------------------------------------
def _guard_both(cls, an, gw, dev):
    """(out, dcls[, danomaly]) of dfine.guard_logits and of the torch expression in fp32 on the device"""
    from defectdetection_viaobjectdetection_amd import dfine
    res = []
    for fn in (dfine.guard_logits, ref.guard_logits):
        ts = [t.to(dev).requires_grad_() for t in ((cls,) if an is None else (cls, an))]
        out = fn(*ts)
        res.append((out,) + torch.autograd.grad((out * gw.to(dev)).sum(), ts))
    return res


@pytest.mark.parametrize("with_anomaly", [False, True])
@pytest.mark.parametrize("rows", [1, 15000])
@pytest.mark.parametrize("C1", [2, 3, 81])
def test_guard_logits_bits(cuda_device, C1, rows, with_anomaly):
    """random logits of standard deviation 12: about a tenth lie beyond +-20"""
    cls, gw = 12.0 * _randn((rows, C1), rows + C1), _randn((rows, C1), 4)
    an = _randn((rows, C1 - 1), rows + C1 + 1) if with_anomaly else None
    got, want = _guard_both(cls, an, gw, cuda_device)
    for name, a, b in zip(("out", "dcls", "danomaly"), got, want):
        assert _bits(a, b), name
    if rows > 1:
        clamped = float((got[0].abs() == 20.0).float().mean())
        assert 0.05 < clamped < 0.2 and float((got[1] == 0).float().mean()) == pytest.approx(clamped, abs=1e-3)


@pytest.mark.parametrize("with_anomaly", [False, True])
def test_guard_logits_table(cuda_device, with_anomaly):
    cls, gw = torch.tensor([ref.LOGIT_TABLE[0], ref.LOGIT_TABLE[0][::-1]]), torch.ones(2, 8)
    an = torch.zeros(2, 7) if with_anomaly else None
    got, want = _guard_both(cls, an, gw, cuda_device)
    for name, a, b in zip(("out", "dcls", "danomaly"), got, want):
        assert _bits(a, b), name
    assert torch.equal(got[0][0].cpu(), torch.tensor(ref.LOGIT_TABLE[1])) and torch.equal(got[1][0].cpu(), torch.tensor(ref.LOGIT_TABLE[2]))
    if with_anomaly:
        assert torch.equal(got[2][0].cpu(), torch.tensor(ref.LOGIT_TABLE[2][:7]))


def test_guard_logits_leading_dims_and_no_grad(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    cls, an = (12.0 * _randn((4, 10, 3), 1)).to(cuda_device), _randn((4, 10, 2), 2).to(cuda_device)
    n, plain = _packs(lambda: dfine.guard_logits(cls, an))
    assert n == 0 and plain.grad_fn is None and _bits(plain, ref.guard_logits(cls, an))
    with torch.no_grad():
        n, off = _packs(lambda: dfine.guard_logits(cls.clone().requires_grad_(), an))
    assert n == 0 and off.grad_fn is None and _bits(off, plain)
    a = an.clone().requires_grad_()   # the anomaly scores alone under autograd
    d_a, = torch.autograd.grad(dfine.guard_logits(cls, a).sum(), a)
    a2 = an.clone().requires_grad_()
    assert _bits(d_a, torch.autograd.grad(ref.guard_logits(cls, a2).sum(), a2)[0])


# ---- decode_boxes(guard=True) --------------------------------------------------------------------------------------------------
REG_SCALE = 4.0


def _decode_inputs(n, nb1):
    from defectdetection_viaobjectdetection_amd import dfine
    project = dfine.weighting_function(nb1 - 1, torch.tensor([0.5]), REG_SCALE) if nb1 > 5 else torch.linspace(-2.0, 2.0, nb1)
    return 2.0 * _randn((n, 4 * nb1), n + nb1), project.float(), _rand((n, 4), n + nb1 + 1), _randn((n, 4), n + nb1 + 2)


@pytest.mark.parametrize("clamp01", [False, True])
@pytest.mark.parametrize("n", [1, 129])
@pytest.mark.parametrize("nb1", [5, 33])
def test_idle_guard_changes_no_bit(cuda_device, nb1, n, clamp01):
    """finite inputs (reference points over all of [0, 1]: some coordinates clamp): guard=True gives the bits of guard=False"""
    from defectdetection_viaobjectdetection_amd import dfine
    corners, project, points, gw = (t.to(cuda_device) for t in _decode_inputs(n, nb1))
    res = []
    for guard in (False, True):
        c, p = corners.clone().requires_grad_(), points.clone().requires_grad_()
        out = dfine.decode_boxes(c, project, p, REG_SCALE, clamp01, guard=guard)
        res.append((out,) + torch.autograd.grad((out * gw).sum(), [c, p]))
        assert _bits(dfine.decode_boxes(corners, project, points, REG_SCALE, clamp01, guard=guard), out)   # the no-grad path
    for name, a, b in zip(("boxes", "dcorners", "dpoints"), *res):
        assert _bits(a, b), name


@pytest.mark.parametrize("clamp01", [False, True])
@pytest.mark.parametrize("n", [1, 129])
@pytest.mark.parametrize("nb1", [5, 33])
def test_guarded_decode_with_planted_values(cuda_device, nb1, n, clamp01):
    """NaN, +inf and -inf among the logits and a NaN centre among the reference points.  The replaced coordinates (cx and w of the
    box with the NaN centre) are exactly 0.5, the planted logits and everything behind the replaced coordinates receive exactly 0,
    and every tensor as a whole keeps the three-way rule (no value of the float64 reference is non-finite)."""
    from defectdetection_viaobjectdetection_amd import dfine
    corners, project, points, gw = _decode_inputs(n, nb1)
    points = 0.2 + 0.4 * points                       # inside the image, so that most coordinates carry a gradient
    rows = [0, n // 3, n // 2, n - 1]                 # one box takes all four when n == 1
    planted = [(rows[0], 3, NAN), (rows[1], nb1 + 1, INF), (rows[2], 2 * nb1, -INF)]
    for i, k, v in planted:
        corners[i, k] = v
    points[rows[3], 0] = NAN
    res = _three_ways(lambda c, p: dfine.decode_boxes(c, project.to(cuda_device), p, REG_SCALE, clamp01, guard=True),
                      lambda c, p: ref.decode_boxes(c, project.to(c.device, c.dtype), p, REG_SCALE, clamp01, True), [corners, points], gw,
                      cuda_device)
    assert all(torch.isfinite(t).all() for t in res[2])
    _check_three_ways(f"decode_boxes guard n={n} bins+1={nb1} clamp01={clamp01}", ("boxes", "dcorners", "dpoints"), res)
    boxes, d_c, d_p = (t.detach() for t in res[0])
    k = rows[3]
    assert float(boxes[k, 0]) == 0.5 and float(boxes[k, 2]) == 0.5
    assert float(res[2][0].detach()[k, 0]) == 0.5 and float(res[2][0].detach()[k, 2]) == 0.5
    for i, j, _ in planted:
        assert float(d_c[i, j]) == 0.0 and float(res[2][1][i, j]) == 0.0, (i, j)
    assert float(d_p[k, 0]) == 0.0 and float(d_p[k, 2]) == 0.0
    assert int((d_c[k, :nb1] != 0).sum()) == 0 and int((d_c[k, 2 * nb1:3 * nb1] != 0).sum()) == 0   # the x sides of that box
    if n > 1:
        assert int((d_c[k, nb1:2 * nb1] != 0).sum()) > 0                                            # its y sides are alive


def test_unguarded_decode_is_the_old_entry(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    from defectdetection_viaobjectdetection_amd._capi import check, lib
    corners, project, points, _ = (t.to(cuda_device) for t in _decode_inputs(129, 33))
    for clamp01 in (0, 1):
        direct = torch.empty(129, 4, device=cuda_device)
        check(lib.m355_dfine_decode(corners.data_ptr(), project.data_ptr(), points.data_ptr(), direct.data_ptr(), 129, 33, REG_SCALE,
                                    clamp01, torch.cuda.current_stream().cuda_stream))
        assert _bits(dfine.decode_boxes(corners, project, points, REG_SCALE, bool(clamp01)), direct)
        assert _bits(dfine.decode_boxes(corners, project, points, REG_SCALE, bool(clamp01), guard=False), direct)


# ---- noobject_loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("class_index", [-1, 0])
@pytest.mark.parametrize("shape", [(1, 1, 2), (3, 300, 3), (50, 65, 81)])   # one row; the trainers' frame; rows of two lane trips
def test_noobject_loss(cuda_device, shape, class_index):
    """logits of standard deviation 15 clamped to the guard's bound: about a fifth sit at +-20 exactly"""
    from defectdetection_viaobjectdetection_amd import dfine
    x, gw = (15.0 * _randn(shape, sum(shape))).clamp(-20.0, 20.0), _randn(shape[:1], 5)
    res = _three_ways(lambda t: dfine.noobject_loss(t, class_index), lambda t: ref.noobject_loss(t, class_index), [x], gw, cuda_device)
    _check_three_ways(f"noobject_loss {shape} class {class_index}", ("loss", "dlogits"), res)
    assert res[0][0].shape == shape[:1]
    if shape[0] > 1:   # the loss loop uses the entries of the frames without ground truth: the other frames receive nothing
        t = x.to(cuda_device).requires_grad_()
        dfine.noobject_loss(t, class_index)[::2].sum().backward()
        assert int((t.grad[1::2] != 0).sum()) == 0 and int((t.grad[::2] != 0).sum()) > 0
    with torch.no_grad():
        n, off = _packs(lambda: dfine.noobject_loss(x.to(cuda_device).requires_grad_(), class_index))
    assert n == 0 and off.grad_fn is None and _bits(off, res[0][0].detach())


# ---- consistency_loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 1), (50, 300, 2), (7, 65, 5), (3, 70, 65)])   # the last: two chunks per frame, the second partial
def test_consistency_loss(cuda_device, shape):
    from defectdetection_viaobjectdetection_amd import dfine
    a, gw = _randn(shape, sum(shape)), torch.tensor(0.7)
    res = _three_ways(dfine.consistency_loss, ref.consistency_loss, [a], gw, cuda_device)
    _check_three_ways(f"consistency_loss {shape}", ("loss", "da"), res)
    assert res[0][0].shape == ()
    t = a.to(cuda_device)
    assert _bits(dfine.consistency_loss(t), res[0][0].detach()) and _bits(dfine.consistency_loss(t), dfine.consistency_loss(t))
    with torch.no_grad():
        assert _packs(lambda: dfine.consistency_loss(t.clone().requires_grad_()))[0] == 0


def test_consistency_loss_of_one_frame_is_zero(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    out = dfine.consistency_loss(_randn((1, 4, 2), 1).to(cuda_device).requires_grad_())
    assert out.shape == () and out.is_cuda and float(out) == 0.0 and float(ref.consistency_loss(_randn((1, 4, 2), 1))) == 0.0


# ---- temporal_head ---------------------------------------------------------------------------------------------------------------
class _Heads(torch.nn.Module):
    """a stand-in for the trainers' module: random nn.Linear heads of the trainers' widths"""

    def __init__(self, D=256, C1=3, nb1=33):
        super().__init__()
        torch.manual_seed(0)
        self.class_head, self.bbox_head = torch.nn.Linear(D, C1), torch.nn.Linear(D, 4 * nb1)
        self.anomaly_detector = torch.nn.Linear(D, C1 - 1)


@pytest.mark.parametrize("variant", ["plain", "improved"])
def test_temporal_head(cuda_device, variant):
    from defectdetection_viaobjectdetection_amd import dfine
    T, Q, D, nb1 = 4, 10, 256, 33
    improved = variant == "improved"
    fused, init_ref = _randn((T, Q, D), 1), 0.2 + 0.4 * _rand((T, Q, 4), 2)
    scores, context = (_randn((T, Q, 1), 3), _randn((T, Q, D), 4)) if improved else (None, None)
    project = dfine.weighting_function(nb1 - 1, torch.tensor([0.5]), REG_SCALE).float()
    weights = [_randn((T, Q, 3), 5), _randn((T, Q, 4), 6), _randn((T, Q, 2), 7)]
    heads = _Heads()
    res, before = [], dict(dfine.temporal_calls)
    for kind in ("kernel", "torch", "ref64"):
        to = (lambda t: t.double()) if kind == "ref64" else (lambda t: t.to(cuda_device))
        m = copy.deepcopy(heads)
        m = m.double() if kind == "ref64" else m.to(cuda_device)
        f = to(fused).requires_grad_()
        kw = dict(scores=to(scores), context=to(context), anomaly_head=m.anomaly_detector) if improved else {}
        fn = dfine.temporal_head if kind == "kernel" else ref.temporal_head
        outs = fn(f, to(init_ref), m.class_head, m.bbox_head, to(project), REG_SCALE, **kw)
        outs = [o for o in outs if o is not None]
        assert len(outs) == (3 if improved else 2)
        params = [p for p in m.parameters() if improved or not any(p is q for q in m.anomaly_detector.parameters())]
        loss = sum((o * to(w)).sum() for o, w in zip(outs, weights))
        res.append(tuple(outs) + torch.autograd.grad(loss, [f] + params))
    names = (["cls_logits", "bbox_pred"] + (["anomaly"] if improved else []) + ["dfused"]
             + [f"d{n}" for n, _ in heads.named_parameters() if improved or not n.startswith("anomaly")])
    assert len(names) == len(res[0])
    _check_three_ways(f"temporal_head {variant}", names, res)
    assert dfine.temporal_calls["torch"] == before["torch"] and dfine.temporal_calls["kernel"] == before["kernel"] + (3 if improved else 2)
    # under no_grad nothing is saved, by the ops or by the heads
    m = copy.deepcopy(heads).to(cuda_device)
    kw = dict(scores=scores.to(cuda_device), context=context.to(cuda_device), anomaly_head=m.anomaly_detector) if improved else {}
    with torch.no_grad():
        n, outs = _packs(lambda: dfine.temporal_head(fused.to(cuda_device).requires_grad_(), init_ref.to(cuda_device), m.class_head,
                                                     m.bbox_head, project.to(cuda_device), REG_SCALE, **kw))
    assert n == 0 and all(o is None or o.grad_fn is None for o in outs)
    for got, want in zip(outs, res[0]):
        if got is not None:
            assert _bits(got, want.detach())
