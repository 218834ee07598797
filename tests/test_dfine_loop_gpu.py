"""The decoder-loop ops on the GPU (csrc/dfine_loop.hip): dfine.query_pos_hidden, refine_reference, refine_boxes and their gradients.

Every output and gradient tensor is held to the float64 restatement of tests/dfine_loop_ref.py on the CPU by the project's standing
rule (tests/test_dfine_decoder_gpu.py): max |kernel - ref64| <= 2 * max |torch fp32 on this device - ref64| + 1e-6 * max |ref64|,
where "torch fp32" is the same restatement in fp32 on the GPU.  The float64 inputs are the fp32 inputs widened, so that no input
rounding enters either error."""
import pytest
import torch

import dfine_loop_ref as ref

pytestmark = pytest.mark.gpu

QP_SLAB_ROWS = 64     # csrc/dfine_loop.hip: the rows one block of the query_pos backward covers, one partial row of dweight | dbias
QP_MAX_SLABS = 256    # ... while there are at most this many slabs; beyond QP_SLAB_ROWS * QP_MAX_SLABS rows the slabs grow instead
RB_ROWS = 32          # rows of one block of refine_boxes


def _judge(name, kernel, torch32, want, failures):
    w = want.detach().double().cpu()
    e_k = float((kernel.detach().double().cpu() - w).abs().max())
    e_t = float((torch32.detach().double().cpu() - w).abs().max())
    scale = float(w.abs().max())
    print(f"{name}: max error vs float64: kernel {e_k:.3e}, torch fp32 {e_t:.3e} (max |ref| {scale:.4g})")
    assert tuple(kernel.shape) == tuple(w.shape), name
    assert kernel.is_cuda and kernel.dtype == torch.float32 and torch.isfinite(kernel).all(), name
    if not e_k <= 2 * e_t + 1e-6 * scale:
        failures.append((name, e_k, e_t, scale))


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _run(fn, inputs, gws, to, leaves):
    """outputs of fn(*inputs) (a tensor or a tuple), then the gradients of sum_j (out_j * gws[j]).sum() for inputs[leaves]"""
    ts = [None if t is None else to(t) for t in inputs]
    for i in leaves:
        ts[i].requires_grad_()
    outs = fn(*ts)
    outs = outs if isinstance(outs, tuple) else (outs,)
    grads = torch.autograd.grad(sum((o * to(g)).sum() for o, g in zip(outs, gws)), [ts[i] for i in leaves]) if leaves else ()
    return tuple(outs) + tuple(grads)


def _three_ways(fn_kernel, fn_ref, inputs, gws, dev, leaves):
    return (_run(fn_kernel, inputs, gws, lambda t: t.to(dev), leaves), _run(fn_ref, inputs, gws, lambda t: t.to(dev), leaves),
            _run(fn_ref, inputs, gws, lambda t: t.double(), leaves))


def _check(title, names, res):
    failures = []
    for name, k, t, w in zip(names, *res):
        _judge(f"{title} {name}", k, t, w, failures)
    assert not failures, failures


# ---- query_pos_hidden --------------------------------------------------------------------------------------------------------------
QP_NAMES = ("out", "dref", "dweight", "dbias")


def _qp_inputs(N, H):
    r, w, b = _rand((N, 4), N + H), 0.5 * _randn((H, 4), N + H + 1), 0.3 * _randn((H,), N + H + 2)
    b[: H // 2] = 0.0
    r[N // 2] = 0.0   # with the zero bias entries: pre-activations of exactly 0 in row N // 2, columns [0, H / 2)
    return [r, w, b], [_randn((N, H), N + H + 3)]


def _qp_check(N, H, dev, leaves=(0, 1, 2)):
    from defectdetection_viaobjectdetection_amd import dfine
    inputs, gws = _qp_inputs(N, H)
    res = _three_ways(dfine.query_pos_hidden, ref.query_pos_hidden, inputs, gws, dev, leaves)
    _check(f"query_pos_hidden {N}x{H}", ("out",) + tuple(QP_NAMES[1 + i] for i in leaves), res)
    return inputs, gws, res[0]


# one row; a last slab of 63 rows; 5 slabs; 15 slabs, the last of 5 rows.  H = 8: two lanes of a wave; H = 512: two column chunks
@pytest.mark.parametrize("H", [8, 512])
@pytest.mark.parametrize("N", [1, 63, 300, 901])
def test_query_pos_hidden(cuda_device, N, H):
    _qp_check(N, H, cuda_device)


@pytest.mark.parametrize("N,H", [(QP_SLAB_ROWS + 1, 512), (QP_SLAB_ROWS * QP_MAX_SLABS + 1, 8)])
def test_query_pos_hidden_past_one_slab(cuda_device, N, H):
    """one row more than a single block and a single partial row cover; one row more than QP_MAX_SLABS slabs of QP_SLAB_ROWS rows
    cover, where the slabs grow to 65 rows and the last one is empty"""
    _qp_check(N, H, cuda_device)


@pytest.mark.parametrize("leaves", [(0,), (1,), (2,), (1, 2), (0, 2), ()])
def test_query_pos_hidden_subset_of_gradients(cuda_device, leaves):
    """the gradients not asked for are null pointers in the backward call"""
    _qp_check(63, 512, cuda_device, leaves)


def test_query_pos_hidden_zero_preactivation_passes_no_gradient(cuda_device):
    """torch's ReLU mask: where the pre-activation is exactly 0 the output is 0 and what arrives there is dropped, so changing it
    changes no bit of any gradient"""
    from defectdetection_viaobjectdetection_amd import dfine
    N, H = 63, 512
    inputs, gws = _qp_inputs(N, H)
    to = lambda t: t.to(cuda_device)  # noqa: E731
    out, *g1 = _run(dfine.query_pos_hidden, inputs, gws, to, (0, 1, 2))
    assert torch.equal(out[N // 2, : H // 2], torch.zeros(H // 2, device=out.device))
    other = gws[0].clone()
    other[N // 2, : H // 2] += 100.0
    _, *g2 = _run(dfine.query_pos_hidden, inputs, [other], to, (0, 1, 2))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    # a bias of zeros everywhere: the whole row is at the kink and its dref is exactly 0
    inputs[2] = torch.zeros(H)
    _, dref, _, _ = _run(dfine.query_pos_hidden, inputs, gws, to, (0, 1, 2))
    assert torch.equal(dref[N // 2], torch.zeros(4, device=dref.device)) and float(dref.abs().max()) > 0


# ---- refine_reference --------------------------------------------------------------------------------------------------------------
EPS = 1e-5
REF_EDGES = (0.0, 1.0, 1e-6, 1.0 - 1e-6, EPS, -0.2, 1.3, 0.5)


def _rr_inputs(N, scale):
    d, r = scale * _randn((N, 4), N + 40), _rand((N, 4), N + 41)
    flat = r.reshape(-1)
    edges = torch.tensor(REF_EDGES)[: flat.numel()]
    flat[: edges.numel()] = edges
    return [d, r], [_randn((N, 4), N + 42)]


@pytest.mark.parametrize("scale", [1.0, 30.0])   # 30: saturated sigmoids, their derivative down to 0 in fp32
@pytest.mark.parametrize("N", [1, 63, 1200])      # N = 1 holds the first four edge values
def test_refine_reference(cuda_device, N, scale):
    from defectdetection_viaobjectdetection_amd import dfine
    inputs, gws = _rr_inputs(N, scale)
    res = _three_ways(lambda d, r: dfine.refine_reference(d, r, EPS), lambda d, r: ref.refine_reference(d, r, EPS), inputs, gws,
                      cuda_device, (0,))
    _check(f"refine_reference {N} delta*{scale:g}", ("out", "ddelta"), res)


def test_refine_reference_with_a_ref_that_requires_grad_takes_torch(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    inputs, gws = _rr_inputs(63, 1.0)
    inputs[1] = inputs[1].clamp(0.05, 0.95)
    to = lambda t: t.to(cuda_device)  # noqa: E731
    got = _run(lambda d, r: dfine.refine_reference(d, r, EPS), inputs, gws, to, (0, 1))
    want = _run(lambda d, r: dfine.refine_reference_torch(d, r, EPS), inputs, gws, to, (0, 1))
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- refine_boxes ------------------------------------------------------------------------------------------------------------------
REG_SCALE = 4.0


def _project(nb1):
    return ref.weighting_function(nb1 - 1, torch.tensor([0.5]), torch.tensor([REG_SCALE]))


def _rb_inputs(N, nb1, with_prev):
    delta, prev = 2.0 * _randn((N, 4 * nb1), N + nb1 + 60), 2.0 * _randn((N, 4 * nb1), N + nb1 + 61)
    for row, side, hot, sign in ((0, 1, 0, 1.0), (N // 2, 2, nb1 - 1, 1.0), (N - 1, 0, nb1 // 2, -1.0)):
        # logits of +-80 (with prev: +-40 in each addend): a one-hot softmax (or one bin at exactly 0), no overflow
        seg = slice(side * nb1, (side + 1) * nb1)
        delta[row, seg] = -80.0 * sign if not with_prev else -40.0 * sign
        prev[row, seg] = -40.0 * sign
        delta[row, side * nb1 + hot] = 80.0 * sign if not with_prev else 40.0 * sign
        prev[row, side * nb1 + hot] = 40.0 * sign
    points = _rand((N, 4), N + nb1 + 62) * torch.tensor([1.0, 1.0, 0.4, 0.4]) + torch.tensor([0.0, 0.0, 0.02, 0.02])
    gws = [0.1 * _randn((N, 4 * nb1), N + nb1 + 63), _randn((N, 4), N + nb1 + 64)]
    return [delta, prev if with_prev else None, _project(nb1), points], gws


def _rb_fns():
    from defectdetection_viaobjectdetection_amd import dfine
    return (lambda d, p, pr, pt: dfine.refine_boxes(d, p, pr, pt, REG_SCALE), lambda d, p, pr, pt: ref.refine_boxes(d, p, pr, pt, REG_SCALE))


# one row; a last block of 31 rows; 10 blocks, the last of 12 rows; 29 blocks, the last of 5 rows.  bins + 1: 5 and 17 (sides that
# straddle 16-byte words), 33 (the default)
@pytest.mark.parametrize("want_dpoints", [False, True])
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("nb1", [5, 17, 33])
@pytest.mark.parametrize("N", [1, 63, 300, 901])
def test_refine_boxes(cuda_device, N, nb1, with_prev, want_dpoints):
    inputs, gws = _rb_inputs(N, nb1, with_prev)
    leaves = (0,) + ((1,) if with_prev else ()) + ((3,) if want_dpoints else ())
    fn_kernel, fn_ref = _rb_fns()
    res = _three_ways(fn_kernel, fn_ref, inputs, gws, cuda_device, leaves)
    names = ("pred_corners", "boxes", "ddelta") + (("dprev",) if with_prev else ()) + (("dpoints",) if want_dpoints else ())
    _check(f"refine_boxes {N}x{nb1} prev={with_prev}", names, res)
    pred = res[0][0]
    dev = lambda t: t.to(cuda_device)  # noqa: E731
    assert torch.equal(pred, dev(inputs[0]) + dev(inputs[1]) if with_prev else dev(inputs[0]))   # torch's add, bit for bit
    if with_prev:
        assert torch.equal(res[0][2], res[0][3])   # one gradient serves both addends


def test_refine_boxes_without_grad_and_with_bins_at_the_limit(cuda_device):
    """the plain forward path, and bins + 1 = 64 (the largest LDS segment) and 2 (the smallest)"""
    fn_kernel, fn_ref = _rb_fns()
    for nb1 in (64, 2):
        inputs, gws = _rb_inputs(63, nb1, True)
        inputs[2] = torch.linspace(-2.0, 2.0, nb1)
        with torch.no_grad():
            res = _three_ways(fn_kernel, fn_ref, inputs, gws, cuda_device, ())
        _check(f"refine_boxes 63x{nb1} no grad", ("pred_corners", "boxes"), res)
        res = _three_ways(fn_kernel, fn_ref, inputs, gws, cuda_device, (0, 1, 3))
        _check(f"refine_boxes 63x{nb1}", ("pred_corners", "boxes", "ddelta", "dprev", "dpoints"), res)


def test_refine_boxes_gradient_of_one_output_alone(cuda_device):
    """only pred_corners or only boxes reaches the loss: the other gradient arrives as None"""
    fn_kernel, fn_ref = _rb_fns()
    inputs, gws = _rb_inputs(63, 33, True)
    for keep in (0, 1):
        pick = lambda fn: (lambda *t: fn(*t)[keep])  # noqa: E731
        res = _three_ways(pick(fn_kernel), pick(fn_ref), inputs, [gws[keep]], cuda_device, (0, 1))
        _check(f"refine_boxes output {keep} alone", (("pred_corners", "boxes")[keep], "ddelta", "dprev"), res)


# ---- bitwise reproducibility -------------------------------------------------------------------------------------------------------
def _op_cases(dev):
    from defectdetection_viaobjectdetection_amd import dfine
    fn_rb, _ = _rb_fns()
    # (name, fn, inputs at N, leaves, per-row results among (outputs + gradients))
    return [
        ("query_pos_hidden", dfine.query_pos_hidden, lambda N: _qp_inputs(N, 512), (0, 1, 2), (0, 1)),
        ("refine_reference", lambda d, r: dfine.refine_reference(d, r, EPS), lambda N: _rr_inputs(N, 1.0), (0,), (0, 1)),
        ("refine_boxes", fn_rb, lambda N: _rb_inputs(N, 33, True), (0, 1, 3), (0, 1, 2, 3, 4)),
        ("refine_boxes layer 0", fn_rb, lambda N: _rb_inputs(N, 33, False), (0, 3), (1, 2, 3)),
    ]


def test_each_op_twice_gives_equal_bits(cuda_device):
    to = lambda t: t.to(cuda_device)  # noqa: E731
    for name, fn, make, leaves, _ in _op_cases(cuda_device):
        inputs, gws = make(901)
        first, second = _run(fn, inputs, gws, to, leaves), _run(fn, inputs, gws, to, leaves)
        assert all(torch.equal(a, b) for a, b in zip(first, second)), name


def test_a_rows_results_do_not_depend_on_the_rows_around_it(cuda_device):
    """rows [0, 63) of an N = 901 call against the same rows as a call of their own: outputs and per-row gradients, bit for bit"""
    to = lambda t: t.to(cuda_device)  # noqa: E731
    n = 63
    for name, fn, make, leaves, per_row in _op_cases(cuda_device):
        inputs, gws = make(901)
        cut = lambda t: t if t is None or t.shape[0] != 901 else t[:n].contiguous()  # noqa: E731
        big = _run(fn, inputs, gws, to, leaves)
        small = _run(fn, [cut(t) for t in inputs], [cut(g) for g in gws], to, leaves)
        for j in per_row:
            assert torch.equal(big[j][:n], small[j]), (name, j)
