"""The decoder-layer ops on the GPU (csrc/dfine_decoder.hip and the gate and clamp sources of csrc/dfine_rowln.hip):
dfine.gate_layer_norm, add_layer_norm(clamp=...), lqe_statistics, their gradients, and transformers' DFineDecoderLayer / DFineLQE
bound with dfine.bind_decoder.

Every output and gradient tensor is held to the float64 restatement of tests/dfine_decoder_ref.py on the CPU by the project's
standing rule (tests/test_dfine_encoder_gpu.py): max |kernel - ref64| <= 2 * max |torch fp32 on this device - ref64| + 1e-6 * max |ref64|,
where "torch fp32" is the same restatement in fp32 on the GPU.  The float64 inputs are the fp32 inputs widened, so that no input
rounding enters either error."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import dfine_decoder_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [(8, 8), (4, 4), (2, 2)]   # the cross-attention's feature levels in the layer tests: 84 pixels


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


def _grads(out, leaves, weight):
    return torch.autograd.grad((out * weight.to(out.device, out.dtype)).sum(), leaves)


def _three_ways(fn_kernel, fn_ref, inputs, gw, dev, leaves=None):
    """(out, grads of `leaves` (indices into inputs; default all)) of the kernel, of torch fp32 on the device, of float64 on the CPU"""
    res = []
    for kind in ("kernel", "torch", "ref64"):
        to = (lambda t: t.double()) if kind == "ref64" else (lambda t: t.to(dev))
        ts = [to(t) for t in inputs]
        want = range(len(ts)) if leaves is None else leaves
        for i in want:
            ts[i].requires_grad_()
        out = (fn_kernel if kind == "kernel" else fn_ref)(*ts)
        res.append((out,) + tuple(_grads(out, [ts[i] for i in want], gw)))
    return res


# ---- DFineGate behind its nn.Linear ------------------------------------------------------------------------------------------------
GATE_NAMES = ("out", "dx1", "dx2", "dgate", "dweight", "dbias")


def _gate_inputs(M, D, scale, constant_row=True):
    x1, x2, g = _randn((M, D), M + D), _randn((M, D), M + D + 1), scale * _randn((M, 2 * D), M + D + 2)
    if M > 1 and constant_row:   # variance 0, eps alone keeps it finite; its gradients of about 1 / sqrt(eps) set the largest error
        x1[M // 2] = 0.7
        x2[M // 2] = 0.7
        g[M // 2] = 0.0
    return [x1, x2, g, 1.0 + 0.1 * _randn((D,), 5), 0.1 * _randn((D,), 6)], _randn((M, D), 8)


def _gate_check(M, D, scale, dev, leaves=None, constant_row=True):
    from defectdetection_viaobjectdetection_amd import dfine
    inputs, gw = _gate_inputs(M, D, scale, constant_row)
    res = _three_ways(lambda *t: dfine.gate_layer_norm(*t, 1e-5), lambda *t: ref.gate_layer_norm(*t, 1e-5), inputs, gw, dev, leaves)
    names = GATE_NAMES if leaves is None else ("out",) + tuple(GATE_NAMES[1 + i] for i in leaves)
    failures = []
    for name, k, t, w in zip(names, *res):
        assert k.is_cuda and k.dtype == torch.float32 and torch.isfinite(k).all(), name
        _judge(f"gate_layer_norm {M}x{D} logits*{scale:g} {name}", k, t, w, failures)
    assert not failures, failures


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("M", [1, 63, 300, 900])   # one row; a last block of 3 rows; more blocks than rows per block; 225 blocks
def test_gate_layer_norm(cuda_device, M, D):
    _gate_check(M, D, 1.0, cuda_device)


def test_gate_layer_norm_saturated_sigmoids(cuda_device):
    """logits of about +-30 and beyond: both gates at 0 or 1 to fp32, their derivative down to 1e-40.  Without the constant row,
    whose gradients would hide every other element's error"""
    _gate_check(300, 256, 30.0, cuda_device, constant_row=False)


@pytest.mark.parametrize("leaves", [(0,), (2,), (1, 4), (3, 4), (0, 1, 2)])
def test_gate_layer_norm_subset_of_gradients(cuda_device, leaves):
    """the outputs not asked for are null pointers in the backward call: x1 alone, the logits alone, x2 + dbias, the two column
    sums alone (no per-row output at all), the three per-row outputs without the column sums"""
    _gate_check(63, 64, 1.0, cuda_device, leaves)


# ---- LayerNorm(clamp(x + y)) ---------------------------------------------------------------------------------------------------------
LO, HI = ref.CLAMP


def _clamp_inputs(M, D):
    x, y = _randn((M, D), M + D + 20), _randn((M, D), M + D + 21)
    r = M // 2
    outside = [(r, 3, 7.0e4), (r, 100, -6.6e4), (0, D - 1, 1.0e5), (M - 1, 64, -3.0e38), (M - 1, 0, 65505.0)]   # (row, column, sum)
    on_bound = [(r, 5, HI), (0, 17, LO)]                                                                        # the gradient passes
    for i, c, v in outside + on_bound:
        x[i, c], y[i, c] = v, 0.0
    return [x, y, 1.0 + 0.1 * _randn((D,), 25), 0.1 * _randn((D,), 26)], _randn((M, D), 28), outside, on_bound


@pytest.mark.parametrize("M", [1, 300])
def test_add_clamp_layer_norm(cuda_device, M):
    from defectdetection_viaobjectdetection_amd import dfine
    D = 256
    inputs, gw, outside, on_bound = _clamp_inputs(M, D)
    res = _three_ways(lambda *t: dfine.add_layer_norm(*t, 1e-5, clamp=(LO, HI)), lambda *t: ref.add_clamp_layer_norm(*t, 1e-5), inputs,
                      gw, cuda_device)
    failures = []
    for name, k, t, w in zip(("out", "dx", "dy", "dweight", "dbias"), *res):
        assert torch.isfinite(k).all(), name
        _judge(f"add_layer_norm clamp {M}x{D} {name}", k, t, w, failures)
    assert not failures, failures
    dx, dy = res[0][1], res[0][2]
    for i, c, _ in outside:
        assert float(dx[i, c]) == 0.0 and float(dy[i, c]) == 0.0, (i, c)       # exactly 0, as torch's clamp backward
    for i, c, _ in on_bound:
        assert float(dx[i, c]) != 0.0 and float(dy[i, c]) != 0.0, (i, c)       # the bounds are included
    assert int((dx == 0).sum()) == len(outside)


def test_clamp_none_is_the_old_call_and_an_idle_clamp_changes_no_bit(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    dev = cuda_device
    x, y, wt, bs, gw = (_randn(s, 40 + i).to(dev) for i, s in enumerate([(300, 256), (300, 256), (256,), (256,), (300, 256)]))

    def run(**kw):
        leaves = [t.clone().requires_grad_() for t in (x, y, wt, bs)]
        out = dfine.add_layer_norm(*leaves, 1e-5, **kw)
        return (out,) + tuple(_grads(out, leaves, gw))

    old, none, idle = run(), run(clamp=None), run(clamp=(LO, HI))
    for i, (a, b, c) in enumerate(zip(old, none, idle)):
        assert torch.equal(a, b) and torch.equal(a, c), i
    with torch.no_grad():
        assert torch.equal(dfine.add_layer_norm(x, y, wt, bs, 1e-5, clamp=None), old[0])
        assert torch.equal(dfine.add_layer_norm(x, y, wt, bs, 1e-5, clamp=(LO, HI)), old[0])


# ---- the row sources of csrc/dfine_rowln.hip against each other and at the edges of D ---------------------------------------------------
def test_saturated_gate_is_the_add_instance_bit_for_bit(cuda_device):
    """gate logits of +200 | -200: sigmoid is exactly 1 | 0 and its derivative exactly 0, so z = 1 * x1 + 0 * x2 has the bits of
    x1 + 0 and the gate instance must give what the add instance gives on (x1, zeros): the shared statistics, dz expression and
    column sums are one text in two instances, contracted alike"""
    from defectdetection_viaobjectdetection_amd import dfine
    dev, M, D = cuda_device, 63, 256
    x1, x2, wt, bs, gw = (_randn(s, 90 + i).to(dev) for i, s in enumerate([(M, D), (M, D), (D,), (D,), (M, D)]))
    g = torch.cat([torch.full((M, D), 200.0), torch.full((M, D), -200.0)], dim=-1).to(dev)
    gate_leaves = [t.clone().requires_grad_() for t in (x1, x2, g, wt, bs)]
    gate_out = dfine.gate_layer_norm(*gate_leaves, 1e-5)
    dx1, _, dgate, gate_dw, gate_db = _grads(gate_out, gate_leaves, gw)
    add_leaves = [t.clone().requires_grad_() for t in (x1, torch.zeros_like(x1), wt, bs)]
    add_out = dfine.add_layer_norm(*add_leaves, 1e-5)
    dx, _, add_dw, add_db = _grads(add_out, add_leaves, gw)
    assert torch.equal(gate_out, add_out)
    assert torch.equal(dx1, dx) and torch.equal(gate_dw, add_dw) and torch.equal(gate_db, add_db)
    assert int((dgate != 0).sum()) == 0


# (M, D): one live lane; two blocks and lane 0 alone in the second float4 slot; the widest row, every slot of every lane
ROWLN_EDGES = [(1, 4), (5, 260), (63, 1024)]
ROWLN_SEED, ROWLN_P = 0xD1CE, 0.1


@pytest.mark.parametrize("M, D", ROWLN_EDGES)
@pytest.mark.parametrize("form", ["add", "add_dropout", "add_clamp", "gate"])
def test_row_layer_norms_at_the_edges_of_d(cuda_device, form, M, D):
    """every source of the row-LayerNorm kernels where D is not 64, 128 or 256: forward and every gradient"""
    import dfine_encoder_ref as enc_ref
    from defectdetection_viaobjectdetection_amd import dfine
    x, y, gw = _randn((M, D), 3 * M + D), _randn((M, D), 3 * M + D + 1), _randn((M, D), 3 * M + D + 2)
    wt, bs = 1.0 + 0.1 * _randn((D,), 95), 0.1 * _randn((D,), 96)
    if form == "gate":
        inputs, names = [x, y, _randn((M, 2 * D), 3 * M + D + 3), wt, bs], GATE_NAMES
        fn, fn_ref = (lambda *t: dfine.gate_layer_norm(*t, 1e-5)), (lambda *t: ref.gate_layer_norm(*t, 1e-5))
    else:
        inputs, names = [x, y, wt, bs], ("out", "dx", "dy", "dweight", "dbias")
        if form == "add":
            fn, fn_ref = (lambda *t: dfine.add_layer_norm(*t, 1e-5)), (lambda *t: enc_ref.add_layer_norm(*t, 1e-5))
        elif form == "add_dropout":
            mask = dfine.dropout_keep_mask(ROWLN_SEED, dfine.SITE_FFN_OUT, (M, D), ROWLN_P, cuda_device)
            fn = lambda *t: dfine.add_layer_norm(*t, 1e-5, dropout_p=ROWLN_P, seed=ROWLN_SEED, site=dfine.SITE_FFN_OUT)  # noqa: E731
            fn_ref = lambda *t: enc_ref.add_layer_norm(*t, 1e-5, mask, ROWLN_P)  # noqa: E731
        else:   # one sum far outside each bound (no gradient), one on a bound (the gradient passes)
            x[0, D - 1], y[0, D - 1] = 1.0e5, 0.0
            x[M - 1, 1], y[M - 1, 1] = -7.0e4, 0.0
            x[M // 2, 2], y[M // 2, 2] = HI, 0.0
            fn, fn_ref = (lambda *t: dfine.add_layer_norm(*t, 1e-5, clamp=(LO, HI))), (lambda *t: ref.add_clamp_layer_norm(*t, 1e-5))
    res = _three_ways(fn, fn_ref, inputs, gw, cuda_device)
    failures = []
    for name, k, t, w in zip(names, *res):
        assert k.is_cuda and k.dtype == torch.float32 and torch.isfinite(k).all(), name
        _judge(f"{form} {M}x{D} {name}", k, t, w, failures)
    assert not failures, failures
    if form == "add_clamp":
        dx, dy = res[0][1], res[0][2]
        assert float(dx[0, D - 1]) == 0.0 and float(dy[M - 1, 1]) == 0.0 and float(dx[M // 2, 2]) != 0.0


# ---- the LQE statistics ----------------------------------------------------------------------------------------------------------------
def _lqe_inputs(M, nb1, k, scale, seed=0):
    # The reference must be well-posed: the probabilities of a side apart by far more than fp32 rounding, else "which bin is the
    # j-th largest" (and with it where the gradient goes) is decided by rounding in any implementation, and among 1200 x 4 sides
    # of plain normal logits some pair always comes that close.  So a side's logits are a random permutation of an even grid
    # over +-1.7 (standard deviation 1) that is jittered by up to a quarter of its spacing.
    g = torch.Generator().manual_seed(50 + M + nb1 + seed)
    order = torch.rand((M, 4, nb1), generator=g).argsort(-1)
    step = 3.4 / max(nb1 - 1, 1)
    grid = torch.linspace(-1.7, 1.7, nb1)[order] + (torch.rand((M, 4, nb1), generator=g) - 0.5) * 0.5 * step
    c = (scale * grid).reshape(M, 4 * nb1).float()
    p = torch.softmax(c.double().reshape(M, 4, nb1), -1).sort(-1, descending=True).values[..., :k + 1]
    gap = (p[..., :-1] - p[..., 1:]) / p[..., :-1]
    assert float(gap.min()) > 1e-5, float(gap.min())
    return c, _randn((M, 4 * (k + 1)), 51)


def _lqe_check(c, gw, nb1, k, dev, tag, forward_only=False):
    from defectdetection_viaobjectdetection_amd import dfine
    res = _three_ways(lambda t: dfine.lqe_statistics(t, nb1 - 1, k), lambda t: ref.lqe_statistics(t, nb1 - 1, k), [c], gw, dev)
    failures = []
    for name, kk, t, w in list(zip(("stat", "d_pred_corners"), *res))[:1 if forward_only else 2]:
        assert kk.is_cuda and kk.dtype == torch.float32 and torch.isfinite(kk).all(), name
        _judge(f"lqe_statistics {tag} {name}", kk, t, w, failures)
    assert not failures, failures
    return res[0]


@pytest.mark.parametrize("nb1, k", [(33, 4), (17, 1), (64, 8), (4, 4)])   # D-FINE's own; k = 1; both limits; every bin chosen
@pytest.mark.parametrize("M", [1, 65, 1200])
def test_lqe_statistics(cuda_device, M, nb1, k):
    c, gw = _lqe_inputs(M, nb1, k, 3.0)
    stat = _lqe_check(c, gw, nb1, k, cuda_device, f"{M}x4x{nb1} top {k}")[0]
    s = stat.reshape(M, 4, k + 1)
    assert bool((s[..., :k - 1] >= s[..., 1:k]).all())   # descending


def test_lqe_statistics_peaked(cuda_device):
    """logits * 20: one bin takes nearly all the mass, the others reach down to 1e-30 and below"""
    c, gw = _lqe_inputs(65, 33, 4, 20.0)
    _lqe_check(c.reshape(5, 13, 4 * 33), gw.reshape(5, 13, 20), 33, 4, cuda_device, "65x4x33 top 4 logits*20")


def _tied_logits(M, nb1, seed):
    """integer logits 0..2: every side has many exactly equal probabilities, in fp32 and in float64 alike"""
    return torch.randint(0, 3, (M, 4 * nb1), generator=torch.Generator().manual_seed(seed)).float()


def test_lqe_statistics_exact_ties_forward(cuda_device):
    """the values do not depend on which of two equal bins is taken"""
    c = _tied_logits(65, 33, 60)
    c[7] = 0.0   # a row of all-equal bins: every probability 1 / 33
    _lqe_check(c, _randn((65, 20), 61), 33, 4, cuda_device, "65x4x33 top 4 ties", forward_only=True)


def test_lqe_tie_gradient_lands_on_the_lowest_index(cuda_device):
    """with ties the rule decides where the gradient goes: the float64 restatement takes the lowest bin first (a stable sort), and so
    must the kernel; a side of all-equal bins sends the top-k gradient to bins 0 .. k - 1"""
    from defectdetection_viaobjectdetection_amd import dfine
    nb1, k, M = 33, 4, 65
    c = _tied_logits(M, nb1, 62)
    c[7] = 0.0
    stat, gc = _lqe_check(c, _randn((M, 4 * (k + 1)), 63), nb1, k, cuda_device, "65x4x33 top 4 tie gradient")
    x = torch.zeros(1, 4 * nb1, device=cuda_device, requires_grad=True)
    gw = torch.zeros(1, 4, k + 1, device=cuda_device)
    gw[..., :k] = 1.0   # d stat = 1 on the k probabilities, 0 on the mean: dp = 1 on the chosen bins
    g, = torch.autograd.grad((dfine.lqe_statistics(x, nb1 - 1, k).reshape(1, 4, k + 1) * gw).sum(), [x])
    g = g.reshape(4, nb1)
    assert bool((g[:, :k] > 0).all()) and bool((g[:, k:] < 0).all())
    np.testing.assert_allclose(g[:, :k].cpu().numpy(), (1 - k / nb1) / nb1, rtol=1e-5)
    np.testing.assert_allclose(g[:, k:].cpu().numpy(), -(k / nb1) / nb1, rtol=1e-5)


# ---- determinism -------------------------------------------------------------------------------------------------------------------------
def _ops_run(dev, sl):
    """outputs and per-row gradients of the three ops on rows `sl` of fixed inputs"""
    from defectdetection_viaobjectdetection_amd import dfine
    D, nb1, k = 256, 33, 4
    x1, x2, g, w = (_randn(s, 70 + i).to(dev) for i, s in enumerate([(3, 300, D), (3, 300, D), (3, 300, 2 * D), (3, 300, D)]))
    wt, bs = _randn((D,), 75).to(dev), _randn((D,), 76).to(dev)
    c, cw = 3.0 * _randn((3, 300, 4 * nb1), 77).to(dev), _randn((3, 300, 4 * (k + 1)), 78).to(dev)
    a, b, gg = (t[sl].clone().requires_grad_() for t in (x1, x2, g))
    n = dfine.gate_layer_norm(a, b, gg, wt, bs, 1e-5)
    xs, ys = x1[sl].clone().requires_grad_(), x2[sl].clone().requires_grad_()
    m = dfine.add_layer_norm(xs, ys, wt, bs, 1e-5, clamp=(-1.5, 1.5))   # a clamp that bites
    cs = c[sl].clone().requires_grad_()
    s = dfine.lqe_statistics(cs, nb1 - 1, k)
    return (n,) + tuple(_grads(n, [a, b, gg], w[sl])) + (m,) + tuple(_grads(m, [xs, ys], w[sl])) + (s, _grads(s, [cs], cw[sl])[0])


def test_row_of_a_batch_equals_the_row_alone(cuda_device):
    """frame 1 of a batch of 3 against the same frame as a batch of 1, bit for bit.  dweight / dbias are sums over all rows and
    are not compared."""
    full, alone = _ops_run(cuda_device, slice(0, 3)), _ops_run(cuda_device, slice(1, 2))
    for i, (f, a) in enumerate(zip(full, alone)):
        assert torch.equal(f[1:2], a), i


def test_two_runs_give_the_same_bits(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    one, two = _ops_run(cuda_device, slice(0, 3)), _ops_run(cuda_device, slice(0, 3))
    for i, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a, b), i
    inputs, gw = _gate_inputs(900, 256, 1.0)   # the column sums: partial rows of 225 blocks added in a fixed order
    runs = []
    for _ in range(2):
        leaves = [t.to(cuda_device).requires_grad_() for t in inputs]
        runs.append(_grads(dfine.gate_layer_norm(*leaves, 1e-5), leaves, gw))
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i


def test_nothing_is_saved_without_grad(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    dev = cuda_device
    x, g, wt, bs = _randn((9, 64), 81).to(dev), _randn((9, 128), 82).to(dev), torch.ones(64, device=dev), torch.zeros(64, device=dev)
    c = _randn((9, 4 * 33), 83).to(dev)
    assert dfine.gate_layer_norm(x, x, g, wt, bs, 1e-5).grad_fn is None
    assert dfine.add_layer_norm(x, x, wt, bs, 1e-5, clamp=(LO, HI)).grad_fn is None
    assert dfine.lqe_statistics(c, 32, 4).grad_fn is None
    x.requires_grad_(), c.requires_grad_()
    assert dfine.gate_layer_norm(x, x, g, wt, bs, 1e-5).grad_fn is not None
    assert dfine.add_layer_norm(x, x, wt, bs, 1e-5, clamp=(LO, HI)).grad_fn is not None
    assert dfine.lqe_statistics(c, 32, 4).grad_fn is not None
    with torch.no_grad():
        assert dfine.gate_layer_norm(x, x, g, wt, bs, 1e-5).grad_fn is None
        assert dfine.add_layer_norm(x, x, wt, bs, 1e-5, clamp=(LO, HI)).grad_fn is None
        assert dfine.lqe_statistics(c, 32, 4).grad_fn is None


# ---- the bound layer and the bound quality head ----------------------------------------------------------------------------------------
def _modeling():
    try:
        from transformers import DFineConfig
        from transformers.models.d_fine import modeling_d_fine as M
    except Exception as ex:  # noqa: BLE001
        pytest.skip(f"transformers D-FINE not importable here: {ex}")
    return DFineConfig, M


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "dfine_decoder_golden.npz"))


def _load(module, G, prefix):
    with torch.no_grad():
        for n, p in module.named_parameters():
            p.copy_(torch.from_numpy(G[f"{prefix}.{n}"]))
    return module


@pytest.mark.parametrize("attention", [True, False])
def test_bound_layer_and_lqe_give_the_golden_outputs(cuda_device, attention):
    """transformers' own modules with the golden parameters, bound, on the golden inputs: the outputs transformers gave on the CPU,
    to the golden-file tolerance of tests/test_dfine_oracle.py (the arithmetic differs in order only)"""
    from defectdetection_viaobjectdetection_amd import dfine
    DFineConfig, M = _modeling()
    G, dev = _golden(), cuda_device
    cfg = DFineConfig(d_model=64, decoder_attention_heads=2, decoder_ffn_dim=128, decoder_n_points=[3, 6, 3])
    shapes = [tuple(int(v) for v in hw) for hw in G["shapes"]]
    t = lambda key: torch.from_numpy(G[key]).to(dev)  # noqa: E731
    layer = dfine.bind_decoder(_load(M.DFineDecoderLayer(cfg), G, "layer").to(dev).eval(), attention=attention)
    head = dfine.bind_decoder(_load(M.DFineLQE(cfg), G, "lqe").to(dev).eval())
    before = dict(dfine.decoder_calls)
    with torch.no_grad():
        y = layer(t("layer_hidden"), position_embeddings=t("layer_pos"), reference_points=t("layer_ref"),
                  spatial_shapes=torch.tensor(shapes, device=dev), spatial_shapes_list=shapes, encoder_hidden_states=t("layer_enc"))
        s = head(t("lqe_scores"), t("lqe_corners"))
    assert dfine.decoder_calls == {"kernel": before["kernel"] + 2, "torch": before["torch"]}
    for name, got, key in (("layer", y, "layer_out"), ("lqe", s, "lqe_out")):
        err = np.abs(got.cpu().numpy() - G[key]).max()
        print(f"{name}: max |bound - transformers on the CPU| {err:.3e} (max |ref| {np.abs(G[key]).max():.4g})")
        assert got.shape == G[key].shape and err <= 2e-6 * max(1.0, np.abs(G[key]).max()), name


def _layer_inputs(B, Q, D, seed):
    S = sum(h * w for h, w in MAPS)
    g = torch.Generator().manual_seed(seed)
    x, pos = torch.randn(B, Q, D, generator=g), torch.randn(B, Q, D, generator=g).clamp(-10, 10)
    rp = torch.rand(B, Q, 1, 4, generator=g) * torch.tensor([1.0, 1.0, 0.4, 0.4]) + torch.tensor([0.0, 0.0, 0.02, 0.02])
    return x, pos, rp, torch.randn(B, S, D, generator=g), torch.randn(B, Q, D, generator=g)


@functools.lru_cache(maxsize=None)
def _layer_case(B, Q):
    """a default-config layer (256 wide, 8 heads, 12 points) with random LayerNorm parameters, its inputs, and the restatement's
    output and gradients in fp32 on the GPU and in float64 on the CPU: computed once per shape, read-only afterwards"""
    DFineConfig, M = _modeling()
    cfg = DFineConfig(dropout=0.0, attention_dropout=0.0)
    with torch.random.fork_rng():
        torch.manual_seed(11)
        layer = M.DFineDecoderLayer(cfg)
        for m in layer.modules():
            if isinstance(m, torch.nn.LayerNorm):
                with torch.no_grad():
                    m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                    m.bias.copy_(0.2 * torch.randn_like(m.bias))
    x, pos, rp, enc, w = _layer_inputs(B, Q, cfg.d_model, 12 + Q)
    res = []
    for kind in ("torch", "ref64"):
        m = copy.deepcopy(layer).double() if kind == "ref64" else copy.deepcopy(layer).cuda()
        to = (lambda t: t.double()) if kind == "ref64" else (lambda t: t.cuda())
        xi, ei = to(x).requires_grad_(), to(enc).requires_grad_()
        P = ref.layer_params(m)
        out = ref.decoder_layer(xi, to(pos), to(rp), ei, MAPS, P, cfg.decoder_attention_heads, layer.encoder_attn.num_points_list,
                                cfg.decoder_offset_scale, cfg.layer_norm_eps)
        res.append(tuple(t.detach() for t in (out,) + tuple(_grads(out, [xi, ei] + list(P.values()), w))))
    return layer, (x, pos, rp, enc, w), res


@pytest.mark.parametrize("attention", [True, False])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("B, Q", [(2, 37), (3, 300)])
def test_bound_layer_against_float64(cuda_device, B, Q, mode, attention):
    from defectdetection_viaobjectdetection_amd import dfine
    layer, (x, pos, rp, enc, w), (res_t, res_w) = _layer_case(B, Q)
    dev = cuda_device
    bound = dfine.bind_decoder(copy.deepcopy(layer).to(dev), attention=attention).train(mode == "train")
    xi, ei = x.to(dev).requires_grad_(), enc.to(dev).requires_grad_()
    before = dict(dfine.decoder_calls)
    out = bound(xi, position_embeddings=pos.to(dev), reference_points=rp.to(dev), spatial_shapes=torch.tensor(MAPS, device=dev),
                spatial_shapes_list=MAPS, encoder_hidden_states=ei)
    assert dfine.decoder_calls == {"kernel": before["kernel"] + 1, "torch": before["torch"]}
    res_k = (out,) + tuple(_grads(out, [xi, ei] + list(ref.layer_params(bound).values()), w))
    failures = []
    for n, k, t, wv in zip(("output", "d_hidden_states", "d_encoder_hidden_states") + ref.LAYER_PARAM_NAMES, res_k, res_t, res_w):
        _judge(f"layer ({B}, {Q}, 256) {mode} attention={attention} {n}", k, t, wv, failures)
    assert not failures, failures


def test_fallbacks_on_the_device(cuda_device):
    """a mask (the denoising groups), dropout > 0 in training, fp16: the class's own forward, the same bits as the unbound module"""
    from defectdetection_viaobjectdetection_amd import dfine
    DFineConfig, M = _modeling()
    dev = cuda_device
    x, pos, rp, enc, _ = (t.to(dev) for t in _layer_inputs(2, 37, 256, 90))
    kw = dict(position_embeddings=pos, reference_points=rp, spatial_shapes=torch.tensor(MAPS, device=dev), spatial_shapes_list=MAPS,
              encoder_hidden_states=enc)
    torch.manual_seed(13)
    plain = M.DFineDecoderLayer(DFineConfig(dropout=0.0, attention_dropout=0.0)).to(dev).eval()
    bound = dfine.bind_decoder(copy.deepcopy(plain))

    def calls(fn):
        before = dict(dfine.decoder_calls)
        out = fn()
        return out, {k: dfine.decoder_calls[k] - before[k] for k in before}

    with torch.no_grad():
        _, n = calls(lambda: bound(x, **kw))
        assert n == {"kernel": 1, "torch": 0}
        mask = torch.zeros(2, 1, 37, 37, device=dev)
        mask[..., 30:] = float("-inf")
        got, n = calls(lambda: bound(x, encoder_attention_mask=mask, **kw))
        assert n == {"kernel": 0, "torch": 1} and torch.equal(got, plain(x, encoder_attention_mask=mask, **kw))
        half, hkw = copy.deepcopy(plain).half(), {k: (v.half() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in kw.items()}
        got, n = calls(lambda: dfine.bind_decoder(copy.deepcopy(half))(x.half(), **hkw))
        assert n == {"kernel": 0, "torch": 1} and got.dtype == torch.float16 and torch.equal(got, half(x.half(), **hkw))
        got, n = calls(lambda: bound(x, output_attentions=True, **kw))
        assert n == {"kernel": 0, "torch": 1} and torch.equal(got, plain(x, **kw))
    dropping = dfine.bind_decoder(M.DFineDecoderLayer(DFineConfig(dropout=0.1, attention_dropout=0.0)).to(dev))
    _, n = calls(lambda: dropping.train()(x, **kw))
    assert n == {"kernel": 0, "torch": 1}
    with torch.no_grad():
        _, n = calls(lambda: dropping.eval()(x, **kw))   # no dropout outside training
    assert n == {"kernel": 1, "torch": 0}

    head = dfine.bind_decoder(M.DFineLQE(DFineConfig()).to(dev))
    scores, corners = torch.randn(2, 37, 80, device=dev), torch.randn(2, 37, 4 * 33, device=dev)
    with torch.no_grad():
        _, n = calls(lambda: head(scores, corners))
        assert n == {"kernel": 1, "torch": 0}
        got, n = calls(lambda: dfine.bind_decoder(copy.deepcopy(head).half())(scores.half(), corners.half()))
        assert n == {"kernel": 0, "torch": 1} and got.dtype == torch.float16
        _, n = calls(lambda: dfine.bind_decoder(copy.deepcopy(head).cpu())(scores.cpu(), corners.cpu()))
        assert n == {"kernel": 0, "torch": 1}
