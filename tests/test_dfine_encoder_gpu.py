"""The temporal-encoder ops on the GPU (csrc/dfine_encoder.hip): dfine.self_attention, add_layer_norm, relu_dropout, their
gradients, the dropout keep-mask, and the bound nn.TransformerEncoder.

Every output and gradient tensor is held to the float64 restatement of tests/dfine_encoder_ref.py on the CPU by the project's
standing rule (tests/test_dfine_loss_gpu.py): max |kernel - ref64| <= 2 * max |torch fp32 on this device - ref64| + 1e-6 * max |ref64|,
where "torch fp32" is the same restatement in fp32 on the GPU with the same keep-masks.  The float64 inputs are the fp32 inputs
widened, so that no input rounding enters either error."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dfine_encoder_ref as ref

pytestmark = pytest.mark.gpu
P_DROP = 0.1
SEED = (0x1234 << 32) | 0x9abcdef1   # both key words in use


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


# ---- the attention core -----------------------------------------------------------------------------------------------------------
# The forward's tile is 32 queries x 32 keys, the backward's 64 x 64.  S: one key; less than a tile; on and one past each tile size
# (32, 33, 64, 65); one past a multiple of both (129); the trainers' 300 (neither tile divides it); D = 128.
ATTN_CASES = [(1, 1, 8, 1.0), (2, 17, 8, 1.0), (1, 32, 8, 1.0), (1, 64, 8, 1.0), (1, 65, 8, 8.0), (1, 129, 8, 1.0), (3, 300, 8, 1.0),
              (3, 300, 8, 8.0), (2, 33, 4, 1.0)]


def _attn_case(B, S, H, qscale, p, dev):
    """kernel, torch fp32 and float64 (out, d_qkv) of one case"""
    from defectdetection_viaobjectdetection_amd import dfine
    D = 32 * H
    x = _randn((B, S, 3 * D), 100 + S + H)
    x[..., :D] *= qscale   # logits of about +-30 at qscale 8: the softmax away from the uniform regime
    w = _randn((B, S, D), 7)
    mask = dfine.dropout_keep_mask(SEED, ref.SITE_ATTN, (B, H, S, S), p, dev) if p else None
    xk = x.to(dev).requires_grad_()
    out_k = dfine.self_attention(xk, H, p, SEED if p else None)
    res_k = (out_k, _grads(out_k, [xk], w)[0])
    xt = x.to(dev).requires_grad_()
    out_t = ref.self_attention(xt, H, mask, p)
    res_t = (out_t, _grads(out_t, [xt], w)[0])
    x64 = x.double().requires_grad_()
    out_w = ref.self_attention(x64, H, None if mask is None else mask.cpu(), p)
    res_w = (out_w, _grads(out_w, [x64], w)[0])
    return res_k, res_t, res_w


@pytest.mark.parametrize("B, S, H, qscale", ATTN_CASES)
def test_self_attention_forward_and_dqkv(cuda_device, B, S, H, qscale):
    res_k, res_t, res_w = _attn_case(B, S, H, qscale, 0.0, cuda_device)
    failures = []
    for name, k, t, w in zip(("out", "d_qkv"), res_k, res_t, res_w):
        assert k.is_cuda and k.dtype == torch.float32
        _judge(f"attention {B}x{S}x{H} q*{qscale:g} {name}", k, t, w, failures)
    assert not failures, failures


@pytest.mark.parametrize("B, S, H, qscale", [(2, 17, 8, 1.0), (1, 65, 8, 8.0), (3, 300, 8, 1.0), (2, 33, 4, 1.0)])
def test_self_attention_with_dropout(cuda_device, B, S, H, qscale):
    """p = 0.1: the float64 restatement is fed the mask the kernels use (odd S: a row's runs of four keys start at every alignment of the generator's groups of four)"""
    res_k, res_t, res_w = _attn_case(B, S, H, qscale, P_DROP, cuda_device)
    failures = []
    for name, k, t, w in zip(("out", "d_qkv"), res_k, res_t, res_w):
        _judge(f"attention p=0.1 {B}x{S}x{H} q*{qscale:g} {name}", k, t, w, failures)
    assert not failures, failures


def test_self_attention_non_contiguous_qkv(cuda_device):
    """a column slice of a wider buffer and a transposed view: handled (copied once), never read wrongly; the gradient comes
    back in the view's shape"""
    from defectdetection_viaobjectdetection_amd import dfine
    B, S, H = 2, 37, 2
    x = _randn((B, S, 3 * 32 * H), 3).to(cuda_device)
    want = dfine.self_attention(x, H)
    wide = torch.zeros(B, S, 3 * 32 * H + 5, device=cuda_device)
    wide[..., 5:] = x
    view = wide[..., 5:]            # row pitch 197 floats, start 20 bytes into the buffer
    assert not view.is_contiguous()
    assert torch.equal(dfine.self_attention(view, H), want)
    tview = x.transpose(0, 1).contiguous().transpose(0, 1).requires_grad_()
    assert not tview.is_contiguous()
    out = dfine.self_attention(tview, H)
    assert torch.equal(out, want)
    xr = x.clone().requires_grad_()
    g, = torch.autograd.grad(out.square().sum(), [tview])
    gw, = torch.autograd.grad(dfine.self_attention(xr, H).square().sum(), [xr])
    assert g.shape == x.shape and torch.equal(g, gw)


# ---- LayerNorm(x + dropout(y)) and dropout(relu(h)) -------------------------------------------------------------------------------
def _addln_case(M, D, p, dev):
    from defectdetection_viaobjectdetection_amd import dfine
    x, y = _randn((M, D), M + D), _randn((M, D), M + D + 1)
    if M > 1:   # a constant row: variance 0, eps alone keeps it finite
        x[M // 2] = 0.7
        y[M // 2] = 0.0
    wt, bs, gw = 1.0 + 0.1 * _randn((D,), 5), 0.1 * _randn((D,), 6), _randn((M, D), 8)
    mask = dfine.dropout_keep_mask(SEED, ref.SITE_FFN_OUT, (M, D), p, dev) if p else None
    res = []
    for kind in ("kernel", "torch", "ref64"):
        to = (lambda t: t.double()) if kind == "ref64" else (lambda t: t.to(dev))
        leaves = [to(t).requires_grad_() for t in (x, y, wt, bs)]
        if kind == "kernel":
            out = dfine.add_layer_norm(*leaves, 1e-5, p, SEED if p else None, site=ref.SITE_FFN_OUT)
        else:
            out = ref.add_layer_norm(*leaves, 1e-5, None if mask is None else (mask.cpu() if kind == "ref64" else mask), p)
        res.append((out,) + tuple(_grads(out, leaves, gw)))
    return res


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("M", [1, 63, 300, 900])
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_add_layer_norm(cuda_device, M, D, p):
    res_k, res_t, res_w = _addln_case(M, D, p, cuda_device)
    failures = []
    for name, k, t, w in zip(("out", "dx", "dy", "dweight", "dbias"), res_k, res_t, res_w):
        assert torch.isfinite(k).all(), name
        _judge(f"add_layer_norm {M}x{D} p={p:g} {name}", k, t, w, failures)
    assert not failures, failures


@pytest.mark.parametrize("shape", [(1, 1024), (63, 1024), (300, 1024), (5, 1023)])
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_relu_dropout(cuda_device, shape, p):
    """the hidden width 1024, and a tensor whose last group of four is short"""
    from defectdetection_viaobjectdetection_amd import dfine
    h, gw = _randn(shape, 11), _randn(shape, 12)
    mask = dfine.dropout_keep_mask(SEED, ref.SITE_FFN, shape, p, cuda_device) if p else None
    hk = h.to(cuda_device).requires_grad_()
    out_k = dfine.relu_dropout(hk, p, SEED if p else None)
    ht = h.to(cuda_device).requires_grad_()
    out_t = ref.relu_dropout(ht, mask, p)
    h64 = h.double().requires_grad_()
    out_w = ref.relu_dropout(h64, None if mask is None else mask.cpu(), p)
    failures = []
    _judge(f"relu_dropout {shape} p={p:g} out", out_k, out_t, out_w, failures)
    _judge(f"relu_dropout {shape} p={p:g} dh", _grads(out_k, [hk], gw)[0], _grads(out_t, [ht], gw)[0], _grads(out_w, [h64], gw)[0], failures)
    assert not failures, failures


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site, shape", [(ref.SITE_ATTN, (2, 4, 17, 17)), (ref.SITE_ATTN_OUT, (7, 251)), (ref.SITE_FFN, (5, 1023)),
                                         (ref.SITE_FFN_OUT, (3, 3, 3)), (ref.SITE_ATTN, (1,))])
def test_keep_mask_equals_the_numpy_restatement(cuda_device, site, shape):
    from defectdetection_viaobjectdetection_amd import dfine
    got = dfine.dropout_keep_mask(SEED, site, shape, P_DROP, cuda_device)
    assert got.dtype == torch.bool and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), ref.keep_mask(SEED, site, shape, P_DROP))


def test_keep_rate_and_seeds(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    n = 8 * 300 * 300
    a = dfine.dropout_keep_mask(SEED, ref.SITE_ATTN, (8, 300, 300), P_DROP, cuda_device)
    rate = float(a.float().mean())
    print(f"keep rate {rate:.6f} on {n} elements")
    assert abs(rate - (1 - P_DROP)) <= 4 * math.sqrt(P_DROP * (1 - P_DROP) / n)
    b = dfine.dropout_keep_mask(SEED + 1, ref.SITE_ATTN, (8, 300, 300), P_DROP, cuda_device)
    assert not torch.equal(a, b)
    assert dfine.dropout_keep_mask(SEED, ref.SITE_ATTN, (64, 64), 0.0, cuda_device).all()


def _three_ops(dev, p, seed, B=3, S=70, H=2):
    """the three ops and all their gradients on fixed inputs -> dict of tensors"""
    from defectdetection_viaobjectdetection_amd import dfine
    D = 32 * H
    kw = {} if p is None else {"dropout_p": p, "seed": seed}
    out = {}
    qkv = _randn((B, S, 3 * D), 21).to(dev).requires_grad_()
    a = dfine.self_attention(qkv, H, **kw)
    out["attn"], out["d_qkv"] = a, _grads(a, [qkv], _randn((B, S, D), 22))[0]
    leaves = [t.to(dev).requires_grad_() for t in (_randn((B, S, D), 23), _randn((B, S, D), 24), _randn((D,), 25), _randn((D,), 26))]
    n = dfine.add_layer_norm(*leaves, 1e-5, **kw)
    out["ln"] = n
    out["ln_dx"], out["ln_dy"], out["ln_dw"], out["ln_db"] = _grads(n, leaves, _randn((B, S, D), 27))
    h = _randn((B, S, 1024), 28).to(dev).requires_grad_()
    r = dfine.relu_dropout(h, **kw)
    out["relu"], out["relu_dh"] = r, _grads(r, [h], _randn((B, S, 1024), 29))[0]
    return out


def test_same_seed_same_bits_and_p0_is_the_plain_call(cuda_device):
    a, b = _three_ops(cuda_device, P_DROP, SEED), _three_ops(cuda_device, P_DROP, SEED)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = _three_ops(cuda_device, P_DROP, SEED + 1)
    assert not torch.equal(a["attn"], c["attn"]) and not torch.equal(a["ln"], c["ln"]) and not torch.equal(a["relu"], c["relu"])
    plain, p0 = _three_ops(cuda_device, None, None), _three_ops(cuda_device, 0.0, SEED)
    for k in plain:
        assert torch.equal(plain[k], p0[k]), k


def test_seed_none_draws_from_the_default_generator(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    h = _randn((64, 1024), 1).to(cuda_device)
    torch.manual_seed(77)
    a = dfine.relu_dropout(h, P_DROP)
    b = dfine.relu_dropout(h, P_DROP)
    torch.manual_seed(77)
    assert torch.equal(dfine.relu_dropout(h, P_DROP), a) and not torch.equal(a, b)


def test_frame_of_a_batch_equals_the_frame_alone(cuda_device):
    """frame 1 of a batch of 3 against the same frame as a batch of 1, bit for bit, outputs and per-frame gradients of the three
    ops (p = 0: a frame's mask index contains its position).  dweight / dbias are sums over all frames and are not compared."""
    from defectdetection_viaobjectdetection_amd import dfine
    dev, H, S, D = cuda_device, 8, 300, 256
    qkv, w = _randn((3, S, 3 * D), 31).to(dev), _randn((3, S, D), 32).to(dev)
    x, y, wt, bs = _randn((3, S, D), 33).to(dev), _randn((3, S, D), 34).to(dev), _randn((D,), 35).to(dev), _randn((D,), 36).to(dev)
    h, hw = _randn((3, S, 1024), 37).to(dev), _randn((3, S, 1024), 38).to(dev)

    def run(sl):
        q = qkv[sl].clone().requires_grad_()
        a = dfine.self_attention(q, H)
        xs, ys = x[sl].clone().requires_grad_(), y[sl].clone().requires_grad_()
        n = dfine.add_layer_norm(xs, ys, wt, bs, 1e-5)
        hs = h[sl].clone().requires_grad_()
        r = dfine.relu_dropout(hs)
        return (a, _grads(a, [q], w[sl])[0], n) + tuple(_grads(n, [xs, ys], w[sl])) + (r, _grads(r, [hs], hw[sl])[0])

    full, alone = run(slice(0, 3)), run(slice(1, 2))
    for i, (f, a) in enumerate(zip(full, alone)):
        assert torch.equal(f[1:2], a), i


def test_nothing_is_saved_without_grad(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    qkv = _randn((1, 9, 96), 41).to(cuda_device)
    assert dfine.self_attention(qkv, 1).grad_fn is None
    qkv.requires_grad_()
    assert dfine.self_attention(qkv, 1).grad_fn is not None
    with torch.no_grad():
        assert dfine.self_attention(qkv, 1).grad_fn is None
        assert dfine.relu_dropout(qkv).grad_fn is None
        assert dfine.add_layer_norm(qkv, qkv, torch.ones(96, device=cuda_device), torch.zeros(96, device=cuda_device), 1e-5).grad_fn is None


# ---- the layer and the encoder ------------------------------------------------------------------------------------------------------
ENC_SHAPE = (3, 300, 256)


def _encoder_grads(enc, x, w):
    xr = x.clone().requires_grad_()
    out = enc(xr)
    params = [p for layer in enc.layers for p in ref.layer_params(layer).values()]
    grads = torch.autograd.grad((out * w.to(out.device, out.dtype)).sum(), [xr] + params)
    return out, grads


@pytest.fixture(scope="module", params=["tiny", "default"])
def encoder_case(request):
    """4 layers as the trainers build and initialise them (or torch's default initialisation), the input, and the float64 output
    and gradients of torch's own module on the CPU: computed once, shared, left unchanged"""
    enc = ref.make_encoder(request.param, seed=3)
    x, w = _randn(ENC_SHAPE, 51), _randn(ENC_SHAPE, 52)
    enc64 = copy.deepcopy(enc).double().train()
    out, grads = _encoder_grads(enc64, x.double(), w)
    return request.param, enc, x, w, out.detach(), [g.detach() for g in grads]


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_bound_encoder_against_float64(cuda_device, encoder_case, mode):
    """output, d_input and the 12 parameter gradients of each of the 4 layers; dropout 0, so eval and training agree in float64"""
    from defectdetection_viaobjectdetection_amd import dfine
    init, enc, x, w, out_w, grads_w = encoder_case
    unbound = copy.deepcopy(enc).to(cuda_device)
    bound = dfine.bind_encoder(copy.deepcopy(enc).to(cuda_device))
    getattr(unbound, mode)()
    getattr(bound, mode)()
    before = dict(dfine.encoder_calls)
    out_k, grads_k = _encoder_grads(bound, x.to(cuda_device), w)
    assert dfine.encoder_calls == {"kernel": before["kernel"] + 4, "torch": before["torch"]}   # the kernels ran: no fallback
    out_t, grads_t = _encoder_grads(unbound, x.to(cuda_device), w)
    names = ["d_input"] + [f"layers.{i}.{n}" for i in range(4) for n in ref.PARAM_NAMES]
    failures = []
    _judge(f"{init} {mode} output", out_k, out_t, out_w, failures)
    for n, k, t, wv in zip(names, grads_k, grads_t, grads_w):
        _judge(f"{init} {mode} {n}", k, t, wv, failures)
    assert not failures, failures


def test_bound_layer_with_dropout_against_float64(cuda_device):
    """one trainers' layer in training mode at p = 0.1: the four seeds are the next four draws of the default generator, in the
    order attention, after out_proj, FFN, after linear2; the float64 restatement is fed the masks of those seeds"""
    from defectdetection_viaobjectdetection_amd import dfine
    B, S, D, H = 2, 65, 256, 8
    torch.manual_seed(4)
    layer = torch.nn.TransformerEncoderLayer(D, H, 1024, P_DROP, batch_first=True)
    x, w = _randn((B, S, D), 61), _randn((B, S, D), 62)
    bound = dfine.bind_encoder(copy.deepcopy(layer).to(cuda_device)).train()
    torch.manual_seed(9)
    seeds = [dfine._draw_seed() for _ in range(4)]
    shapes = {ref.SITE_ATTN: (B, H, S, S), ref.SITE_ATTN_OUT: (B, S, D), ref.SITE_FFN: (B, S, 1024), ref.SITE_FFN_OUT: (B, S, D)}
    masks = {site: dfine.dropout_keep_mask(seed, site, shapes[site], P_DROP, cuda_device) for site, seed in zip(shapes, seeds)}
    torch.manual_seed(9)
    xk = x.to(cuda_device).requires_grad_()
    out_k = bound(xk)
    pk = list(ref.layer_params(bound).values())
    res_k = (out_k,) + tuple(_grads(out_k, [xk] + pk, w))
    torch.manual_seed(9)
    assert torch.equal(bound(xk), out_k)                      # torch.manual_seed makes the run reproducible
    assert not torch.equal(bound(xk), out_k)                  # and the next call draws new seeds
    res = []
    for kind in ("torch", "ref64"):
        m = copy.deepcopy(layer).double() if kind == "ref64" else copy.deepcopy(layer).to(cuda_device)
        xi = (x.double() if kind == "ref64" else x.to(cuda_device)).requires_grad_()
        mk = {s: (v.cpu() if kind == "ref64" else v) for s, v in masks.items()}
        out = ref.encoder_layer(xi, ref.layer_params(m), H, m.norm1.eps, mk, P_DROP)
        res.append((out,) + tuple(_grads(out, [xi] + list(ref.layer_params(m).values()), w)))
    failures = []
    for n, k, t, wv in zip(("output", "d_input") + ref.PARAM_NAMES, res_k, *res):
        _judge(f"layer p=0.1 {n}", k, t, wv, failures)
    assert not failures, failures
    bound.eval()
    assert torch.equal(bound(xk), bound(xk))                  # no dropout outside training


def _adam_run(enc, heads, x, target, steps=3):
    """the trainers' loop: Adam(lr=1e-5) on the encoder's parameters alone, clip_grad_norm_ 1.0"""
    opt = torch.optim.Adam(enc.parameters(), lr=1e-5)
    enc.train()
    for _ in range(steps):
        fused = enc(x)
        loss = heads[0](fused).clamp(-20, 20).logsumexp(-1).mean() + (heads[1](fused).sigmoid() - target).abs().mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(enc.parameters(), max_norm=1.0)
        opt.step()
    return [p.detach() for p in enc.parameters()]


@pytest.mark.parametrize("init", ["tiny", "default"])
def test_three_adam_steps(cuda_device, init):
    """the parameters after three steps of the trainers' optimiser on a loss of two nn.Linear heads, bound and unbound, against
    the same three steps in float64, per parameter tensor by the rule at the top of this file.

    A sensitive check by construction: Adam's step lr * m / (sqrt(v) + eps) has slope lr * eps / (|g| + eps)^2 in the gradient,
    1e3 where |g| is below its eps of 1e-8, so a tensor's largest error is set by the few elements whose gradient lies within
    a few 1e-8 of zero, where the fp32 rounding noise of either path is multiplied by up to 1e3.  Measured on an MI355X, tensor
    self_attn.out_proj.weight of the four "tiny" layers, kernel / torch fp32: 5.3e-8 / 8.2e-8, 4.2e-8 / 2.6e-8, 1.14e-7 / 8.6e-8,
    2.6e-8 / 2.5e-8 (max |ref| 5e-3): torch's own error spreads 3.4 x over the layers.  All 96 tensors meet the rule."""
    from defectdetection_viaobjectdetection_amd import dfine
    enc = ref.make_encoder(init, seed=5)
    with torch.random.fork_rng():
        torch.manual_seed(6)
        heads = [torch.nn.Linear(256, 12), torch.nn.Linear(256, 4)]
    for hd in heads:
        hd.requires_grad_(False)
    x, target = _randn((2, 150, 256), 71), torch.rand((2, 150, 4), generator=torch.Generator().manual_seed(72))
    want = _adam_run(copy.deepcopy(enc).double(), [copy.deepcopy(hd).double() for hd in heads], x.double(), target.double())
    dev_heads = [copy.deepcopy(hd).to(cuda_device) for hd in heads]
    base = _adam_run(copy.deepcopy(enc).to(cuda_device), dev_heads, x.to(cuda_device), target.to(cuda_device))
    before = dict(dfine.encoder_calls)
    got = _adam_run(dfine.bind_encoder(copy.deepcopy(enc).to(cuda_device)), dev_heads, x.to(cuda_device), target.to(cuda_device))
    assert dfine.encoder_calls == {"kernel": before["kernel"] + 12, "torch": before["torch"]}
    names = [n for n, _ in enc.named_parameters()]
    failures = []
    for n, k, t, w in zip(names, got, base, want):
        _judge(f"adam {init} {n}", k, t, w, failures)
    assert any(not torch.equal(k.cpu(), p0.detach()) for k, p0 in zip(got, enc.parameters()))   # the steps moved the parameters
    assert not failures, failures


def test_state_dict_is_unchanged_on_the_device(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    enc = ref.make_encoder("tiny", seed=8, num_layers=2).to(cuda_device)
    want = {k: v.clone() for k, v in enc.state_dict().items()}
    assert dfine.bind_encoder(enc) is enc
    got = enc.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    other = ref.make_encoder("default", seed=9, num_layers=2)
    enc.load_state_dict(other.state_dict())
    x = _randn((1, 20, 256), 81).to(cuda_device)
    with torch.no_grad():
        a, b = enc.eval()(x), other.to(cuda_device).eval()(x)
    assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())   # the loaded weights are the ones that run


def test_fallbacks_on_the_device(cuda_device):
    """a mask, autocast and fp64 on CUDA tensors go to torch's forward: the unbound layer's bits, and the path counter says so"""
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(3)
    layer = torch.nn.TransformerEncoderLayer(64, 2, 128, 0.0, batch_first=True).to(cuda_device)
    bound = dfine.bind_encoder(copy.deepcopy(layer))
    x = _randn((2, 9, 64), 91).to(cuda_device)
    before = dict(dfine.encoder_calls)
    mask = torch.zeros(9, 9, device=cuda_device)
    assert torch.equal(bound(x, src_mask=mask), layer(x, src_mask=mask))
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(bound(x), layer(x))
    assert torch.equal(bound.double()(x.double()), layer.double()(x.double()))
    assert dfine.encoder_calls == {"kernel": before["kernel"], "torch": before["torch"] + 3}
    bound.float()(x)
    assert dfine.encoder_calls["kernel"] == before["kernel"] + 1


def test_c_entries_reject_bad_arguments_on_the_device(cuda_device):
    """real device buffers: every bad call returns M355_ERR_INVALID (-1) and leaves the outputs untouched (nothing launched)"""
    from defectdetection_viaobjectdetection_amd import _capi
    lib = _capi.lib
    qkv = torch.zeros(1, 4, 3 * 256, device=cuda_device)
    out = torch.full((1, 4, 256), 7.0, device=cuda_device)
    lse = torch.full((1, 8, 4), 7.0, device=cuda_device)
    work = torch.zeros(16, dtype=torch.uint8, device=cuda_device)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.m355_dfine_attn_forward(None, 1, 4, 8, 32, 0.0, 0, 0, p(out), p(lse), None) == -1
    assert lib.m355_dfine_attn_forward(p(qkv), 1, 0, 8, 32, 0.0, 0, 0, p(out), p(lse), None) == -1
    assert lib.m355_dfine_attn_forward(p(qkv), 1, 4, 8, 64, 0.0, 0, 0, p(out), p(lse), None) == -1
    assert lib.m355_dfine_attn_forward(p(qkv), 1, 4, 8, 32, 1.0, 0, 0, p(out), p(lse), None) == -1
    assert lib.m355_dfine_addln_backward(p(out), p(out), p(out), p(out), p(lse), p(lse), 4, 256, 0.0, 0, 1, p(out), p(out), p(out),
                                         p(out), p(work), work.numel(), None) == -1
    assert b"workspace" in lib.m355_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())
