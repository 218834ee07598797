"""The context GRU on the GPU (csrc/dfine_gru.hip): dfine.gru_recurrence, its gradients, and the bound nn.GRU.

Every output and gradient tensor is held to float64 on the CPU by the project's standing rule (tests/test_dfine_encoder_gpu.py):
max |kernel - ref64| <= 2 * max |torch fp32 on this device - ref64| + 1e-6 * max |ref64|.  ref64 is nn.GRU in float64 on the CPU with
the fp32 parameters and inputs widened; "torch fp32" is the unbound nn.GRU on the GPU.  For gru_recurrence, whose input is the
pre-activation gi itself, both references are an nn.GRU whose weight_ih picks its direction's columns of gi (ones and zeros) and
whose bias_ih is zero: that product is exact in either precision, and the gradient of its input is d_gi."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
H = 256


def _judge(name, kernel, torch32, want, failures):
    w = want.detach().double().cpu()
    e_k = float((kernel.detach().double().cpu() - w).abs().max())
    e_t = float((torch32.detach().double().cpu() - w).abs().max())
    scale = float(w.abs().max())
    print(f"{name}: max error vs float64: kernel {e_k:.3e}, torch fp32 {e_t:.3e} (max |ref| {scale:.4g})")
    assert tuple(kernel.shape) == tuple(w.shape), name
    if not e_k <= 2 * e_t + 1e-6 * scale:
        failures.append((name, e_k, e_t, scale))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _inputs(B, S, D, scale, with_h0):
    """gi as the projection of unit-variance inputs through default-init weights leaves it (std 0.58), weight_hh / bias_hh at
    torch's default init U(-1/16, 1/16); scale 4 multiplies gi and weight_hh so that the gates saturate"""
    g = _gen(1000 * S + 10 * B + D)
    gi = torch.randn((B, S, D * 3 * H), generator=g) * (0.58 * scale)
    w = (torch.rand((D, 3 * H, H), generator=g) * 2 - 1) / 16 * scale
    b = (torch.rand((D, 3 * H), generator=g) * 2 - 1) / 16
    h0 = torch.randn((D, B, H), generator=g) * 0.5 if with_h0 else None
    w_out = torch.randn((B, S, D * H), generator=g)
    w_hn = torch.randn((D, B, H), generator=g)
    return gi, w, b, h0, w_out, w_hn


def _selector_gru(w, b, dtype, device):
    """nn.GRU(D * 3H, H) whose input projection hands column block d of its input to direction d unchanged"""
    D = w.shape[0]
    gru = torch.nn.GRU(D * 3 * H, H, batch_first=True, bidirectional=D == 2)
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")[:D]):
            sel = torch.zeros(3 * H, D * 3 * H)
            sel[:, d * 3 * H:(d + 1) * 3 * H] = torch.eye(3 * H)
            getattr(gru, f"weight_ih_l0{sfx}").copy_(sel)
            getattr(gru, f"bias_ih_l0{sfx}").zero_()
            getattr(gru, f"weight_hh_l0{sfx}").copy_(w[d])
            getattr(gru, f"bias_hh_l0{sfx}").copy_(b[d])
    return gru.to(device=device, dtype=dtype)


def _through_torch(B, S, D, scale, with_h0, use_hn, dtype, device):
    """out, h_n, d_gi, d_w_hh, d_b_hh, d_h0 (None without h0) of torch's own GRU"""
    gi, w, b, h0, w_out, w_hn = _inputs(B, S, D, scale, with_h0)
    gru = _selector_gru(w, b, dtype, device)
    x = gi.to(device=device, dtype=dtype).requires_grad_()
    h = None if h0 is None else h0.to(device=device, dtype=dtype).requires_grad_()
    out, h_n = gru(x, h)
    loss = (out * w_out.to(out)).sum()
    if use_hn:
        loss = loss + (h_n * w_hn.to(out)).sum()
    loss.backward()
    sfx = ("", "_reverse")[:D]
    return (out.detach(), h_n.detach(), x.grad, torch.stack([getattr(gru, f"weight_hh_l0{s}").grad for s in sfx]),
            torch.stack([getattr(gru, f"bias_hh_l0{s}").grad for s in sfx]), None if h is None else h.grad)


@functools.lru_cache(maxsize=None)
def _ref64(B, S, D, scale, with_h0, use_hn=True):
    return _through_torch(B, S, D, scale, with_h0, use_hn, torch.float64, "cpu")


def _through_kernel(B, S, D, scale, with_h0, use_hn, device, only_gi=False):
    from defectdetection_viaobjectdetection_amd import dfine
    gi, w, b, h0, w_out, w_hn = _inputs(B, S, D, scale, with_h0)
    leaves = [t.to(device).requires_grad_(not only_gi or i == 0) if t is not None else None for i, t in enumerate((gi, w, b, h0))]
    out, h_n = dfine.gru_recurrence(*leaves)
    loss = (out * w_out.to(device)).sum()
    if use_hn:
        loss = loss + (h_n * w_hn.to(device)).sum()
    loss.backward()
    return (out.detach(), h_n.detach()) + tuple(None if t is None else t.grad for t in leaves)


NAMES = ("out", "h_n", "d_gi", "d_w_hh", "d_b_hh", "d_h0")
# S: one step (no exchange at all in the forward), the first exchanges, both slots of the two-slot ring (2, 3), around a
# 32-step boundary, the trainers' Q = 300, and a prime over 1024; B: several chains per direction, and the most the grid takes.
SHAPES = [(1, S, D) for S in (1, 2, 3, 31, 32, 33, 300, 1031) for D in (1, 2)] + [(3, 33, 1), (3, 33, 2), (8, 2, 1), (8, 2, 2)]


@pytest.mark.parametrize("with_h0", [False, True], ids=["zeros", "h0"])
@pytest.mark.parametrize("scale", [1, 4], ids=["default", "saturated"])
@pytest.mark.parametrize("B, S, D", SHAPES)
def test_recurrence_and_gradients_against_float64(cuda_device, B, S, D, scale, with_h0):
    got = _through_kernel(B, S, D, scale, with_h0, True, cuda_device)
    base = _through_torch(B, S, D, scale, with_h0, True, torch.float32, cuda_device)
    want = _ref64(B, S, D, scale, with_h0)
    failures = []
    for name, k, t, w in zip(NAMES, got, base, want):
        if w is None:
            assert k is None, name
            continue
        _judge(f"B{B} S{S} D{D} x{scale} {name}", k, t, w, failures)
    assert not failures, failures


def test_without_grad_h_n(cuda_device):
    B, S, D = 1, 33, 2
    got = _through_kernel(B, S, D, 1, True, False, cuda_device)
    base = _through_torch(B, S, D, 1, True, False, torch.float32, cuda_device)
    want = _ref64(B, S, D, 1, True, False)
    failures = []
    for name, k, t, w in zip(NAMES, got, base, want):
        _judge(f"no grad_h_n {name}", k, t, w, failures)
    assert not failures, failures


def test_only_gi_requires_grad(cuda_device):
    B, S, D = 3, 33, 2
    got = _through_kernel(B, S, D, 1, True, True, cuda_device, only_gi=True)
    assert got[3] is None and got[4] is None and got[5] is None
    base = _through_torch(B, S, D, 1, True, True, torch.float32, cuda_device)
    want = _ref64(B, S, D, 1, True)
    failures = []
    for i in (0, 1, 2):
        _judge(f"only gi {NAMES[i]}", got[i], base[i], want[i], failures)
    assert not failures, failures
    full = _through_kernel(B, S, D, 1, True, True, cuda_device)
    assert torch.equal(full[2], got[2])


def test_nothing_is_saved_without_grad(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    gi, w, b, h0, _, _ = _inputs(1, 33, 2, 1, True)
    args = [t.to(cuda_device) for t in (gi, w, b, h0)]
    plain = dfine.gru_recurrence(*args)
    assert plain[0].grad_fn is None and plain[1].grad_fn is None
    with torch.no_grad():
        quiet = dfine.gru_recurrence(*[t.clone().requires_grad_() for t in args])
    assert quiet[0].grad_fn is None and not quiet[0].requires_grad
    kept = dfine.gru_recurrence(args[0].clone().requires_grad_(), *args[1:])
    assert kept[0].grad_fn is not None
    for a, c in zip(plain + quiet, kept + kept):
        assert torch.equal(a, c.detach())
    # the workspace of a call that keeps nothing is the exchange area alone
    from defectdetection_viaobjectdetection_amd._capi import lib
    assert lib.m355_dfine_gru_workspace_bytes(1, 0, H, 2) == 2 * 2 * 768 * 8


def test_reverse_direction_is_the_flipped_forward_direction(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    gi, w, b, h0, w_out, _ = (t.to(cuda_device) for t in _inputs(1, 33, 2, 1, True))
    w2, b2 = w.clone(), b.clone()
    w2[0], b2[0] = 0, 0
    both = [t.requires_grad_() for t in (gi.clone(), w2, b2, h0.clone())]
    out2, hn2 = dfine.gru_recurrence(*both)
    g2 = torch.autograd.grad((out2[..., H:] * w_out[..., H:]).sum(), [both[0], both[3]])
    one = [t.requires_grad_() for t in (gi[..., 3 * H:].flip(1).contiguous(), w[1:].clone(), b[1:].clone(), h0[1:].clone())]
    out1, hn1 = dfine.gru_recurrence(*one)
    g1 = torch.autograd.grad((out1 * w_out[..., H:].flip(1)).sum(), [one[0], one[3]])
    assert torch.equal(out2[..., H:], out1.flip(1)) and torch.equal(hn2[1], hn1[0])
    assert torch.equal(g2[0][..., 3 * H:], g1[0].flip(1)) and torch.equal(g2[1][1], g1[1][0])


def test_two_calls_give_equal_bits(cuda_device):
    for B, S, D in ((1, 300, 2), (3, 33, 2)):
        first = _through_kernel(B, S, D, 1, True, True, cuda_device)
        second = _through_kernel(B, S, D, 1, True, True, cuda_device)
        for name, a, c in zip(NAMES, first, second):
            assert torch.equal(a, c), (B, S, D, name)


def test_sequence_of_a_batch_equals_the_sequence_alone(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    gi, w, b, h0, w_out, w_hn = (t.to(cuda_device) for t in _inputs(3, 33, 2, 1, True))

    def run(sl):
        leaves = [gi[sl].clone().requires_grad_(), w, b, h0[:, sl].clone().requires_grad_()]
        out, h_n = dfine.gru_recurrence(*leaves)
        ((out * w_out[sl]).sum() + (h_n * w_hn[:, sl]).sum()).backward()
        return out.detach(), h_n.detach(), leaves[0].grad, leaves[3].grad

    batch, alone = run(slice(0, 3)), run(slice(1, 2))
    assert torch.equal(batch[0][1:2], alone[0]) and torch.equal(batch[1][:, 1:2], alone[1])
    assert torch.equal(batch[2][1:2], alone[2]) and torch.equal(batch[3][:, 1:2], alone[3])


def test_non_contiguous_gi(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    gi, w, b, h0, w_out, _ = (t.to(cuda_device) for t in _inputs(1, 33, 2, 1, True))
    wide = torch.zeros((1, 33, 2 * 3 * H + 8), device=cuda_device)
    wide[..., 4:4 + 2 * 3 * H] = gi
    view = wide[..., 4:4 + 2 * 3 * H]
    assert not view.is_contiguous()
    res = []
    for x in (gi.clone(), view):
        x = x.detach().requires_grad_()
        out, h_n = dfine.gru_recurrence(x, w, b, h0)
        (out * w_out).sum().backward()
        res.append((out.detach(), h_n.detach(), x.grad))
    for a, c in zip(*res):
        assert torch.equal(a, c)


# ---- the bound module -------------------------------------------------------------------------------------------------------------
def _module_run(gru, x, w_out, w_hn):
    x = x.clone().requires_grad_()
    out, h_n = gru(x)
    gru.zero_grad()
    ((out * w_out.to(out)).sum() + (h_n * w_hn.to(out)).sum()).backward()
    return [out.detach(), h_n.detach(), x.grad] + [p.grad.clone() for p in gru.parameters()]


@pytest.mark.parametrize("shape", [(1, 21, 256), (2, 300, 256)])
def test_bound_module_against_float64(cuda_device, shape):
    from defectdetection_viaobjectdetection_amd import dfine
    with torch.random.fork_rng():
        torch.manual_seed(17)
        gru = torch.nn.GRU(256, 256, batch_first=True, bidirectional=True)
    g = _gen(shape[1])
    x, w_out, w_hn = torch.randn(shape, generator=g), torch.randn(shape[:2] + (512,), generator=g), torch.randn((2, shape[0], 256), generator=g)
    want = _module_run(copy.deepcopy(gru).double(), x.double(), w_out, w_hn)
    base = _module_run(copy.deepcopy(gru).to(cuda_device), x.to(cuda_device), w_out, w_hn)
    bound = dfine.bind_gru(copy.deepcopy(gru).to(cuda_device))
    before = dict(dfine.gru_calls)
    got = _module_run(bound, x.to(cuda_device), w_out, w_hn)
    assert dfine.gru_calls == {"kernel": before["kernel"] + 1, "torch": before["torch"]}
    names = ["output", "h_n", "d_input"] + ["d_" + n for n, _ in gru.named_parameters()]
    assert len(names) == 11
    failures = []
    for n, k, t, w in zip(names, got, base, want):
        _judge(f"bound {shape} {n}", k, t, w, failures)
    assert not failures, failures


def test_bound_module_loads_an_unbound_state_dict(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(21)
    bound = dfine.bind_gru(torch.nn.GRU(256, 256, batch_first=True, bidirectional=True).to(cuda_device))
    other = torch.nn.GRU(256, 256, batch_first=True, bidirectional=True)
    keys = list(bound.state_dict())
    bound.load_state_dict(other.state_dict())
    assert list(bound.state_dict()) == keys == list(other.state_dict())
    x = torch.randn((1, 21, 256), generator=_gen(4)).to(cuda_device)
    with torch.no_grad():
        a, b = bound(x), other.to(cuda_device)(x)
    assert float((a[0] - b[0]).abs().max()) <= 1e-4 * float(b[0].abs().max())   # the loaded weights are the ones that run
    assert type(bound).forward is torch.nn.GRU.forward


@pytest.mark.parametrize("kind", ["hidden128", "two_layers", "time_major", "fp16"])
def test_fallbacks_return_torchs_bits(cuda_device, kind):
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(23)
    gru = {"hidden128": lambda: torch.nn.GRU(256, 128, batch_first=True, bidirectional=True),
           "two_layers": lambda: torch.nn.GRU(256, 256, num_layers=2, batch_first=True, bidirectional=True),
           "time_major": lambda: torch.nn.GRU(256, 256, batch_first=False, bidirectional=True),
           "fp16": lambda: torch.nn.GRU(256, 256, batch_first=True, bidirectional=True).half()}[kind]().to(cuda_device)
    bound = dfine.bind_gru(copy.deepcopy(gru))
    x = torch.randn((2, 9, 256), generator=_gen(5)).to(cuda_device)
    if kind == "fp16":
        x = x.half()
    before = dict(dfine.gru_calls)
    with torch.no_grad():
        got, want = bound(x), gru(x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert dfine.gru_calls == {"kernel": before["kernel"], "torch": before["torch"] + 1}


# ---- end to end -------------------------------------------------------------------------------------------------------------------
class _ContextStack(torch.nn.Module):
    """what the improved trainer applies to the temporal encoder's output `fused` (T, Q, 256): per-query frame weights from a
    two-layer scorer, the bidirectional GRU over all T * Q tokens as one sequence, a projection back to 256"""

    def __init__(self):
        super().__init__()
        self.scorer = torch.nn.Sequential(torch.nn.Linear(256, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1))
        self.context_aggregator = torch.nn.GRU(256, 256, batch_first=True, bidirectional=True)
        self.context_projector = torch.nn.Linear(512, 256)

    def forward(self, fused):
        T, Q, Dm = fused.shape
        weights = torch.softmax(self.scorer(fused), dim=0)
        context, _ = self.context_aggregator(fused.view(1, T * Q, Dm))
        return fused * weights + self.context_projector(context).view(T, Q, Dm)


def _adamw_run(model, fused, target, steps=3):
    opt = torch.optim.AdamW(model.parameters(), lr=5e-4, weight_decay=0.01)
    for _ in range(steps):
        loss = (model(fused) - target).pow(2).mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()
    return [p.detach() for p in model.parameters()]


def test_three_adamw_steps_of_the_context_stack(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    with torch.random.fork_rng():
        torch.manual_seed(29)
        model = _ContextStack()
    fused, target = torch.randn((3, 7, 256), generator=_gen(6)), torch.randn((3, 7, 256), generator=_gen(7))
    want = _adamw_run(copy.deepcopy(model).double(), fused.double(), target.double())
    base = _adamw_run(copy.deepcopy(model).to(cuda_device), fused.to(cuda_device), target.to(cuda_device))
    bound = copy.deepcopy(model).to(cuda_device)
    dfine.bind_gru(bound.context_aggregator)
    before = dict(dfine.gru_calls)
    got = _adamw_run(bound, fused.to(cuda_device), target.to(cuda_device))
    assert dfine.gru_calls == {"kernel": before["kernel"] + 3, "torch": before["torch"]}
    failures = []
    for (n, p0), k, t, w in zip(model.named_parameters(), got, base, want):
        _judge(f"adamw {n}", k, t, w, failures)
        assert not torch.equal(k.cpu(), p0.detach()), n   # the steps moved it
    assert not failures, failures


def test_status_word_is_clear_after_this_module(cuda_device):
    """last in the file: no workgroup of any launch above gave up waiting for its chain's other workgroups"""
    from defectdetection_viaobjectdetection_amd import dfine
    assert dfine.gru_status() == 0
