"""The context GRU without a GPU: the float64 restatement of tests/dfine_gru_ref.py against torch's own nn.GRU, the binding's
fallback on CPU tensors, and the host-side argument checks of the three C entry points (csrc/dfine_gru.hip)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import dfine_gru_ref as ref

FAKE = C.c_void_p(0x1000)   # never dereferenced: every rejection precedes every HIP call


def _pack(gru):
    sfx = ("", "_reverse") if gru.bidirectional else ("",)
    get = lambda name: [getattr(gru, f"{name}_l0{s}").detach() for s in sfx]
    return torch.cat(get("weight_ih")), torch.cat(get("bias_ih")), torch.stack(get("weight_hh")), torch.stack(get("bias_hh"))


@pytest.mark.parametrize("bidirectional", [False, True])
@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("B, S", [(1, 1), (2, 7)])
def test_restatement_equals_float64_gru(bidirectional, with_h0, B, S):
    I, H, D = 5, 6, 2 if bidirectional else 1
    gen = torch.Generator().manual_seed(11 + S)
    with torch.random.fork_rng():
        torch.manual_seed(3)
        gru = torch.nn.GRU(I, H, batch_first=True, bidirectional=bidirectional).double()
    x = torch.randn((B, S, I), generator=gen, dtype=torch.float64, requires_grad=True)
    h0 = torch.randn((D, B, H), generator=gen, dtype=torch.float64, requires_grad=True) if with_h0 else None
    w_out = torch.randn((B, S, D * H), generator=gen, dtype=torch.float64)
    w_hn = torch.randn((D, B, H), generator=gen, dtype=torch.float64)
    out, h_n = gru(x, h0)
    ((out * w_out).sum() + (h_n * w_hn).sum()).backward()

    w_ih, b_ih, w_hh, b_hh = (t.numpy() for t in _pack(gru))
    xn = x.detach().numpy()
    gi = xn @ w_ih.T + b_ih
    o, hn, gates = ref.forward(gi, w_hh, b_hh, None if h0 is None else h0.detach().numpy())
    g_gi, g_w, g_b, g_h0 = ref.backward(w_out.numpy(), w_hn.numpy(), w_hh, gates)
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy() if torch.is_tensor(b) else b, rtol=1e-10, atol=1e-12)
    close(o, out)
    close(hn, h_n)
    close(g_gi @ w_ih, x.grad)
    flat = g_gi.reshape(B * S, -1)
    sfx = ("", "_reverse") if bidirectional else ("",)
    close(flat.T @ xn.reshape(B * S, I), torch.cat([getattr(gru, f"weight_ih_l0{s}").grad for s in sfx]))
    close(flat.sum(0), torch.cat([getattr(gru, f"bias_ih_l0{s}").grad for s in sfx]))
    close(g_w, torch.stack([getattr(gru, f"weight_hh_l0{s}").grad for s in sfx]))
    close(g_b, torch.stack([getattr(gru, f"bias_hh_l0{s}").grad for s in sfx]))
    if with_h0:
        close(g_h0, h0.grad)


def test_backward_without_grad_h_n():
    gen = np.random.default_rng(5)
    gi, w, b = gen.standard_normal((2, 4, 18)), gen.standard_normal((1, 18, 6)), gen.standard_normal((1, 18))
    g = gen.standard_normal((2, 4, 6))
    _, _, gates = ref.forward(gi, w, b)
    for got, want in zip(ref.backward(g, None, w, gates), ref.backward(g, np.zeros((1, 2, 6)), w, gates)):
        assert np.array_equal(got, want)


def test_bound_gru_on_cpu_returns_torchs_bits():
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(1)
    gru = torch.nn.GRU(256, 256, batch_first=True, bidirectional=True)
    bound = dfine.bind_gru(copy.deepcopy(gru))
    x = torch.randn(1, 9, 256)
    h0 = torch.randn(2, 1, 256)
    before = dict(dfine.gru_calls)
    for args in ((x,), (x, h0)):
        got, want = bound(*args), gru(*args)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # CPU tensors are the fallback's: the torch counter moves, the kernel counter stays (it moves in tests/test_dfine_gru_gpu.py)
    assert dfine.gru_calls == {"kernel": before["kernel"], "torch": before["torch"] + 2}
    assert set(dfine.gru_calls) == {"kernel", "torch"}


def test_bind_gru_leaves_class_and_state_dict_alone():
    from defectdetection_viaobjectdetection_amd import dfine
    class_forward = torch.nn.GRU.forward
    holder = torch.nn.Sequential(torch.nn.Linear(4, 4))
    holder.add_module("context_aggregator", torch.nn.GRU(256, 256, batch_first=True, bidirectional=True))
    keys = list(holder.state_dict())
    names = [n for n, _ in holder.named_parameters()]
    assert dfine.bind_gru(holder) is holder
    assert torch.nn.GRU.forward is class_forward
    assert list(holder.state_dict()) == keys and [n for n, _ in holder.named_parameters()] == names
    assert holder.context_aggregator.forward.__func__ is dfine.gru_forward
    assert "forward" not in vars(torch.nn.GRU(4, 4))            # another instance is untouched
    fresh = torch.nn.GRU(256, 256, batch_first=True, bidirectional=True)
    holder.context_aggregator.load_state_dict(fresh.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(holder.context_aggregator.state_dict().values(), fresh.state_dict().values()))


def _fwd(lib, *, gi=FAKE, w=FAKE, b=FAKE, h0=None, B=1, S=4, H=256, D=2, out=FAKE, h_n=FAKE, work=FAKE, work_bytes=None, keep=1,
         status=FAKE):
    if work_bytes is None:
        work_bytes = lib.m355_dfine_gru_workspace_bytes(B, S if keep else 0, H, D) or 1 << 30
    return lib.m355_dfine_gru_forward(gi, w, b, h0, B, S, H, D, out, h_n, work, work_bytes, keep, status, None)


def _bwd(lib, *, go=FAKE, ghn=None, w=FAKE, h0=None, out=FAKE, B=1, S=4, H=256, D=2, ggi=FAKE, gan=FAKE, gh0=FAKE, work=FAKE,
         work_bytes=None, status=FAKE):
    if work_bytes is None:
        work_bytes = lib.m355_dfine_gru_workspace_bytes(B, S, H, D) or 1 << 30
    return lib.m355_dfine_gru_backward(go, ghn, w, h0, out, B, S, H, D, ggi, gan, gh0, work, work_bytes, status, None)


def test_c_entries_refuse_every_limit_before_any_device_work():
    """fake device pointers on a machine that may have no GPU: M355_ERR_INVALID (-1) means the host check decided"""
    from defectdetection_viaobjectdetection_amd import _capi
    lib = _capi.lib
    odd = C.c_void_p(0x1004)
    need = lib.m355_dfine_gru_workspace_bytes(1, 4, 256, 2)
    bad_shapes = [dict(H=128), dict(H=512), dict(D=0), dict(D=3), dict(B=0), dict(B=9), dict(B=9, D=1), dict(B=16, D=1), dict(B=-1),
                  dict(S=0), dict(S=-5), dict(S=(1 << 24) + 1)]
    fwd_bad = bad_shapes + [dict(gi=None), dict(w=None), dict(b=None), dict(out=None), dict(h_n=None), dict(work=None),
                            dict(status=None), dict(gi=odd), dict(w=odd), dict(b=odd), dict(h0=odd), dict(out=odd), dict(h_n=odd),
                            dict(work=odd), dict(status=C.c_void_p(0x1002)), dict(work_bytes=need - 1), dict(work_bytes=-1),
                            dict(work_bytes=lib.m355_dfine_gru_workspace_bytes(1, 0, 256, 2) - 1, keep=0)]
    for kw in fwd_bad:
        assert _fwd(lib, **kw) == -1, kw
        assert b"dfine_gru_forward" in lib.m355_last_error(None), kw
    bwd_bad = bad_shapes + [dict(go=None), dict(w=None), dict(out=None), dict(ggi=None), dict(gan=None), dict(gh0=None),
                            dict(work=None), dict(status=None), dict(go=odd), dict(ghn=odd), dict(w=odd), dict(h0=odd), dict(out=odd),
                            dict(ggi=odd), dict(gan=odd), dict(gh0=odd), dict(work=odd), dict(work_bytes=need - 1),
                            dict(work_bytes=lib.m355_dfine_gru_workspace_bytes(1, 0, 256, 2))]   # the keep == 0 size: no gates
    for kw in bwd_bad:
        assert _bwd(lib, **kw) == -1, kw
        assert b"dfine_gru_backward" in lib.m355_last_error(None), kw


def test_workspace_bytes_is_monotone_and_zero_outside_the_limits():
    from defectdetection_viaobjectdetection_amd import _capi
    size = _capi.lib.m355_dfine_gru_workspace_bytes
    for D in (1, 2):
        for B in range(1, 9):
            row = [size(B, S, 256, D) for S in (0, 1, 2, 3, 300, 1031, 15000)]
            assert row[0] > 0 and all(a < b for a, b in zip(row, row[1:])), (B, D, row)
            assert size(B, 5, 256, D) - size(B, 4, 256, D) == B * D * 4 * 256 * 4     # r, z, n, a_n of one step
        for S in (0, 1, 300):
            col = [size(B, S, 256, D) for B in range(1, 9)]
            assert all(a < b for a, b in zip(col, col[1:])), (S, D, col)
    assert size(1, 15000, 256, 2) % 16 == 0
    for bad in ((0, 4, 256, 2), (9, 4, 256, 2), (9, 4, 256, 1), (16, 0, 256, 1), (1, -1, 256, 2), (1, 4, 128, 2), (1, 4, 256, 3)):
        assert size(*bad) == 0, bad
