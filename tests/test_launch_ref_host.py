"""CPU checks of tests/launch_ref.py: the packed layouts (written from include/mi355yolo.h), unpacked by plain restatements of
the kernels' arithmetic, reproduce F.conv2d / autograd; and the per-element check and the guard band catch what rel-L2 misses."""
import pytest
import torch
import torch.nn.functional as F

import launch_ref as L


def _operands(B, H, W, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g).half().double()
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half().double()
    return x, w, g


@pytest.mark.parametrize("B,H,W,cin,cout,k,s", [(2, 7, 9, 8, 24, 3, 1), (1, 9, 6, 16, 8, 3, 2), (2, 5, 5, 24, 16, 1, 1),
                                                (1, 6, 8, 8, 16, 2, 2)])
def test_forward_packing_reproduces_conv2d(B, H, W, cin, cout, k, s):
    x, w, _ = _operands(B, H, W, cin, cout, k, B + H + cin)
    pad = k // 2 if k != 2 else 0
    got = L.igemm_conv(x.float(), L.pack_fwd(w), cout, k, s, pad)
    assert L.pack_fwd(w).shape[0] % 128 == 0 and L.pack_fwd(w).shape[1] % 64 == 0
    assert torch.allclose(got.double(), L.conv_ref(x, w, s, pad), atol=1e-5)


def _autograd_dx(x, w, stride, pad):
    xa = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xa, w, None, stride, pad)
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64).half().double()
    y.backward(dy)
    return dy.permute(0, 2, 3, 1), xa.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,H,W,cin,cout,k", [(2, 7, 9, 16, 24, 3), (1, 5, 6, 8, 8, 1)])
def test_stride1_dgrad_packing_is_the_flipped_conv(B, H, W, cin, cout, k):
    x, w, _ = _operands(B, H, W, cin, cout, k, 11)
    dy, dx = _autograd_dx(x, w, 1, k // 2)
    got = L.igemm_conv(dy.float(), L.pack_dgrad_s1(w), cin, k, 1, k // 2)
    assert torch.allclose(got.double(), dx, atol=1e-5)
    assert torch.allclose(L.dgrad_ref(dy, w, H, W, 1, k // 2), dx, atol=1e-10)


@pytest.mark.parametrize("H,W", [(8, 10), (7, 9), (6, 5)])
def test_gather_packing_reproduces_the_stride2_input_gradient(H, W):
    x, w, _ = _operands(2, H, W, 16, 24, 3, H * W)
    dy, dx = _autograd_dx(x, w, 2, 1)
    got = L.igemm_gather(dy.float(), L.pack_dgrad_gather(w), H, W, 16)
    assert torch.allclose(got.double(), dx, atol=1e-5)


@pytest.mark.parametrize("cin,cout,compact", [(16, 24, False), (64, 64, True), (64, 96, False), (8, 32, False), (32, 64, False)])
def test_phase_packing_four_2x2_convs_equal_the_stride2_input_gradient(cin, cout, compact):
    """The four 2x2 phase convs over dY rebuilt from the packed rows (window or compact slots) equal x.grad of the stride-2 conv."""
    x, w, _ = _operands(2, 10, 6, cin, cout, 3, cin + cout)
    dy, dx = _autograd_dx(x, w, 2, 1)
    packed = L.pack_dgrad_phase(w, compact)
    assert packed.shape == (L.ceil_to(4 * cin, 128), L.ceil_to(4 * cout, 64))
    got = L.igemm_phase(dy.float(), packed, cin, compact)
    assert torch.allclose(got.double(), dx, atol=1e-5)
    if compact:   # compact: a phase's taps occupy only its first (1 + a)(1 + b) slots; the rest of the row is zero
        for a in (0, 1):
            for b in (0, 1):
                q, n = 2 * a + b, (1 + a) * (1 + b)
                assert not packed[q * cin:(q + 1) * cin, n * cout:].any()


def test_phase_form_rule():
    """Compact only where the K axis is whole 64-channel slices; window slots where a tile holds whole phases without a residual."""
    assert L.phase_form(64, 64, False) == 3 and L.phase_form(128, 256, True) == 3
    assert L.phase_form(64, 96, False) == 2 and L.phase_form(64, 96, True) == 2
    assert L.phase_form(32, 64, False) == 2 and L.phase_form(16, 32, False) == 2
    assert L.phase_form(32, 64, True) == 0 and L.phase_form(8, 32, False) == 0 and L.phase_form(48, 64, False) == 0


def test_convt_packing_reproduces_conv_transpose2d():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 7, 24, generator=g).half().double()
    w = (torch.randn(24, 16, 2, 2, generator=g) / 24 ** 0.5).half().double()
    got = L.igemm_convt(x.float(), L.pack_convt(w), 16)
    assert torch.allclose(got.double(), L.convt_ref(x, w), atol=1e-5)


def test_convt_dgrad_is_a_2x2_stride2_conv_in_the_forward_layout():
    """ConvT backward dX = the 2x2 / s2 conv of dY with the ConvT weight read as (cin rows, cout input channels)."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 6, 24, generator=g).double().permute(0, 3, 1, 2).requires_grad_(True)
    w = (torch.randn(24, 16, 2, 2, generator=g) / 24 ** 0.5).half().double()
    y = F.conv_transpose2d(x, w, None, 2)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64).half().double()
    y.backward(gy)
    got = L.igemm_conv(gy.permute(0, 2, 3, 1).float(), L.pack_fwd(w), 24, 2, 2, 0)
    assert torch.allclose(got.double(), x.grad.permute(0, 2, 3, 1), atol=1e-5)


def _ref_with_dropped_term():
    """A 3x3 conv whose output is 40 x 40 with 96 channels (ragged last 64-wide channel tile, ragged last 16-pixel tile),
    and the same output with ONE product term removed at the last tile's bottom-right corner pixel."""
    x, w, _ = _operands(2, 40, 40, 64, 96, 3, 21)
    ref, S = L.conv_ref(x, w, 1, 1), L.conv_ref(x.abs(), w.abs(), 1, 1)
    bad = ref.clone()
    b, h, wx, co = 1, 39, 39, 95                                # corner pixel of the last tile, last channel
    kh, kw, ci = 0, 0, 5                                        # tap (0, 0) reads input pixel (38, 38)
    bad[b, h, wx, co] -= x[b, h - 1 + kh, wx - 1 + kw, ci] * w[co, ci, kh, kw]
    return ref, S, bad, 9 * 64


def test_elementwise_bound_catches_one_dropped_product_that_rel_l2_misses():
    ref, S, bad, K = _ref_with_dropped_term()
    bound = L.elem_bound(ref, S, K)
    ok_ratio, ok_rel, _ = L.check_elementwise(ref.half().double(), ref, bound)      # a correct fp16 result passes
    assert ok_ratio <= 1.0 and ok_rel <= 1e-3
    ratio, rel, desc = L.check_elementwise(bad.half().double(), ref, bound)
    assert rel <= 1e-3, rel                                     # rel-L2 alone would accept it ...
    assert ratio > 1.0, desc                                    # ... the element-wise bound does not
    assert "(1, 39, 39, 95)" in desc


def test_elementwise_bound_rejects_a_doubled_product_of_average_size():
    x, w, _ = _operands(1, 6, 6, 32, 8, 3, 9)
    ref, S = L.conv_ref(x, w, 1, 1), L.conv_ref(x.abs(), w.abs(), 1, 1)
    K = 9 * 32
    bound = L.elem_bound(ref, S, K)
    bad = ref.clone()
    bad[0, 3, 3, 2] += S[0, 3, 3, 2] / K                        # one extra term of the average magnitude
    assert L.check_elementwise(bad, ref, bound)[0] > 1.0


def test_guard_band_catches_a_write_one_channel_past_the_slice():
    buf = L.Guarded(2, 3, 5, 40, "cpu")
    v = torch.randn(2, 3, 5, 16).half()
    buf.write(8, v)
    got, nbad, _ = buf.slice_and_guard(8, 16)
    assert nbad == 0 and torch.equal(got, v.float())
    buf.values()[1, 2, 4, 24] = 1.0                             # channel 24 = one past the slice [8, 24)
    _, nbad, first = buf.slice_and_guard(8, 16)
    assert nbad == 1 and "channel 24" in L.guard_report(buf, nbad, first)
    buf2 = L.Guarded(1, 2, 2, 8, "cpu", f32=True, bstride=64)   # image stride past the map: the gap is guarded too
    buf2.write(0, torch.zeros(1, 2, 2, 8))
    assert buf2.slice_and_guard(0, 8)[1] == 0
    buf2.bits[L.GUARD + 40] = 0                                 # inside the image-stride gap
    assert buf2.slice_and_guard(0, 8)[1] == 1
    buf2.bits[L.GUARD - 1] = 0                                  # the guard before the allocation
    assert buf2.slice_and_guard(0, 8)[1] == 2


def test_sentinels_are_nan_with_their_payloads():
    assert torch.isnan(torch.tensor([L.SENT16], dtype=torch.int16).view(torch.float16)).all()
    assert torch.isnan(torch.tensor([L.SENT32], dtype=torch.int32).view(torch.float32)).all()
