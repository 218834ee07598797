"""Host-side checks of the temporal-encoder work (no GPU): the torch restatement against the real module, the numpy mask generator
against published Philox vectors, bind_encoder's fallback on CPU tensors and for every condition the kernels do not take, and the C
entry points' argument checks with a fake device pointer (each rejection precedes every HIP call)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import dfine_encoder_ref as ref


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max())


def test_restatement_equals_the_torch_module_in_float64():
    """masks None: the restatement is nn.TransformerEncoderLayer(256, 8, 1024, 0.0, batch_first=True) to 1e-12 relative, values and
    gradients, so that the float64 reference of the GPU tests is torch's own module"""
    torch.manual_seed(0)
    layer = torch.nn.TransformerEncoderLayer(256, 8, 1024, 0.0, batch_first=True).double()
    x = torch.randn(2, 19, 256, dtype=torch.float64, requires_grad=True)
    for mode in (layer.train, layer.eval):
        mode()
        want = layer(x)
        got = ref.encoder_layer(x, ref.layer_params(layer), 8, layer.norm1.eps)
        assert _rel(got, want) <= 1e-12
        names = list(ref.PARAM_NAMES)
        params = [ref.layer_params(layer)[n] for n in names]
        w = torch.randn_like(want)
        g_want = torch.autograd.grad((want * w).sum(), [x] + params)
        g_got = torch.autograd.grad((got * w).sum(), [x] + params)
        for n, a, b in zip(["input"] + names, g_got, g_want):
            assert _rel(a, b) <= 1e-12, n


def test_restatement_ops_compose_to_the_layer():
    """the three op restatements with all-True masks equal the mask-free ones bit for bit when p = 0"""
    x = torch.randn(2, 5, 96, dtype=torch.float64)
    m = torch.ones(2, 1, 5, 5, dtype=torch.bool)
    assert torch.equal(ref.self_attention(x, 1, m, 0.0), ref.self_attention(x, 1))
    h = torch.randn(7, 12, dtype=torch.float64)
    assert torch.equal(ref.relu_dropout(h, torch.ones(7, 12, dtype=torch.bool), 0.0), torch.relu(h))


def test_philox_known_answer_vectors():
    """Random123's kat_vectors for philox4x32, 10 rounds"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        got = tuple(int(w[0]) for w in ref.philox4x32_10(counter, key))
        assert got == want, (counter, key, [hex(g) for g in got])


def test_numpy_mask_is_a_function_of_seed_site_and_index():
    a = ref.keep_mask(1234, ref.SITE_FFN, (3, 7, 5), 0.1)
    assert a.dtype == np.bool_ and a.shape == (3, 7, 5)
    assert np.array_equal(a.reshape(-1)[:50], ref.keep_mask(1234, ref.SITE_FFN, (50,), 0.1))      # the flat index alone
    assert not np.array_equal(a, ref.keep_mask(1235, ref.SITE_FFN, (3, 7, 5), 0.1))
    assert not np.array_equal(a, ref.keep_mask(1234, ref.SITE_FFN_OUT, (3, 7, 5), 0.1))
    assert not np.array_equal(a, ref.keep_mask(1234 + (1 << 32), ref.SITE_FFN, (3, 7, 5), 0.1))    # the seed's high word counts
    assert ref.keep_mask(7, 0, (1000,), 0.0).all()
    n = 8 * 300 * 300
    rate = ref.keep_mask(99, ref.SITE_ATTN, (n,), 0.1).mean()
    assert abs(rate - 0.9) <= 4 * np.sqrt(0.1 * 0.9 / n)


def _small_encoder(**kw):
    args = dict(d_model=64, nhead=2, dim_feedforward=128, dropout=0.0, batch_first=True)
    args.update(kw)
    torch.manual_seed(1)
    return torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(**args), num_layers=2, enable_nested_tensor=False)


def test_bind_encoder_on_cpu_tensors_is_the_unbound_encoder():
    from defectdetection_viaobjectdetection_amd import dfine
    enc = _small_encoder()
    bound = dfine.bind_encoder(copy.deepcopy(enc))
    assert bound is not enc and all("forward" in vars(l) for l in bound.layers)
    assert torch.nn.TransformerEncoderLayer.forward is not dfine.encoder_layer_forward      # torch's class is untouched
    assert all("forward" not in vars(l) for l in enc.layers)
    x = torch.randn(3, 11, 64)
    before = dict(dfine.encoder_calls)
    for mode in ("train", "eval"):
        getattr(enc, mode)()
        getattr(bound, mode)()
        assert torch.equal(bound(x), enc(x)), mode
    assert dfine.encoder_calls["kernel"] == before["kernel"] and dfine.encoder_calls["torch"] == before["torch"] + 4
    # gradients flow through the fallback as through torch's module
    x1, x2 = x.clone().requires_grad_(), x.clone().requires_grad_()
    enc.train()
    bound.train()
    bound(x1).square().sum().backward()
    enc(x2).square().sum().backward()
    assert torch.equal(x1.grad, x2.grad)
    for (n, a), (_, b) in zip(bound.named_parameters(), enc.named_parameters()):
        assert torch.equal(a.grad, b.grad), n


def test_bind_encoder_keeps_the_state_dict():
    from defectdetection_viaobjectdetection_amd import dfine
    enc = _small_encoder()
    want = {k: v.clone() for k, v in enc.state_dict().items()}
    bound = dfine.bind_encoder(enc)
    assert bound is enc
    got = enc.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    other = _small_encoder()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    enc.load_state_dict(other.state_dict())   # an unbound encoder's dict loads, strict
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), other.state_dict().values()))


@pytest.mark.parametrize("why, layer_kw, call_kw", [
    ("mask", {}, {"src_mask": torch.zeros(11, 11)}),
    ("padding mask", {}, {"src_key_padding_mask": torch.zeros(3, 11, dtype=torch.bool)}),
    ("is_causal", {}, {"src_mask": torch.nn.Transformer.generate_square_subsequent_mask(11), "is_causal": True}),
    ("norm_first", {"norm_first": True}, {}),
    ("gelu", {"activation": "gelu"}, {}),
    ("batch_first=False", {"batch_first": False}, {}),
    ("head dim 16", {"nhead": 4}, {}),
    ("float64", {"dtype": torch.float64}, {}),
    ("cpu", {}, {}),
])
def test_every_fallback_condition_goes_to_torchs_forward(why, layer_kw, call_kw):
    """each condition the kernels do not take: the bound layer's output on the CPU is the unbound layer's, bit for bit, and
    the conditions that lie in the module's settings are refused by the settings check alone, which does not look at the device"""
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(2)
    args = dict(d_model=64, nhead=2, dim_feedforward=128, dropout=0.0, batch_first=True)
    args.update(layer_kw)
    layer = torch.nn.TransformerEncoderLayer(**args)
    dtype = layer_kw.get("dtype", torch.float32)
    x = torch.randn(3, 11, 64, dtype=dtype)
    want = layer(x, **call_kw)
    bound = dfine.bind_encoder(copy.deepcopy(layer))
    before = dict(dfine.encoder_calls)
    got = bound(x, **call_kw)
    assert torch.equal(got, want)
    assert dfine.encoder_calls == {"kernel": before["kernel"], "torch": before["torch"] + 1}
    plain = torch.nn.TransformerEncoderLayer(d_model=64, nhead=2, dim_feedforward=128, dropout=0.0, batch_first=True)
    assert dfine._layer_is_kernel_shaped(plain) is True
    if why in ("norm_first", "gelu", "batch_first=False", "head dim 16"):   # decided by the module's settings, whatever the device
        assert dfine._layer_is_kernel_shaped(layer) is False
    else:                                                                   # decided by the call's arguments or tensors
        assert dfine._layer_is_kernel_shaped(layer) is True


def test_autocast_falls_back():
    from defectdetection_viaobjectdetection_amd import dfine
    plain = torch.nn.TransformerEncoderLayer(d_model=64, nhead=2, dim_feedforward=128, dropout=0.0, batch_first=True)
    x = torch.randn(2, 5, 64)
    bound = dfine.bind_encoder(copy.deepcopy(plain))
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert torch.equal(bound(x), plain(x))


def test_python_argument_checks():
    from defectdetection_viaobjectdetection_amd import dfine
    with pytest.raises(ValueError, match="head dim 32"):
        dfine.self_attention(torch.zeros(1, 4, 3 * 48), 3)
    with pytest.raises(ValueError, match="dropout_p"):
        dfine.self_attention(torch.zeros(1, 4, 96), 1, dropout_p=1.0)
    with pytest.raises(ValueError, match="multiple of 4"):
        dfine.add_layer_norm(torch.zeros(2, 6), torch.zeros(2, 6), torch.ones(6), torch.zeros(6), 1e-5)
    with pytest.raises(ValueError, match="one shape"):
        dfine.add_layer_norm(torch.zeros(2, 8), torch.zeros(3, 8), torch.ones(8), torch.zeros(8), 1e-5)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        dfine.relu_dropout(torch.zeros(8))    # the ops themselves have no CPU path: only the layer falls back


def test_seed_comes_from_the_default_generator():
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(5)
    a = [dfine._draw_seed() for _ in range(3)]
    torch.manual_seed(5)
    b = [dfine._draw_seed() for _ in range(3)]
    assert a == b and len(set(a)) == 3 and all(0 <= s < 1 << 62 for s in a)


def test_c_entries_reject_bad_arguments_before_any_hip_call():
    """null pointer, S = 0, head dim != 32, p outside [0, 1), short workspace, misalignment: M355_ERR_INVALID (-1) with a message.
    The device pointers are fake and never dereferenced: the rejection precedes every HIP call, so this runs without a GPU."""
    from defectdetection_viaobjectdetection_amd import _capi
    lib = _capi.lib
    d = C.c_void_p(0x1000)
    odd = C.c_void_p(0x1004)
    need = lib.m355_dfine_addln_workspace_bytes(300, 256)
    assert need > 0 and need % 16 == 0
    assert lib.m355_dfine_addln_workspace_bytes(3 * 300, 256) >= need
    bad = [
        ("null pointer", lambda: lib.m355_dfine_attn_forward(None, 1, 4, 8, 32, 0.0, 0, 0, d, d, None)),
        ("null pointer", lambda: lib.m355_dfine_attn_forward(d, 1, 4, 8, 32, 0.0, 0, 0, None, d, None)),
        ("S >= 1", lambda: lib.m355_dfine_attn_forward(d, 1, 0, 8, 32, 0.0, 0, 0, d, d, None)),
        ("head dim must be 32", lambda: lib.m355_dfine_attn_forward(d, 1, 4, 8, 64, 0.0, 0, 0, d, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_attn_forward(d, 1, 4, 8, 32, 1.0, 0, 0, d, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_attn_forward(d, 1, 4, 8, 32, -0.1, 0, 0, d, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_attn_forward(d, 1, 4, 8, 32, float("nan"), 0, 0, d, d, None)),
        ("16-byte", lambda: lib.m355_dfine_attn_forward(odd, 1, 4, 8, 32, 0.0, 0, 0, d, d, None)),
        ("[1, 65535]", lambda: lib.m355_dfine_attn_forward(d, 70000, 4, 8, 32, 0.0, 0, 0, d, d, None)),
        ("null pointer", lambda: lib.m355_dfine_attn_backward(d, d, d, None, 1, 4, 8, 32, 0.0, 0, 0, d, None)),
        ("S >= 1", lambda: lib.m355_dfine_attn_backward(d, d, d, d, 1, 0, 8, 32, 0.0, 0, 0, d, None)),
        ("head dim must be 32", lambda: lib.m355_dfine_attn_backward(d, d, d, d, 1, 4, 8, 16, 0.0, 0, 0, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_attn_backward(d, d, d, d, 1, 4, 8, 32, 1.5, 0, 0, d, None)),
        ("null pointer", lambda: lib.m355_dfine_addln_forward(d, None, d, d, 4, 256, 1e-5, 0.0, 0, 1, d, d, d, None)),
        ("rows", lambda: lib.m355_dfine_addln_forward(d, d, d, d, 0, 256, 1e-5, 0.0, 0, 1, d, d, d, None)),
        ("multiple of 4", lambda: lib.m355_dfine_addln_forward(d, d, d, d, 4, 250, 1e-5, 0.0, 0, 1, d, d, d, None)),
        ("multiple of 4", lambda: lib.m355_dfine_addln_forward(d, d, d, d, 4, 2048, 1e-5, 0.0, 0, 1, d, d, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_addln_forward(d, d, d, d, 4, 256, 1e-5, 1.0, 0, 1, d, d, d, None)),
        ("workspace", lambda: lib.m355_dfine_addln_backward(d, d, d, d, d, d, 300, 256, 0.0, 0, 1, d, d, d, d, d, need - 1, None)),
        ("workspace", lambda: lib.m355_dfine_addln_backward(d, d, d, d, d, d, 300, 256, 0.0, 0, 1, d, d, d, d, None, need, None)),
        ("null pointer", lambda: lib.m355_dfine_addln_backward(d, d, d, d, None, d, 300, 256, 0.0, 0, 1, d, d, d, d, d, need, None)),
        ("[0, 1)", lambda: lib.m355_dfine_addln_backward(d, d, d, d, d, d, 300, 256, 2.0, 0, 1, d, d, d, d, d, need, None)),
        ("null pointer", lambda: lib.m355_dfine_relu_dropout_forward(None, 8, 0.0, 0, 2, d, None)),
        ("1 <= n", lambda: lib.m355_dfine_relu_dropout_forward(d, 0, 0.0, 0, 2, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_relu_dropout_forward(d, 8, 1.0, 0, 2, d, None)),
        ("site", lambda: lib.m355_dfine_relu_dropout_forward(d, 8, 0.5, 0, -1, d, None)),
        ("null pointer", lambda: lib.m355_dfine_relu_dropout_backward(d, None, 8, 0.0, 0, 2, d, None)),
        ("16-byte", lambda: lib.m355_dfine_relu_dropout_backward(d, d, 8, 0.0, 0, 2, odd, None)),
        ("null pointer", lambda: lib.m355_dfine_dropout_mask(8, 0.1, 0, 0, None, None)),
        ("1 <= n", lambda: lib.m355_dfine_dropout_mask(0, 0.1, 0, 0, d, None)),
        ("[0, 1)", lambda: lib.m355_dfine_dropout_mask(8, 1.0, 0, 0, d, None)),
    ]
    for i, (text, call) in enumerate(bad):
        rc = call()
        msg = lib.m355_last_error(None).decode()
        assert rc == -1, (i, text, rc)
        assert text in msg, (i, text, msg)
