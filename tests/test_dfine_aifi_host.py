"""The AIFI layer, the map / token layout ops and the memory assembly without a GPU: the *_torch fallbacks are upstream's expressions
bit for bit, a bound layer and a bound model on CPU tensors run the classes' own code, and every new C entry refuses bad arguments
with M355_ERR_INVALID before any HIP call (fake device pointers, as tests/test_capi_symbols.py)."""
import copy
import ctypes as C

import pytest
import torch


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


LEVELS = [(3, 5), (2, 2), (1, 1)]


def test_torch_fallbacks_are_upstreams_expressions():
    from defectdetection_viaobjectdetection_amd import dfine
    B, D = 2, 6   # D = 6 is outside the kernels' limits as well
    maps = [_randn((B, D, h, w), 10 + i) for i, (h, w) in enumerate(LEVELS)]
    S = sum(h * w for h, w in LEVELS)
    want = torch.cat([m.flatten(2).transpose(1, 2) for m in maps], 1)
    before = dict(dfine.layout_calls)
    tokens, extra = dfine.maps_to_tokens(maps)
    assert extra is None and torch.equal(tokens, want)
    pos = _randn((S, D), 3)
    tokens, extra = dfine.maps_to_tokens(maps, pos=pos)
    assert torch.equal(tokens, want) and torch.equal(extra, want + pos)
    mask = (torch.arange(S) % 3 != 0).reshape(1, S, 1)   # upstream's valid_mask: bool (1, S, 1)
    tokens, extra = dfine.maps_to_tokens(maps, mask=mask)
    assert torch.equal(tokens, want) and torch.equal(extra, mask.to(want.dtype) * want)
    back = dfine.tokens_to_maps(want, LEVELS)
    s = 0
    for m, (h, w), got in zip(maps, LEVELS, back):
        ref = want[:, s:s + h * w].transpose(1, 2).reshape(B, D, h, w).contiguous()
        assert got.is_contiguous() and torch.equal(got, ref) and torch.equal(got, m)
        s += h * w
    assert dfine.layout_calls == {"kernel": before["kernel"], "torch": before["torch"] + 4}
    for f in (dfine.maps_to_tokens_torch, ):
        t2, e2 = f(maps, mask=mask)
        assert torch.equal(t2, want) and torch.equal(e2, extra)


def test_layout_argument_errors():
    from defectdetection_viaobjectdetection_amd import dfine
    maps = [_randn((1, 4, 2, 2), 0)]
    with pytest.raises(ValueError):
        dfine.maps_to_tokens(maps, pos=torch.zeros(4, 4), mask=torch.ones(4))
    with pytest.raises(ValueError):
        dfine.maps_to_tokens(maps, pos=torch.zeros(4, 4, requires_grad=True))
    with pytest.raises(ValueError):
        dfine.maps_to_tokens(maps, mask=torch.ones(4, requires_grad=True))
    with pytest.raises(ValueError):
        dfine.maps_to_tokens(maps + [_randn((2, 4, 1, 1), 1)])
    with pytest.raises(ValueError):
        dfine.tokens_to_maps(torch.zeros(1, 5, 4), [(2, 2)])


def test_gelu_torch_against_float64():
    from defectdetection_viaobjectdetection_amd import dfine
    h = torch.cat([3 * _randn((1000,), 5), torch.tensor([0.0, -0.0, 0.5, -0.5, 5.5, -5.5, 10.0, -10.0, 40.0, -40.0, 1e-40])])
    h64 = h.double()
    want = h64 * 0.5 * (1 + torch.erf(h64 / 2 ** 0.5))
    got = dfine.gelu(h)   # a CPU tensor: gelu_torch
    assert got.dtype == torch.float32 and torch.equal(got, dfine.gelu_torch(h))
    assert float((got.double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())   # a few fp32 roundings of the largest


def test_bound_aifi_layer_on_cpu_runs_the_class_forward():
    from transformers import DFineConfig
    from transformers.models.d_fine import modeling_d_fine as M
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(0)
    layer = M.DFineAIFILayer(DFineConfig(encoder_hidden_dim=64, encoder_attention_heads=2, encoder_ffn_dim=128)).eval()
    keys = list(layer.state_dict())
    for attention in (False, True):
        bound = dfine.bind_aifi(copy.deepcopy(layer), attention=attention)
        assert list(bound.state_dict()) == keys and type(bound) is M.DFineAIFILayer
        x = _randn((2, 64, 3, 5), 1)
        before = dict(dfine.aifi_calls)
        with torch.no_grad():
            got, want = bound(x), layer(x)
        assert torch.equal(got, want)
        assert dfine.aifi_calls == {"kernel": before["kernel"], "torch": before["torch"] + 1}


def test_bind_all_on_cpu_keeps_the_model():
    try:
        from transformers import DFineConfig, DFineForObjectDetection
    except Exception as ex:
        pytest.skip(f"transformers D-FINE not importable here: {ex}")
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(0)
    config = DFineConfig(dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, num_queries=30)
    try:
        model = DFineForObjectDetection(config)
    except ImportError as ex:
        pytest.skip(f"DFineForObjectDetection(DFineConfig()) cannot be built here: {ex}")
    # train mode: batch statistics keep the random backbone's tokens apart, so that no two scores tie (among equal scores the
    # bound selection has its own order rule); dropout is 0 and without labels there is no denoising group: nothing random
    model.train()
    twin = copy.deepcopy(model)
    bound = dfine.bind_all(twin)
    assert bound is twin
    assert list(bound.state_dict()) == list(model.state_dict())
    assert bound.model._m355_assembly in (True, False) and "_m355_assembly" not in bound.state_dict()
    x = _randn((2, 3, 64, 64), 2)
    before = dict(dfine.layout_calls)
    with torch.no_grad():
        want, got = model(pixel_values=x), bound(pixel_values=x)
    scores = want.enc_outputs_class.max(-1).values
    assert all(row.unique().numel() == row.numel() for row in scores), "tied scores: the comparison below would test the tie rule"
    for field in ("logits", "pred_boxes", "enc_outputs_class", "enc_outputs_coord_logits", "init_reference_points", "last_hidden_state"):
        assert torch.equal(got[field], want[field]), field
    assert dfine.layout_calls["kernel"] == before["kernel"]


# ---- the C entries refuse bad arguments on the host ---------------------------------------------------------------------------------
FAKE = 0x1000   # never dereferenced: the refusal precedes every HIP call


def _maps_to_tokens(lib, maps=(FAKE,), shapes=((2, 2),), L=None, B=1, D=8, pos=None, mask=None, tokens=FAKE, extra=None, table=True):
    ptrs = (C.c_void_p * max(len(maps), 1))(*maps)
    sh = (C.c_int32 * (2 * max(len(shapes), 1)))(*[v for hw in shapes for v in hw])
    return lib.m355_dfine_maps_to_tokens(ptrs if table else None, sh, len(shapes) if L is None else L, B, D, pos, mask, tokens, extra, None)


def _tokens_to_maps(lib, tokens=FAKE, extra=None, mask=None, maps=(FAKE,), shapes=((2, 2),), L=None, B=1, D=8):
    ptrs = (C.c_void_p * max(len(maps), 1))(*maps)
    sh = (C.c_int32 * (2 * max(len(shapes), 1)))(*[v for hw in shapes for v in hw])
    return lib.m355_dfine_tokens_to_maps(tokens, extra, mask, sh, len(shapes) if L is None else L, B, D, ptrs, None)


NINE = dict(maps=(FAKE,) * 9, shapes=((1, 1),) * 9)
BAD_LAYOUT = [
    ("null tokens", dict(tokens=None), b"null pointer"),
    ("null map in the table", dict(maps=(None,)), b"null pointer"),
    ("D = 6", dict(D=6), b"multiple of 4"),
    ("D = 1028", dict(D=1028), b"multiple of 4"),
    ("L = 0", dict(L=0), b"levels"),
    ("L = 9", dict(L=9, **NINE), b"levels"),
    ("h = 0", dict(shapes=((0, 2),)), b"h, w >= 1"),
    ("B = 0", dict(B=0), b"B >= 1"),
    ("misaligned tokens", dict(tokens=FAKE + 4), b"16-byte"),
    ("misaligned map", dict(maps=(FAKE + 8,)), b"16-byte"),
]


@pytest.mark.parametrize("name, kwargs, why", BAD_LAYOUT, ids=[c[0] for c in BAD_LAYOUT])
def test_layout_entries_refuse_bad_arguments(name, kwargs, why):
    from defectdetection_viaobjectdetection_amd import _capi
    lib = _capi.lib
    for call in (_maps_to_tokens, _tokens_to_maps):
        assert call(lib, **kwargs) == -1, (name, call.__name__)
        assert why in lib.m355_last_error(None), (name, lib.m355_last_error(None))


def test_maps_to_tokens_refuses_pos_with_mask_and_a_stray_extra():
    from defectdetection_viaobjectdetection_amd import _capi
    lib = _capi.lib
    assert _maps_to_tokens(lib, pos=FAKE, mask=FAKE, extra=FAKE) == -1 and b"exclude" in lib.m355_last_error(None)
    assert _maps_to_tokens(lib, pos=FAKE) == -1 and b"extra" in lib.m355_last_error(None)         # pos without extra
    assert _maps_to_tokens(lib, extra=FAKE) == -1 and b"extra" in lib.m355_last_error(None)       # extra without pos or mask
    assert _maps_to_tokens(lib, table=False) == -1 and b"null pointer" in lib.m355_last_error(None)
    assert _maps_to_tokens(lib, pos=FAKE + 4, extra=FAKE) == -1 and b"16-byte" in lib.m355_last_error(None)
    assert _tokens_to_maps(lib, tokens=None) == -1 and b"null pointer" in lib.m355_last_error(None)
    assert _tokens_to_maps(lib, mask=FAKE) == -1 and b"mask without extra" in lib.m355_last_error(None)
    # S = 2^31 tokens: 65536 x 32768
    assert _maps_to_tokens(lib, shapes=((65536, 32768),)) == -1 and b"2^31" in lib.m355_last_error(None)


def test_gelu_entries_refuse_bad_arguments():
    from defectdetection_viaobjectdetection_amd import _capi
    lib = _capi.lib
    for n, h, out, why in ((-1, FAKE, FAKE, b"1 <= n"), (0, FAKE, FAKE, b"1 <= n"), (8, None, FAKE, b"null pointer"),
                           (8, FAKE, None, b"null pointer"), (8, FAKE + 4, FAKE, b"16-byte"), (8, FAKE, FAKE + 4, b"16-byte")):
        assert lib.m355_dfine_gelu_forward(h, n, out, None) == -1 and why in lib.m355_last_error(None)
        assert lib.m355_dfine_gelu_backward(FAKE, h, n, out, None) == -1 and why in lib.m355_last_error(None)
    assert lib.m355_dfine_gelu_backward(None, FAKE, 8, FAKE, None) == -1 and b"null pointer" in lib.m355_last_error(None)
