"""Backward of the D-FINE ops (HIP kernels behind torch.autograd.Function) against float64 autograd through the CPU
restatement tests/msda_grad_ref.py.

Bound per gradient tensor: |err|max <= 1e-5 * max(1, |ref|max) -- fp32 on both sides with a different summation order,
the convention of tests/test_dfine_gpu.py.  Every test also runs the restatement in float32 against itself in float64
(the "floor": what fp32 arithmetic alone costs on these inputs) and asserts floor <= 0.5 * bound, so that an input on
which fp32 itself cannot meet the bound is noticed instead of passing or failing by luck.  At the config-5 map (sums of
~10^2 terms per pixel over 57 600 points) the bound is 3 x the measured floor instead of the fixed 1e-5: both sides are
fp32 and differ only in summation order."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import msda_grad_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "dfine_golden.npz"))
SHAPES = [tuple(int(v) for v in hw) for hw in G["shapes"]]
T = lambda k: torch.from_numpy(np.ascontiguousarray(G[k]))  # noqa: E731
TOL = 1e-5


def _scale(ref):
    return max(1.0, float(ref.abs().max()))


def _check(name, got, ref64, ref32, tol=TOL, floor_mult=None):
    """got: GPU gradient; ref64 / ref32: the restatement's gradient in float64 / float32"""
    scale = _scale(ref64)
    floor = float((ref32.double() - ref64).abs().max()) / scale
    err = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    bound = tol if floor_mult is None else floor_mult * floor
    print(f"{name}: err {err:.2e}, fp32 floor {floor:.2e}, bound {bound:.2e} (of scale {scale:.3g})")
    assert floor <= 0.5 * bound, (name, floor, bound)
    assert err <= bound, (name, err, bound)


def _core_reference(shapes, pts, value, loc, attn, method, seed=11):
    g = torch.Generator().manual_seed(seed)
    go = torch.randn(value.shape[0], loc.shape[1], value.shape[2] * value.shape[3], generator=g)
    f = lambda value, loc, attn: R.msda(value, shapes, loc, attn, pts, method)  # noqa: E731
    inputs = dict(value=value, loc=loc, attn=attn)
    return go, R.grads(f, inputs, go, torch.float64), R.grads(f, inputs, go, torch.float32)


def _core_gpu(dev, shapes, pts, value, loc, attn, method, go, needs=(True, True, True)):
    from defectdetection_viaobjectdetection_amd import dfine
    leaves = [t.to(dev).requires_grad_(n) for t, n in zip((value, loc, attn), needs)]
    out = dfine.multi_scale_deformable_attention_v2(leaves[0], shapes, leaves[1], leaves[2], pts, method)
    out.backward(go.to(dev))
    return out, [t.grad for t in leaves]


def _check_core(dev, shapes, pts, value, loc, attn, method, floor_mult=None, loc_gpu=None):
    go, (out64, g64), (_, g32) = _core_reference(shapes, pts, value, loc, attn, method)
    out, grads = _core_gpu(dev, shapes, pts, value, loc if loc_gpu is None else loc_gpu, attn, method, go)
    assert float((out.detach().cpu().double() - out64).abs().max()) <= TOL * _scale(out64)
    for name, g in zip(("value", "loc", "attn"), grads):
        _check(f"{method} grad_{name}", g.reshape(g64[name].shape), g64[name], g32[name], floor_mult=floor_mult)
    return grads


@pytest.mark.parametrize("method", ["default", "discrete"])
def test_ragged_and_edges(method, cuda_device):
    """One-pixel level, a 1 x 7 strip, corners outside the map, a batch element entirely outside, 6-d locations."""
    shapes, pts, value, loc, attn = R.ragged_case()
    gv, gl, ga = _check_core(cuda_device, shapes, pts, value, loc, attn, method, loc_gpu=loc[:, :, :, None])
    assert gl.shape == (3, 5, 2, 1, 8, 2)                       # the gradient comes back in the 6-d shape it was given in
    if method == "default":
        assert not gv[1].any() and not gl[1].any() and not ga[1].any()   # zero padding everywhere: exactly zero
    else:
        assert not gl.any()                                     # nearest pixel: no location gradient


@pytest.mark.parametrize("pts", [[6, 6, 8], [16, 0, 0], [1, 0, 0]])
@pytest.mark.parametrize("method", ["default", "discrete"])
def test_many_points_scalar_form(pts, method, cuda_device):
    """More than 16 points per head (two chunks of (point, corner) pairs per wave), exactly 16, one; empty levels."""
    g = torch.Generator().manual_seed(9)
    shapes, (B, Q, H, P) = [(9, 11), (4, 6), (2, 3)], (2, 19, 3, sum(pts))
    value = torch.randn(B, 129, H, 32, generator=g)
    loc = torch.rand(B, Q, H, P, 2, generator=g) * 1.4 - 0.2
    attn = torch.rand(B, Q, H, P, generator=g)
    _check_core(cuda_device, shapes, pts, value, loc, attn, method)


def test_collisions(cuda_device):
    """Every location of 300 queries x 4 points inside one cell of a 4 x 4 map: four pixels each sum 1 200 terms."""
    g = torch.Generator().manual_seed(21)
    value = torch.randn(1, 16, 1, 32, generator=g)
    loc = 0.4 + torch.rand(1, 300, 1, 4, 2, generator=g) * 0.05
    attn = torch.rand(1, 300, 1, 4, generator=g)
    gv, _, _ = _check_core(cuda_device, [(4, 4)], [4], value, loc, attn, "default")
    assert int((gv.abs().sum(-1) > 0).sum()) == 4


@pytest.mark.parametrize("method", ["default", "discrete"])
def test_locations_on_cell_borders(method, cuda_device):
    """Every location exactly on a pixel centre, i.e. on the border between two bilinear cells (pixel coordinate an integer,
    exact in float32 and float64 alike: power-of-two maps), the first and last row and column included.  Forward and
    backward must take the same cell there -- the one floor() names, as grid_sample does: weight 1 on one corner, and the
    location gradient is that cell's slope."""
    g = torch.Generator().manual_seed(31)
    shapes, pts = [(4, 8), (2, 2)], [6, 2]
    B, Q, H = 2, 7, 2
    value = torch.randn(B, 36, H, 32, generator=g)
    size = torch.tensor([[8.0, 4.0]] * 6 + [[2.0, 2.0]] * 2)                     # (w, h) of each point's level
    k = torch.floor(torch.rand(B, Q, H, 8, 2, generator=g) * size)              # pixel index per axis, 0 .. size - 1
    loc = (k + 0.5) / size
    attn = torch.rand(B, Q, H, 8, generator=g)
    _check_core(cuda_device, shapes, pts, value, loc, attn, method)


@functools.lru_cache(maxsize=None)
def _seams_case():
    """Config-5 value map at batch 2; computed once, shared by the tests below, never modified."""
    g = torch.Generator().manual_seed(5)
    shapes, pts = [(80, 80), (40, 40), (20, 20)], [4, 4, 4]
    value = torch.randn(2, 8400, 8, 32, generator=g)
    # Locations in [-0.1, 1.1].  The location gradient jumps at a cell border, and among 115 200 coordinates one lands
    # within fp32 rounding of a border, where float32 and float64 differentiate different cells: every pixel coordinate
    # keeps 1 % of a cell away from the borders (frac in [0.01, 0.99]).
    u = (torch.rand(2, 300, 8, 12, 2, generator=g).double() * 1.2 - 0.1)
    size = torch.tensor([w for _, w in shapes], dtype=torch.float64).repeat_interleave(4).reshape(1, 1, 1, 12, 1)   # square levels
    pix = u * size - 0.5
    pix = pix.floor() + 0.01 + 0.98 * (pix - pix.floor())
    loc = ((pix + 0.5) / size).float()
    attn = torch.softmax(torch.randn(2, 300, 8, 12, generator=g), -1)
    return (shapes, pts, value, loc, attn) + _core_reference(shapes, pts, value, loc, attn, "default")


def test_ownership_seams(cuda_device):
    """80^2 + 40^2 + 20^2, 300 queries, 8 heads: every ownership range of pass 2, its level ends included."""
    shapes, pts, value, loc, attn, go, (_, g64), (_, g32) = _seams_case()
    _, grads = _core_gpu(cuda_device, shapes, pts, value, loc, attn, "default", go)
    for name, g in zip(("value", "loc", "attn"), grads):
        _check(f"seams grad_{name}", g, g64[name], g32[name], floor_mult=3.0)


def test_bitwise_reproducible(cuda_device):
    shapes, pts, value, loc, attn, go = _seams_case()[:6]
    runs = [_core_gpu(cuda_device, shapes, pts, value, loc, attn, "default", go)[1] for _ in range(3)]
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_partial_needs(which, cuda_device):
    shapes, pts, value, loc, attn = R.ragged_case()
    go, (_, g64), (_, g32) = _core_reference(shapes, pts, value, loc, attn, "default")
    needs = tuple(i == which for i in range(3))
    _, grads = _core_gpu(cuda_device, shapes, pts, value, loc, attn, "default", go, needs)
    name = ("value", "loc", "attn")[which]
    assert [g is None for g in grads] == [not n for n in needs]
    _check(f"only grad_{name}", grads[which], g64[name], g32[name])


def test_no_grad_path(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    shapes, pts, value, loc, attn = R.ragged_case()
    v, l, a = (t.to(cuda_device) for t in (value, loc, attn))
    plain = dfine.multi_scale_deformable_attention_v2(v, shapes, l, a, pts)
    assert plain.grad_fn is None and not plain.requires_grad
    tracked = dfine.multi_scale_deformable_attention_v2(v.clone().requires_grad_(True), shapes, l, a, pts)
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), plain)
    with torch.no_grad():
        off = dfine.multi_scale_deformable_attention_v2(v.clone().requires_grad_(True), shapes, l, a, pts)
    assert off.grad_fn is None and torch.equal(off, plain)


def test_gradient_dtype_follows_input(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    shapes, pts, value, loc, attn = R.ragged_case()
    v = value.to(cuda_device).half().requires_grad_(True)
    a = attn.to(cuda_device).double().requires_grad_(True)
    dfine.multi_scale_deformable_attention_v2(v, shapes, loc.to(cuda_device), a, pts).sum().backward()
    assert v.grad.dtype == torch.float16 and a.grad.dtype == torch.float64


def test_module_backward(cuda_device):
    """deformable_attention on the golden module tensors: gradients of hidden_states, both linear layers, the reference
    points and the encoder map (5e-5 of scale: the forward test's allowance for the GEMM order ahead of the kernel), and
    m355_msda_module_backward alone on the golden offsets and logits (1e-5)."""
    from defectdetection_viaobjectdetection_amd import dfine
    from defectdetection_viaobjectdetection_amd._capi import check, lib
    B, S, H, D = G["value"].shape
    Q, pts, scale = G["mod_ref"].shape[1], [4, 4, 4], float(G["mod_offset_scale"])
    go = torch.randn(B, Q, H * D, generator=torch.Generator().manual_seed(13))
    inputs = dict(hidden=T("mod_hidden"), ref=T("mod_ref"), enc=T("value").reshape(B, S, H * D), w_off=T("mod_w_off"),
                  b_off=T("mod_b_off"), w_att=T("mod_w_att"), b_att=T("mod_b_att"))
    f = lambda **k: R.deformable_attention(shapes=SHAPES, num_points_list=pts, n_heads=H, offset_scale=scale, **k)  # noqa: E731
    (_, g64), (_, g32) = R.grads(f, inputs, go, torch.float64), R.grads(f, inputs, go, torch.float32)
    dev = cuda_device
    lin_o, lin_a = torch.nn.Linear(256, 192).to(dev), torch.nn.Linear(256, 96).to(dev)
    with torch.no_grad():
        lin_o.weight.copy_(inputs["w_off"]); lin_o.bias.copy_(inputs["b_off"])
        lin_a.weight.copy_(inputs["w_att"]); lin_a.bias.copy_(inputs["b_att"])
    hidden, ref, enc = (inputs[k].to(dev).requires_grad_(True) for k in ("hidden", "ref", "enc"))
    y = dfine.deformable_attention(hidden, ref[:, :, None], enc, SHAPES, lin_o, lin_a, pts, H, scale)
    y.backward(go.to(dev))
    got = dict(hidden=hidden.grad, ref=ref.grad, enc=enc.grad, w_off=lin_o.weight.grad, b_off=lin_o.bias.grad,
               w_att=lin_a.weight.grad, b_att=lin_a.bias.grad)
    for k, g in got.items():
        _check(f"module grad_{k}", g, g64[k], g32[k], tol=5e-5)
    # the entry alone, fed with the reference's own linear outputs
    inputs = dict(value=T("value"), ref=T("mod_ref"), offsets=T("mod_offsets"), logits=T("mod_logits"))
    f = lambda **k: R.module(shapes=SHAPES, num_points_list=pts, offset_scale=scale, **k)  # noqa: E731
    (_, g64), (_, g32) = R.grads(f, inputs, go, torch.float64), R.grads(f, inputs, go, torch.float32)
    dv = {k: v.to(dev).contiguous() for k, v in inputs.items()}
    out = {k: torch.empty_like(v) for k, v in dv.items()}
    work = torch.empty(int(lib.m355_msda_backward_workspace_bytes(B, Q, H, 12)), dtype=torch.uint8, device=dev)
    sh = (C.c_int32 * 6)(*[v for hw in SHAPES for v in hw]); pp = (C.c_int32 * 3)(*pts)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    god = go.to(dev)
    check(lib.m355_msda_module_backward(P(god), P(dv["value"]), B, S, H, D, sh, 3, P(dv["ref"]), P(dv["offsets"]), P(dv["logits"]),
                                        pp, Q, 12, scale, P(out["value"]), P(out["ref"]), P(out["offsets"]), P(out["logits"]),
                                        P(work), work.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for k, g in out.items():
        _check(f"module entry grad_{k}", g, g64[k], g32[k])


@pytest.mark.parametrize("clamp", [False, True])
def test_decode_backward(clamp, cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    fin = torch.isfinite(T("boxes")).all(-1)                    # the golden points hold pre-sigmoid values: inf - inf rows
    dist, points, proj = T("dist")[fin], T("points")[fin], T("project")
    assert dist.shape[0] >= 8
    go = torch.randn(dist.shape[0], 4, generator=torch.Generator().manual_seed(17))
    f = lambda pred_corners, points: R.decode_boxes(pred_corners, proj.to(points.dtype), points, 4.0, clamp)  # noqa: E731
    inputs = dict(pred_corners=dist, points=points)
    (_, g64), (_, g32) = R.grads(f, inputs, go, torch.float64), R.grads(f, inputs, go, torch.float32)
    d, p = dist.to(cuda_device).requires_grad_(True), points.to(cuda_device).requires_grad_(True)
    dfine.decode_boxes(d, proj.to(cuda_device), p, 4.0, clamp01=clamp).backward(go.to(cuda_device))
    for name, got in (("pred_corners", d.grad), ("points", p.grad)):
        np.testing.assert_allclose(g32[name].numpy(), g64[name].numpy(), rtol=5e-6, atol=5e-6)     # the fp32 floor
        np.testing.assert_allclose(got.cpu().numpy(), g64[name].numpy(), rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError):
        dfine.decode_boxes(d, proj.to(cuda_device).requires_grad_(True), p, 4.0)
