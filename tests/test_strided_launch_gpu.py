"""Per-launch parity of the raw strided C-ABI the training step drives (include/mi355yolo.h, "raw strided launches"):
m355_conv_launch, m355_wgrad_launch, m355_bn_train_fwd_launch and m355_bn_train_bwd_launch on channel slices of larger NHWC
buffers, against fp32/fp64 references on the same fp16 operands (tests/launch_ref.py).

Every conv case names the kernel route it is meant to reach (the `_ok` predicate it satisfies in op_entries.hip's m355_conv_launch)
and checks: rc 0; the slice per element within 2^-10 |ref| + c S (c = min(2^-13, 1 / 2K)) and rel-L2 <= 1e-3; every element
outside the output slice still the sentinel NaN, bit for bit (guard bands before / after the allocation, other channels, the
image-stride gap)."""
import ctypes as C

import pytest
import torch

import launch_ref as L
from launch_ref import ConvGeom as G, WgradGeom as WG

pytestmark = pytest.mark.gpu


def _capi():
    from defectdetection_viaobjectdetection_amd import _capi
    return _capi


def _conv(B, H, W, cin, cout, k, s, **kw):
    pad = k // 2 if k != 2 else 0
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    return G(B, H, W, cin, Ho, Wo, cout, k, s, pad, **kw)


def _gather(B, H, W, fcin, fcout, **kw):
    """tmode 1: x = dY (B, Ho, Wo, fcout) of a 3x3 / s2 / p1 conv, y = dX (B, H, W, fcin)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return G(B, Ho, Wo, fcout, H, W, fcin, 3, 1, 1, tmode=1, bias=False, fwd_cout=fcout, **kw)


def _phase(B, H, W, fcin, fcout, **kw):
    """tmode 2: the same gradient as four 2x2 phase convs over dY (H, W even)."""
    return G(B, H // 2, W // 2, fcout, H // 2, W // 2, 4 * fcin, 2, 1, 0, tmode=2, convt_co=fcin, bias=False, fwd_cout=fcout, **kw)


def _convt(B, h, w, cin, cout, **kw):
    return G(B, h, w, cin, h, w, 4 * cout, 1, 1, 0, convt_co=cout, **kw)


def _variants(route, g, res=True, big_bstride=True):
    """The slice forms of one route: input and output slices at channel offsets inside wider rows, a residual on its own
    slice and in place (y += conv), and a larger image stride than H W ld on every operand."""
    ldx = g.cin + 32 + 64
    ycy = g.convt_co if g.convt_co else g.cout
    ldy = ycy + 64 + 32
    base = dict(ldx=ldx, x_off=32, ldy=ldy, y_off=64)
    out = [(route, G(**{**g.__dict__, **base}))]
    if res:
        out.append((route + "+res", G(**{**g.__dict__, **base, "res": "own", "ldr": ycy + 24, "r_off": 16})))
        out.append((route + "+inplace", G(**{**g.__dict__, **base, "res": "inplace"})))
    if big_bstride:
        hy, wy = (2 * g.ho, 2 * g.wo) if g.tmode == 2 or g.convt_co else (g.ho, g.wo)
        out.append((route + "+bstride", G(**{**g.__dict__, **base, "x_bs": g.hi * g.wi * ldx + 8 * 37,
                                             "y_bs": hy * wy * ldy + 8 * 53})))
    return out


CONV_CASES = (
    # halo (conv3x3_halo_ok: 3x3 / s1, cin % 64 == 0, cout >= 64, 16-wide tiles within 30 % waste; m32 / wide kernels by shape)
    _variants("halo", _conv(2, 16, 32, 64, 96, 3, 1, act=1))
    + _variants("halo-b1", _conv(1, 24, 48, 128, 224, 3, 1))
    # conv1x1_wreg (1x1, K in {128 .. 512}, cout % 128 == 0, no residual, dense image stride): a residual or a larger image
    # stride sends the launch to the implicit GEMM
    + _variants("conv1x1_wreg", _conv(2, 10, 13, 128, 128, 1, 1, act=1))
    + _variants("conv1x1_wreg-b3", _conv(3, 7, 9, 256, 256, 1, 1))
    # conv3x3_c32 (32 -> 32, 3x3 / s1)
    + _variants("conv3x3_c32", _conv(2, 20, 20, 32, 32, 3, 1, act=1))
    + _variants("conv3x3_c32-b1", _conv(1, 13, 19, 32, 32, 3, 1))
    # dgrad_s2c32 (tmode 2, 32 forward input channels, forward cout 64, dY width a multiple of 32, no residual)
    + _variants("dgrad_s2c32", _phase(2, 32, 64, 32, 64), res=False)
    # igemm phase 2: whole phases inside a tile (cin 16, 32: no residual) or a tile inside a phase with cout % 64 != 0
    + _variants("phase2-shared", _phase(2, 34, 22, 32, 64), res=False)
    + _variants("phase2-c16", _phase(1, 20, 12, 16, 32), res=False)
    + _variants("phase2-c64-k96", _phase(2, 32, 32, 64, 96))
    # igemm phase 3 (compact taps: cin and cout multiples of 64)
    + _variants("phase3", _phase(2, 20, 36, 64, 128))
    + _variants("phase3-c192", _phase(1, 16, 16, 192, 64))
    # tmode 1 transposed-stride gather: odd maps, and the channel counts no phase form tiles (cin 8)
    + _variants("gather", _gather(2, 33, 21, 64, 128))
    + _variants("gather-c8", _gather(2, 32, 32, 8, 32))
    + _variants("gather-b1", _gather(1, 17, 40, 96, 64))
    # generic implicit GEMM: strided forward, ragged channel tiles, ConvT's input gradient (2x2 / s2 conv)
    + _variants("igemm-s2", _conv(2, 17, 23, 64, 96, 3, 2, act=1))
    + _variants("igemm-s1-c32", _conv(1, 11, 30, 32, 224, 3, 1))
    + _variants("igemm-1x1", _conv(2, 9, 11, 96, 48, 1, 1, act=1))
    + _variants("igemm-k2s2", _conv(2, 16, 22, 64, 96, 2, 2, bias=False))
    # ConvTranspose forward (convt_co): fast stores (convt_co % tile == 0, 2w % 16 == 0, no residual) and the generic epilogue
    + _variants("convt-fast", _convt(2, 8, 16, 128, 64), res=False)
    + _variants("convt-generic", _convt(1, 7, 9, 64, 32), res=False)
)

# out_f32: 1x1 head convs into the fp32 raw-head rows (64 box logits | nc class logits | 32 coefficients), odd row width 97,
# image stride = rows of every level x 97, channel offsets 0, 64 and 65 (4-byte aligned only: no vector store may assume more)
F32_CASES = [
    ("out_f32-box", G(2, 8, 12, 64, 8, 12, 64, 1, 1, 0, out_f32=1, ldx=128, x_off=64, ldy=97, y_off=0, y_bs=130 * 97)),
    ("out_f32-cls", G(2, 8, 12, 64, 8, 12, 1, 1, 1, 0, out_f32=1, ldx=64, ldy=97, y_off=64, y_bs=130 * 97)),
    ("out_f32-coef", G(2, 8, 12, 96, 8, 12, 32, 1, 1, 0, out_f32=1, ldx=224, x_off=96, ldy=97, y_off=65, y_bs=130 * 97)),
    ("out_f32-b1", G(1, 5, 7, 64, 5, 7, 33, 1, 1, 0, out_f32=1, ldx=128, ldy=97, y_off=64, y_bs=40 * 97)),
]

# the two stride-2 dgrad shapes of the phase-form selection fix, as m355_conv_launch twins of the new DGRAD_CASES: tmode 2 with
# forward cout 96 (window slots, not compact), and the gather for cin 8 (no phase form tiles 4 x 8 = 32 virtual channels)
FIX_CASES = [
    ("fix-phase-64x96", _phase(2, 32, 32, 64, 96)),
    ("fix-gather-8x32", _gather(2, 32, 32, 8, 32)),
]


@pytest.mark.parametrize("name,g", CONV_CASES + F32_CASES + FIX_CASES, ids=[n for n, _ in CONV_CASES + F32_CASES + FIX_CASES])
def test_conv_launch_slices(name, g, cuda_device):
    r = L.run_conv_geom(_capi(), g, cuda_device, seed=len(name) * 31 + g.cin)
    assert r["rc"] == 0, f"{name}: rc {r['rc']}: {r['err']}"
    print(f"{name}: worst err/bound {r['ratio']:.3f}, rel-L2 {r['rel']:.2e}, K {r['K']}; {r['desc']}")
    assert r["guard"] == 0, f"{name}: {r['desc']}"
    assert r["rel"] <= 1e-3, f"{name}: rel-L2 {r['rel']:.3e}"
    assert r["ratio"] <= 1.0, f"{name}: {r['desc']}"


def test_conv_launch_refuses_layouts_it_cannot_compute(cuda_device):
    """M355_ERR_INVALID with a message, and no launch, for: tmode 2 with cin 8 (4 x 8 virtual channels: no tile holds whole
    phases) or cin 32 with a residual (tiles shared by phases do not accumulate); a ConvTranspose with a residual (it would be
    read at the pre-shuffle pixel: before the check, rel-L2 15 on its own slice, NaN in place)."""
    capi = _capi()
    for g, msg in ((_phase(2, 16, 16, 8, 32), "tmode 2"), (G(**{**_phase(2, 16, 32, 32, 64).__dict__, "res": "inplace"}), "tmode 2"),
                   (G(**{**_convt(1, 7, 9, 64, 32).__dict__, "res": "inplace"}), "residual"),
                   (G(**{**_convt(2, 8, 16, 128, 64).__dict__, "res": "own", "ldr": 64}), "residual")):
        r = L.run_conv_geom(capi, g, cuda_device)
        assert r["rc"] == -1 and msg in r["err"], r


WGRAD_CASES = [
    # name, geometry (x slice at ldx > cin, dZ slice at lddz > cout unless the route needs dense rows), outcome with a workspace
    # one byte short of m355_wgrad_workspace_bytes: "invalid" (the route's split-K slabs no longer fit) or "ok" with the right
    # gradient (the size covers the pixel-axis GEMM's plan too: the stem, the patch kernel's smaller plans and wgrad_s2c32, which
    # deals its chunks to as many slabs as fit, still run)
    ("wgrad_stem", WG(2, 128, 128, 8, 64, 64, 32, 3, 2, 1, ldx=8, lddz=96, dz_off=32), "ok"),
    ("wgrad_stem->gemm", WG(2, 64, 128, 8, 32, 64, 32, 3, 2, 1, ldx=24, x_off=8, lddz=64, dz_off=16), "invalid"),
    ("wgrad_s2c32", WG(2, 128, 128, 32, 64, 64, 64, 3, 2, 1, ldx=96, x_off=32, lddz=128, dz_off=64), "ok"),
    ("wgrad_s2c32-ragged", WG(1, 64, 160, 32, 32, 80, 64, 3, 2, 1, ldx=64, x_off=32, lddz=192, dz_off=128,
                              x_bs=64 * 160 * 64 + 64), "ok"),
    ("conv_wgrad3", WG(2, 16, 48, 48, 16, 48, 96, 3, 1, 1, ldx=112, x_off=64, lddz=160, dz_off=32), "ok"),
    ("conv_wgrad3-ragged", WG(1, 19, 35, 32, 19, 35, 64, 3, 1, 1, ldx=96, x_off=8, lddz=72, dz_off=8), "invalid"),
    ("gemm-1x1", WG(2, 10, 12, 96, 10, 12, 48, 1, 1, 0, ldx=192, x_off=96, lddz=64, dz_off=8), "invalid"),
    ("gemm-s2", WG(2, 17, 23, 64, 9, 12, 96, 3, 2, 1, ldx=128, x_off=32, lddz=160, dz_off=64), "invalid"),
    ("gemm-k2s2", WG(2, 16, 20, 64, 8, 10, 48, 2, 2, 0, ldx=96, x_off=16, lddz=48, x_bs=16 * 20 * 96 + 32), "invalid"),
    ("gemm-splitk", WG(4, 40, 40, 128, 40, 40, 64, 1, 1, 0, ldx=256, x_off=128, lddz=96, dz_off=32), "invalid"),
]


@pytest.mark.parametrize("name,g,short", WGRAD_CASES, ids=[n for n, _, _ in WGRAD_CASES])
def test_wgrad_launch_slices(name, g, short, cuda_device):
    capi = _capi()
    r = L.run_wgrad_geom(capi, g, cuda_device, seed=len(name) + g.cin)
    assert r["rc"] == 0, f"{name}: rc {r['rc']}: {r['err']}"
    print(f"{name}: worst err/bound {r['ratio']:.3f}, rel-L2 {r['rel']:.2e}, K {r['K']}, workspace {r['need']} B; {r['desc']}")
    assert r["guard"] == 0, f"{name}: dW written past its {g.cout} x {g.k} x {g.k} x {g.cin} floats"
    assert r["bitwise"], f"{name}: a repeat run gave different bits"
    assert r["rel"] <= 1e-3, f"{name}: rel-L2 {r['rel']:.3e}"
    assert r["ratio"] <= 1.0, f"{name}: {r['desc']}"
    if r["need"] > 0:
        s = L.run_wgrad_geom(capi, g, cuda_device, seed=len(name) + g.cin, ws_delta=-1, repeat=False)
        taken = "invalid" if s["rc"] == -1 else "ok"
        print(f"{name}: one byte short of the workspace -> {taken}")
        assert s["rc"] in (0, -1), s
        assert taken == short, f"{name}: expected {short} with a short workspace, got {taken}"
        if taken == "ok":
            assert s["guard"] == 0 and s["rel"] <= 1e-3 and s["ratio"] <= 1.0, s
        else:
            assert "workspace" in s["err"], s


def test_wgrad_splitk_plan_uses_several_slabs(cuda_device):
    """The split-K case above needs a workspace (several partial slabs): 0 bytes would mean a single slab."""
    capi = _capi()
    g = WGRAD_CASES[-1][1]
    need = int(capi.lib.m355_wgrad_workspace_bytes(g.batch, g.ho, g.wo, g.cin, g.cout, g.k))
    assert need >= 2 * g.cout * g.k * g.k * g.cin * 4, need


# ---------------------------------------------------------------------------------------------------- batch norm
BN_CASES = [
    # npix-shape (B, H, W), C, ldz, ldy / y_off, ldr / r_off (0 = none), act
    ((2, 9, 13), 48, 64, (96, 32), (0, 0), 1),
    ((2, 9, 13), 48, 48, (80, 8), (72, 16), 0),
    ((3, 5, 7), 128, 192, (256, 64), (136, 8), 1),
    ((2, 1, 1), 64, 96, (128, 0), (0, 0), 0),          # npix = 2: the unbiased variance is twice the biased one
    ((1, 1, 3), 24, 24, (40, 16), (0, 0), 1),
]


def _bn_ws(capi, Cc, dev):
    return torch.zeros(int(capi.lib.m355_bn_workspace_floats(Cc)), device=dev)


@pytest.mark.parametrize("shape,Cc,ldz,yl,rl,act", BN_CASES)
def test_bn_train_launch_slices(shape, Cc, ldz, yl, rl, act, cuda_device):
    capi = _capi()
    dev = cuda_device
    B, H, W = shape
    npix = B * H * W
    g = torch.Generator().manual_seed(Cc + npix)
    z = (torch.randn(B, H, W, Cc, generator=g) * 1.7 + 0.3).half()
    gamma = 0.8 + 0.4 * torch.rand(Cc, generator=g)
    beta = 0.2 * torch.rand(Cc, generator=g) - 0.1
    rm0 = torch.randn(Cc, generator=g) * 0.1
    rv0 = 0.5 + torch.rand(Cc, generator=g)
    mom, eps = 0.03, 1e-3
    zb = L.Guarded(B, H, W, ldz, dev)
    zb.fill_random(g, 4.0)
    zoff = ldz - Cc
    zb.write(zoff, z)
    ldy, yoff = yl
    yb = L.Guarded(B, H, W, ldy, dev)
    ldr, roff = rl
    res = None
    if ldr:
        rb = L.Guarded(B, H, W, ldr, dev)
        rb.fill_random(g, 4.0)
        res = torch.randn(B, H, W, Cc, generator=g).half()
        rb.write(roff, res)
    d_g, d_b = gamma.to(dev), beta.to(dev)
    d_m, d_is = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
    d_rm, d_rv = rm0.clone().to(dev), rv0.clone().to(dev)
    ws = _bn_ws(capi, Cc, dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(capi.lib.m355_bn_train_fwd_launch(zb.ptr(zoff), npix, ldz, Cc, d_g.data_ptr(), d_b.data_ptr(), eps, act,
                                                 yb.ptr(yoff), ldy, rb.ptr(roff) if ldr else 0, ldr, d_m.data_ptr(), d_is.data_ptr(),
                                                 ws.data_ptr(), d_rm.data_ptr(), d_rv.data_ptr(), mom, st))
    torch.cuda.synchronize()
    zd = z.double().reshape(npix, Cc)
    mean, var_b = zd.mean(0), zd.var(0, unbiased=False)
    var_u = zd.var(0, unbiased=True) if npix > 1 else var_b
    invstd = 1 / torch.sqrt(var_b + eps)
    assert torch.allclose(d_m.cpu().double(), mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(d_is.cpu().double(), invstd, rtol=1e-5)
    assert torch.allclose(d_rm.cpu().double(), (1 - mom) * rm0.double() + mom * mean, rtol=1e-5, atol=1e-7)
    assert torch.allclose(d_rv.cpu().double(), (1 - mom) * rv0.double() + mom * var_u, rtol=1e-5, atol=1e-7), \
        "running_var: momentum update with the unbiased batch variance (n / (n - 1))"
    u = (zd - mean) * invstd * gamma.double() + beta.double()
    yref = L.silu(u) if act else u
    if ldr:
        yref = yref + res.double().reshape(npix, Cc)
    yref = yref.reshape(B, H, W, Cc)
    got, nbad, first = yb.slice_and_guard(yoff, Cc)
    assert nbad == 0, L.guard_report(yb, nbad, first)
    extra = res.double().abs() if ldr else 0.0
    bound = 2.0 ** -10 * yref.abs() + 2.0 ** -11 * (u.abs().reshape(B, H, W, Cc) * 1.1 + extra) + 1e-5
    ratio, rel, desc = L.check_elementwise(got.double(), yref, bound)
    print(f"bn fwd {shape} C{Cc}: worst err/bound {ratio:.3f}, rel-L2 {rel:.2e}")
    assert ratio <= 1.0, desc

    # backward with dY and dZ slices (lddy, lddz != C), against autograd
    lddy, lddz = ldy + 8, ldz + 16
    dy = torch.randn(B, H, W, Cc, generator=g).half()
    dyb = L.Guarded(B, H, W, lddy, dev)
    dyb.fill_random(g, 4.0)
    dyb.write(8, dy)
    dzb = L.Guarded(B, H, W, lddz, dev)
    d_gb = torch.empty(2 * Cc, device=dev)
    capi.check(capi.lib.m355_bn_train_bwd_launch(zb.ptr(zoff), dyb.ptr(8), npix, ldz, lddy, Cc, d_m.data_ptr(), d_is.data_ptr(),
                                                 d_g.data_ptr(), d_b.data_ptr(), act, dzb.ptr(16), lddz, d_gb.data_ptr(),
                                                 ws.data_ptr(), st))
    torch.cuda.synchronize()
    za = zd.clone().requires_grad_(True)
    ga = gamma.double().requires_grad_(True)
    ba = beta.double().requires_grad_(True)
    m_ = za.mean(0)
    ua = (za - m_) / torch.sqrt(za.var(0, unbiased=False) + eps) * ga + ba
    ya = L.silu(ua) if act else ua
    ya.backward(dy.double().reshape(npix, Cc))
    got_dz, nbad, first = dzb.slice_and_guard(16, Cc)
    assert nbad == 0, L.guard_report(dzb, nbad, first)
    assert torch.isfinite(got_dz).all()
    ref_dz = za.grad.reshape(B, H, W, Cc)
    if npix > 2:
        assert L.rel_l2(got_dz, ref_dz) <= 2e-3
    else:   # two pixels: dz = +-(something) of tiny magnitude after the mean subtraction; compare absolutely
        assert torch.allclose(got_dz.double(), ref_dz, atol=2e-3 * (float(ref_dz.abs().max()) + 1e-3) + 1e-4)
    assert L.rel_l2(d_gb[:Cc].cpu(), ba.grad) <= 1e-3
    assert L.rel_l2(d_gb[Cc:].cpu(), ga.grad) <= 1e-3 or float(ga.grad.abs().max()) < 1e-6

