"""The train-mode BatchNorm(+SiLU)(+residual) launches, m355_bn_train_fwd_launch and m355_bn_train_bwd_launch (bn_stats_kernel,
bn_stats_merge_kernel, bn_silu_apply_kernel, bn_silu_bwd_reduce_kernel, bn_finalize_kernel, bn_silu_bwd_apply_kernel of
csrc/train_kernels.hip), judged against the float64 reference and the derived bounds of tests/bn_ref.py:

  * statistics per channel against float64, at the project's tolerances (mean rtol 1e-5 atol 1e-6, invstd rtol 1e-5, running
    statistics rtol 1e-5 atol 1e-7), on channels whose |mean| / std runs from 0 to 1500 and on constant channels, plain and with
    two far outliers (bn_ref.FAMILIES);
  * y per element against the reference evaluated with the kernel's own returned statistics (the apply alone), act 0 / 1,
    with and without a residual;
  * the backward fed float64 statistics rounded once to fp32 (independent of the forward): dbeta / dgamma per channel, dz per
    element against the reference evaluated with the kernel's own returned sums;
  * every pixel counted once: one spike per channel on the seams of the reduction walk, and constant channels with integer dy
    whose sums are exact in fp32;
  * two launches give the same bits.
Every buffer is a guard-banded slice (ld != C, launch_ref.Guarded) and every workspace is pre-filled with NaN: a kernel that
reads a partial row nobody wrote fails.  Shapes: bn_ref.SHAPES, the smallest that reach each path of the reduction launches.

Not covered here: the 2 048-block cap of the apply kernels' grid (grid_px; it needs about 67 M elements), the second and later
four-pixel trips of the reduction walks (8.4 M elements), and C above 2048, which the launcher refuses (test below).
"""
import ctypes as C
import functools

import pytest
import torch

import bn_ref as R
import launch_ref as L

pytestmark = pytest.mark.gpu

MOM = 0.03


def _capi():
    from defectdetection_viaobjectdetection_amd import _capi
    return _capi


def _nan_ws(capi, Cc, dev):
    return torch.full((int(capi.lib.m355_bn_workspace_floats(Cc)),), float("nan"), device=dev)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in_slice(shape, Cc, extra, off, v, dev, seed):
    """v (npix, C) in channels [off, off + C) of a guard-banded (B, H, W, C + extra) buffer full of finite garbage."""
    B, H, W = shape
    buf = L.Guarded(B, H, W, Cc + extra, dev)
    buf.fill_random(torch.Generator().manual_seed(seed), 4.0)
    buf.write(off, v.reshape(B, H, W, Cc))
    return buf


def _out_slice(buf, off, Cc, what):
    got, nbad, first = buf.slice_and_guard(off, Cc)
    assert nbad == 0, f"{what}: {L.guard_report(buf, nbad, first)}"
    return got.reshape(-1, Cc).double()


def run_fwd(shape, z, gamma, beta, act, res, rm0, rv0, dev, repeat=True):
    """One forward launch on slices.  Returns y (npix, C) float64 and mean, invstd, running_mean, running_var (CPU fp32)."""
    capi = _capi()
    B, H, W = shape
    npix, Cc = z.shape
    zb = _in_slice(shape, Cc, 16, 8, z, dev, 1)
    rb = _in_slice(shape, Cc, 8, 0, res, dev, 2) if res is not None else None
    d_g, d_b = gamma.float().to(dev), beta.float().to(dev)
    outs = []
    for _ in range(2 if repeat else 1):
        yb = L.Guarded(B, H, W, Cc + 24, dev)
        st = [torch.full((Cc,), float("nan"), device=dev) for _ in range(2)] + [rm0.clone().to(dev), rv0.clone().to(dev)]
        ws = _nan_ws(capi, Cc, dev)
        capi.check(capi.lib.m355_bn_train_fwd_launch(zb.ptr(8), npix, Cc + 16, Cc, d_g.data_ptr(), d_b.data_ptr(), R.EPS, act,
                                                     yb.ptr(16), Cc + 24, rb.ptr(0) if rb else 0, Cc + 8 if rb else 0,
                                                     st[0].data_ptr(), st[1].data_ptr(), ws.data_ptr(), st[2].data_ptr(),
                                                     st[3].data_ptr(), MOM, _stream()))
        torch.cuda.synchronize()
        outs.append((yb, st))
    if repeat:
        assert torch.equal(outs[0][0].bits, outs[1][0].bits), "y: a repeat launch gave different bits"
        for a, b, what in zip(outs[0][1], outs[1][1], ("mean", "invstd", "running_mean", "running_var")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: a repeat launch gave different bits"
    yb, st = outs[0]
    return (_out_slice(yb, 16, Cc, "y"),) + tuple(t.cpu() for t in st)


def run_bwd(shape, z, dy, mean, invstd, gamma, beta, act, dev, repeat=True):
    """One backward launch on slices with the statistics given.  Returns dz (npix, C) float64, dbeta, dgamma (CPU fp32)."""
    capi = _capi()
    B, H, W = shape
    npix, Cc = z.shape
    zb = _in_slice(shape, Cc, 16, 8, z, dev, 3)
    dyb = _in_slice(shape, Cc, 8, 8, dy, dev, 4)
    d = [t.float().to(dev) for t in (mean, invstd, gamma, beta)]
    outs = []
    for _ in range(2 if repeat else 1):
        dzb = L.Guarded(B, H, W, Cc + 32, dev)
        sums = torch.full((2 * Cc,), float("nan"), device=dev)
        ws = _nan_ws(capi, Cc, dev)
        capi.check(capi.lib.m355_bn_train_bwd_launch(zb.ptr(8), dyb.ptr(8), npix, Cc + 16, Cc + 8, Cc, d[0].data_ptr(), d[1].data_ptr(),
                                                     d[2].data_ptr(), d[3].data_ptr(), act, dzb.ptr(24), Cc + 32, sums.data_ptr(),
                                                     ws.data_ptr(), _stream()))
        torch.cuda.synchronize()
        outs.append((dzb, sums))
    if repeat:
        assert torch.equal(outs[0][0].bits, outs[1][0].bits), "dz: a repeat launch gave different bits"
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), "dbeta / dgamma: a repeat launch gave different bits"
    dzb, sums = outs[0]
    sums = sums.cpu()
    return _out_slice(dzb, 24, Cc, "dz"), sums[:Cc], sums[Cc:]


@functools.lru_cache(maxsize=2)
def _case(name, shift, variant):
    """Inputs and float64 statistics of one case, shared by the forward and the backward test (and left unchanged)."""
    Cc, shape = R.SHAPES[name]
    npix = R.case_npix(name)
    z, gamma, beta = R.draw_z(npix, Cc, variant, 1000 + npix + shift, shift)
    g = torch.Generator().manual_seed(npix + 17 * shift)
    res = torch.randn(npix, Cc, generator=g).half().double()
    dy = torch.randn(npix, Cc, generator=g).half().double()
    rm0, rv0 = torch.randn(Cc, generator=g) * 0.1, 0.5 + torch.rand(Cc, generator=g)
    return shape, z, gamma, beta, res, dy, rm0, rv0, R.stats64(z)


def check_stats(z, stats, got, rm0, rv0, shift, note):
    """mean, invstd, running_mean, running_var of one launch against float64, every channel; the worst ratios to the tolerances."""
    mean, _, var_u, invstd = stats
    want = {"mean": mean, "invstd": invstd, "running_mean": (1 - MOM) * rm0.double() + MOM * mean,
            "running_var": (1 - MOM) * rv0.double() + MOM * var_u}
    worst = {k: float(R.stat_ratio(g, want[k], k).max()) for k, g in zip(want, got)}
    print(f"{note}: worst ratio to tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, g in zip(want, got):
        R.check_stat(g, want[k], k, shift, note + ": ")


# each variant runs two of the four (act, residual) forms, so every shape sees all four
_FORMS = {"plain": ((1, True), (0, False)), "outliers": ((1, False), (0, True))}
FWD_CASES = [(n, s, v, act, r) for n, s in R.STAT_CASES for v in R.VARIANTS for act, r in _FORMS[v]]
BWD_CASES = [(n, s, v, act) for n, s in R.STAT_CASES for v in R.VARIANTS for act in (0, 1)]


def _id(c):
    return f"{c[0]}{c[1]}-{c[2]}-" + ("silu" if c[3] else "linear") + ("+res" if len(c) > 4 and c[4] else "")


@pytest.mark.parametrize("name,shift,variant,act,use_res", FWD_CASES, ids=[_id(c) for c in FWD_CASES])
def test_forward_hard_statistics(name, shift, variant, act, use_res, cuda_device):
    shape, z, gamma, beta, res, _, rm0, rv0, stats = _case(name, shift, variant)
    res = res if use_res else None
    y, mean, invstd, rm, rv = run_fwd(shape, z, gamma, beta, act, res, rm0, rv0, cuda_device)
    note = f"fwd {name}{shift} {variant} act {act} res {use_res}"
    m, i = mean.double(), invstd.double()
    y64, u64 = R.fwd_ref(z, m, i, gamma, beta, act, res)
    w = R.check_elements(y, y64, R.fwd_tol(z, y64, u64, m, i, gamma, beta, act, res), note + " y (with the returned statistics)", shift)
    print(f"{note}: y worst |err| / bound {w:.3f}")
    check_stats(z, stats, (mean, invstd, rm, rv), rm0, rv0, shift, note)


def check_bwd(shape, z, dy, mean, invstd, gamma, beta, act, dev, note, shift=0):
    """One backward launch judged: dbeta / dgamma per channel, dz per element with the returned sums.  Returns (dbeta, dgamma)."""
    mean, invstd = mean.float().double(), invstd.float().double()          # float64 statistics, rounded once to fp32
    dz, dbeta, dgamma = run_bwd(shape, z, dy, mean, invstd, gamma, beta, act, dev)
    xh, du, e_du = R.bwd_terms(z, dy, mean, invstd, gamma, beta, act)
    db64, dg64, tb, tg = R.bwd_sums_ref(xh, du, e_du)
    wb = R.check_elements(dbeta.double(), db64, tb, note + " dbeta", shift)
    wg = R.check_elements(dgamma.double(), dg64, tg, note + " dgamma", shift)
    dz64, tz = R.bwd_dz_ref(xh, du, e_du, invstd, gamma, dbeta.double(), dgamma.double())
    wz = R.check_elements(dz, dz64, tz, note + " dz (with the returned sums)", shift)
    print(f"{note}: worst |err| / bound dbeta {wb:.3g}, dgamma {wg:.3g}, dz {wz:.3f}")
    return dbeta, dgamma


@pytest.mark.parametrize("name,shift,variant,act", BWD_CASES, ids=[_id(c) for c in BWD_CASES])
def test_backward_hard_statistics(name, shift, variant, act, cuda_device):
    shape, z, gamma, beta, _, dy, _, _, stats = _case(name, shift, variant)
    check_bwd(shape, z, dy, stats[0], stats[3], gamma, beta, act, cuda_device, f"bwd {name}{shift} {variant} act {act}", shift)


# ---------------------------------------------------------------------------------------------------- every pixel once
def _spikes(npix, Cc):
    """z and dy zero except one spike per channel: channel c at seam_pixels[c mod 8]; gamma 1, beta 0."""
    seams = R.seam_pixels(npix, Cc)
    z, dy = torch.zeros(npix, Cc, dtype=torch.float64), torch.zeros(npix, Cc, dtype=torch.float64)
    c = torch.arange(Cc)
    px = torch.tensor(seams)[c % len(seams)]
    z[px, c] = 3.0 + (c % 5).double()
    dy[px, c] = torch.tensor([2.0, 1.0, -1.0], dtype=torch.float64)[c % 3]
    return z, dy, torch.ones(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)


@pytest.mark.parametrize("name", ["c", "d", "e"])
def test_every_pixel_counted_once_spikes(name, cuda_device):
    """A dropped or doubled seam pixel changes that channel's mean, dbeta and dgamma by 100 %."""
    Cc, shape = R.SHAPES[name]
    npix = R.case_npix(name)
    z, dy, gamma, beta = _spikes(npix, Cc)
    stats = R.stats64(z)
    rm0, rv0 = torch.zeros(Cc), torch.ones(Cc)
    note = f"spikes {name} (seam pixels {R.seam_pixels(npix, Cc)})"
    y, mean, invstd, rm, rv = run_fwd(shape, z, gamma, beta, 0, None, rm0, rv0, cuda_device, repeat=False)
    check_stats(z, stats, (mean, invstd, rm, rv), rm0, rv0, None, note)
    m, i = mean.double(), invstd.double()
    y64, u64 = R.fwd_ref(z, m, i, gamma, beta, 0)
    R.check_elements(y, y64, R.fwd_tol(z, y64, u64, m, i, gamma, beta, 0), note + " y", None)
    check_bwd(shape, z, dy, stats[0], stats[3], gamma, beta, 0, cuda_device, note, None)


@pytest.mark.parametrize("name", ["c", "d", "e"])
def test_every_pixel_counted_once_constant_channels(name, cuda_device):
    """Constant channels (0, 12.5, -3, 0.25 ...) and integer dy: dbeta is the exact integer sum (exact in fp32 in any order
    below 2^24), dgamma is exactly 0 (xhat is), the variance is exactly 0, and the mean meets rtol 1e-5: one pixel counted
    twice moves it by 1 / npix > 1e-5 at these sizes."""
    Cc, shape = R.SHAPES[name]
    npix = R.case_npix(name)
    assert 1.0 / npix > 1e-5
    g = torch.Generator().manual_seed(npix)
    const = torch.tensor([0.0, 12.5, -3.0, 0.25, 1000.0, 12.5, 0.0, -60.0], dtype=torch.float64)[torch.arange(Cc) % 8]
    z = const.expand(npix, Cc).contiguous()
    dy = torch.randint(-3, 4, (npix, Cc), generator=g).double()
    gamma, beta = torch.ones(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    stats = R.stats64(z)
    assert float(stats[1].max()) == 0.0
    rm0, rv0 = torch.zeros(Cc), torch.ones(Cc)
    note = f"constant channels {name}"
    _, mean, invstd, rm, rv = run_fwd(shape, z, gamma, beta, 0, None, rm0, rv0, cuda_device, repeat=False)
    check_stats(z, stats, (mean, invstd, rm, rv), rm0, rv0, None, note)
    dbeta, dgamma = check_bwd(shape, z, dy, stats[0], stats[3], gamma, beta, 0, cuda_device, note, None)
    assert torch.equal(dbeta.double(), dy.sum(0)), f"{note}: dbeta is not the exact sum; worst difference {float((dbeta.double() - dy.sum(0)).abs().max())}"
    assert float(dgamma.abs().max()) == 0.0


def test_launcher_refuses_more_than_2048_channels(cuda_device):
    """C / 8 > 256 channel groups do not fit a block: an error, no launch (C = 2048 itself is shape f above)."""
    capi = _capi()
    dev = cuda_device
    Cc = 2056
    t = [torch.zeros(Cc, device=dev) for _ in range(4)]
    buf = torch.zeros(2 * Cc, dtype=torch.float16, device=dev)
    ws = _nan_ws(capi, Cc, dev)
    rc = capi.lib.m355_bn_train_fwd_launch(buf.data_ptr(), 2, Cc, Cc, t[0].data_ptr(), t[1].data_ptr(), R.EPS, 1, buf.data_ptr(), Cc, 0, 0,
                                           t[2].data_ptr(), t[3].data_ptr(), ws.data_ptr(), 0, 0, MOM, _stream())
    assert rc != 0
    sums = torch.zeros(2 * Cc, device=dev)
    rc = capi.lib.m355_bn_train_bwd_launch(buf.data_ptr(), buf.data_ptr(), 2, Cc, Cc, Cc, t[2].data_ptr(), t[3].data_ptr(), t[0].data_ptr(),
                                           t[1].data_ptr(), 1, buf.data_ptr(), Cc, sums.data_ptr(), ws.data_ptr(), _stream())
    assert rc != 0
    torch.cuda.synchronize()
