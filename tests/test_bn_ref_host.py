"""Host checks of tests/bn_ref.py, the yardstick of tests/test_bn_train_gpu.py (no GPU):

  * the bounds are sound: an fp32 numpy restatement of the kernels' apply and backward arithmetic (csrc/train_kernels.hip), given
    accurate statistics, stays at |err| / bound <= 1 on every input family;
  * the bounds are sharp: four small mutants of that restatement exceed 1, on the channel they touch and on no other;
  * the cases are fair: torch's own fp32 batch norm on the CPU meets the statistic tolerances on every family, variant and shape
    the GPU test uses;
  * an fp32 scheme that meets them exists: a numpy model of the scheme bn_stats_kernel / bn_stats_merge_kernel use (per-thread
    pivot, shifted sums, fixed-order merges of (n, pivot + offset, M2)), and the geometry restatement it walks.
"""
import numpy as np
import pytest
import torch

import bn_ref as R

F32 = np.float32


# ---------------------------------------------------------------------------------------------------- fp32 restatements
def _sig32(t):
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-t, dtype=F32))).astype(F32)


def apply32(z, mean, invstd, gamma, beta, act, res=None, is_scale=None, drop_sh=None, res_roll=None):
    """bn_silu_apply_kernel's arithmetic in fp32, rounding for rounding; returns fp16 values as float64.
    Mutants: is_scale = (channel, factor) on invstd, drop_sh = channel without its shift, res_roll = channel whose residual
    is read one pixel late."""
    z, m, is_, g, b = (np.asarray(a, dtype=np.float64).astype(F32) for a in (z, mean, invstd, gamma, beta))
    if is_scale is not None:
        is_ = is_.copy()
        is_[is_scale[0]] *= F32(is_scale[1])
    sc = g * is_
    sh = b - m * sc
    if drop_sh is not None:
        sh[drop_sh] = 0
    t = z * sc + sh
    r = t * _sig32(t) if act else t
    if res is not None:
        rr = np.asarray(res, dtype=np.float64).astype(F32)
        if res_roll is not None:
            rr = rr.copy()
            rr[:, res_roll] = np.roll(rr[:, res_roll], 1)
        r = r + rr
    return torch.from_numpy(r.astype(np.float16).astype(np.float64))


def bwd32(z, dy, mean, invstd, gamma, beta, act, order="pairwise", skip=None):
    """bn_silu_bwd_reduce_kernel + bn_silu_bwd_apply_kernel in fp32: (dz as float64 of fp16 values, dbeta, dgamma as float64 of
    fp32 values).  order: how the fp32 sums run ("pairwise": numpy's, "sequential": pixel after pixel).  skip = (pixel,
    channel): that pixel is left out of the channel's two sums (mutant)."""
    z, dy, m, is_, g, b = (np.asarray(a, dtype=np.float64).astype(F32) for a in (z, dy, mean, invstd, gamma, beta))
    n = z.shape[0]
    xh = (z - m) * is_
    du = dy
    if act:
        t = g * xh + b
        sg = _sig32(t)
        du = dy * (sg * (F32(1) + t * (F32(1) - sg)))
    t1, t2 = du.copy(), du * xh
    if skip is not None:
        t1[skip] = 0
        t2[skip] = 0
    if order == "pairwise":
        dbeta, dgamma = t1.sum(0, dtype=F32), t2.sum(0, dtype=F32)
    else:
        dbeta, dgamma = np.cumsum(t1, 0, dtype=F32)[-1], np.cumsum(t2, 0, dtype=F32)[-1]
    inv_n = F32(1) / F32(n)
    dz = (g * is_) * ((du - dbeta * inv_n) - xh * (dgamma * inv_n))
    return (torch.from_numpy(dz.astype(np.float16).astype(np.float64)), torch.from_numpy(dbeta.astype(np.float64)),
            torch.from_numpy(dgamma.astype(np.float64)))


def _merge(a, b):
    """merge_moments of csrc/train_kernels.hip on tuples (n, pivot, offset, M2, sum) of fp32 arrays: pivot + offset is the mean
    the M2 merges use, sum / n the mean that is returned."""
    (na, pa, oa, qa, sa), (nb, pb, ob, qb, sb) = a, b
    n = na + nb
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(n > 0, nb / n, F32(0)).astype(F32)
    d = (pb - pa) + (ob - oa)
    empty = na == 0                                             # an empty partial has no pivot: take b as it is
    return (n, np.where(empty, pb, pa), np.where(empty, ob, oa + d * w), np.where(empty, qb, qa + (qb + d * d * (na * w))), sa + sb)


def stats_model32(z, C):
    """The forward statistics as bn_stats_kernel and bn_stats_merge_kernel compute them, in fp32 numpy: per-thread pivot and
    shifted sums, pairwise merge over a block's pixel lanes, rows merged pairwise by 64 row groups, groups merged pairwise.
    Returns (mean, M2) fp32 per channel."""
    z = np.asarray(z, dtype=np.float64).astype(F32)
    npix = z.shape[0]
    lp, rows, st = R.lanes_px(C), R.red_rows(npix, C), R.red_stride(npix, C)
    trips = (npix + st - 1) // st
    zz = np.zeros((trips * st, C), F32)
    zz[:npix] = z
    zz = zz.reshape(trips, st, C)
    valid = (np.arange(trips * st) < npix).reshape(trips, st, 1).astype(F32)
    K = zz[0]
    s, q = np.zeros((st, C), F32), np.zeros((st, C), F32)
    for k in range(trips):
        d = (zz[k] - K) * valid[k]
        s += d
        q += d * d
    n = np.broadcast_to(valid.sum(0), (st, C)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        off = np.where(n > 0, s / n, F32(0)).astype(F32)
    m = tuple(a.reshape(rows, lp, C) for a in (n, K, off, np.maximum(q - s * off, F32(0)), n * K + s))
    ln = lp
    while ln > 1:                                               # lanes of a block, pairwise: lane l takes lane l + ceil(ln / 2)
        half, h = (ln + 1) // 2, ln // 2
        merged = _merge(tuple(a[:, :h] for a in m), tuple(a[:, half:half + h] for a in m))
        m = tuple(np.concatenate([x, a[:, h:half]], 1) for x, a in zip(merged, m))
        ln = half
    m = tuple(a[:, 0] for a in m)
    slot = tuple(np.zeros((8, 64, C), F32) for _ in range(5))   # row group g holds rows g, g + 64, ...; the rest stay empty
    for a, src in zip(slot, m):
        a.reshape(512, C)[:rows] = src
    h = 1
    while h < 8:                                                # a group's rows, pairwise in registers
        for u in range(0, 8, 2 * h):
            for dst, src in zip(slot, _merge(tuple(a[u] for a in slot), tuple(a[u + h] for a in slot))):
                dst[u] = src
        h *= 2
    wave = tuple(a[0] for a in slot)
    h = 32
    while h >= 1:                                               # the 64 row groups, pairwise
        wave = _merge(tuple(a[:h] for a in wave), tuple(a[h:2 * h] for a in wave))
        h //= 2
    assert float(wave[0][0, 0]) == npix
    return wave[4][0] / wave[0][0], wave[3][0]


def running32(mean, var_b, npix, rm0, rv0, mom):
    """the apply kernel's running-statistics update in fp32."""
    mom, n = F32(mom), F32(npix)
    rm = (F32(1) - mom) * rm0.astype(F32) + mom * mean
    rv = (F32(1) - mom) * rv0.astype(F32) + mom * var_b * (n / max(n - F32(1), F32(1)))
    return rm, rv


# ---------------------------------------------------------------------------------------------------- geometry
def test_geometry_follows_the_launcher():
    """The rows the issue's shape table was built from (grid_red) and the walk the model relies on: every pixel belongs to
    exactly one (block, lane), block b owns pixels [b lanes_px, (b + 1) lanes_px) of every stride."""
    want = {"a": (256, 1), "b": (3, 6), "c": (8, 120), "d": (8, 512), "e": (32, 512), "f": (1, 5)}
    for name, (C, _) in R.SHAPES.items():
        npix = R.case_npix(name)
        assert (R.lanes_px(C), R.red_rows(npix, C)) == want[name], name
        for p in R.seam_pixels(npix, C):
            assert 0 <= p < npix
    assert R.idle_threads(576) == 40 and R.idle_threads(256) == 0
    assert R.seam_pixels(65792, 64)[:7] == [0, 65791, 16383, 16384, 65535, 65536, 65536]
    assert R.apply_blocks(20200, 256) == 158 and R.apply_blocks(10 ** 7, 8) == 2048


# ---------------------------------------------------------------------------------------------------- soundness
def _inputs(npix, C, variant, seed, shift=0):
    z, gamma, beta = R.draw_z(npix, C, variant, seed, shift)
    g = torch.Generator().manual_seed(seed + 1)
    res = torch.randn(npix, C, generator=g).half().double()
    dy = torch.randn(npix, C, generator=g).half().double()
    mean, _, _, invstd = R.stats64(z)
    return z, gamma, beta, res, dy, mean.float().double(), invstd.float().double()     # statistics rounded once to fp32


SOUND_SHAPES = [(26, 24, 0), (3698, 24, 5), (21, 8, 6), (70, 576, 0), (65536, 16, 0)]


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("npix,C,shift", SOUND_SHAPES)
def test_bounds_are_sound(npix, C, shift, variant):
    z, gamma, beta, res, dy, mean, invstd = _inputs(npix, C, variant, 11 * npix + C, shift)
    for act in (0, 1):
        for r in (None, res):
            y64, u64 = R.fwd_ref(z, mean, invstd, gamma, beta, act, r)
            tol = R.fwd_tol(z, y64, u64, mean, invstd, gamma, beta, act, r)
            assert float(y64.abs().max()) < 60000
            w = R.check_elements(apply32(z, mean, invstd, gamma, beta, act, r), y64, tol, f"y act {act} res {r is not None}", shift)
            print(f"y npix {npix} C {C} {variant} act {act} res {r is not None}: worst ratio {w:.3f}")
        xh, du, e_du = R.bwd_terms(z, dy, mean, invstd, gamma, beta, act)
        db64, dg64, tb, tg = R.bwd_sums_ref(xh, du, e_du)
        for order in ("pairwise", "sequential"):
            dz, db, dg = bwd32(z, dy, mean, invstd, gamma, beta, act, order)
            wb = R.check_elements(db, db64, tb, f"dbeta act {act} {order}", shift)
            wg = R.check_elements(dg, dg64, tg, f"dgamma act {act} {order}", shift)
            dz64, tz = R.bwd_dz_ref(xh, du, e_du, invstd, gamma, db, dg)
            wz = R.check_elements(dz, dz64, tz, f"dz act {act} {order}", shift)
            print(f"bwd npix {npix} C {C} {variant} act {act} {order}: worst ratio dbeta {wb:.3f} dgamma {wg:.3f} dz {wz:.3f}")


# ---------------------------------------------------------------------------------------------------- sharpness
def _only_channel(got, want, tol, c):
    """the mutant exceeds its bound on channel c, and no other channel does."""
    ratio = (got - want).abs() / tol
    per_ch = ratio.reshape(-1, ratio.shape[-1]).max(0).values
    assert float(per_ch[c]) > 1.0, f"channel {c}: the mutant stays at ratio {float(per_ch[c]):.3g}"
    others = per_ch.clone()
    others[c] = 0
    assert float(others.max()) <= 1.0, f"channel {int(others.argmax())} moved too: {float(others.max()):.3g}"
    return float(per_ch[c])


@pytest.mark.parametrize("c", [0, 4, 7, 9], ids=["plain", "mean100", "mean2048", "std30"])
@pytest.mark.parametrize("act", [0, 1])
def test_bounds_are_sharp_forward(c, act):
    npix, C = 3698, 24
    z, gamma, beta, res, _, mean, invstd = _inputs(npix, C, "plain", 77)
    y64, u64 = R.fwd_ref(z, mean, invstd, gamma, beta, act, res)
    tol = R.fwd_tol(z, y64, u64, mean, invstd, gamma, beta, act, res)
    for name, kw in (("invstd * (1 + 1e-3)", dict(is_scale=(c, 1 + 1e-3))), ("sh dropped", dict(drop_sh=c)),
                     ("residual one pixel late", dict(res_roll=c))):
        r = _only_channel(apply32(z, mean, invstd, gamma, beta, act, res, **kw), y64, tol, c)
        print(f"{name}, channel {c} {R.family_name(c)}, act {act}: ratio {r:.3g}")


def spike_inputs(npix, C, act=0):
    """z and dy zero except one spike per channel (channel c at seam_pixels[c % 8]), gamma 1, beta 0."""
    seams = R.seam_pixels(npix, C)
    z, dy = torch.zeros(npix, C, dtype=torch.float64), torch.zeros(npix, C, dtype=torch.float64)
    for c in range(C):
        z[seams[c % len(seams)], c] = 3.0 + (c % 5)
        dy[seams[c % len(seams)], c] = (2.0, 1.0, -1.0)[c % 3]
    return z, dy, torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), seams


def test_bounds_are_sharp_backward_sums():
    """One pixel left out of the backward reduction of one channel in a spike case: that channel's dbeta and dgamma miss."""
    npix, C = 3840, 16
    z, dy, gamma, beta, seams = spike_inputs(npix, C)
    mean, _, _, invstd = R.stats64(z)
    mean, invstd = mean.float().double(), invstd.float().double()
    xh, du, e_du = R.bwd_terms(z, dy, mean, invstd, gamma, beta, 0)
    db64, dg64, tb, tg = R.bwd_sums_ref(xh, du, e_du)
    _, db, dg = bwd32(z, dy, mean, invstd, gamma, beta, 0)
    R.check_elements(db, db64, tb, "dbeta")
    R.check_elements(dg, dg64, tg, "dgamma")
    for c in (0, 3, 6, 7):
        _, db, dg = bwd32(z, dy, mean, invstd, gamma, beta, 0, skip=(seams[c], c))
        _only_channel(db, db64, tb, c)
        _only_channel(dg, dg64, tg, c)


# ---------------------------------------------------------------------------------------------------- fair cases, a scheme that meets them
_RUN = {"mom": 0.03}


def _running_start(C):
    g = torch.Generator().manual_seed(C)
    return (torch.randn(C, generator=g) * 0.1), (0.5 + torch.rand(C, generator=g))


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("name,shift", R.STAT_CASES, ids=[f"{n}{s}" for n, s in R.STAT_CASES])
def test_cases_are_fair_and_an_fp32_scheme_meets_them(name, shift, variant):
    """torch's fp32 batch norm on the CPU, and the numpy model of the kernels' scheme, against float64: the project's
    tolerances (mean rtol 1e-5 atol 1e-6, invstd rtol 1e-5, running statistics rtol 1e-5 atol 1e-7) on every channel."""
    C = R.SHAPES[name][0]
    npix = R.case_npix(name)
    z, _, _ = R.draw_z(npix, C, variant, 1000 + npix + shift, shift)
    mean, var_b, var_u, invstd = R.stats64(z)
    mom = _RUN["mom"]
    rm0, rv0 = _running_start(C)
    want_rm, want_rv = (1 - mom) * rm0.double() + mom * mean, (1 - mom) * rv0.double() + mom * var_u

    rm, rv = rm0.clone(), rv0.clone()
    _, t_mean, t_is = torch.native_batch_norm(z.float().t().contiguous().reshape(1, C, npix, 1), None, None, rm, rv, True, mom, R.EPS)
    worst = [R.check_stat(t_mean, mean, "mean", shift, "torch fp32 ")[0], R.check_stat(t_is, invstd, "invstd", shift, "torch fp32 ")[0],
             R.check_stat(rm, want_rm, "running_mean", shift, "torch fp32 ")[0],
             R.check_stat(rv, want_rv, "running_var", shift, "torch fp32 ")[0]]
    print(f"{name}{shift} {variant} torch fp32: worst ratio to tolerance mean {worst[0]:.3g} invstd {worst[1]:.3g} "
          f"running_mean {worst[2]:.3g} running_var {worst[3]:.3g}")

    m32, m2 = stats_model32(z, C)
    v32 = np.maximum(m2 * (F32(1) / F32(npix)), F32(0))
    is32 = (F32(1) / np.sqrt(v32 + F32(R.EPS), dtype=F32)).astype(F32)
    rm32, rv32 = running32(m32, v32, npix, rm0.numpy(), rv0.numpy(), mom)
    t = torch.from_numpy
    worst = [R.check_stat(t(m32), mean, "mean", shift, "model ")[0], R.check_stat(t(is32), invstd, "invstd", shift, "model ")[0],
             R.check_stat(t(rm32), want_rm, "running_mean", shift, "model ")[0],
             R.check_stat(t(rv32), want_rv, "running_var", shift, "model ")[0]]
    print(f"{name}{shift} {variant} model: worst ratio to tolerance mean {worst[0]:.3g} invstd {worst[1]:.3g} "
          f"running_mean {worst[2]:.3g} running_var {worst[3]:.3g}")


def test_the_cancelling_form_misses_on_the_hard_families():
    """Why the cases exist: sum z^2 / n - mean^2 from fp32 sums misses invstd by far more than rtol 1e-5 where |mean| >> std."""
    npix, C = 3840, 24
    z, _, _ = R.draw_z(npix, C, "plain", 5)
    _, _, _, invstd = R.stats64(z)
    z32 = z.numpy().astype(F32)
    m = z32.sum(0, dtype=F32) / F32(npix)
    var = np.maximum((z32 * z32).sum(0, dtype=F32) / F32(npix) - m * m, F32(0))
    r = R.stat_ratio(torch.from_numpy(F32(1) / np.sqrt(var + F32(R.EPS))), invstd, "invstd")
    assert float(r[0]) <= 1.0 and float(r[4]) > 100 and float(r[6]) > 100, r
