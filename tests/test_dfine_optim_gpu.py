"""dfine.clip_grad_norm_ and dfine.bind_optimizer on the GPU (csrc/dfine_optim.hip) against the float64 restatement of
tests/dfine_optim_ref.py, with torch's own fp32 step on the same GPU as the yardstick of what fp32 can deliver.

Rule (1), for every tensor and each of p, m, v:   max|got - ref64| <= 2 max|torch_fp32 - ref64| + 2^-23 max|ref64|.

The parameters are synthetic.  Every p, g, m, v of the bound arm is a slice of a larger buffer filled with a sentinel word; the
slices start 0, 4, 8 or 12 bytes after a 16-byte boundary, in the four roles independently, and every sentinel word is checked
after every call.  Sizes: around 64, 256, 1024 and the chunk size CH, one 2-D tensor, and one tensor of 260 chunks so that the
sum of the chunks' partial sums (256 threads) takes a second trip."""
import functools
import io
import warnings

import numpy as np
import pytest
import torch

import dfine_optim_ref as ref

pytestmark = pytest.mark.gpu

from defectdetection_viaobjectdetection_amd._capi import DFINE_OPTIM_CHUNK as CH   # noqa: E402

SHAPES = [(n,) for n in (1, 3, 7, 63, 64, 65, 255, 256, 257, 1023, CH - 1, CH, CH + 1, 2 * CH + 5)] + [(256, 132), (260 * CH,)]
HUGE = 2                  # the tensor whose gradients are all 1e18
# element offsets from a 16-byte boundary of (p, g, m, v), tensor i takes OFFSETS[i % 9]
OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 0)]
SENTINEL = 0x4B4B4B4B
STEPS = 5
EPS32 = 2.0 ** -23
KINDS = ("adam", "adam_wd", "adamw", "groups")
GROUPS3 = [dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8),
           dict(lr=3e-4, weight_decay=0.05, betas=(0.8, 0.99), eps=1e-6),
           dict(lr=2e-4, weight_decay=0.0, betas=(0.4, 0.95), eps=1e-7)]


def _numel(shape):
    return int(np.prod(shape))


@functools.lru_cache(None)
def host_values(huge: bool = True, steps: int = STEPS):
    """-> (parameters, gradients[step][tensor]) as fp32 arrays: normal gradients with exact zeros, -0 and 1e-20 among them, and
    with `huge` one tensor of 1e18"""
    rng = np.random.default_rng(5)
    params = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    grads = []
    for _ in range(steps):
        gs = []
        for i, s in enumerate(SHAPES):
            g = (rng.standard_normal(s) * 0.05).astype(np.float32)
            flat = g.reshape(-1)
            if flat.size >= 7:
                flat[0::7] = 0.0
                flat[1::7] = -0.0
                flat[2::7] = 1e-20
            if huge and i == HUGE:
                flat[:] = 1e18
            gs.append(g)
        gs[4][:] = 1e-20            # a whole tensor whose g^2 underflows
        grads.append(gs)
    return params, grads


class Placed:
    """one role's tensors as slices of a sentinel-filled buffer"""

    def __init__(self, role: int, device):
        starts, at = [], 8
        for i, s in enumerate(SHAPES):
            at = (at + 3) // 4 * 4 + OFFSETS[i % len(OFFSETS)][role]
            starts.append(at)
            at += _numel(s) + 8
        self.buf = torch.full((at + 8,), SENTINEL, dtype=torch.int32, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.mask = torch.ones(at + 8, dtype=torch.bool, device=device)
        self.views = []
        for i, (s, a) in enumerate(zip(SHAPES, starts)):
            self.mask[a:a + _numel(s)] = False
            self.views.append(self.buf.view(torch.float32)[a:a + _numel(s)].view(s))
            assert self.views[-1].data_ptr() % 16 == 4 * OFFSETS[i % len(OFFSETS)][role]

    def intact(self) -> bool:
        return bool((self.buf[self.mask] == SENTINEL).all())


def make_optimizer(kind: str, params, **flags):
    if kind == "adam":
        return torch.optim.Adam(params, lr=1e-3, **flags)
    if kind == "adam_wd":
        return torch.optim.Adam(params, lr=1e-3, weight_decay=0.01, **flags)
    if kind == "adamw":
        return torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01, **flags)
    assert kind == "groups"
    return torch.optim.AdamW([dict(params=params[j::3], **h) for j, h in enumerate(GROUPS3)], **flags)


def make_ref(kind: str, values):
    if kind == "groups":
        return ref.AdamRef(values, [i % 3 for i in range(len(values))], GROUPS3, True)
    wd = 0.0 if kind == "adam" else 0.01
    return ref.AdamRef(values, [0] * len(values), [dict(lr=1e-3, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)], kind == "adamw")


class Arm:
    """one optimizer over the synthetic tensors: `placed` puts p, g, m, v into sentinel buffers (m, v as pre-created state in
    torch's layout), otherwise they are ordinary tensors and the state is created by the step"""

    def __init__(self, kind, values, device, placed: bool, bind: bool, max_norm=None):
        self.device, self.roles = device, None
        if placed:
            self.roles = [Placed(r, device) for r in range(4)]
            for view, v in zip(self.roles[0].views, values):
                view.copy_(torch.from_numpy(v))
            self.params = [torch.nn.Parameter(view) for view in self.roles[0].views]
        else:
            self.params = [torch.nn.Parameter(torch.from_numpy(v).to(device)) for v in values]
        self.opt = make_optimizer(kind, self.params)
        if placed:
            for p, m, v in zip(self.params, self.roles[2].views, self.roles[3].views):
                self.opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m.zero_(), "exp_avg_sq": v.zero_()}
        if bind:
            from defectdetection_viaobjectdetection_amd import dfine
            assert dfine.bind_optimizer(self.opt, max_norm=max_norm) is self.opt and "step" in vars(self.opt)

    def set_grads(self, grads):
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
            elif self.roles is not None:
                p.grad = self.roles[1].views[i].copy_(torch.from_numpy(g))
            else:
                p.grad = torch.from_numpy(g).to(self.device)

    def intact(self) -> bool:
        return self.roles is None or all(r.intact() for r in self.roles)

    def snapshot(self):
        """[(p, m, v, step)] per tensor on the host; m, v None and step 0 without state"""
        out = []
        for p in self.params:
            st = self.opt.state.get(p) or {}
            out.append((p.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy() if st else None,
                        st["exp_avg_sq"].cpu().numpy().copy() if st else None, float(st["step"]) if st else 0.0))
        return out


def ref_snapshot(model):
    return [(p.copy(), m.copy(), v.copy(), float(t)) for p, m, v, t in zip(model.p, model.m, model.v, model.t)]


def assert_rule1(got, tor, want, what, finite_only=False):
    """rule (1) on one tensor; got, tor fp32 arrays, want float64"""
    got, tor = got.astype(np.float64), tor.astype(np.float64)
    if finite_only:
        keep = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), keep) and np.array_equal(np.isnan(got), np.isnan(tor)), what
        if not keep.any():
            return
        got, tor, want = got[keep], tor[keep], want[keep]
    with np.errstate(all="ignore"):
        err, floor, top = np.abs(got - want).max(), np.abs(tor - want).max(), np.abs(want).max()
    assert err <= 2 * floor + EPS32 * top, (what, err, floor, top)


def assert_snapshots(got, tor, want, what, finite_only=False):
    for i, (g, t, w) in enumerate(zip(got, tor, want)):
        assert g[3] == t[3] == w[3], (what, i, "step", g[3], t[3], w[3])
        for k, name in enumerate("pmv"):
            if t[k] is None:
                assert g[k] is None or not g[k].any(), (what, i, name)
                continue
            assert_rule1(g[k], t[k], w[k], (what, i, name), finite_only)


def run_updates(kind: str, max_norm=None):
    """the three arms over STEPS steps of the same gradients -> {1: (got, torch, ref64), 5: ...}, the norms per step, and whether
    every sentinel stayed and every .grad kept its bits"""
    from defectdetection_viaobjectdetection_amd import dfine
    device = torch.device("cuda", 0)
    calls = dict(dfine.optim_calls)
    values, grads = host_values(huge=max_norm is None)
    bound = Arm(kind, values, device, placed=True, bind=True, max_norm=max_norm)
    plain = Arm(kind, values, device, placed=False, bind=False)
    model = make_ref(kind, values)
    shots, norms, intact, grads_kept = {}, [], True, True
    for k in range(STEPS):
        bound.set_grads(grads[k])
        plain.set_grads(grads[k])
        bound.opt.step()
        intact = intact and bound.intact()
        grads_kept = grads_kept and all(np.array_equal(p.grad.cpu().numpy().view(np.int32), g.view(np.int32))
                                        for p, g in zip(bound.params, grads[k]))
        tor_norm = torch.nn.utils.clip_grad_norm_(plain.params, max_norm) if max_norm is not None else None
        plain.opt.step()
        want_norm = model.step(grads[k], max_norm)
        if max_norm is not None:
            norms.append((float(bound.opt.last_grad_norm), float(tor_norm), want_norm))
        if k + 1 in (1, STEPS):
            shots[k + 1] = (bound.snapshot(), plain.snapshot(), ref_snapshot(model))
    assert dfine.optim_calls == {"kernel": calls["kernel"] + STEPS, "torch": calls["torch"]}    # every bound step took the kernels
    return shots, norms, intact, grads_kept


updates = functools.lru_cache(None)(run_updates)   # computed once, shared by the tests that read it


def assert_norm(got, tor, want, what):
    assert abs(got - want) / want <= 2 * abs(tor - want) / want + EPS32, (what, got, tor, want)


@pytest.mark.parametrize("kind", KINDS)
def test_update_against_float64(cuda_device, kind):
    shots, _, intact, _ = updates(kind)
    assert intact, "a sentinel word next to a tensor changed"
    for n in (1, STEPS):
        assert_snapshots(*shots[n], (kind, n))
        assert all(s[3] == n for s in shots[n][0])


@pytest.mark.parametrize("kind", ("adamw", "groups"))
def test_fused_clip(cuda_device, kind):
    shots, norms, intact, grads_kept = updates(kind, 1.0)
    assert intact, "a sentinel word next to a tensor changed"
    assert grads_kept, "the fused clip must leave .grad as backward left it"
    for n in (1, STEPS):
        assert_snapshots(*shots[n], (kind, "clip", n))
    for k, (got, tor, want) in enumerate(norms):
        assert want > 1.0                      # the clip is active
        assert_norm(got, tor, want, (kind, k))


def _placed_grads(device, arrays):
    """parameters whose gradients sit in a sentinel buffer"""
    role = Placed(1, device)
    params = [torch.nn.Parameter(torch.empty(s, device=device)) for s in SHAPES]
    for p, view, a in zip(params, role.views, arrays):
        p.grad = view.copy_(torch.from_numpy(a))
    return role, params


def test_norm_exact_integer_probe(cuda_device):
    """gradients from {-1, 0, 1, 2}: every partial sum is an integer below 2^24, exact in fp32 in any order, so the norm is
    float32(sqrt(sum)) to the bit; a dropped or doubled chunk cannot hide"""
    from defectdetection_viaobjectdetection_amd import dfine
    rng = np.random.default_rng(3)
    arrays = [rng.integers(-1, 3, s).astype(np.float32) for s in SHAPES]
    sums = [float(np.square(a.astype(np.float64)).sum()) for a in arrays]
    assert 4 * sum(sums) < 2 ** 24
    exact = lambda total: np.float32(np.sqrt(np.float64(total)))   # noqa: E731
    role, params = _placed_grads(cuda_device, arrays)
    got = dfine.clip_grad_norm_(params, 1e30)
    assert got.dim() == 0 and got.is_cuda
    assert np.float32(got.item()) == exact(sum(sums)) and role.intact()
    assert all(np.array_equal(p.grad.cpu().numpy(), a) for p, a in zip(params, arrays))   # nothing scaled: the coefficient is 1
    # every chunk of every tensor zeroed in turn
    norms, wants = [], []
    for i, a in enumerate(arrays):
        flat_dev, flat = role.views[i].view(-1), a.reshape(-1)
        for c0 in range(0, flat.size, CH):
            part = float(np.square(flat[c0:c0 + CH].astype(np.float64)).sum())
            if part == 0:
                continue
            flat_dev[c0:c0 + CH] = 0
            norms.append(dfine.clip_grad_norm_(params, 1e30))
            wants.append(exact(sum(sums) - part))
            flat_dev[c0:c0 + CH] = torch.from_numpy(flat[c0:c0 + CH]).to(cuda_device)
    assert len(norms) > 256
    got = torch.stack(norms).cpu().numpy()
    assert np.array_equal(got, np.array(wants, np.float32)) and not (got == exact(sum(sums))).any()
    # one tensor counted twice
    for i in (9, 13, 14):
        role.views[i].mul_(2)
        got = np.float32(dfine.clip_grad_norm_(params, 1e30).item())
        assert got == exact(sum(sums) + 3 * sums[i]) and got != exact(sum(sums)), i
        role.views[i].copy_(torch.from_numpy(arrays[i]))
    assert role.intact()


def test_norm_and_clip_on_random_data(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    _, grads = host_values(huge=False)
    arrays = grads[0]
    want = ref.total_norm(arrays)
    role, params = _placed_grads(cuda_device, arrays)
    plain = [torch.nn.Parameter(torch.empty(s, device=cuda_device)) for s in SHAPES]
    for max_norm in (1.0, 0.01):
        for p, view, a in zip(plain, role.views, arrays):
            p.grad = torch.from_numpy(a).to(cuda_device)
            view.copy_(p.grad)
        got = dfine.clip_grad_norm_(params, max_norm)
        tor = torch.nn.utils.clip_grad_norm_(plain, max_norm)
        assert role.intact()
        assert want > max_norm
        assert_norm(float(got), float(tor), want, max_norm)
        c = ref.clip_coefficient(want, max_norm)
        for i, (p, q, a) in enumerate(zip(params, plain, arrays)):
            assert_rule1(p.grad.cpu().numpy(), q.grad.cpu().numpy(), a.astype(np.float64) * c, (max_norm, i))
    # below max_norm nothing changes, to the bit
    for view, a in zip(role.views, arrays):
        view.copy_(torch.from_numpy(a))
    got = dfine.clip_grad_norm_(params, 2 * want)
    assert_norm(float(got), float(tor), want, "unclipped")
    assert all(np.array_equal(p.grad.cpu().numpy().view(np.int32), a.view(np.int32)) for p, a in zip(params, arrays))
    assert role.intact()


def test_two_runs_give_the_same_bits(cuda_device):
    runs = []
    for _ in range(2):
        shots, norms, _, _ = run_updates("groups", 1.0)
        runs.append((shots[STEPS][0], [n[0] for n in norms]))
    (a, na), (b, nb) = runs
    assert np.array_equal(np.array(na, np.float32).view(np.int32), np.array(nb, np.float32).view(np.int32))
    for x, y in zip(a, b):
        for k in range(3):
            assert np.array_equal(x[k].view(np.int32), y[k].view(np.int32))


def test_parameters_without_gradient_are_skipped(cuda_device):
    """gradient None: p, m, v and `step` stay to the bit, also for a tensor that was updated before (its t then lags)"""
    values, grads = host_values()
    skip = {1: {0, 5, 11, 13}, 2: {5, 15}}            # step index -> tensors without a gradient; 3: never a gradient
    never = 3
    bound = Arm("groups", values, cuda_device, placed=True, bind=True)
    plain = Arm("groups", values, cuda_device, placed=False, bind=False)
    plain.params[never].requires_grad_(False)
    bound.params[never].requires_grad_(False)
    model = make_ref("groups", values)
    for k in range(4):
        gs = [None if i == never or i in skip.get(k, ()) else g for i, g in enumerate(grads[k])]
        before = bound.snapshot()
        for arm in (bound, plain):
            arm.set_grads(gs)
            arm.opt.step()
        model.step(gs)
        after = bound.snapshot()
        assert bound.intact()
        for i, g in enumerate(gs):
            if g is None:
                assert before[i][3] == after[i][3]
                assert all(np.array_equal(before[i][j].view(np.int32), after[i][j].view(np.int32)) for j in range(3)), (k, i)
            else:
                assert after[i][3] == before[i][3] + 1
    got, tor = bound.snapshot(), plain.snapshot()
    assert [s[3] for s in got] == [s[3] for s in tor] == [float(t) for t in model.t]
    assert got[5][3] == 2 and got[never][3] == 0 and got[1][3] == 4
    # the plain arm has no state for the tensor that never had a gradient; the placed arm's pre-created state is untouched
    assert tor[never][1] is None and not got[never][1].any() and not got[never][2].any()
    assert_snapshots(got, tor, ref_snapshot(model), "skipping")


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_non_finite_gradients_behave_as_in_torch(cuda_device, bad):
    values, grads = host_values(huge=False)
    gs = [g.copy() for g in grads[0]]
    gs[8].reshape(-1)[100] = bad
    bound = Arm("adamw", values, cuda_device, placed=True, bind=True, max_norm=1.0)
    plain = Arm("adamw", values, cuda_device, placed=False, bind=False)
    model = make_ref("adamw", values)
    bound.set_grads(gs)
    plain.set_grads(gs)
    bound.opt.step()
    tor_norm = torch.nn.utils.clip_grad_norm_(plain.params, 1.0)
    plain.opt.step()
    model.step(gs, 1.0)
    norm = float(bound.opt.last_grad_norm)
    assert bound.intact()
    assert (norm == np.inf and float(tor_norm) == np.inf) if bad == np.inf else (np.isnan(norm) and np.isnan(float(tor_norm)))
    got, tor, want = bound.snapshot(), plain.snapshot(), ref_snapshot(model)
    for i, (g, t) in enumerate(zip(got, tor)):
        for k in range(3):
            assert np.array_equal(np.isnan(g[k]), np.isnan(t[k])) and np.array_equal(np.isfinite(g[k]), np.isfinite(t[k])), (i, k)
    if bad == np.inf:     # one NaN element, every other gradient scaled to 0
        assert sum(int(np.isnan(g[0]).sum()) for g in got) == 1 and np.isnan(got[8][0].reshape(-1)[100])
    else:                 # a NaN norm poisons everything
        assert all(np.isnan(g[k]).all() for g in got for k in range(3))
    assert_snapshots(got, tor, want, bad, finite_only=True)


@pytest.mark.parametrize("bound_first", [True, False], ids=["bound_then_torch", "torch_then_bound"])
def test_state_dict_interchange(cuda_device, bound_first):
    from defectdetection_viaobjectdetection_amd import dfine
    values, grads = host_values()
    first = Arm("groups", values, cuda_device, placed=False, bind=bound_first)
    for k in range(3):
        first.set_grads(grads[k])
        first.opt.step()
    steps = [first.opt.state[p]["step"] for p in first.params]
    assert all(t.dim() == 0 and t.dtype is torch.float32 and t.device.type == "cpu" and float(t) == 3 for t in steps)   # torch's layout
    second = Arm("groups", [p.detach().cpu().numpy() for p in first.params], cuda_device, placed=False, bind=False)
    blob = io.BytesIO()
    torch.save({"optimizer_state_dict": first.opt.state_dict()}, blob)     # through a checkpoint, as the trainers write it
    blob.seek(0)
    second.opt.load_state_dict(torch.load(blob)["optimizer_state_dict"])
    if not bound_first:
        assert dfine.bind_optimizer(second.opt) is second.opt and "step" in vars(second.opt)
    for k in range(3, STEPS):
        second.set_grads(grads[k])
        second.opt.step()
    shots, _, _, _ = updates("groups")
    _, tor, want = shots[STEPS]
    assert_snapshots(second.snapshot(), tor, want, "interchange")


@pytest.mark.parametrize("case", ["amsgrad", "maximize", "fused", "cpu", "fp16"])
def test_fallbacks_leave_the_optimizer_unbound(cuda_device, case):
    from defectdetection_viaobjectdetection_amd import dfine
    rng = np.random.default_rng(2)
    values = [rng.standard_normal(s).astype(np.float32) for s in ((5,), (3, 4), (300,))]
    grads = [rng.standard_normal(v.shape).astype(np.float32) for v in values]
    flags = {case: True} if case in ("amsgrad", "maximize", "fused") else {}

    def build():
        ps = [torch.nn.Parameter(torch.from_numpy(v.copy()).to(cuda_device)) for v in values]
        if case == "cpu":
            ps[1] = torch.nn.Parameter(torch.from_numpy(values[1].copy()))
        if case == "fp16":
            ps[1] = torch.nn.Parameter(torch.from_numpy(values[1].copy()).to(cuda_device).half())
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(device=p.device, dtype=p.dtype)
        return ps, torch.optim.AdamW(ps, lr=1e-3, weight_decay=0.01, **flags)

    (pa, a), (pb, b) = build(), build()
    assert dfine.bind_optimizer(a, max_norm=1.0) is a
    assert "step" not in vars(a) and not hasattr(a, "_m355_optim")
    a.step()
    b.step()
    for x, y in zip(pa, pb):
        assert torch.equal(x.detach().cpu(), y.detach().cpu())
        assert torch.equal(a.state[x]["exp_avg_sq"].cpu(), b.state[y]["exp_avg_sq"].cpu())


def _sync_debug_mode_is_honoured(dev):
    t = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_clip_and_step_do_not_synchronise(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    values, grads = host_values(huge=False)
    arms = [Arm("groups", values, cuda_device, placed=False, bind=True, max_norm=m) for m in (None, 1.0)]
    for arm in arms:
        arm.set_grads(grads[0])

    def run():
        out = [dfine.clip_grad_norm_(arms[0].params, 1.0)]
        for arm in arms:
            arm.opt.step()
        return out + [arms[1].opt.last_grad_norm]

    run()                                  # warm-up: lazy initialisation and the first pinned allocations may synchronise
    torch.cuda.synchronize()
    before = dict(dfine.optim_calls)
    if _sync_debug_mode_is_honoured(cuda_device):
        print("sync detector: torch.cuda.set_sync_debug_mode('error')")
        torch.cuda.set_sync_debug_mode("error")
        try:
            norms = run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        print("sync detector: torch.profiler, no device-to-host copy")
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            norms = run()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()]
        assert not [n for n in names if "dtoh" in n.lower().replace(" ", "").replace("_", "") or "DeviceToHost" in n], names
    assert dfine.optim_calls["kernel"] == before["kernel"] + 3 and dfine.optim_calls["torch"] == before["torch"]
    assert all(n.dim() == 0 and n.is_cuda and bool(torch.isfinite(n)) for n in norms)


@pytest.mark.parametrize("bind_first", [True, False], ids=["bound_before_scheduler", "bound_after_scheduler"])
def test_scheduler_order(cuda_device, bind_first):
    """torch's call-order tracking survives the binding in either order, and the next step uses the scheduler's new lr"""
    from defectdetection_viaobjectdetection_amd import dfine
    values = [np.ones((300,), np.float32), np.ones((5, 3), np.float32)]
    grads = [np.full(v.shape, 0.5, np.float32) for v in values]
    params = [torch.nn.Parameter(torch.from_numpy(v.copy()).to(cuda_device)) for v in values]
    opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=0.0)
    model = ref.AdamRef(values, [0, 0], [dict(lr=1e-2, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8)], True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if bind_first:
            dfine.bind_optimizer(opt)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=2)
        if not bind_first:
            dfine.bind_optimizer(opt)
        assert "step" in vars(opt) and hasattr(opt, "_m355_optim")
        calls = dfine.optim_calls["kernel"]
        for k in range(2):
            for p, g in zip(params, grads):
                p.grad = torch.from_numpy(g).to(cuda_device)
            model.groups[0]["lr"] = ref.cosine_lr(1e-2, k, 2)
            assert abs(opt.param_groups[0]["lr"] - model.groups[0]["lr"]) < 1e-12
            opt.step()
            sched.step()
            model.step(grads)
        assert dfine.optim_calls["kernel"] == calls + 2
    assert model.groups[0]["lr"] == 5e-3 or abs(model.groups[0]["lr"] - 5e-3) < 1e-15
    for p, w in zip(params, model.p):        # with the first lr in both steps the result would be 2.5e-3 away
        np.testing.assert_allclose(p.detach().cpu().numpy(), w, rtol=0, atol=2e-6)


def test_end_to_end_small(cuda_device):
    """DFineForObjectDetection with the backbone frozen, three groups as in the improved trainer: one bound step against one
    unbound step from the same state and the same gradients"""
    try:
        from transformers import DFineConfig, DFineForObjectDetection
    except Exception as ex:  # noqa: BLE001
        pytest.skip(f"transformers D-FINE not importable here: {ex}")
    import copy
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(0)
    try:
        model_a = DFineForObjectDetection(DFineConfig(dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)).to(cuda_device).train()
    except ImportError as ex:
        pytest.skip(f"DFineForObjectDetection(DFineConfig()) cannot be built here: {ex}")
    for n, p in model_a.named_parameters():
        if "backbone" in n:
            p.requires_grad_(False)
    model_b = copy.deepcopy(model_a)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(cuda_device)
    out = model_a.model(pixel_values=x)
    out.last_hidden_state.square().mean().mul(100).backward()

    def groups(model):
        named = [(n, p) for n, p in model.named_parameters() if "backbone" not in n]
        return [dict(params=[p for n, p in named if "decoder" in n], lr=1e-4),
                dict(params=[p for n, p in named if "encoder" in n and "decoder" not in n], lr=5e-5),
                dict(params=[p for n, p in named if "encoder" not in n and "decoder" not in n], lr=2e-4)]

    opt_a = dfine.bind_optimizer(torch.optim.AdamW(groups(model_a), weight_decay=0.01), max_norm=1.0)
    opt_b = torch.optim.AdamW(groups(model_b), weight_decay=0.01)
    assert "step" in vars(opt_a)
    pa, pb = dict(model_a.named_parameters()), dict(model_b.named_parameters())
    names = [n for n in pa if "backbone" not in n]
    for n in names:
        pb[n].grad = None if pa[n].grad is None else pa[n].grad.clone()
    start = {n: pa[n].detach().double().cpu().numpy() for n in names}
    g64 = {n: None if pa[n].grad is None else pa[n].grad.double().cpu().numpy() for n in names}
    order = [n for g in groups(model_a) for p in g["params"] for n in names if pa[n] is p]
    group_of = [j for j, g in enumerate(groups(model_a)) for _ in g["params"]]
    hyper = [dict(lr=lr, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8) for lr in (1e-4, 5e-5, 2e-4)]
    model = ref.AdamRef([start[n] for n in order], group_of, hyper, True)
    before = dfine.optim_calls["kernel"]
    opt_a.step()
    assert dfine.optim_calls["kernel"] == before + 1
    tor_norm = torch.nn.utils.clip_grad_norm_([pb[n] for n in names], 1.0)
    opt_b.step()
    want_norm = model.step([g64[n] for n in order], 1.0)
    assert_norm(float(opt_a.last_grad_norm), float(tor_norm), want_norm, "e2e norm")
    untouched = lambda ps, opt: {n for n in names if not opt.state.get(ps[n])}   # noqa: E731
    assert untouched(pa, opt_a) == untouched(pb, opt_b) == {n for n in names if g64[n] is None}
    assert len(order) == len(names) > 500 and len(untouched(pa, opt_a)) < len(names)
    for i, n in enumerate(order):
        if g64[n] is None:
            assert np.array_equal(pa[n].detach().double().cpu().numpy(), start[n]), n
            continue
        sa, sb = opt_a.state[pa[n]], opt_b.state[pb[n]]
        assert float(sa["step"]) == float(sb["step"]) == 1.0
        assert_rule1(pa[n].detach().cpu().numpy(), pb[n].detach().cpu().numpy(), model.p[i], (n, "p"))
        assert_rule1(sa["exp_avg"].cpu().numpy(), sb["exp_avg"].cpu().numpy(), model.m[i], (n, "m"))
        assert_rule1(sa["exp_avg_sq"].cpu().numpy(), sb["exp_avg_sq"].cpu().numpy(), model.v[i], (n, "v"))
