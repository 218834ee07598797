"""Replay of the training step's real strided launches.  One forward + backward step of TrainEngine at a small size records the
geometry of every m355_conv_launch and m355_wgrad_launch it issues (shapes, ld*, image strides, channel offsets, k / s / tmode /
convt_co / out_f32 / act, whether the residual aliases the output); each distinct geometry is then launched again on fresh
guard-banded buffers with random operands packed by tests/launch_ref.py and checked against the fp32 reference.  A layout a
future graph change creates is tested without anyone adding a row to test_strided_launch_gpu.py."""
import pytest
import torch

import launch_ref as L
from helpers import synthetic_bscans

pytestmark = pytest.mark.gpu

SHAPE, BATCH = (96, 128), 2


def _allocations(eng):
    """(data_ptr, nbytes, element size) of every device buffer a training launch may point into."""
    out = []

    def add(t):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            out.append((t.data_ptr(), t.numel() * t.element_size(), t.element_size()))
    for t in list(eng.tensors) + [g for g in eng.gtensors if g is not None] + [eng.raw]:
        add(t)
    for sv in eng.saved.values():
        for t in sv.values():
            add(t)
    for op in eng.ops:
        for k, t in op.items():
            if k.startswith("_"):
                add(t)
    return out


def _channel_off(allocs, ptr, ld, esize):
    for base, nbytes, es in allocs:
        if base <= ptr < base + nbytes:
            assert es == esize and (ptr - base) % es == 0
            return ((ptr - base) // es) % ld
    raise AssertionError(f"pointer {ptr:#x} is in none of the engine's buffers")


def _record(scale, monkeypatch, device):
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    from defectdetection_viaobjectdetection_amd.train_engine import TrainEngine
    eng = TrainEngine(scale, 1, SHAPE, BATCH)
    eng.load_state_dict(synthetic_state_dict(scale, 1, seed=3))
    convs, wgrads = [], []
    orig_c, orig_w = TrainEngine._conv_launch, TrainEngine._wgrad_launch

    def conv(self, x_ptr, x_bs, ldx, hi, wi, cin, w, y_ptr, y_bs, ldy, ho, wo, cout, k, stride, pad, bias=None, res_ptr=0, r_bs=0,
             ldr=0, act=0, out_f32=0, convt_co=0, tmode=0):
        convs.append(dict(x_ptr=x_ptr, x_bs=x_bs, ldx=ldx, hi=hi, wi=wi, cin=cin, y_ptr=y_ptr, y_bs=y_bs, ldy=ldy, ho=ho, wo=wo,
                          cout=cout, k=k, stride=stride, pad=pad, bias=bias is not None, res_ptr=res_ptr, r_bs=r_bs, ldr=ldr,
                          act=act, out_f32=out_f32, convt_co=convt_co, tmode=tmode))
        return orig_c(self, x_ptr, x_bs, ldx, hi, wi, cin, w, y_ptr, y_bs, ldy, ho, wo, cout, k, stride, pad, bias, res_ptr, r_bs,
                      ldr, act, out_f32, convt_co, tmode)

    def wgrad(self, dz, lddz, dz_bs, x_ptr, x_bs, ldx, hi, wi, cin, ho, wo, cout, k, stride, pad, dw):
        wgrads.append(dict(dz=dz, lddz=lddz, dz_bs=dz_bs, x_ptr=x_ptr, x_bs=x_bs, ldx=ldx, hi=hi, wi=wi, cin=cin, ho=ho, wo=wo,
                           cout=cout, k=k, stride=stride, pad=pad))
        return orig_w(self, dz, lddz, dz_bs, x_ptr, x_bs, ldx, hi, wi, cin, ho, wo, cout, k, stride, pad, dw)

    monkeypatch.setattr(TrainEngine, "_conv_launch", conv)
    monkeypatch.setattr(TrainEngine, "_wgrad_launch", wgrad)
    imgs = torch.from_numpy(synthetic_bscans(BATCH, SHAPE[0], SHAPE[1], seed=9)).to(device)
    raw, pr = eng.forward(imgs)
    g = torch.Generator().manual_seed(1)
    eng.backward(torch.randn(raw.shape, generator=g).to(device), torch.randn(pr.shape, generator=g).to(device))
    torch.cuda.synchronize()
    allocs = _allocations(eng)
    geoms = {}
    for r in convs:
        es_y = 4 if r["out_f32"] else 2
        dense_x = r["x_bs"] == r["hi"] * r["wi"] * r["ldx"]
        hy, wy = (2 * r["ho"], 2 * r["wo"]) if (r["tmode"] == 2 or r["convt_co"]) else (r["ho"], r["wo"])
        dense_y = r["y_bs"] == hy * wy * r["ldy"]
        if r["res_ptr"] == 0:
            res, ldr, r_off, r_bs = "none", 0, 0, None
        elif r["res_ptr"] == r["y_ptr"]:
            assert r["ldr"] == r["ldy"] and r["r_bs"] == r["y_bs"]
            res, ldr, r_off, r_bs = "inplace", 0, 0, None
        else:
            res, ldr = "own", r["ldr"]
            r_off = _channel_off(allocs, r["res_ptr"], r["ldr"], 2)
            r_bs = None if r["r_bs"] == hy * wy * r["ldr"] else r["r_bs"]
        gm = L.ConvGeom(BATCH, r["hi"], r["wi"], r["cin"], r["ho"], r["wo"], r["cout"], r["k"], r["stride"], r["pad"],
                        tmode=r["tmode"], convt_co=r["convt_co"], out_f32=r["out_f32"], act=r["act"], fwd_cout=0,
                        ldx=r["ldx"], x_off=_channel_off(allocs, r["x_ptr"], r["ldx"], 2), x_bs=None if dense_x else r["x_bs"],
                        ldy=r["ldy"], y_off=_channel_off(allocs, r["y_ptr"], r["ldy"], es_y), y_bs=None if dense_y else r["y_bs"],
                        res=res, ldr=ldr, r_off=r_off, r_bs=r_bs, bias=r["bias"])
        geoms.setdefault(gm.key(), gm)
    wgeoms = {}
    for r in wgrads:
        gm = L.WgradGeom(BATCH, r["hi"], r["wi"], r["cin"], r["ho"], r["wo"], r["cout"], r["k"], r["stride"], r["pad"],
                         ldx=r["ldx"], x_off=_channel_off(allocs, r["x_ptr"], r["ldx"], 2),
                         x_bs=None if r["x_bs"] == r["hi"] * r["wi"] * r["ldx"] else r["x_bs"],
                         lddz=r["lddz"], dz_off=_channel_off(allocs, r["dz"], r["lddz"], 2),
                         dz_bs=None if r["dz_bs"] == r["ho"] * r["wo"] * r["lddz"] else r["dz_bs"])
        wgeoms.setdefault(gm.key(), gm)
    return len(convs), list(geoms.values()), len(wgrads), list(wgeoms.values())


def _describe(g):
    return ", ".join(f"{k}={v}" for k, v in g.__dict__.items() if v not in (0, None, "", "none", False) or k in ("cin", "cout"))


@pytest.mark.parametrize("scale", ["n", "s", "m", "9c"])
def test_replay_training_launch_geometries(scale, cuda_device, monkeypatch):
    from defectdetection_viaobjectdetection_amd import _capi as capi
    nconv, geoms, nwg, wgeoms = _record(scale, monkeypatch, cuda_device)
    monkeypatch.undo()
    assert nconv > 0 and nwg > 0
    kinds = {(g.tmode, g.convt_co > 0, g.out_f32, g.res) for g in geoms}
    assert any(k[3] == "inplace" for k in kinds), "no accumulating input gradient recorded"
    assert any(k[2] for k in kinds), "no out_f32 head conv recorded"
    fails, worst = [], {}
    for i, g in enumerate(geoms):
        r = L.run_conv_geom(capi, g, cuda_device, seed=1000 + i)
        tag = ("tmode%d" % g.tmode if g.tmode else "convt" if g.convt_co else "f32" if g.out_f32 else f"k{g.k}s{g.stride}") + \
              ("+" + g.res if g.res != "none" else "")
        if r["rc"] or r["guard"] or r["rel"] > 1e-3 or r["ratio"] > 1.0:
            fails.append(f"conv {_describe(g)}: {r}")
            continue
        worst[tag] = max(worst.get(tag, 0.0), r["ratio"])
    for i, g in enumerate(wgeoms):
        r = L.run_wgrad_geom(capi, g, cuda_device, seed=2000 + i)
        tag = f"wgrad k{g.k}s{g.stride}"
        if r["rc"] or r["guard"] or r["rel"] > 1e-3 or r["ratio"] > 1.0 or not r["bitwise"]:
            fails.append(f"wgrad {_describe(g)}: {r}")
            continue
        worst[tag] = max(worst.get(tag, 0.0), r["ratio"])
    print(f"\n{scale}: {nconv} conv launches -> {len(geoms)} distinct geometries, {nwg} wgrad launches -> {len(wgeoms)} distinct; "
          "worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not fails, "\n".join(fails[:20])
