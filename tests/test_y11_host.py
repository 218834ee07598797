"""YOLO11 detection (BscanBased/yolo/yolo_bbox_retrain.py trains yolo11n, yolo/yolo_eval.py predicts with it)
on the host: the spec and the CPU reference pinned by the published parameter counts and GFLOPs, upstream's state-dict
layout, the YOLO facade (yaml, save / load, no training), upstream-style checkpoints, and the argument checks of the two new
entries and of m355_create's family / scale code (decided before any HIP call, so they run without a GPU).  CPU only."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import yolo11_det_ref as ref
from defectdetection_viaobjectdetection_amd import _capi
from defectdetection_viaobjectdetection_amd.model import YOLO
from defectdetection_viaobjectdetection_amd.spec import (conv_specs, count_parameters, fold_bn, init_state_dict, state_dict_keys,
                                                         synthetic_state_dict, y11_gflops)
from defectdetection_viaobjectdetection_amd.upstream_ckpt import load_upstream_checkpoint

SCALES = ("11n", "11s", "11m")
C0 = {"11n": 16, "11s": 32, "11m": 64}


@pytest.mark.parametrize("scale", SCALES)
def test_parameter_counts_and_gflops_pin_the_graph(scale):
    m80 = ref.DetectionModelY11(scale, 80)
    assert ref.count_parameters(m80) == ref.PARAMS_NC80[scale]
    assert count_parameters(init_state_dict(scale, 80)) == ref.PARAMS_NC80[scale]
    assert count_parameters(init_state_dict(scale, 1)) == ref.count_parameters(ref.DetectionModelY11(scale, 1))
    assert round(ref.upstream_gflops(scale, 80), 1) == ref.GFLOPS_640[scale]
    assert round(y11_gflops(scale, 80), 1) == ref.GFLOPS_640[scale]
    assert abs(y11_gflops(scale, 80) - ref.upstream_gflops(scale, 80)) < 1e-9


@pytest.mark.parametrize("scale", SCALES)
def test_state_dict_keys_and_shapes_follow_upstream_layout(scale):
    model = ref.DetectionModelY11(scale, 1)
    want = model.state_dict()
    keys = state_dict_keys(scale, 1)
    assert keys == list(want.keys())
    sd = init_state_dict(scale, 1)
    assert [tuple(sd[k].shape) for k in keys] == [tuple(want[k].shape) for k in keys]
    for k in ("model.10.m.0.attn.qkv.conv.weight", "model.10.m.0.attn.pe.conv.weight", "model.10.m.0.ffn.1.bn.bias",
              "model.23.cv3.0.0.0.conv.weight", "model.23.cv3.2.1.1.conv.weight", "model.23.cv3.1.2.weight",
              "model.23.dfl.conv.weight"):
        assert k in keys, k
    assert not any(k.startswith("model.24.") or ".cv4." in k or "proto" in k for k in keys)
    assert tuple(sd["model.0.conv.weight"].shape) == (C0[scale], 3, 3, 3)
    c = {"11n": 128, "11s": 256, "11m": 256}[scale]     # C2PSA width c1 / 2: 2 heads at n, 4 at s and m
    assert tuple(sd["model.10.m.0.attn.pe.conv.weight"].shape) == (c, 1, 3, 3)
    # m scale: every C3k2 uses C3k; n / s: only model.6, .8 and .22 do
    c3k = sorted({s.name.split(".")[1] for s in conv_specs(scale, 1) if ".m.0.m.1." in s.name})
    assert c3k == (["13", "16", "19", "2", "22", "4", "6", "8"] if scale == "11m" else ["22", "6", "8"])
    specs = {s.name: s for s in conv_specs(scale, 1)}
    assert not specs["model.10.m.0.attn.qkv"].act and not specs["model.10.m.0.attn.proj"].act
    assert not specs["model.10.m.0.ffn.1"].act and specs["model.10.m.0.ffn.0"].act
    assert specs["model.10.m.0.attn.pe"].groups == c and specs["model.23.cv3.0.0.0"].groups == specs["model.23.cv3.0.0.0"].cin
    model.load_state_dict(synthetic_state_dict(scale, 1, seed=0), strict=True)


def test_fold_bn_of_a_depthwise_conv_equals_conv_bn_eval():
    sd = synthetic_state_dict("11n", 1, seed=3)
    spec = next(s for s in conv_specs("11n", 1) if s.name == "model.23.cv3.1.0.0")
    w, b = fold_bn(sd, spec)
    assert tuple(w.shape) == (spec.cout, 1, 3, 3)
    m = ref.ConvGA(spec.cin, spec.cout, 3, 1, spec.groups, act=False).eval()
    m.load_state_dict({k[len(spec.name) + 1:]: v for k, v in sd.items() if k.startswith(spec.name + ".")})
    x = torch.randn(2, spec.cin, 7, 9)
    with torch.no_grad():
        want = m(x)
    got = torch.nn.functional.conv2d(x, w, b, padding=1, groups=spec.groups)
    assert float((got - want).abs().max()) < 1e-4


@pytest.mark.parametrize("scale", SCALES)
def test_synthetic_gains_keep_activations_alive(scale):
    """Calibrated gains (data/synth_gains_11{n,s,m}.json, measured on the seed-0 weights): the raw head maps neither saturate
    nor vanish, so parity compares signal.  (The narrow n / s layers make the gains seed-specific: the GPU tests use seed 0.)"""
    sd = synthetic_state_dict(scale, 1, seed=0, cls_bias=-2.5)
    model = ref.DetectionModelY11(scale, 1)
    model.load_state_dict(sd)
    model.eval()
    from helpers import synthetic_bscans
    imgs = synthetic_bscans(1, 320, 320, seed=5)
    x = torch.from_numpy(imgs.transpose(0, 3, 1, 2).copy()).float() / 255.0
    with torch.no_grad():
        raw = model.forward_raw(x)
        preds = model(x)
    for r in raw:
        assert 0.3 < float(r[:, :64].std()) < 20.0 and 0.3 < float(r[:, 64:].std()) < 20.0
    sc = preds[:, 4]
    assert 0 < int((sc > 0.25).sum()) < sc.numel()


def test_yolo_facade_builds_saves_and_refuses_training(tmp_path):
    m = YOLO("yolo11s.yaml")
    assert m.task == "detect" and m.scale == "11s" and m.nc == 80 and m.info()[1] == ref.PARAMS_NC80["11s"]
    y = tmp_path / "yolo11n.yaml"
    y.write_text("nc: 3\n")
    m3 = YOLO(str(y))
    assert m3.scale == "11n" and m3.nc == 3 and m3.task == "detect"
    assert m3.info()[1] == count_parameters(init_state_dict("11n", 3))
    for bad in ("yolo11n-seg.yaml", "yolo11l.yaml", "yolo11x.yaml"):
        with pytest.raises(NotImplementedError):
            YOLO(bad)
    with pytest.raises(NotImplementedError, match="detect training"):
        m3.train(data="data.yaml", epochs=1)
    with pytest.raises(NotImplementedError, match="detect training"):
        m3.val(data="data.yaml")
    m3.load_state_dict(synthetic_state_dict("11n", 3, seed=1))
    p = m3.save(str(tmp_path / "w" / "best.pt"))
    back = YOLO(p)
    assert back.scale == "11n" and back.nc == 3 and back.task == "detect"
    assert back.state_dict.keys() == m3.state_dict.keys()
    assert all(torch.equal(back.state_dict[k], m3.state_dict[k]) for k in m3.state_dict)
    with pytest.raises(NotImplementedError, match="upstream export"):
        m3.save(str(tmp_path / "up.pt"), upstream=True)


FAKE = {"Conv": "ultralytics.nn.modules.conv", "ConvGA": "ultralytics.nn.modules.conv", "Bottleneck": "ultralytics.nn.modules.block",
        "C3k": "ultralytics.nn.modules.block", "C3k2": "ultralytics.nn.modules.block", "SPPF": "ultralytics.nn.modules.block",
        "Attention": "ultralytics.nn.modules.block", "PSABlock": "ultralytics.nn.modules.block", "C2PSA": "ultralytics.nn.modules.block",
        "DFL": "ultralytics.nn.modules.block", "Detect": "ultralytics.nn.modules.head", "DetectionModelY11": "ultralytics.nn.tasks"}


def _owner(cls_name):
    import yolov8_seg_oracle as orc
    return ref if hasattr(ref, cls_name) and getattr(ref, cls_name).__module__ == ref.__name__ else orc


@pytest.mark.parametrize("scale,nc", [("11n", 1), ("11s", 3), ("11m", 2)])
def test_upstream_style_y11_checkpoint_loads(tmp_path, scale, nc):
    """An upstream DetectionModel pickle whose classes are not importable (the stand-ins are pickled under upstream's module
    paths, which are then removed): recognised by its tensors, mapped to the right scale and nc."""
    sd = synthetic_state_dict(scale, nc, seed=4)
    model = ref.DetectionModelY11(scale, nc)
    model.load_state_dict(sd)
    model.names = {i: f"defect{i}" for i in range(nc)}
    saved, created = {}, []
    path = str(tmp_path / "best.pt")
    try:
        for cls_name, mod_name in FAKE.items():
            cls = getattr(_owner(cls_name), cls_name)
            saved[cls] = cls.__module__
            parts = mod_name.split(".")
            for i in range(1, len(parts) + 1):
                mn = ".".join(parts[:i])
                if mn not in sys.modules:
                    sys.modules[mn] = types.ModuleType(mn)
                    created.append(mn)
            setattr(sys.modules[mod_name], cls_name, cls)
            cls.__module__ = mod_name
        torch.save({"epoch": 9, "model": model.half(), "ema": None, "train_args": {"imgsz": 320, "data": "data.yaml"}}, path)
    finally:
        for cls, mn in saved.items():
            cls.__module__ = mn
        for mn in created:
            sys.modules.pop(mn, None)
    up = load_upstream_checkpoint(path)
    assert up["scale"] == scale and up["nc"] == nc and up["names"] == {i: f"defect{i}" for i in range(nc)}
    for k, v in sd.items():
        got = up["state_dict"][k]
        assert torch.equal(got.float(), v.half().float()) if v.is_floating_point() else torch.equal(got, v), k
    m = YOLO(path)
    assert m.scale == scale and m.nc == nc and m.task == "detect" and m.train_args["imgsz"] == 320


def test_other_graphs_are_still_rejected(tmp_path):
    p = str(tmp_path / "other.pt")
    sd = {"model.0.conv.weight": torch.zeros(16, 3, 3, 3), "model.10.m.0.attn.qkv.conv.weight": torch.zeros(256, 128, 1, 1),
          "model.23.cv3.0.2.weight": torch.zeros(1, 64, 1, 1), "model.23.proto.cv1.conv.weight": torch.zeros(64, 64, 3, 3)}
    torch.save({"model": sd, "train_args": {}}, p)     # a yolo11-seg layout: not built
    with pytest.raises(ValueError, match="not a YOLOv8-seg graph"):
        load_upstream_checkpoint(p)
    sd = {"model.0.conv.weight": torch.zeros(80, 3, 3, 3), "model.10.m.0.attn.qkv.conv.weight": torch.zeros(512, 256, 1, 1),
          "model.23.cv3.0.2.weight": torch.zeros(1, 64, 1, 1)}
    torch.save({"model": sd, "train_args": {}}, p)     # yolo11x's stem width
    with pytest.raises(ValueError, match="only the n, s and m scales"):
        load_upstream_checkpoint(p)


def test_dwconv_entry_rejects_bad_arguments_without_a_gpu():
    """m355_dwconv3x3_fwd validates every argument on the host before any HIP call: -1 (M355_ERR_INVALID); the fake device
    pointers are never dereferenced."""
    w = np.zeros((64, 1, 3, 3), np.float32)
    b = np.zeros(64, np.float32)
    wp, bp = w.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0x1000)
    f = _capi.lib.m355_dwconv3x3_fwd
    for c in (0, 4, 12, 63, -8):
        assert f(fake, 1, 8, 8, c, 64, wp, bp, 1, fake, 64, None) == -1, c
        assert b"C must be" in _capi.lib.m355_last_error(None)
    for ldx, ldy in ((32, 64), (64, 32), (68, 64), (64, 72 + 4)):
        assert f(fake, 1, 8, 8, 64, ldx, wp, bp, 1, fake, ldy, None) == -1, (ldx, ldy)
    for (bb, h, wd) in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, 8)):
        assert f(fake, bb, h, wd, 64, 64, wp, bp, 0, fake, 64, None) == -1, (bb, h, wd)
    assert f(fake, 1, 8, 8, 64, 64, wp, bp, 2, fake, 64, None) == -1
    assert f(ctypes.c_void_p(0x1008), 1, 8, 8, 64, 64, wp, bp, 1, fake, 64, None) == -1        # not 16-byte aligned
    assert f(fake, 1, 8, 8, 64, 64, wp, bp, 1, ctypes.c_void_p(0x1004), 64, None) == -1
    assert f(None, 1, 8, 8, 64, 64, wp, bp, 1, fake, 64, None) == -1
    assert f(fake, 1, 8, 8, 64, 64, None, bp, 1, fake, 64, None) == -1
    assert f(fake, 1, 8, 8, 64, 64, wp, None, 1, fake, 64, None) == -1
    assert f(fake, 1, 8, 8, 64, 64, wp, bp, 1, None, 64, None) == -1


def test_psa_attn_entry_rejects_bad_arguments_without_a_gpu():
    w = np.zeros((256, 1, 3, 3), np.float32)
    b = np.zeros(256, np.float32)
    wp, bp = w.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0x1000)
    f = _capi.lib.m355_psa_attn_fwd
    for kd, hd in ((16, 64), (64, 64), (32, 32), (32, 128), (0, 0)):
        assert f(fake, 1, 20, 20, 4, kd, hd, wp, bp, fake, None) == -1, (kd, hd)
        assert b"key_dim must be 32" in _capi.lib.m355_last_error(None)
    for heads in (0, -1, 65):
        assert f(fake, 1, 20, 20, heads, 32, 64, wp, bp, fake, None) == -1, heads
    for (bb, h, wd) in ((0, 20, 20), (65536, 20, 20), (1, 0, 20), (1, 20, 0), (1, 8192, 4096)):
        assert f(fake, bb, h, wd, 4, 32, 64, wp, bp, fake, None) == -1, (bb, h, wd)
    assert f(ctypes.c_void_p(0x1008), 1, 20, 20, 4, 32, 64, wp, bp, fake, None) == -1
    assert f(fake, 1, 20, 20, 4, 32, 64, wp, bp, ctypes.c_void_p(0x1002), None) == -1
    assert f(None, 1, 20, 20, 4, 32, 64, wp, bp, fake, None) == -1
    assert f(fake, 1, 20, 20, 4, 32, 64, None, bp, fake, None) == -1
    assert f(fake, 1, 20, 20, 4, 32, 64, wp, None, fake, None) == -1
    assert f(fake, 1, 20, 20, 4, 32, 64, wp, bp, None, None) == -1


@pytest.mark.parametrize("code", [(ord("1") << 8) | ord("l"), (ord("1") << 8) | ord("x"), (ord("1") << 8) | ord("c"),
                                  (ord("5") << 8) | ord("x"), (ord("2") << 8) | ord("n"), (0x7f << 8) | ord("s"), ord("q")])
def test_create_refuses_bad_family_or_scale_without_a_gpu(code):
    desc = _capi.ModelDesc(code, 1, 640, 640, 1)
    h = ctypes.c_void_p()
    assert _capi.lib.m355_create(ctypes.byref(desc), ctypes.byref(h)) == -1 and not h.value
    assert b"unknown family or scale" in _capi.lib.m355_last_error(None)


def test_conv_info_carries_groups_as_its_last_field():
    names = [f[0] for f in _capi.ConvInfo._fields_]
    assert names[-1] == "groups" and names[-2] == "act"
    assert ctypes.sizeof(_capi.ConvInfo) == 64 + 8 * 4
