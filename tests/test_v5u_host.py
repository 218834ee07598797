"""YOLOv5u detection (/root/reference/BscanBased/yolo5s_retrain.py:6 loads yolov5su.pt) on the host: the spec
and the CPU reference pinned by the published parameter counts and GFLOPs, upstream's state-dict layout, the YOLO facade
(yaml, offline .pt names, save / load, no training yet), upstream-style checkpoints, and the stem entry's argument checks
(decided before any HIP call, so they run without a GPU).  CPU only."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import yolov5u_det_ref as ref
from defectdetection_viaobjectdetection_amd.model import YOLO, OfflineModelError
from defectdetection_viaobjectdetection_amd.spec import (conv_specs, count_parameters, init_state_dict, state_dict_keys,
                                                         synthetic_state_dict)
from defectdetection_viaobjectdetection_amd.upstream_ckpt import load_upstream_checkpoint

SCALES = ("5n", "5s", "5m")
C0 = {"5n": 16, "5s": 32, "5m": 48}


@pytest.mark.parametrize("scale", SCALES)
def test_parameter_counts_and_gflops_pin_the_graph(scale):
    m80 = ref.DetectionModelV5u(scale, 80)
    assert ref.count_parameters(m80) == ref.PARAMS_NC80[scale]
    assert count_parameters(init_state_dict(scale, 80)) == ref.PARAMS_NC80[scale]
    m1 = ref.DetectionModelV5u(scale, 1)
    assert count_parameters(init_state_dict(scale, 1)) == ref.count_parameters(m1)
    assert round(2 * ref.conv_macs_per_image(scale, 80) / 1e9, 1) == ref.GFLOPS_640[scale]


@pytest.mark.parametrize("scale", SCALES)
def test_state_dict_keys_follow_upstream_layout(scale):
    keys = state_dict_keys(scale, 1)
    assert keys == list(ref.DetectionModelV5u(scale, 1).state_dict().keys())
    for k in ("model.0.conv.weight", "model.2.cv3.conv.weight", "model.2.m.0.cv2.conv.weight", "model.9.cv2.conv.weight",
              "model.24.cv3.0.2.weight", "model.24.cv2.2.2.bias", "model.24.dfl.conv.weight"):
        assert k in keys, k
    assert not any(k.startswith("model.22.") or ".cv4." in k or "proto" in k for k in keys)
    sd = synthetic_state_dict(scale, 1, seed=0)
    assert tuple(sd["model.0.conv.weight"].shape) == (C0[scale], 3, 6, 6)
    assert [s.k for s in conv_specs(scale, 1)].count(6) == 1 and conv_specs(scale, 1)[0].k == 6
    ref.DetectionModelV5u(scale, 1).load_state_dict(sd, strict=True)


def test_synthetic_gains_keep_activations_alive():
    """Calibrated gains (data/synth_gains_5s.json): the raw head maps neither saturate nor vanish, so parity compares signal."""
    sd = synthetic_state_dict("5s", 1, seed=2, cls_bias=-2.5)
    model = ref.DetectionModelV5u("5s", 1)
    model.load_state_dict(sd)
    model.eval()
    from helpers import synthetic_bscans
    imgs = synthetic_bscans(1, 320, 320, seed=5)
    x = torch.from_numpy(imgs.transpose(0, 3, 1, 2).copy()).float() / 255.0
    with torch.no_grad():
        raw = model.forward_raw(x)
        preds = model(x)
    for r in raw:
        assert 0.3 < float(r[:, :64].std()) < 20.0
    sc = preds[:, 4]
    assert 0 < int((sc > 0.25).sum()) < sc.numel()


def test_yolo_facade_builds_saves_and_refuses_training(tmp_path):
    m = YOLO("yolov5su.yaml")
    assert m.task == "detect" and m.scale == "5s" and m.nc == 80
    y = tmp_path / "yolov5nu.yaml"
    y.write_text("nc: 3\n")
    m3 = YOLO(str(y))
    assert m3.scale == "5n" and m3.nc == 3 and m3.task == "detect"
    assert m3.info()[1] == count_parameters(init_state_dict("5n", 3))
    with pytest.raises(OfflineModelError):
        YOLO("yolov5su.pt")
    with pytest.raises(NotImplementedError, match="YOLOv5u scales l and x"):
        YOLO("yolov5lu.yaml")
    with pytest.raises(NotImplementedError):
        YOLO("yolo11n-seg.yaml")
    with pytest.raises(NotImplementedError, match="detect training"):
        m3.train(data="data.yaml", epochs=1)
    with pytest.raises(NotImplementedError, match="detect training"):
        m3.val(data="data.yaml")
    m3.load_state_dict(synthetic_state_dict("5n", 3, seed=1))
    p = m3.save(str(tmp_path / "w" / "best.pt"))
    back = YOLO(p)
    assert back.scale == "5n" and back.nc == 3 and back.task == "detect"
    assert back.state_dict.keys() == m3.state_dict.keys()
    assert all(torch.equal(back.state_dict[k], m3.state_dict[k]) for k in m3.state_dict)


FAKE = {"Conv": "ultralytics.nn.modules.conv", "Bottleneck": "ultralytics.nn.modules.block", "C3": "ultralytics.nn.modules.block",
        "SPPF": "ultralytics.nn.modules.block", "DFL": "ultralytics.nn.modules.block", "Detect": "ultralytics.nn.modules.head",
        "DetectionModelV5u": "ultralytics.nn.tasks", "Stem6": "ultralytics.nn.modules.conv"}


def _owner(cls_name):
    import yolov8_seg_oracle as orc
    return ref if hasattr(ref, cls_name) and getattr(ref, cls_name).__module__ == ref.__name__ else orc


@pytest.mark.parametrize("scale,nc", [("5n", 1), ("5s", 3), ("5m", 2)])
def test_upstream_style_v5u_checkpoint_loads(tmp_path, scale, nc):
    """An upstream DetectionModel pickle whose classes are not importable (the stand-ins are pickled under upstream's module
    paths, which are then removed): recognised by its tensors, mapped to the right scale and nc."""
    sd = synthetic_state_dict(scale, nc, seed=4)
    model = ref.DetectionModelV5u(scale, nc)
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
    sd = {"model.0.conv.weight": torch.zeros(16, 3, 6, 6), "model.2.cv3.conv.weight": torch.zeros(32, 32, 1, 1)}
    torch.save({"model": sd, "train_args": {}}, p)     # a 6x6 stem without the Detect head at model.24
    with pytest.raises(ValueError, match="not a YOLOv8-seg graph"):
        load_upstream_checkpoint(p)


def test_stem6_entry_rejects_bad_arguments_without_a_gpu():
    """m355_stem6_fwd validates every argument on the host before any HIP call: -1 (M355_ERR_INVALID), a fake device pointer
    that is never dereferenced."""
    from defectdetection_viaobjectdetection_amd import _capi
    w = np.zeros((48, 3, 6, 6), np.float32)
    b = np.zeros(48, np.float32)
    wp, bp = w.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0x1000)
    f = _capi.lib.m355_stem6_fwd
    for c0 in (0, 8, 24, 64, 80):
        assert f(fake, 1, 64, 64, wp, bp, c0, fake, None) == -1, c0
        assert b"C0" in _capi.lib.m355_last_error(None)
    for (bb, h, wd) in ((1, 63, 64), (1, 64, 63), (1, 0, 64), (1, 64, 0), (1, -64, 64), (0, 64, 64), (1, 64, 40)):
        assert f(fake, bb, h, wd, wp, bp, 32, fake, None) == -1, (bb, h, wd)
    assert f(None, 1, 64, 64, wp, bp, 32, fake, None) == -1
    assert f(fake, 1, 64, 64, None, bp, 32, fake, None) == -1
    assert f(fake, 1, 64, 64, wp, None, 32, fake, None) == -1
    assert f(fake, 1, 64, 64, wp, bp, 32, None, None) == -1
