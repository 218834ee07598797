"""YOLOv5u detection on the HIP engine (/root/reference/BscanBased/yolo5s_retrain.py:6, yolo/yolo_eval.py) against
its CPU reference (tests/yolov5u_det_ref.py) with calibrated synthetic weights: raw head maps by rel-L2, decoded boxes and
scores by percentiles (the bounds of test_v9c_gpu.py), NMS rows bit-exact on the engine's own predictions, batch invariance,
and the yolo_eval.py call shape end to end (boxes, no masks, plot)."""
import os

import numpy as np
import pytest
import torch

import yolov5u_det_ref as ref
from helpers import synthetic_bscans

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("scale", ["5n", "5s", "5m"])
@pytest.mark.parametrize("nc,shape,batch", [(1, (320, 320), 3), (1, (640, 640), 2), (3, (256, 384), 1)])
def test_v5u_forward_and_nms_parity(scale, nc, shape, batch, cuda_device):
    from defectdetection_viaobjectdetection_amd.engine import SegEngine
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    sd = synthetic_state_dict(scale, nc, seed=2, cls_bias=-2.5)
    eng = SegEngine(scale, nc, shape, max_batch=batch)
    assert eng.nm == 0 and eng.pred_width == 4 + nc and eng.proto_hw == (0, 0)
    eng.load_state_dict(sd)
    model = ref.DetectionModelV5u(scale, nc)
    model.load_state_dict(sd)
    model.eval()
    imgs = synthetic_bscans(batch, shape[0], shape[1], seed=5)
    x = torch.from_numpy(imgs.transpose(0, 3, 1, 2).copy()).float() / 255.0
    with torch.no_grad():
        raw_l = model.forward_raw(x)
        o_preds = model(x)
    preds, protos = eng.forward(torch.from_numpy(imgs).to(cuda_device))
    assert protos is None
    raw = eng.raw_head(batch).cpu()
    torch.cuda.synchronize()
    A = o_preds.shape[2]
    assert preds.shape == (batch, A, 4 + nc) and raw.shape == (batch, A, 64 + nc) and torch.isfinite(preds).all()
    o_raw = torch.cat([r.view(batch, 64 + nc, -1) for r in raw_l], 2).permute(0, 2, 1)
    e_box, e_cls = rel_l2(raw[..., :64], o_raw[..., :64]), rel_l2(raw[..., 64:], o_raw[..., 64:])
    gp, op = preds.cpu(), o_preds.permute(0, 2, 1)
    dbox = (gp[..., :4] - op[..., :4]).abs().flatten()
    dsc = (gp[..., 4:] - op[..., 4:]).abs().flatten()
    q = lambda t, f: float(t.kthvalue(max(1, int(t.numel() * f)))[0])  # noqa: E731
    print(f"v5u {scale} nc={nc} {shape} b={batch}: raw box {e_box:.2e} cls {e_cls:.2e} | box px median {q(dbox, .5):.4f} "
          f"p99 {q(dbox, .99):.3f} max {float(dbox.max()):.3f} | score p99 {q(dsc, .99):.2e} max {float(dsc.max()):.2e}")
    assert e_box <= 1e-2 and e_cls <= 2e-2
    assert q(dbox, .5) <= 0.05 and q(dbox, .99) <= 0.5 and q(dsc, .99) <= 3e-3
    for conf, iou, max_det in ((0.25, 0.7, 300), (0.05, 0.5, 20)):
        dets, counts, masks = eng.postprocess(preds, None, conf, iou, max_det)
        torch.cuda.synchronize()
        assert masks is None and dets.shape == (batch, max_det, 6)
        want = ref.non_max_suppression(preds.cpu().permute(0, 2, 1).numpy(), nc, conf, iou, max_det)
        for b in range(batch):
            n = int(counts[b])
            assert n == want[b].shape[0] and np.array_equal(dets[b, :n].cpu().numpy(), want[b])
    eng.close()


@pytest.mark.parametrize("shape,batch", [((64, 64), 12), ((64, 640), 2)])   # the smallest net shape of the family and a thin one: maps of 8 x 80 .. 2 x 20 and 2 x 2
def test_v5u_narrow_net_shapes(shape, batch, cuda_device):
    test_v5u_forward_and_nms_parity("5s", 1, shape, batch, cuda_device)


def test_v5u_batch_invariance(cuda_device):
    """An image's predictions are bit-identical alone and at position 2 of a batch of 4."""
    from defectdetection_viaobjectdetection_amd.engine import SegEngine
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    eng = SegEngine("5s", 1, (640, 640), max_batch=4, keep_raw=False)
    eng.load_state_dict(synthetic_state_dict("5s", 1, seed=2, cls_bias=-2.5))
    imgs = torch.from_numpy(synthetic_bscans(4, 640, 640, seed=9)).to(cuda_device)
    p4, _ = eng.forward(imgs)
    p1, _ = eng.forward(imgs[2:3].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(p4[2], p1[0])
    eng.close()


def test_yolo_eval_call_shape_with_a_v5u_model(tmp_path, cuda_device):
    """yolo/yolo_eval.py: YOLO(best.pt) -> predict(png) -> res.boxes.xyxy / conf / cls, res.plot()."""
    from ultralytics import YOLO
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    m = YOLO("yolov5su.yaml")
    m.set_classes(1, {0: "defect"})
    m.load_state_dict(synthetic_state_dict("5s", 1, seed=2, cls_bias=-2.5))
    path = m.save(str(tmp_path / "train" / "weights" / "best.pt"))
    model = YOLO(path)
    assert model.task == "detect" and model.scale == "5s"
    png = os.path.join(GOLDEN, "bscans", "787-225_01_Ch-0_51.png")
    res = model.predict(png, save=True, project=str(tmp_path / "runs"), name="predict", verbose=False)[0]
    assert res.masks is None and res.boxes.data.shape[1] == 6
    assert res.boxes.xyxy.shape[1] == 4 and res.boxes.conf.shape == res.boxes.cls.shape
    img = res.plot()
    assert isinstance(img, np.ndarray) and img.shape[:2] == res.orig_shape and img.dtype == np.uint8
    assert isinstance(res.verbose(), str) and os.listdir(str(tmp_path / "runs" / "predict"))
