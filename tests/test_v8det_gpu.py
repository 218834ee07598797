"""YOLOv8 detection models on the GPU: predict parity against the CPU reference (tests/yolov8_det_ref.py) under the rules of
tests/test_v5u_gpu.py, TrainEngine's detect form under the rule of tests/test_train_engine_gpu.py, the class-BCE kernel against
float64, ``DetCriterion`` on the device against the float64 reference loss, the train / val / resume API on a box-label dataset
and the detect validator against the oracle's matcher.  Reference: signals/improved_multisignal/visualization/yolo_detector.py:20
(``YOLO('yolov8n.pt')``) and the box-label training scripts (BscanBased/yolo/yolo_bbox_retrain.py)."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import yolov8_det_ref as ref
import yolov8_seg_train_oracle as tro
from helpers import synthetic_bscans
from keepset import _xyxy, common_order_ok, compare_keepsets
from test_loss_host import _case
from test_v8det_host import check_against_reference

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


# ---------------------------------------------------------------------------------------------------- 1. forward / predict parity
def _anchors_of_boxes(dets, preds, nc):
    """Anchor of every NMS row of a box-only model (tests/keepset.py identifies rows by their mask coefficients, which a detection
    row has not): the anchor whose best class and score are the row's, bit for bit; among several, the nearest box."""
    score, cls = preds[:, 4:4 + nc].max(1), preds[:, 4:4 + nc].argmax(1)
    box = _xyxy(preds)
    out = []
    for r in dets:
        cand = np.nonzero((score == r[4]) & (cls == int(r[5])))[0]
        assert cand.size, r
        out.append(int(cand[np.abs(box[cand] - r[:4]).sum(1).argmin()]))
    return out


@pytest.mark.parametrize("scale,shape,batch,nc", [("8n", (64, 96), 2, 3), ("8s", (96, 96), 3, 1), ("8m", (64, 64), 1, 80),
                                                  ("8n", (32, 32), 1, 1)])   # the last: level maps 4x4, 2x2, 1x1 under the detect head
def test_v8det_forward_and_nms_parity(scale, shape, batch, nc, cuda_device):
    from defectdetection_viaobjectdetection_amd.engine import SegEngine
    from defectdetection_viaobjectdetection_amd.spec import conv_specs_v8det, synthetic_state_dict
    # seed 0: the weights the calibrated gains (data/synth_gains_{n,s,m}.json, shared with the seg graph) were measured on; at the n
    # scale other seeds let the activations decay to a head that outputs its biases, which any engine reproduces
    sd = synthetic_state_dict(scale, nc, seed=0, cls_bias=-2.5)
    eng = SegEngine(scale, nc, shape, max_batch=batch)
    assert eng.nm == 0 and eng.pred_width == 4 + nc and eng.proto_hw == (0, 0)
    # m355_get_conv_info order = conv_specs_v8det order
    got = [(ci.name.decode(), ci.cin, ci.cout, ci.k, ci.stride, bool(ci.has_bn)) for ci in eng.conv_infos()]
    assert got == [(s.name, s.cin, s.cout, s.k, s.stride, s.has_bn) for s in conv_specs_v8det(scale, nc)]
    eng.load_state_dict(sd)
    model = ref.DetectionModelV8(scale, nc)
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
    assert A == sum((shape[0] // s) * (shape[1] // s) for s in (8, 16, 32))
    assert preds.shape == (batch, A, 4 + nc) and raw.shape == (batch, A, 64 + nc) and torch.isfinite(preds).all()
    o_raw = torch.cat([r.view(batch, 64 + nc, -1) for r in raw_l], 2).permute(0, 2, 1)
    e_box, e_cls = rel_l2(raw[..., :64], o_raw[..., :64]), rel_l2(raw[..., 64:], o_raw[..., 64:])
    gp, op = preds.cpu(), o_preds.permute(0, 2, 1)
    dbox = (gp[..., :4] - op[..., :4]).abs().flatten()
    dsc = (gp[..., 4:] - op[..., 4:]).abs().flatten()
    q = lambda t, f: float(t.kthvalue(max(1, int(t.numel() * f)))[0])  # noqa: E731
    print(f"v8det {scale} nc={nc} {shape} b={batch}: raw box {e_box:.2e} cls {e_cls:.2e} | box px median {q(dbox, .5):.4f} "
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
    # end to end against the reference's own predictions + NMS: the keep-set margin rule (tests/keepset.py, SURVEY 8d's margins)
    conf, iou, m_conf, m_iou = 0.25, 0.7, 2e-3, 1e-3
    dets, counts, _ = eng.postprocess(preds, None, conf, iou, 300)
    torch.cuda.synchronize()
    want = ref.non_max_suppression(o_preds.numpy(), nc, conf, iou, 300)
    n_exc = n_det = 0
    for b in range(batch):
        g_p, o_p = gp[b].numpy(), op[b].contiguous().numpy()
        kg = _anchors_of_boxes(dets[b, :int(counts[b])].cpu().numpy(), g_p, nc)
        kr = _anchors_of_boxes(want[b], o_p, nc)
        exc, bad = compare_keepsets(kg, g_p, kr, o_p, conf, iou, m_conf, m_iou, nc=nc)
        for side, a, why in exc:
            print(f"  excepted: image {b} anchor {a} kept by {'HIP' if side == 'a' else 'reference'} only, rule '{why}'")
        assert not bad, (b, bad)
        assert common_order_ok(kg, kr, o_p[:, 4:4 + nc].max(1), m_conf)
        n_exc, n_det = n_exc + len(exc), n_det + len(kr)
    print(f"  keep-set: {n_det} reference detections, {n_exc} excepted")
    eng.close()


def test_predict_of_a_saved_v8_detect_model(tmp_path, cuda_device):
    from ultralytics import YOLO
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    m = YOLO("yolov8n.yaml")
    m.set_classes(1, {0: "defect"})
    m.load_state_dict(synthetic_state_dict("8n", 1, seed=2, cls_bias=-2.5))
    model = YOLO(m.save(str(tmp_path / "train" / "weights" / "best.pt")))
    assert model.task == "detect" and model.scale == "8n"
    img = synthetic_bscans(1, 96, 128, seed=3)[0][:, :, ::-1].copy()
    res = model.predict(img, imgsz=128, save=True, project=str(tmp_path / "runs"), name="predict", verbose=False)[0]
    assert res.masks is None and res.boxes.data.shape[1] == 6 and res.boxes.conf.shape == res.boxes.cls.shape
    assert os.listdir(str(tmp_path / "runs" / "predict"))          # runs/<task>/predict when project is absent: model.task = detect


# ---------------------------------------------------------------------------------------------------- 2. train forward / backward
def _emulate_fp16_storage(oracle):
    """As tests/test_train_engine_gpu.py: conv and block outputs (and, through the same casts, their gradients) rounded to fp16."""
    import torch.nn as nn
    import yolov8_seg_oracle as orc

    def rnd(mod, inp, out):
        return out.half().float()
    for m in oracle.modules():
        if isinstance(m, (nn.Conv2d, orc.Conv)) and m is not oracle.model[22].dfl.conv:
            m.register_forward_hook(rnd)


def _ref_grads(scale, nc, sd, x, R1, batch, emulate):
    model = ref.DetectionModelV8(scale, nc)
    model.load_state_dict(sd)
    model.train()
    if emulate:
        _emulate_fp16_storage(model)
    raw_l = model.forward_raw(x)
    o_raw = torch.cat([r.view(batch, 64 + nc, -1) for r in raw_l], 2).permute(0, 2, 1)          # (B, A, 64 + nc)
    (o_raw * R1).sum().backward()
    return model, o_raw.detach(), {k: v.grad for k, v in model.named_parameters()}


@pytest.mark.parametrize("scale,shape,batch,nc", [("8n", (64, 96), 2, 3), ("8s", (96, 96), 3, 1), ("8n", (64, 96), 2, 80)])
def test_v8det_train_forward_backward_parity(scale, shape, batch, nc, cuda_device):
    """The procedure and the acceptance rule of tests/test_train_engine_gpu.py::test_train_forward_backward_parity on the detect
    reference with loss (raw * R1).sum(): the HIP path against fp32 autograd, held to the format floor (the fp16-storage-emulating
    reference against the fp32 one): medians x 1.5, per tensor x 2.5, the cosine rule.  nc = 80 gives the class branch its one
    width that is not a multiple of 32."""
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    from defectdetection_viaobjectdetection_amd.train_engine import TrainEngine
    sd = synthetic_state_dict(scale, nc, seed=3)
    eng = TrainEngine(scale, nc, shape, batch)
    eng.load_state_dict(sd)
    assert eng.rw == 64 + nc and eng.protos_t is None and not any("proto" in o.get("name", "") or "cv4" in o.get("name", "") for o in eng.ops)
    imgs = synthetic_bscans(batch, shape[0], shape[1], seed=9)
    x = torch.from_numpy(imgs.transpose(0, 3, 1, 2).copy()).float() / 255.0
    A = sum((shape[0] // s) * (shape[1] // s) for s in (8, 16, 32))
    R1 = torch.randn((batch, A, 64 + nc), generator=torch.Generator().manual_seed(1))
    oracle, o_raw, g32 = _ref_grads(scale, nc, sd, x, R1, batch, False)
    _, f_raw, g16 = _ref_grads(scale, nc, sd, x, R1, batch, True)
    raw, pr = eng.forward(torch.from_numpy(imgs).to(cuda_device))
    torch.cuda.synchronize()
    assert pr is None and raw.shape == (batch, A, 64 + nc)
    e_raw, fl_raw = rel_l2(raw.cpu(), o_raw), rel_l2(f_raw, o_raw)
    print(f"forward: raw rel-L2 {e_raw:.2e} (format floor {fl_raw:.2e})")
    assert e_raw <= 1.5 * fl_raw + 2e-3
    eng.backward(R1.to(cuda_device), None)
    torch.cuda.synchronize()
    assert set(k for k, _, _ in eng.trainable()) == {k for k, v in g32.items() if v is not None}      # (all but the fixed DFL conv)
    rows = []
    cosf = lambda a, b: float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))  # noqa: E731
    for name, p, gr in eng.trainable():
        want = g32[name]
        got = gr.cpu()
        if got.dim() == 4:
            got = got.permute(0, 3, 1, 2)                                     # KRSC -> OIHW
        assert got.shape == want.shape and torch.isfinite(got).all(), name
        rows.append((name, rel_l2(got, want), rel_l2(g16[name], want), cosf(got, want), cosf(g16[name], want)))
    hip = np.array([r[1] for r in rows]); floor = np.array([r[2] for r in rows])
    cos_h = np.array([r[3] for r in rows]); cos_f = np.array([r[4] for r in rows])
    worst = sorted(rows, key=lambda r: -r[1])[:5]
    print("worst parameter-gradient rel-L2 (HIP, floor):", [(n, f"{e:.2e}", f"{f:.2e}") for n, e, f, _, _ in worst])
    print(f"{len(rows)} tensors: rel-L2 median HIP {np.median(hip):.2e} floor {np.median(floor):.2e}; max HIP {hip.max():.2e} floor {floor.max():.2e}; "
          f"min cosine HIP {cos_h.min():.4f} floor {cos_f.min():.4f}")
    assert np.median(hip) <= 1.5 * np.median(floor) + 2e-3
    assert (hip <= 2.5 * np.maximum(floor, np.median(floor)) + 5e-3).all(), [r for r in rows if r[1] > 2.5 * max(r[2], np.median(floor)) + 5e-3]
    assert 1.0 - cos_h.min() <= 3.0 * (1.0 - cos_f.min()) + 1e-3
    rm = eng.params["model.0.bn.running_mean"].cpu()
    assert torch.allclose(rm, oracle.model[0].bn.running_mean, atol=2e-3)
    # the state dict goes back to upstream's names, the detect head's included
    back = eng.state_dict()
    assert set(back) == set(sd) and all(back[k].shape == sd[k].shape for k in sd)


def test_v8det_forward_backward_is_bitwise_reproducible(cuda_device):
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    from defectdetection_viaobjectdetection_amd.train_engine import TrainEngine
    scale, shape, batch, nc = "8n", (64, 96), 2, 3
    eng = TrainEngine(scale, nc, shape, batch)
    eng.load_state_dict(synthetic_state_dict(scale, nc, seed=3))
    imgs = torch.from_numpy(synthetic_bscans(batch, shape[0], shape[1], seed=9)).to(cuda_device)
    A = sum((shape[0] // s) * (shape[1] // s) for s in (8, 16, 32))
    R1 = torch.randn((batch, A, 64 + nc), generator=torch.Generator().manual_seed(1)).to(cuda_device)
    outs = []
    for _ in range(2):
        raw, _ = eng.forward(imgs, update_running_stats=False)
        eng.backward(R1, None)
        torch.cuda.synchronize()
        outs.append((raw.clone(), eng.flat_grads.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]), int((outs[0][1] != outs[1][1]).sum())
    # the re-pack job kernel on the detect spec list writes what the torch copies write
    eng.repack()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in eng.packed.items()}
    for v in eng.packed.values():
        v.zero_()
    eng._repack_torch()
    torch.cuda.synchronize()
    assert all(torch.equal(got[k], v) for k, v in eng.packed.items())


# ---------------------------------------------------------------------------------------------------- 3. the class-BCE kernel
def _bce_case(B, A, nc, seed):
    g = torch.Generator().manual_seed(seed)
    rw = 64 + nc
    raw = torch.randn((B, A, rw), generator=g) * 3.0
    x = raw[..., 64:]
    special = torch.tensor([0.0, 30.0, -30.0, 88.0, -88.0])
    flat = x.reshape(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:min(5, flat.numel())]] = special[:min(5, flat.numel())]
    raw[..., 64:] = flat.view(B, A, nc)
    t = torch.zeros(B * A * nc)
    n_soft = max(1, round(0.01 * t.numel()))
    t[torch.randperm(t.numel(), generator=g)[:n_soft]] = 1.0 - torch.rand(n_soft, generator=g)       # soft values in (0, 1]
    return raw, t.view(B, A, nc)


@pytest.mark.parametrize("B,A,nc", [(2, 84, 1), (2, 84, 3), (3, 126, 80), (1, 21, 3)])   # nets of 64x64, 64x96, 32x32; the last is 63 elements < a wave
def test_cls_bce_kernel_against_float64(B, A, nc, cuda_device):
    """m355_cls_bce_launch against float64 torch.  Yardstick: torch's own fp32 BCE-with-logits + autograd on the same data against
    float64.  The kernel's loss sum may be off by twice torch-fp32's relative error + 1e-6, its gradient by twice torch-fp32's maximum
    absolute error + one fp32 ulp of |s|.  The columns of d_raw outside the class block keep their sentinel; two runs give the same bits."""
    import torch.nn.functional as F
    from defectdetection_viaobjectdetection_amd.loss import cls_bce_device
    raw, t = _bce_case(B, A, nc, seed=B * 1000 + nc)
    s = 0.5 * B * 1024.0 / max(float(t.sum()), 1.0)             # gain * B * loss scale / denom
    x64 = raw[..., 64:].double().requires_grad_(True)
    l64 = F.binary_cross_entropy_with_logits(x64, t.double(), reduction="sum")
    (l64 * s).backward()
    x32 = raw[..., 64:].clone().requires_grad_(True)
    l32 = F.binary_cross_entropy_with_logits(x32, t, reduction="sum")
    (l32 * torch.tensor(s, dtype=torch.float32)).backward()
    ref_rel = abs(float(l32) - float(l64)) / float(l64)
    ref_abs = float((x32.grad.double() - x64.grad).abs().max())
    ulp_s = float(np.spacing(np.float32(abs(s))))
    d_raw = torch.full(raw.shape, -7.25, device=cuda_device)
    r_dev, t_dev = raw.to(cuda_device), t.to(cuda_device)
    s_dev = torch.tensor(s, dtype=torch.float32, device=cuda_device)
    total = cls_bce_device(r_dev, t_dev, s_dev, d_raw)
    torch.cuda.synchronize()
    got_rel = abs(float(total) - float(l64)) / float(l64)
    got_abs = float((d_raw[..., 64:].cpu().double() - x64.grad).abs().max())
    print(f"cls_bce B={B} A={A} nc={nc}: loss sum rel err kernel {got_rel:.3e} torch-fp32 {ref_rel:.3e} | gradient max abs err kernel "
          f"{got_abs:.3e} torch-fp32 {ref_abs:.3e} (s = {s:.4g}, ulp {ulp_s:.3e})")
    assert got_rel <= 2 * ref_rel + 1e-6
    assert got_abs <= 2 * ref_abs + ulp_s
    assert bool((d_raw[..., :64] == -7.25).all())
    d2 = torch.full(raw.shape, -7.25, device=cuda_device)
    total2 = cls_bce_device(r_dev, t_dev, s_dev, d2)
    torch.cuda.synchronize()
    assert torch.equal(d2, d_raw) and float(total2) == float(total)


# ---------------------------------------------------------------------------------------------------- 4. DetCriterion on the device
def test_det_criterion_on_device_matches_the_reference_loss(cuda_device):
    from defectdetection_viaobjectdetection_amd import loss as L
    B, nc, imgsz, scale = 2, 3, (64, 96), 64.0
    raw, _, batch, hw = _case(2, B, nc, imgsz, 3, True)         # a handful of boxes; image 0 has no labels
    raw = raw[..., :64 + nc].contiguous()
    batch = {k: v for k, v in batch.items() if k != "masks"}
    crit = L.DetCriterion(nc, imgsz)
    r_dev = raw.to(cuda_device)
    items, d_raw, d_pr = crit(r_dev, None, crit.prepare(batch, B, cuda_device), scale)
    torch.cuda.synchronize()
    assert d_pr is None and items.device.type == "cuda" and d_raw.device.type == "cuda" and torch.equal(r_dev.cpu(), raw)
    check_against_reference(items, d_raw, raw, batch, hw, nc, imgsz, scale)
    i2, g2, _ = crit(r_dev, None, {k: v.to(cuda_device) for k, v in batch.items()}, scale)
    torch.cuda.synchronize()
    assert torch.equal(items, i2) and torch.equal(d_raw, g2)     # no atomics anywhere: the same bits
    # no labels at all: only the class term, written by the kernel into an otherwise zero gradient
    empty = {"batch_idx": torch.zeros(0), "cls": torch.zeros(0, 1), "bboxes": torch.zeros(0, 4)}
    items0, d0, _ = crit(r_dev, None, empty, 2.0)
    check_against_reference(items0, d0, raw, empty, hw, nc, imgsz, 2.0)
    assert float(d0[..., :64].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------- 5. API end to end
def make_box_dataset(root, n_train=8, n_val=4, size=64, seed=0):
    """Noise images with one or two bright rectangles each and `cls cx cy w h` label rows + data yaml."""
    import yaml
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    for split, n in (("train", n_train), ("val", n_val)):
        os.makedirs(os.path.join(root, "images", split), exist_ok=True)
        os.makedirs(os.path.join(root, "labels", split), exist_ok=True)
        for i in range(n):
            im = Image.fromarray(rng.normal(60, 12, (size, size)).clip(0, 255).astype(np.uint8)).convert("RGB")
            dr = ImageDraw.Draw(im)
            rows = []
            for _ in range(int(rng.integers(1, 3))):
                w, h = rng.integers(size // 4, size // 2, 2)
                cx = rng.integers(w // 2 + 2, size - w // 2 - 2)
                cy = rng.integers(h // 2 + 2, size - h // 2 - 2)
                dr.rectangle([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], fill=(230, 200, 40))
                rows.append(f"0 {cx / size:.6f} {cy / size:.6f} {w / size:.6f} {h / size:.6f}")
            im.save(os.path.join(root, "images", split, f"bscan_{i:03d}.png"))
            with open(os.path.join(root, "labels", split, f"bscan_{i:03d}.txt"), "w") as f:
                f.write("\n".join(rows) + "\n")
    ypath = os.path.join(root, "data.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump({"train": "images/train", "val": "images/val", "names": {0: "defect"}}, f)
    return ypath


DET_FIELDS = ["epoch", "time", "train/box_loss", "train/cls_loss", "train/dfl_loss", "metrics/precision(B)", "metrics/recall(B)",
              "metrics/mAP50(B)", "metrics/mAP50-95(B)", "lr/pg0", "loss_scale"]


def test_v8det_train_api_end_to_end(tmp_path, cuda_device):
    from ultralytics import YOLO
    from defectdetection_viaobjectdetection_amd.train import _run_dir
    data = make_box_dataset(str(tmp_path / "data"))
    model = YOLO("yolov8n.yaml")
    res = model.train(data=data, epochs=2, imgsz=64, batch=4, project=str(tmp_path), name="d", verbose=False)
    run = str(tmp_path / "d")
    assert res.save_dir == run
    for f in ("weights/last.pt", "weights/best.pt", "results.csv"):
        assert os.path.isfile(os.path.join(run, f)), f
    assert _run_dir(None, None, True, "detect") == os.path.join("runs", "detect", "train")          # the default root, no second run
    assert _run_dir(None, None, True) == os.path.join("runs", "segment", "train")
    with open(os.path.join(run, "results.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0] == DET_FIELDS and len(rows) == 3
    assert len(res.history) == 2 and all(math.isfinite(v) for h in res.history for v in h.values() if isinstance(v, float))
    assert not any("seg" in k or "(M)" in k for k in res.history[-1])
    assert model.task == "detect" and model.nc == 1 and model.names == {0: "defect"}
    img = os.path.join(str(tmp_path / "data"), "images", "val", "bscan_000.png")
    for w in ("best.pt", "last.pt"):
        again = YOLO(os.path.join(run, "weights", w))
        assert again.task == "detect" and again.scale == "8n"
        r = again.predict(source=img, imgsz=64, conf=0.001, verbose=False)
        assert len(r) == 1 and r[0].masks is None and r[0].boxes.data.shape[1] == 6
    m = again.val(data=data, imgsz=64)
    assert 0.0 <= m.box.map50 <= 1.0 and not hasattr(m, "seg") and m.save_dir is None
    assert m.fitness == pytest.approx(0.1 * m.box.map50 + 0.9 * m.box.map) and set(m.results_dict) == set(DET_FIELDS[5:9]) | {"fitness"}
    # last.pt holds the EMA weights the trainer's validator saw after the final epoch: the same numbers
    assert m.results_dict["metrics/mAP50(B)"] == pytest.approx(res.history[-1]["metrics/mAP50(B)"], abs=1e-9)
    # resume: a run interrupted after its first epoch continues from last.pt
    r1 = YOLO("yolov8n.yaml").train(data=data, epochs=2, imgsz=64, batch=4, project=str(tmp_path), name="r", verbose=False, max_steps=2)
    assert len(r1.history) == 1
    r2 = YOLO(os.path.join(str(tmp_path / "r"), "weights", "last.pt")).train(resume=True, verbose=False)
    assert r2.save_dir == str(tmp_path / "r") and [h["epoch"] for h in r2.history] == [1, 2] and r2.optimizer_steps > r1.optimizer_steps


def test_v8det_loss_falls_on_a_fixed_batch(tmp_path, cuda_device):
    """Thirty optimizer steps on one unaugmented batch (the eight training images, every epoch the same batch): the summed loss ends
    below its first value -- a direction check.  Eight images, not fewer: the loss divides by max(sum of target scores, 1), and with
    the fresh head's 120-pixel boxes on four 64 x 64 images that sum starts BELOW 1, where the clamp scales the first value down
    (2.5 against ~10 here) and learning first raises the loss by lifting the sum to 1."""
    from ultralytics import YOLO
    data = make_box_dataset(str(tmp_path / "data"), n_train=8, n_val=1)
    model = YOLO("yolov8n.yaml")
    res = model.train(data=data, epochs=30, imgsz=64, batch=8, project=str(tmp_path), name="f", verbose=False, augment=False, fliplr=0.0,
                      val=False, warmup_epochs=0.0, nbs=8, optimizer="AdamW", lr0=0.002, save=False)
    total = [sum(h[k] for k in ("train/box_loss", "train/cls_loss", "train/dfl_loss")) for h in res.history]
    print("summed loss per step:", [round(v, 3) for v in total])
    assert res.optimizer_steps + res.skipped_steps == 30 and res.optimizer_steps >= 25
    assert all(math.isfinite(v) for v in total) and total[-1] < total[0]


# ---------------------------------------------------------------------------------------------------- 6. validator
def test_v8det_validator_matches_the_oracle_matcher(tmp_path, cuda_device):
    """Box mAP of a detect model through val() equals the number obtained by feeding the same engine's detections through the training
    oracle's match_predictions / ap_per_class (tests/test_loss_val_gpu.py does the same for seg; box half only here).  So that the
    number is not a trivial zero without a trained model, the ground truth is made FROM the model: per image two of its detections
    that lie inside the image, shrunk to 0.95 / 0.8 of their size (IoU 0.90 / 0.64 with their source), written as `cls cx cy w h`."""
    from ultralytics import YOLO
    from defectdetection_viaobjectdetection_amd.dataset import SegDataset, img2label_path, read_data_yaml
    from defectdetection_viaobjectdetection_amd.engine import SegEngine
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    S = 256           # (the synthetic head's boxes are ~120 px wide: they fit inside a 256-pixel image, not a 64-pixel one)
    data = make_box_dataset(str(tmp_path / "data"), n_train=1, n_val=6, size=S, seed=3)
    model = YOLO("yolov8n.yaml")
    model.set_classes(1, {0: "defect"})
    model.load_state_dict(synthetic_state_dict("8n", 1, seed=2, cls_bias=-2.5))       # plenty of detections over conf 0.001
    eng = SegEngine("8n", 1, (S, S), max_batch=4, keep_raw=False)
    eng.load_state_dict(model.state_dict)

    def detections(ds):
        out = []
        for i0 in range(0, len(ds), 4):
            idx = list(range(i0, min(i0 + 4, len(ds))))
            preds, _ = eng.forward(torch.from_numpy(ds.images[idx]).to(cuda_device))
            dets, counts, _ = eng.postprocess(preds, None, 0.001, 0.7, 300, masks=False, multi_label=True)
            out += [dets[j, :int(counts[j]), :6].float().cpu().numpy().astype(np.float64) for j in range(len(idx))]
        return out

    val_dir = read_data_yaml(data)["val"]
    ds = SegDataset(val_dir, S, nc=1)
    n_lab = 0
    for f, d in zip(ds.files, detections(ds)):
        b = d[:, :4]
        inside = np.nonzero((b[:, 0] >= 0) & (b[:, 1] >= 0) & (b[:, 2] <= S) & (b[:, 3] <= S))[0][:2]
        rows = []
        for j, shrink in zip(inside, (0.95, 0.8)):
            cx, cy, w, h = (b[j, 0] + b[j, 2]) / 2, (b[j, 1] + b[j, 3]) / 2, (b[j, 2] - b[j, 0]) * shrink, (b[j, 3] - b[j, 1]) * shrink
            rows.append(f"0 {cx / S:.6f} {cy / S:.6f} {w / S:.6f} {h / S:.6f}")
        n_lab += len(rows)
        with open(img2label_path(f), "w") as fh:
            fh.write("\n".join(rows) + "\n")
    assert n_lab >= 8
    m = model.val(data=data, imgsz=S, batch=4)
    ds = SegDataset(val_dir, S, nc=1)                                                # (the labels just written)
    tp, confs, pcls, gcls = [], [], [], []
    for i, d in enumerate(detections(ds)):
        g_cls = np.array([c for c, _ in ds.labels[i]], np.int64)
        g = np.array([[p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()] for _, p in ds.labels[i]], np.float64).reshape(-1, 4)
        gcls.append(g_cls)
        if d.shape[0] == 0:
            continue
        b = d[:, :4]
        iw = np.clip(np.minimum(g[:, None, 2], b[None, :, 2]) - np.maximum(g[:, None, 0], b[None, :, 0]), 0, None)
        ih = np.clip(np.minimum(g[:, None, 3], b[None, :, 3]) - np.maximum(g[:, None, 1], b[None, :, 1]), 0, None)
        inter = iw * ih
        iou = inter / (((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] - inter + 1e-7)
        c = d[:, 5].astype(np.int64)
        tp.append(tro.match_predictions(c, g_cls, iou)); confs.append(d[:, 4]); pcls.append(c)
    eng.close()
    ap, _ = tro.ap_per_class(np.concatenate(tp), np.concatenate(confs), np.concatenate(pcls), np.concatenate(gcls))
    print(f"val(): mAP50 {m.box.map50:.6f} mAP50-95 {m.box.map:.6f}; oracle matcher on the same detections: {ap[:, 0].mean():.6f} {ap.mean():.6f} "
          f"({n_lab} labels, {sum(len(c) for c in confs)} detections)")
    assert float(ap[:, 0].mean()) > 0, "the labels come from the detections: some must match"
    assert m.box.map50 == pytest.approx(float(ap[:, 0].mean()), abs=1e-9) and m.box.map == pytest.approx(float(ap.mean()), abs=1e-9)
    assert not hasattr(m, "seg")
