"""predict(retina_masks=True, classes=..., agnostic_nms=...) on the HIP path: the NMS options bit-exact against the oracle NMS
on class-filtered scores, the native-resolution mask kernel against the fp64 restatement (tests/native_mask_ref.py), and
the whole predict call on the golden B-scan."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

import native_mask_ref as nref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PNG = os.path.join(GOLDEN, "bscans", "787-225_01_Ch-0_51.png")
CLASS_SETS = [None, [0], [0, 2], [], [-1, 99]]


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _random_preds(rng, B, A, nc, nm):
    """(B, A, 4+nc+nm) f32: boxes in 40 clusters of near-copies (NMS suppresses most of a cluster and keeps well under
    max_det), scores u^4 per class."""
    p = np.zeros((B, A, 4 + nc + nm), np.float32)
    centres = rng.uniform(40, 600, (B, 40, 2))
    sizes = rng.uniform(20, 80, (B, 40, 2))
    pick = rng.integers(0, 40, (B, A))
    p[..., :2] = np.take_along_axis(centres, pick[..., None].repeat(2, -1), 1) + rng.normal(0, 2, (B, A, 2))
    p[..., 2:4] = np.take_along_axis(sizes, pick[..., None].repeat(2, -1), 1) * rng.uniform(0.92, 1.08, (B, A, 2))
    p[..., 4:4 + nc] = rng.uniform(0, 1, (B, A, nc)) ** 4
    p[..., 4 + nc:] = rng.standard_normal((B, A, nm))
    return p


def _rows(dets, counts):
    d, n = dets.cpu().numpy(), counts.cpu().numpy()
    return [d[b, :n[b]] for b in range(len(n))]


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_nms_ex_matches_restatement(cuda_device, nc):
    from defectdetection_viaobjectdetection_amd._capi import lib
    from defectdetection_viaobjectdetection_amd.engine import class_mask
    rng = np.random.default_rng(nc)
    B, A, nm, max_det = 3, 2100, 32, 300
    pn = _random_preds(rng, B, A, nc, nm)
    preds = torch.from_numpy(pn).to(cuda_device)
    dets = torch.empty((B, max_det, 6 + nm), dtype=torch.float32, device=cuda_device)
    counts = torch.empty((B,), dtype=torch.int32, device=cuda_device)
    # the default arguments: bit-identical to m355_nms
    d0 = torch.empty_like(dets)
    c0 = torch.empty_like(counts)
    assert lib.m355_nms(_p(preds), B, A, nc, nm, 0.25, 0.7, max_det, _p(d0), _p(c0), _stream()) == 0
    assert lib.m355_nms_ex(_p(preds), B, A, nc, nm, 0.25, 0.7, max_det, 0, None, _p(dets), _p(counts), _stream()) == 0
    assert torch.equal(counts, c0)
    for a, b in zip(_rows(dets, counts), _rows(d0, c0)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pt = pn.transpose(0, 2, 1).copy()
    for agnostic in (False, True):
        for classes in CLASS_SETS:
            cm = class_mask(classes, nc, cuda_device)
            assert lib.m355_nms_ex(_p(preds), B, A, nc, nm, 0.25, 0.7, max_det, int(agnostic), _p(cm), _p(dets), _p(counts),
                                   _stream()) == 0
            ref = nref.nms_ref(pt, nc, 0.25, 0.7, max_det, agnostic=agnostic, classes=classes)
            got = _rows(dets, counts)
            for b in range(B):
                assert got[b].shape == ref[b].shape, (agnostic, classes, b, got[b].shape, ref[b].shape)
                assert np.array_equal(got[b], ref[b]), (agnostic, classes, b)
            if classes == []:
                assert int(counts.sum()) == 0
            if classes is None and (agnostic or nc < 80):
                assert 0 < int(counts.max()) < max_det, "the case must not be cut at max_det"
            print(f"nc {nc} agnostic {agnostic} classes {classes}: counts {counts.tolist()}")


@pytest.mark.parametrize("nc", [1, 3])
def test_postprocess_ex_matches_restatement(cuda_device, nc):
    from defectdetection_viaobjectdetection_amd._capi import lib
    from defectdetection_viaobjectdetection_amd.engine import SegEngine
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    eng = SegEngine("n", nc, (320, 320), max_batch=2, keep_raw=False)
    eng.load_state_dict(synthetic_state_dict("n", nc, seed=0, cls_bias=-2.0))
    rng = np.random.default_rng(10 + nc)
    B, max_det = 2, 300
    pn = _random_preds(rng, B, eng.num_anchors, nc, eng.nm)
    preds = torch.from_numpy(pn).to(cuda_device)
    protos = torch.from_numpy(rng.standard_normal((B, 80, 80, 32)).astype(np.float16)).to(cuda_device)
    # the default arguments through m355_postprocess_ex: rows, counts and masks bit-identical to m355_postprocess
    outs = []
    for ex in (False, True):
        d = torch.empty((B, max_det, 38), dtype=torch.float32, device=cuda_device)
        c = torch.empty((B,), dtype=torch.int32, device=cuda_device)
        m = torch.zeros((B, max_det, 320, 320), dtype=torch.uint8, device=cuda_device)
        if ex:
            rc = lib.m355_postprocess_ex(eng._h, _p(preds), _p(protos), B, 0.25, 0.7, max_det, 0, None, _p(d), _p(c), _p(m),
                                         _stream())
        else:
            rc = lib.m355_postprocess(eng._h, _p(preds), _p(protos), B, 0.25, 0.7, max_det, _p(d), _p(c), _p(m), _stream())
        assert rc == 0
        outs.append((d, c, m))
    (d0, c0, m0), (d1, c1, m1) = outs
    assert torch.equal(c0, c1) and torch.equal(m0, m1)
    for a, b in zip(_rows(d0, c0), _rows(d1, c1)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pt = pn.transpose(0, 2, 1).copy()
    for agnostic in (False, True):
        for classes in CLASS_SETS:
            dets, counts, masks = eng.postprocess(preds, protos, 0.25, 0.7, max_det, masks=True, agnostic=agnostic,
                                                  classes=classes)
            ref = nref.nms_ref(pt, nc, 0.25, 0.7, max_det, agnostic=agnostic, classes=classes)
            got = _rows(dets, counts)
            for b in range(B):
                assert np.array_equal(got[b], ref[b]), (agnostic, classes, b)
    with pytest.raises(ValueError):
        eng.postprocess(preds, protos, 0.25, 0.7, max_det, multi_label=True, agnostic=True)
    with pytest.raises(ValueError):
        eng.postprocess(preds, protos, 0.25, 0.7, max_det, multi_label=True, classes=[0])
    # the engine entry checks its arguments before any HIP call too
    assert lib.m355_postprocess_ex(eng._h, _p(preds), _p(protos), B, 0.25, 0.7, max_det, 2, None, _p(d0), _p(c0), None,
                                   _stream()) == -1
    assert lib.m355_postprocess_ex(eng._h, _p(preds), _p(protos), 3, 0.25, 0.7, max_det, 0, None, _p(d0), _p(c0), None,
                                   _stream()) == -1
    eng.close()


# ----------------------------------------------------------------------------------------------- native masks
GUARD = 67          # guard bytes in front of the output (an odd count: the planes start off any 16-byte boundary)


def _run_native(cuda_device, protos, coefs, boxes, counts, shapes, max_det, extra_slots=0):
    """Launch m355_proto_masks_native on guard-banded output.  Returns (per image masks (slots, h0, w0), guards intact)."""
    from defectdetection_viaobjectdetection_amd._capi import lib
    B = len(shapes)
    dets = np.zeros((B, max_det, 38), np.float32)
    dets[:, :coefs.shape[1], 6:] = coefs
    bx = np.zeros((B, max_det, 4), np.float32)
    bx[:, :boxes.shape[1]] = boxes
    slots = [min(int(n) + extra_slots, max_det) if n else 0 for n in counts]
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([s * h * w for s, (h, w) in zip(slots, shapes)])
    total = int(off[-1])
    buf = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device=cuda_device)
    hw = np.asarray(shapes, np.int32).reshape(B, 2)
    d_dets = torch.from_numpy(dets).to(cuda_device)
    d_cnt = torch.tensor(np.asarray(counts, np.int32), device=cuda_device)
    d_pr = torch.from_numpy(protos).to(cuda_device)
    d_bx = torch.from_numpy(bx).to(cuda_device)
    mh, mw = protos.shape[1:3]
    rc = lib.m355_proto_masks_native(_p(d_dets), _p(d_cnt), _p(d_pr), B, max_det, mh, mw, hw.ctypes.data_as(C.c_void_p),
                                     _p(d_bx), off.ctypes.data_as(C.c_void_p), C.c_void_p(buf.data_ptr() + GUARD), _stream())
    assert rc == 0, lib.m355_last_error(None)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    guards = bool((h[:GUARD] == 0xA5).all() and (h[GUARD + total:] == 0xA5).all())
    body = h[GUARD:GUARD + total]
    return [body[off[b]:off[b + 1]].reshape(slots[b], *shapes[b]) for b in range(B)], guards, h


def _border_boxes(h0, w0):
    return np.asarray([(0, 0, w0, h0), (0, 0.3 * h0, 0.4 * w0, h0), (0.6 * w0, 0, w0, 0.5 * h0), (0.2 * w0, 0.7 * h0, w0, h0),
                       (0, 0, 0.5 * w0, 0.25 * h0)], np.float32)


NATIVE_CASES = {
    "orig_is_net_320": ((80, 80), [(320, 320)], 20),
    "1920x1080_at_640x384": ((96, 160), [(1080, 1920)], 20),
    "odd_upscale": ((80, 80), [(333, 517), (517, 333)], 12),
    "downscale": ((80, 80), [(50, 70)], 10),
    "mixed_shapes": ((160, 160), [(320, 320), (1080, 1920), (57, 640), (641, 31)], 8),
}


@pytest.mark.parametrize("case", sorted(NATIVE_CASES))
def test_native_masks_match_restatement(cuda_device, case):
    (mh, mw), shapes, n = NATIVE_CASES[case]
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    protos, coefs, boxes = nref.random_case(rng, mh, mw, shapes, n)
    for b, (h0, w0) in enumerate(shapes):   # boxes clipped at each border
        boxes[b, :5] = _border_boxes(h0, w0)
    counts = [n] * len(shapes)
    if len(shapes) > 2:
        counts[1] = 0                          # an image without detections inside the launch
    got, guards, _ = _run_native(cuda_device, protos, coefs, boxes, counts, shapes, 300, extra_slots=1)
    got2, _, _ = _run_native(cuda_device, protos, coefs, boxes, counts, shapes, 300, extra_slots=1)
    assert guards, "a guard byte around the output changed"
    tot_diff, worst = 0, 0.0
    for b, (h0, w0) in enumerate(shapes):
        assert np.array_equal(got[b], got2[b]), "two runs differ"
        k = counts[b]
        assert got[b].shape[0] == (k + 1 if k else 0)
        if k:
            assert not got[b][k:].any(), "slots past the count must be zero"
        ref, info = nref.native_masks(coefs[b, :k], protos[b].astype(np.float64), boxes[b, :k], (h0, w0))
        nd, wr, outside = nref.compare_native(got[b][:k], ref, info)
        assert outside == 0, f"{outside} pixels outside their box are not 0"
        tot_diff += nd
        worst = max(worst, wr)
        assert ref.sum() > 0 or k == 0
    print(f"{case}: {tot_diff} pixels differ from the fp64 restatement, worst |v|/S {worst:.3e} (bound 2^-16 = {2 ** -16:.3e})")
    assert worst <= 2.0 ** -16


def test_native_masks_max_det_rows_and_empty_batch(cuda_device):
    rng = np.random.default_rng(7)
    shapes = [(40, 48)]
    protos, coefs, boxes = nref.random_case(rng, 80, 80, shapes, 300)
    got, guards, _ = _run_native(cuda_device, protos, coefs, boxes, [300], shapes, 300)
    assert guards and got[0].shape == (300, 40, 48)
    ref, info = nref.native_masks(coefs[0], protos[0].astype(np.float64), boxes[0], shapes[0])
    nd, wr, outside = nref.compare_native(got[0], ref, info)
    print(f"max_det 300: {nd} pixels differ, worst |v|/S {wr:.3e}")
    assert outside == 0 and wr <= 2.0 ** -16
    # no detection anywhere: nothing is launched, nothing written
    got, guards, h = _run_native(cuda_device, protos, coefs, boxes, [0], shapes, 300)
    assert guards and got[0].shape == (0, 40, 48) and h.size == 2 * GUARD


# ----------------------------------------------------------------------------------------------- predict end to end
def _big_bscan(tmp_path):
    from PIL import Image
    im = np.asarray(Image.open(PNG).convert("L"))
    big = np.tile(im, (2, 3))                            # 640 x 960
    path = str(tmp_path / "bscan_960x640.png")
    Image.fromarray(big).save(path)
    return path


def _model(arch, scale, nc, seed=0, cls_bias=-2.0):
    from ultralytics import YOLO
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    m = YOLO(arch)
    m.set_classes(nc, {i: f"c{i}" for i in range(nc)})
    m.load_state_dict(synthetic_state_dict(scale, nc, seed=seed, cls_bias=cls_bias))
    return m


def _engine_outputs(model, path, imgsz, conf=0.25, iou=0.7, max_det=300):
    """The engine predict() used, re-run on the same letterboxed input: preds (A, 4+nc+nm) and protos (mh, mw, 32)."""
    from defectdetection_viaobjectdetection_amd.preprocess import letterbox, letterbox_shape, load_image
    img = load_image(path)
    net = letterbox_shape(img.shape[:2], (imgsz, imgsz), True)[3]
    lb = letterbox(img, (imgsz, imgsz), auto=True)
    eng = model._engines[(net[0], net[1], 0)]
    x = torch.from_numpy(np.ascontiguousarray(lb[None, :, :, ::-1])).to(eng.device)
    preds, protos = eng.forward(x)
    torch.cuda.synchronize()
    return img, net, preds[0].cpu().numpy(), None if protos is None else protos[0].cpu().numpy()


def _check_retina(model, path, imgsz, nc, tmp_path, conf=0.25):
    from defectdetection_viaobjectdetection_amd.preprocess import scale_boxes_to_original
    base = model.predict(path, imgsz=imgsz, conf=conf, verbose=False)[0]
    res = model.predict(path, imgsz=imgsz, conf=conf, retina_masks=True, verbose=False)[0]
    assert np.array_equal(res.boxes.data.numpy(), base.boxes.data.numpy())
    h0, w0 = res.orig_shape
    n = len(res.boxes)
    assert n > 0, "the synthetic weights must detect something on the fixture"
    assert tuple(res.masks.data.shape) == (n, h0, w0) and res.masks.data.dtype == torch.uint8
    img, net, preds, protos = _engine_outputs(model, path, imgsz)
    ref_rows = nref.nms_ref(preds.T[None].copy(), nc, conf, 0.7, 300)[0]
    boxes = scale_boxes_to_original(ref_rows[:, :4], net, (h0, w0))
    assert np.array_equal(boxes, res.boxes.data.numpy()[:, :4])
    ref, info = nref.native_masks(ref_rows[:, 6:], protos.astype(np.float64), boxes, (h0, w0))
    nd, worst, outside = nref.compare_native(res.masks.data.numpy(), ref, info)
    print(f"{path} @ {imgsz}: {n} detections, masks {tuple(res.masks.data.shape)}, {nd} pixels differ, worst |v|/S {worst:.3e}")
    assert outside == 0 and worst <= 2.0 ** -16
    for p in res.masks.xy:
        if p.size:
            assert p[:, 0].min() >= 0 and p[:, 0].max() <= w0 and p[:, 1].min() >= 0 and p[:, 1].max() <= h0
    im = res.plot()
    assert im.shape == (h0, w0, 3)
    assert os.path.isfile(res.save(str(tmp_path / f"retina_{os.path.basename(path)}.jpg")))


@pytest.mark.parametrize("nc", [1, 3])
def test_predict_retina_masks_v8(cuda_device, tmp_path, nc):
    model = _model("yolov8n-seg.yaml", "n", nc)
    _check_retina(model, PNG, 640, nc, tmp_path)
    _check_retina(model, _big_bscan(tmp_path), 640, nc, tmp_path)


def test_predict_retina_masks_v9c(cuda_device, tmp_path):
    model = _model("yolov9c-seg.yaml", "9c", 1, seed=2, cls_bias=-2.0)
    _check_retina(model, PNG, 320, 1, tmp_path, conf=0.1)


def _check_classes(model, path, imgsz, nc, classes, agnostic):
    from defectdetection_viaobjectdetection_amd.preprocess import scale_boxes_to_original
    res = model.predict(path, imgsz=imgsz, classes=classes, agnostic_nms=agnostic, retina_masks=True, verbose=False)[0]
    img, net, preds, _ = _engine_outputs(model, path, imgsz)
    ref = nref.nms_ref(preds.T[None].copy(), nc, 0.25, 0.7, 300, agnostic=agnostic, classes=classes)[0]
    got = res.boxes.data.numpy()
    assert got.shape[0] == ref.shape[0], (classes, agnostic, got.shape, ref.shape)
    assert np.array_equal(got[:, 4:6], ref[:, 4:6])
    assert np.array_equal(got[:, :4], scale_boxes_to_original(ref[:, :4], net, img.shape[:2]))
    print(f"classes {classes} agnostic {agnostic}: {len(got)} detections")
    return res


def test_predict_classes_agnostic_v8_nc3(cuda_device, tmp_path):
    model = _model("yolov8n-seg.yaml", "n", 3)
    path = _big_bscan(tmp_path)
    full = model.predict(path, verbose=False)[0]
    print(f"classes detected without a filter: {sorted(set(int(c) for c in full.boxes.cls.tolist()))}")
    for classes, agnostic in ((None, True), ([1], False), ([0, 2], True), (2, False), ([], False)):
        res = _check_classes(model, path, 640, 3, classes, agnostic)
        assert res.masks is not None and tuple(res.masks.data.shape[1:]) == res.orig_shape


def test_predict_classes_agnostic_yolo11(cuda_device, tmp_path):
    model = _model("yolo11n.yaml", "11n", 3, cls_bias=-2.5)
    path = _big_bscan(tmp_path)
    for classes, agnostic in ((None, True), ([0], False), ([1, 2], True)):
        res = _check_classes(model, path, 640, 3, classes, agnostic)
        assert res.masks is None
