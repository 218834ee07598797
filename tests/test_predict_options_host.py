"""predict(retina_masks / classes / agnostic_nms) without a GPU: the fp64 restatement (tests/native_mask_ref.py) pinned by
known answers, the class filter on a hand-built case, and the argument checks of the new C entry points, which are decided
before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import native_mask_ref as nref


def _one(L: np.ndarray, h0: int, w0: int, box=None):
    """Masks and logits of one detection whose logit grid (mh, mw) is L (coefficient e0, prototype channel 0 = L)."""
    mh, mw = L.shape
    P = np.zeros((mh, mw, 32))
    P[..., 0] = L
    c = np.zeros((1, 32))
    c[0, 0] = 1.0
    box = np.asarray([box if box is not None else (0, 0, w0, h0)], np.float32)
    m, info = nref.native_masks(c, P, box, (h0, w0))
    return m[0], info[0]


def test_identity_case_is_interpolate():
    """h0 = 4 mh without pad: the crop is the whole grid and step 3 is F.interpolate(size=(h0, w0), bilinear)."""
    rng = np.random.default_rng(0)
    L = rng.standard_normal((6, 5))
    assert nref.crop(6, 5, 24, 20) == (0, 6, 0, 5)
    m, (rows, cols, v, S) = _one(L, 24, 20)
    want = F.interpolate(torch.from_numpy(L)[None, None], size=(24, 20), mode="bilinear", align_corners=False)[0, 0].numpy()
    assert np.allclose(v, want, rtol=0, atol=1e-12)
    assert np.array_equal(m, (want > 0).astype(np.uint8))
    # the x4 weights spelled out: output 0 clamps to cell 0, output 2 is 7/8 cell 0 + 1/8 cell 1, the last output is the last cell
    assert v[0, 0] == L[0, 0] and np.isclose(v[-1, -1], L[-1, -1], rtol=0, atol=1e-15)
    assert np.isclose(v[0, 2], 0.875 * L[0, 0] + 0.125 * L[0, 1], rtol=0, atol=1e-15)


def test_pure_pad_crops():
    assert nref.crop(8, 8, 4, 8) == (2, 6, 0, 8)              # gain 1: 2 pad rows above and below
    assert nref.crop(160, 160, 1080, 1920) == (35, 125, 0, 160)
    assert nref.crop(96, 160, 1080, 1920) == (3, 93, 0, 160)  # 1920 x 1080 at the 640 x 384 rect letterbox
    assert nref.crop(80, 80, 100, 333) == (27, 52, 0, 80)     # fractional pad 27.99: truncated
    # a pad-only crop: the padded rows never reach the mask
    L = np.full((8, 8), -1.0)
    L[2:6] = 1.0
    m, _ = _one(L, 4, 8)
    assert m.shape == (4, 8) and m.all()


def test_one_cell_box():
    L = np.ones((4, 4))
    m, (rows, cols, _, _) = _one(L, 16, 16, box=(5.0, 7.0, 6.0, 8.0))
    assert list(rows) == [7] and list(cols) == [5]
    assert m.sum() == 1 and m[7, 5] == 1
    m, _ = _one(L, 16, 16, box=(5.5, 7.0, 6.0, 8.0))         # x1 > 5, x2 = 6: no integer column
    assert m.sum() == 0


def test_box_touching_each_border():
    L = np.ones((4, 4))
    m, _ = _one(L, 16, 12, box=(0.0, 0.0, 12.0, 16.0))
    assert m.all()
    m, _ = _one(L, 16, 12, box=(11.0, 15.0, 12.0, 16.0))     # bottom-right pixel only
    assert m.sum() == 1 and m[15, 11] == 1
    m, _ = _one(L, 16, 12, box=(0.0, 0.0, 0.5, 16.0))        # left column
    assert m[:, 0].all() and m.sum() == 16
    m, _ = _one(L, 16, 12, box=(0.0, 0.0, 12.0, 0.25))       # top row
    assert m[0].all() and m.sum() == 12


def test_downscale():
    """An original smaller than the network input: 40 x 40 at an 80 x 80 grid, gain 2: output p reads cells 2p and 2p + 1
    at weight 1/2 each along both axes."""
    rng = np.random.default_rng(1)
    L = rng.standard_normal((80, 80))
    assert nref.crop(80, 80, 40, 40) == (0, 80, 0, 80)
    m, (_, _, v, _) = _one(L, 40, 40)
    want = 0.25 * (L[0::2, 0::2] + L[1::2, 0::2] + L[0::2, 1::2] + L[1::2, 1::2])
    assert np.allclose(v, want, rtol=0, atol=1e-12)
    assert np.array_equal(m, (want > 0).astype(np.uint8))


def test_compare_native_tolerance():
    rng = np.random.default_rng(2)
    protos, coefs, boxes = nref.random_case(rng, 16, 16, [(50, 70)], 5)
    ref, info = nref.native_masks(coefs[0], protos[0], boxes[0], (50, 70))
    assert nref.compare_native(ref.copy(), ref, info) == (0, 0.0, 0)
    bad = ref.copy()
    rows, cols = info[0][0], info[0][1]
    if rows.size and cols.size:
        bad[0, rows[0], cols[0]] ^= 1
        n, worst, _ = nref.compare_native(bad, ref, info)
        assert n == 1 and worst > 0
    out = ref.copy()
    inside = np.zeros((50, 70), bool)
    inside[np.ix_(info[0][0], info[0][1])] = True
    ys, xs = np.nonzero(~inside)
    out[0, ys[0], xs[0]] = 1
    assert nref.compare_native(out, ref, info)[2] == 1


def test_class_filter_drops_excluded_argmax():
    """An anchor whose argmax class is excluded is dropped even when an allowed class also clears conf; an anchor of an
    allowed argmax stays; agnostic NMS merges overlapping boxes of different classes."""
    nc, A = 3, 4
    pred = np.zeros((1, 4 + nc, A), np.float32)
    pred[0, :4, 0] = (50, 50, 20, 20)   # argmax 0 (0.9); class 1 at 0.8 clears conf too
    pred[0, 4:7, 0] = (0.9, 0.8, 0.1)
    pred[0, :4, 1] = (150, 50, 20, 20)  # argmax 1
    pred[0, 4:7, 1] = (0.1, 0.7, 0.0)
    pred[0, :4, 2] = (51, 50, 20, 20)   # overlaps anchor 0, argmax 2
    pred[0, 4:7, 2] = (0.0, 0.1, 0.6)
    pred[0, :4, 3] = (300, 300, 10, 10)  # below conf
    pred[0, 4:7, 3] = (0.1, 0.2, 0.05)
    rows = lambda r: sorted(int(a) for a in r[:, 5])            # noqa: E731
    assert rows(nref.nms_ref(pred, nc, 0.25, 0.7, 300)[0]) == [0, 1, 2]
    only1 = nref.nms_ref(pred, nc, 0.25, 0.7, 300, classes=[1])[0]
    assert rows(only1) == [1] and only1[0, 4] == np.float32(0.7)
    assert rows(nref.nms_ref(pred, nc, 0.25, 0.7, 300, classes=1)[0]) == [1]
    assert rows(nref.nms_ref(pred, nc, 0.25, 0.7, 300, classes=[0, 2])[0]) == [0, 2]
    assert len(nref.nms_ref(pred, nc, 0.25, 0.7, 300, classes=[])[0]) == 0
    assert len(nref.nms_ref(pred, nc, 0.25, 0.7, 300, classes=[7, -1])[0]) == 0
    assert rows(nref.nms_ref(pred, nc, 0.25, 0.7, 300, agnostic=True)[0]) == [0, 1]   # anchor 2 suppressed by anchor 0


def test_class_mask_words():
    from defectdetection_viaobjectdetection_amd.engine import class_mask
    assert class_mask(None, 3, "cpu") is None
    w = class_mask([0, 2, 5, -1], 3, "cpu").numpy().view(np.uint32)
    assert w.tolist() == [0b101]
    w = class_mask(33, 80, "cpu").numpy().view(np.uint32)
    assert w.tolist() == [0, 2, 0]
    assert class_mask([], 80, "cpu").numpy().view(np.uint32).tolist() == [0, 0, 0]
    w = class_mask((31, 63, 79), 80, "cpu").numpy().view(np.uint32)
    assert w.tolist() == [1 << 31, 1 << 31, 1 << 15]


# ----------------------------------------------------------------------------------------------- C entry argument checks
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: the rejection precedes every HIP call


def _lib():
    from defectdetection_viaobjectdetection_amd import _capi
    return _capi.lib


def test_nms_ex_arguments_are_validated_before_any_device_work():
    lib = _lib()
    good = dict(B=1, A=8400, nc=3, nm=32, max_det=300, agnostic=0, mask=None)
    bad = [dict(B=0), dict(A=0), dict(nc=0), dict(nm=-1), dict(max_det=0), dict(max_det=1025), dict(agnostic=2),
           dict(agnostic=-1), dict(nc=1025, mask=FAKE)]
    for b in bad:
        a = {**good, **b}
        rc = lib.m355_nms_ex(FAKE, a["B"], a["A"], a["nc"], a["nm"], 0.25, 0.7, a["max_det"], a["agnostic"], a["mask"],
                             FAKE, FAKE, None)
        assert rc == -1, (b, rc)
    for nul in range(3):
        p = [FAKE, FAKE, FAKE]
        p[nul] = None
        assert lib.m355_nms_ex(p[0], 1, 8400, 3, 32, 0.25, 0.7, 300, 0, None, p[1], p[2], None) == -1
    assert b"null pointer" in lib.m355_last_error(None)


def test_postprocess_ex_refuses_a_null_engine():
    lib = _lib()
    assert lib.m355_postprocess_ex(None, FAKE, FAKE, 1, 0.25, 0.7, 300, 0, None, FAKE, FAKE, None, None) == -1


def _native(lib, B=2, max_det=300, mh=160, mw=160, hw=None, offsets=None, protos=FAKE, out=FAKE, dets=FAKE, boxes=FAKE):
    hw = np.asarray(hw if hw is not None else [(320, 320)] * B, np.int32)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([5 * h * w for h, w in hw])))
    offsets = np.asarray(offsets, np.int64)
    return lib.m355_proto_masks_native(dets, FAKE, protos, B, max_det, mh, mw, hw.ctypes.data_as(ctypes.c_void_p), boxes,
                                       offsets.ctypes.data_as(ctypes.c_void_p), out, None)


@pytest.mark.parametrize("kw", [
    dict(B=0), dict(max_det=0), dict(max_det=1025), dict(mh=0), dict(mw=-4), dict(mw=513), dict(mh=600),
    dict(hw=[(0, 320), (320, 320)]), dict(hw=[(320, -1), (320, 320)]), dict(hw=[(320, 320), (40000, 10)]),
    dict(mh=1, mw=1, hw=[(1000, 1), (1000, 1)]),                      # a crop of no cells (mw odd)
    dict(offsets=[0, 5 * 320 * 320, 4 * 320 * 320]),                  # not monotone
    dict(offsets=[-320 * 320, 0, 320 * 320]),                         # negative start
    dict(offsets=[0, 5 * 320 * 320 + 7, 10 * 320 * 320]),             # not whole planes
    dict(offsets=[0, 301 * 320 * 320, 302 * 320 * 320]),              # more planes than max_det
    dict(protos=ctypes.c_void_p(0x1008)),                             # prototypes not 16-byte aligned
    dict(out=None), dict(dets=None), dict(boxes=None),
])
def test_proto_masks_native_arguments_are_validated_before_any_device_work(kw):
    lib = _lib()
    assert _native(lib, **kw) == -1
    assert lib.m355_last_error(None)


def test_proto_masks_native_null_host_tables():
    lib = _lib()
    hw = np.asarray([(320, 320)], np.int32)
    off = np.asarray([0, 320 * 320], np.int64)
    assert lib.m355_proto_masks_native(FAKE, FAKE, FAKE, 1, 300, 160, 160, None, FAKE, off.ctypes.data_as(ctypes.c_void_p),
                                       FAKE, None) == -1
    assert lib.m355_proto_masks_native(FAKE, FAKE, FAKE, 1, 300, 160, 160, hw.ctypes.data_as(ctypes.c_void_p), FAKE, None,
                                       FAKE, None) == -1
