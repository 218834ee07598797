"""The two kernels every predict() and val() call ends in, at their edges, through the per-op entries alone (no engine):
``proto_masks_kernel`` (m355_proto_masks) per pixel against the fp64 restatement tests/mask_ref.py, on the smallest shapes
that reach every case of its 8 x 32-cell tile, and ``nms_kernel`` (m355_nms / m355_nms_ex) bit for bit against the oracle's
non_max_suppression on hand-built predictions that reach each of its branches.  Every output lies between guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_ref as mref

pytestmark = pytest.mark.gpu
GUARD = 4096            # bytes of 0xA5 around every output


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(nbytes, dev):
    return torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=dev)


def _split(raw, nbytes, what):
    """Host copy of a guarded buffer's body, after checking that the bands around it are unchanged."""
    h = raw.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all(), f"a byte in front of {what} changed"
    assert (h[GUARD + nbytes:] == 0xA5).all(), f"a byte behind {what} changed"
    return h[GUARD:GUARD + nbytes]


# ----------------------------------------------------------------------------------------------- masks
def _run_masks(dev, protos, dets, counts, max_det, shape, mh=None, mw=None):
    from defectdetection_viaobjectdetection_amd._capi import lib
    in_h, in_w = shape
    B = len(counts)
    mh, mw = mh or in_h // 4, mw or in_w // 4
    nbytes = B * max_det * in_h * in_w
    raw = _guarded(nbytes, dev)
    d_dets = torch.from_numpy(dets).to(dev)
    d_cnt = torch.tensor(np.asarray(counts, np.int32), device=dev)
    d_pr = torch.from_numpy(protos).to(dev)
    rc = lib.m355_proto_masks(_p(d_dets), _p(d_cnt), _p(d_pr), B, max_det, mh, mw, in_h, in_w,
                              C.c_void_p(raw.data_ptr() + GUARD), _stream())
    torch.cuda.synchronize()
    return rc, _split(raw, nbytes, "the masks").reshape(B, max_det, in_h, in_w)


@pytest.mark.parametrize("kind", mref.KINDS)
@pytest.mark.parametrize("case", range(len(mref.COUNT_CASES)), ids=[f"counts{c[0]}_maxdet{c[1]}" for c in mref.COUNT_CASES])
@pytest.mark.parametrize("shape", mref.SHAPES, ids=[f"{h}x{w}" for h, w in mref.SHAPES])
def test_proto_masks_per_pixel(cuda_device, shape, case, kind):
    """A pixel may differ from the fp64 restatement only where |v| <= 2^-16 S; a pixel with S == 0 is 0; and no more pixels
    differ than the reference has inside that band.  Slots at and past min(counts[b], max_det) are not checked."""
    counts, max_det = mref.COUNT_CASES[case]
    protos, dets, n = mref.edge_case(shape, counts, max_det, kind, case)
    rc, got = _run_masks(cuda_device, protos, dets, counts, max_det, shape)
    assert rc == 0
    n_diff = n_band = n_sup = unsupported = 0
    worst = 0.0
    for b in range(len(counts)):
        ref, v, S = mref.process_mask_ref(dets[b, :n[b], 6:], protos[b], dets[b, :n[b], :4], shape)
        nd, wr, uns = mref.compare(got[b, :n[b]], ref, v, S)
        sup, bnd = mref.band(v, S)
        n_diff, n_band, n_sup, unsupported, worst = n_diff + nd, n_band + bnd, n_sup + sup, unsupported + uns, max(worst, wr)
    print(f"{shape} counts {counts} max_det {max_det} {kind}: {n_diff} pixels differ, {n_band} band pixels of {n_sup} "
          f"supported, worst |v|/S {worst:.3e} (bound {mref.REL:.3e})")
    assert unsupported == 0, f"{unsupported} pixels outside every kept cell's support are set"
    assert worst <= mref.REL
    assert n_diff <= n_band


def test_proto_masks_refuses_other_geometry(cuda_device):
    """An upsample factor other than 4 and an input width that is no multiple of 16 are refused before the launch: negative
    status, no byte of the output written.  (The entry takes no nm: it passes 32, the only width the kernel is built for.)"""
    rng = np.random.default_rng(0)
    for (mh, mw), shape in (((20, 40), (160, 320)), ((20, 40), (80, 320)), ((20, 42), (80, 168))):
        protos = rng.standard_normal((1, mh, mw, 32)).astype(np.float16)
        dets = np.zeros((1, 4, 38), np.float32)
        dets[..., :4] = (0, 0, shape[1], shape[0])
        dets[..., 6:] = rng.standard_normal((1, 4, 32))
        rc, got = _run_masks(cuda_device, protos, dets, [4], 4, shape, mh, mw)
        assert rc < 0, (mh, mw, shape, rc)
        assert (got == 0xA5).all(), f"{(mh, mw)} -> {shape}: refused, but the output was written"


# ----------------------------------------------------------------------------------------------- NMS
NM = 32


def _run_nms(dev, pn, nc, conf, iou, max_det, agnostic=None, nm=NM):
    """m355_nms (agnostic None) or m355_nms_ex on (B, A, 4+nc+nm) predictions -> (rows per image, counts), guards checked."""
    from defectdetection_viaobjectdetection_amd._capi import lib
    B, A, wd = pn.shape
    assert wd == 4 + nc + nm and pn.dtype == np.float32
    preds = torch.from_numpy(pn).to(dev)
    dbytes = B * max_det * (6 + nm) * 4
    draw, craw = _guarded(dbytes, dev), _guarded(4 * B, dev)
    d_ptr, c_ptr = C.c_void_p(draw.data_ptr() + GUARD), C.c_void_p(craw.data_ptr() + GUARD)
    if agnostic is None:
        rc = lib.m355_nms(_p(preds), B, A, nc, nm, conf, iou, max_det, d_ptr, c_ptr, _stream())
    else:
        rc = lib.m355_nms_ex(_p(preds), B, A, nc, nm, conf, iou, max_det, int(agnostic), None, d_ptr, c_ptr, _stream())
    assert rc == 0, lib.m355_last_error(None)
    torch.cuda.synchronize()
    counts = _split(craw, 4 * B, "counts").view(np.int32).copy()
    dets = _split(draw, dbytes, "dets").view(np.float32).reshape(B, max_det, 6 + nm)
    assert ((counts >= 0) & (counts <= max_det)).all(), counts
    return [dets[b, :counts[b]].copy() for b in range(B)], counts


def _oracle_nms(pn, nc, conf, iou, max_det, agnostic=False):
    import yolov8_seg_oracle as orc
    return orc.non_max_suppression(pn.transpose(0, 2, 1), nc, conf, iou, max_det, agnostic=bool(agnostic))


def _same_bits(got, ref, what):
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, f"{what} image {b}: {g.shape[0]} rows, the oracle has {r.shape[0]}"
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(r).view(np.uint32)), \
            f"{what} image {b}: rows differ"


def _check(dev, pn, nc, conf, iou, max_det, what, agnostic=None):
    got, counts = _run_nms(dev, pn, nc, conf, iou, max_det, agnostic)
    _same_bits(got, _oracle_nms(pn, nc, conf, iou, max_det, agnostic), what)
    return got, counts


def _n_candidates(pn, nc, conf):
    return (pn[..., 4:4 + nc].max(-1) > np.float32(conf)).sum(-1)


def _blank(rng, B, A, nc):
    """Predictions without boxes and scores: random mask coefficients, the first of them the anchor's index (exact in f32), so
    that a row tells which anchor it came from."""
    p = np.zeros((B, A, 4 + nc + NM), np.float32)
    p[..., 4 + nc:] = rng.standard_normal((B, A, NM))
    p[..., 4 + nc] = np.arange(A)
    return p


def _anchors(rows):
    """The anchor each row came from (the first mask coefficient of _blank)."""
    return rows[:, 6].astype(np.int64)


def _disjoint(rng, B, A):
    """cx, cy, w, h of A boxes that do not touch: one per 8 px cell of a 100-column grid, anchors in shuffled cells."""
    out = np.zeros((B, A, 4), np.float32)
    for b in range(B):
        cell = rng.permutation(A)
        out[b, :, 0] = 4 + 8 * (cell % 100)
        out[b, :, 1] = 4 + 8 * (cell // 100)
        out[b, :, 2:] = rng.uniform(3, 6, (A, 2))
    return out


def _clusters(rng, B, A, k, jitter=1.0):
    """Near-copies of k boxes per image: NMS suppresses most of a cluster."""
    centres = rng.uniform(40, 600, (B, k, 2))
    sizes = rng.uniform(20, 80, (B, k, 2))
    pick = rng.integers(0, k, (B, A))[..., None].repeat(2, -1)
    out = np.zeros((B, A, 4), np.float32)
    out[..., :2] = np.take_along_axis(centres, pick, 1) + rng.normal(0, jitter, (B, A, 2))
    out[..., 2:] = np.take_along_axis(sizes, pick, 1) * rng.uniform(0.96, 1.04, (B, A, 2))
    return out


@pytest.mark.parametrize("boxes", ["disjoint", "clusters"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097])
def test_nms_candidate_counts(cuda_device, n, boxes):
    """n candidates among A = 5000 anchors, the others scoring exactly conf (the strict > leaves them out): the chunk of 64, the
    4096 keys the sort holds in LDS, and one more, which moves it to the global workspace and pads it to 8192."""
    A, B, conf = 5000, 2, 0.25
    rng = np.random.default_rng(1000 + n)
    p = _blank(rng, B, A, 1)
    p[..., :4] = _disjoint(rng, B, A) if boxes == "disjoint" else _clusters(rng, B, A, 5, jitter=3.0)
    p[..., 4] = np.float32(conf)
    for b in range(B):
        p[b, rng.choice(A, n, replace=False), 4] = rng.uniform(0.3, 1.0, n)
    assert (_n_candidates(p, 1, conf) == n).all() and ((p[..., 4] == np.float32(conf)).sum(-1) == A - n).all()
    max_det = 1024 if boxes == "disjoint" else 300
    got, counts = _check(cuda_device, p, 1, conf, 0.7, max_det, f"n {n} {boxes}")
    if boxes == "disjoint":
        assert (counts == min(n, max_det)).all(), counts
    else:
        assert (counts == n).all() if n <= 1 else ((counts > 0) & (counts < min(n, max_det))).all(), counts
    print(f"n {n} {boxes}: counts {counts.tolist()}")


def test_nms_global_workspace_sort_is_deterministic(cuda_device):
    """Every one of 8400 anchors a candidate: the keys are sorted in the global workspace, in slots handed out by an atomic
    counter.  Three launches give the same bits."""
    A, B, max_det = 8400, 2, 300
    rng = np.random.default_rng(7)
    p = _blank(rng, B, A, 1)
    p[..., :4] = _clusters(rng, B, A, 40)
    p[..., 4] = rng.uniform(0.3, 1.0, (B, A))
    n = _n_candidates(p, 1, 0.25)
    assert (n == A).all() and A > 4096
    got, counts = _check(cuda_device, p, 1, 0.25, 0.7, max_det, "global sort")
    assert ((counts > 0) & (counts < max_det)).all(), counts
    for _ in range(2):
        again, c2 = _run_nms(cuda_device, p, 1, 0.25, 0.7, max_det)
        assert np.array_equal(counts, c2)
        _same_bits(again, got, "second launch")
    print(f"global sort: n {n.tolist()} counts {counts.tolist()}")


@pytest.mark.parametrize("nc", [1, 3])
def test_nms_score_ties(cuda_device, nc):
    """Scores in sixteenths, some 250 anchors per value, overlapping clusters: among equal scores the lower anchor comes first.
    With nc = 3, anchors whose two best classes tie take the first of them."""
    A, B, max_det = 3000, 2, 300
    rng = np.random.default_rng(20 + nc)
    p = _blank(rng, B, A, nc)
    p[..., :4] = _clusters(rng, B, A, 30, jitter=3.0)
    p[..., 4:4 + nc] = rng.integers(5, 17, (B, A, nc)) / 16.0
    first = {}
    if nc == 3:   # ten anchors apart from every cluster, top score, two equal maxima
        for i, a in enumerate(rng.choice(A, 10, replace=False)):
            sc = [(1.0, 0.5, 1.0), (0.5, 1.0, 1.0), (1.0, 1.0, 1.0)][i % 3]
            p[:, a, :4] = (2000 + 100 * i, 2000, 40, 40)
            p[:, a, 4:7] = sc
            first[int(a)] = int(np.argmax(sc))
    n = _n_candidates(p, nc, 0.25)
    assert (n == A).all() and len(np.unique(p[..., 4:4 + nc])) <= 13
    got, counts = _check(cuda_device, p, nc, 0.25, 0.7, max_det, f"ties nc {nc}")
    assert (counts > 30).all()
    for b in range(B):
        conf, anc = got[b][:, 4], _anchors(got[b])
        assert (np.diff(conf) <= 0).all()
        same = np.diff(conf) == 0
        assert same.sum() > 20 and (np.diff(anc)[same] > 0).all(), "equal scores: the lower anchor must come first"
        for a, cls in first.items():
            row = got[b][anc == a]
            assert row.shape[0] == 1 and row[0, 5] == cls and row[0, 4] == 1.0
    print(f"ties nc {nc}: n {n.tolist()} counts {counts.tolist()}")


@pytest.mark.parametrize("max_det", [1, 63, 64, 65, 300, 1024])
def test_nms_max_det_cut(cuda_device, max_det):
    """1100 boxes that do not touch: the kept list ends at max_det, in the first chunk, at a chunk's end, one past it, in
    mid-chunk, and at the full 1024 the kernel can hold."""
    A, n = 1200, 1100
    rng = np.random.default_rng(31)
    p = _blank(rng, 1, A, 1)
    p[..., :4] = _disjoint(rng, 1, A)
    p[..., 4] = np.float32(0.25)
    cand = rng.choice(A, n, replace=False)
    p[0, cand, 4] = rng.uniform(0.3, 1.0, n)
    assert _n_candidates(p, 1, 0.25)[0] == n
    got, counts = _check(cuda_device, p, 1, 0.25, 0.7, max_det, f"max_det {max_det}")
    assert counts[0] == max_det
    if max_det == 1024:
        cand = np.sort(cand)
        want = cand[np.argsort(-p[0, cand, 4], kind="stable")][:1024]
        assert np.array_equal(_anchors(got[0]), want), "the rows must be the first 1024 candidates by score"
    print(f"max_det {max_det}: n {n} count {counts[0]}")


def _few(rows, nc=1):
    """A handful of anchors given as (cx, cy, w, h, scores...) rows, among anchors that score nothing."""
    rng = np.random.default_rng(len(rows))
    A = len(rows) + 3
    p = _blank(rng, 1, A, nc)
    p[0, :, :4] = (500, 500, 30, 30)
    for i, r in enumerate(rows):
        p[0, i + 1, :4 + nc] = r
    return p


def test_nms_iou_threshold_is_strict(cuda_device):
    """(1, 1, 2, 2) and (1, 0.5, 2, 1): intersection 2, union 4, IoU exactly 0.5.  At iou = 0.5 both stay (suppression needs
    IoU > iou); at one float below 0.5 the second goes."""
    p = _few([(1, 1, 2, 2, 0.9), (1, 0.5, 2, 1, 0.8)])
    assert _n_candidates(p, 1, 0.25)[0] == 2
    got, counts = _check(cuda_device, p, 1, 0.25, 0.5, 300, "IoU == iou")
    assert counts[0] == 2
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    got, counts = _check(cuda_device, p, 1, 0.25, below, 300, "IoU just above iou")
    assert counts[0] == 1 and got[0][0, 4] == np.float32(0.9)
    # score == conf: the candidate test is strict as well
    got, counts = _check(cuda_device, p, 1, float(np.float32(0.8)), 0.5, 300, "score == conf")
    assert counts[0] == 1
    print("thresholds: n 2, counts 2 / 1 / 1")


def test_nms_zero_area_boxes(cuda_device):
    """Five copies of a box without area: their IoU is 0 / 0, which is not above any threshold, so all of them stay, as in
    the oracle; so does the ordinary box that contains them (IoU 0)."""
    p = _few([(10, 10, 0, 0, 0.9 - 0.1 * i) for i in range(5)] + [(10, 10, 8, 8, 0.95)])
    assert _n_candidates(p, 1, 0.25)[0] == 6
    got, counts = _check(cuda_device, p, 1, 0.25, 0.7, 300, "zero area")
    assert counts[0] == 6
    print("zero area: n 6, count 6")


def test_nms_class_offsets_and_agnostic(cuda_device):
    """One box, twelve anchors, eleven classes of 80 (the last class twice): the class offset keeps one per class; agnostic NMS
    keeps one."""
    nc = 80
    classes = [0, 1, 2, 5, 17, 31, 32, 63, 64, 78, 79, 79]
    rows = []
    for i, c in enumerate(classes):
        sc = np.zeros(nc, np.float32)
        sc[c] = 0.9 - 0.01 * i
        rows.append(np.concatenate(((100.3, 200.7, 50.1, 60.9), sc)))
    p = _few(rows, nc)
    assert _n_candidates(p, nc, 0.25)[0] == 12
    got, counts = _check(cuda_device, p, nc, 0.25, 0.7, 300, "class offsets, m355_nms")
    assert counts[0] == 11 and sorted(got[0][:, 5].tolist()) == sorted(set(classes))
    got, counts = _check(cuda_device, p, nc, 0.25, 0.7, 300, "class offsets, m355_nms_ex", agnostic=False)
    assert counts[0] == 11
    got, counts = _check(cuda_device, p, nc, 0.25, 0.7, 300, "agnostic", agnostic=True)
    assert counts[0] == 1 and got[0][0, 5] == 0
    print("classes: n 12, counts 11 / 11 / 1")


def test_nms_large_anchor_count(cuda_device):
    """A = 21504, every anchor a candidate: the sort runs on 32768 keys in the global workspace."""
    A, max_det = 21504, 300
    rng = np.random.default_rng(41)
    p = _blank(rng, 1, A, 1)
    p[..., :4] = _clusters(rng, 1, A, 40)
    p[..., 4] = rng.uniform(0.3, 1.0, (1, A))
    n = _n_candidates(p, 1, 0.25)
    assert n[0] == A
    got, counts = _check(cuda_device, p, 1, 0.25, 0.7, max_det, "A 21504")
    assert 0 < counts[0] < max_det
    print(f"A 21504: n {n[0]} count {counts[0]}")


CAP = 30000     # the candidates that enter the greedy pass (upstream's max_nms)


def _cap_case(rng, n_over, scores_low, low_anchor_order=None):
    """A = 30100: n_over candidates that all overlap the best of them, then disjoint boxes with the lower scores given, at
    shuffled anchors.  Returns (preds, anchors of the low boxes in the order of scores_low)."""
    A = 30100
    n_low = len(scores_low)
    assert n_over + n_low == A
    p = _blank(rng, 1, A, 1)
    anchors = rng.permutation(A)
    over, low = anchors[:n_over], anchors[n_over:]
    if low_anchor_order is not None:
        low = low_anchor_order(low)
    p[0, over, :4] = np.asarray((300, 300, 200, 200)) + rng.uniform(-1, 1, (n_over, 4))
    p[0, over, 4] = rng.uniform(0.5, 1.0, n_over)
    p[0, low, 0] = 1000 + 20 * np.arange(n_low)
    p[0, low, 1] = 1000
    p[0, low, 2:4] = 10
    p[0, low, 4] = scores_low
    return p, low


def test_nms_candidate_cap(cuda_device):
    """Only the first 30000 candidates by score enter the greedy pass.  30050 overlapping candidates, then 50 disjoint ones
    with lower scores: all 50 lie past the cap and 1 box stays (51 without the cap).  With 29990 overlapping ones the first 10
    of 110 low boxes lie inside it: 11 stay, and they are those ten."""
    rng = np.random.default_rng(51)
    p, low = _cap_case(rng, 30050, 0.4 - 0.001 * np.arange(50))
    assert _n_candidates(p, 1, 0.25)[0] == 30100
    got, counts = _check(cuda_device, p, 1, 0.25, 0.7, 300, "cap, every low box past it")
    assert counts[0] == 1
    p, low = _cap_case(rng, 29990, 0.4 - 0.001 * np.arange(110))
    got, counts2 = _check(cuda_device, p, 1, 0.25, 0.7, 300, "cap, ten low boxes inside it")
    assert counts2[0] == 11 and np.array_equal(_anchors(got[0])[1:], low[:10])
    print(f"cap: n 30100, counts {counts[0]} / {counts2[0]}")


def test_nms_candidate_cap_tie_at_the_cut(cuda_device):
    """The 30000th and the 30001st score are equal: the one at the lower anchor is inside the cap."""
    rng = np.random.default_rng(52)
    scores = 0.4 - 0.001 * np.arange(110)
    scores[10] = scores[9]

    def order(low):   # the later of the two in this list gets the lower anchor
        low = low.copy()
        if low[10] > low[9]:
            low[[9, 10]] = low[[10, 9]]
        return low

    p, low = _cap_case(rng, 29990, scores, order)
    assert low[10] < low[9] and p[0, low[9], 4] == p[0, low[10], 4]
    srt = np.sort(p[0, :, 4])[::-1]
    assert srt[CAP - 1] == srt[CAP] and srt[CAP - 2] > srt[CAP - 1] > srt[CAP + 1]
    got, counts = _check(cuda_device, p, 1, 0.25, 0.7, 300, "cap, tie at the cut")
    assert counts[0] == 11 and np.array_equal(_anchors(got[0])[1:], np.concatenate((low[:9], low[10:11])))
    print(f"cap tie: n 30100, count {counts[0]}")
