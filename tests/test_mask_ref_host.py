"""tests/mask_ref.py, the fp64 restatement of the letterboxed mask assembly, against the oracle's process_mask and on cases
that can be checked by hand; and the condition on the GPU test's inputs that makes its per-pixel rule sharp: few of their
supported pixels lie inside the rounding-margin band.  No GPU."""
import numpy as np
import pytest
import torch

import mask_ref as mref

BAND_CAP = 1e-3


def _oracle(protos, dets, n, shape):
    import yolov8_seg_oracle as orc
    p = torch.from_numpy(protos.astype(np.float32)).permute(2, 0, 1).contiguous()
    m = orc.process_mask(p, torch.from_numpy(dets[:n, 6:]), torch.from_numpy(dets[:n, :4]), shape)
    return m.numpy().astype(np.uint8)


def test_crafted_boxes_fill_one_case():
    for shape in mref.SHAPES:
        assert len(mref.crafted_boxes(*shape)) == mref.COUNT_CASES[-1][0][0]
    protos, dets, n = mref.edge_case(mref.SHAPES[0], *mref.COUNT_CASES[-1], "mixed", 0)
    cb = mref.crafted_boxes(*mref.SHAPES[0])
    for b in range(2):   # both images of the last case hold every crafted box
        have = {tuple(r) for r in dets[b, :n[b], :4].tolist()}
        assert all(tuple(r) in have for r in cb.tolist())


@pytest.mark.parametrize("kind", mref.KINDS)
@pytest.mark.parametrize("shape", mref.SHAPES)
def test_restatement_matches_oracle_and_band_is_thin(shape, kind):
    """Every case the GPU test runs (same seeds): pixel for pixel the oracle's masks; at most BAND_CAP of the supported
    pixels of a shape inside the margin band (measured: 1e-4 and below)."""
    sup_total, band_total = 0, 0
    for seed, (counts, max_det) in enumerate(mref.COUNT_CASES):
        protos, dets, n = mref.edge_case(shape, counts, max_det, kind, seed)
        for b in range(len(counts)):
            ref, v, S = mref.process_mask_ref(dets[b, :n[b], 6:], protos[b], dets[b, :n[b], :4], shape)
            assert ref.shape == (n[b],) + shape
            orc_m = _oracle(protos[b], dets[b], n[b], shape)
            assert np.array_equal(ref, orc_m), f"{shape} {kind} {counts} image {b}: {(ref != orc_m).sum()} pixels differ"
            assert not ref[S == 0].any() and not v[S == 0].any()
            sup, bnd = mref.band(v, S)
            sup_total += sup
            band_total += bnd
            if n[b] >= 15:
                assert ref.any() and not ref.all()
    print(f"{shape} {kind}: {band_total} of {sup_total} supported pixels inside the band (share {band_total / sup_total:.2e})")
    assert band_total <= BAND_CAP * sup_total


def _one(box, L, shape):
    """The mask of one detection whose cell logits are L (mh, mw): prototype channel 0 = L, coefficient e_0."""
    mh, mw = L.shape
    protos = np.zeros((mh, mw, 32))
    protos[..., 0] = L
    coefs = np.zeros((1, 32))
    coefs[0, 0] = 1.0
    m, v, S = mref.process_mask_ref(coefs, protos, np.asarray([box], np.float32), shape)
    return m[0], v[0], S[0]


def test_one_cell_set():
    shape = (32, 48)
    L = np.zeros((8, 12))
    L[3, 5] = 1.0
    m, v, S = _one((0, 0, 48, 32), L, shape)
    # cell (3, 5) has its centre at pixel (13.5, 21.5): the hat reaches 4 px to either side, so rows 10..17, columns 18..25
    want = np.zeros(shape, np.uint8)
    want[10:18, 18:26] = 1
    assert np.array_equal(m, want) and np.array_equal(S > 0, want.astype(bool))
    wy = np.asarray([0.125, 0.375, 0.625, 0.875, 0.875, 0.625, 0.375, 0.125])
    assert np.array_equal(v[10:18, 18:26], np.outer(wy, wy))
    # the same cell in the corner: the clamped border replicates it, weight 1 in the outermost two pixels
    L = np.zeros((8, 12))
    L[0, 0] = -2.0
    m, v, S = _one((0, 0, 48, 32), L, shape)
    assert not m.any()
    assert np.array_equal(v[:6, :6], -2.0 * np.outer([1, 1, 0.875, 0.625, 0.375, 0.125], [1, 1, 0.875, 0.625, 0.375, 0.125]))
    assert np.array_equal(S > 0, v < 0) and (S > 0).sum() == 36


def test_integer_edges_keep_cells_k_to_m_minus_1():
    shape = (32, 48)
    for (k, m_), (j, l) in (((2, 7), (1, 4)), ((0, 12), (0, 8)), ((11, 12), (7, 8))):
        keep = mref.kept_cells(np.asarray([(4 * k, 4 * j, 4 * m_, 4 * l)], np.float32), 8, 12, shape)[0]
        want = np.zeros((8, 12), bool)
        want[j:l, k:m_] = True
        assert np.array_equal(keep, want)
    # an edge one pixel inside a cell: x1 = 4 k + 1 drops cell k, x2 = 4 m + 1 adds cell m
    keep = mref.kept_cells(np.asarray([(9, 0, 29, 32)], np.float32), 8, 12, shape)[0]
    assert np.array_equal(np.nonzero(keep[0])[0], np.arange(3, 8))
    # with all logits 1 the mask of cells 2..6 x 1..3 is their pixels plus the half of the hat that stays positive: 2 px
    # (weights 0.375, 0.125) to either side, clipped by nothing here
    m, v, S = _one((8, 4, 28, 16), np.ones((8, 12)), shape)
    want = np.zeros(shape, np.uint8)
    want[2:18, 6:30] = 1
    assert np.array_equal(m, want)
    assert v[10, 6] == 0.125 and v[10, 7] == 0.375 and v[10, 8] == 0.625 and v[10, 9] == 0.875 and v[10, 10] == 1.0


@pytest.mark.parametrize("box", [(50, 10, 50, 40), (60, 10, 40, 40), (10, 20, 30, 20), (-30, -20, -2, -1), (49, 0, 70, 32),
                                 (0, 33, 48, 50), (41, 21, 43, 23)])
def test_empty_and_outside_boxes_give_zeros(box):
    rng = np.random.default_rng(0)
    m, v, S = _one(box, rng.standard_normal((8, 12)), (32, 48))
    assert not m.any() and not v.any() and not S.any()


def test_compare_rule():
    ref = np.asarray([[1, 0, 0, 1]], np.uint8)
    v = np.asarray([[1e-6, -1.0, 0.0, 1.0]])
    S = np.asarray([[1.0, 1.0, 0.0, 1.0]])
    assert mref.compare(ref.copy(), ref, v, S) == (0, 0.0, 0)
    got = np.asarray([[0, 0, 0, 1]], np.uint8)          # differs inside the band
    nd, worst, uns = mref.compare(got, ref, v, S)
    assert (nd, uns) == (1, 0) and worst == 1e-6 and worst <= mref.REL
    got = np.asarray([[1, 1, 0, 1]], np.uint8)          # differs far outside it
    nd, worst, uns = mref.compare(got, ref, v, S)
    assert (nd, uns) == (1, 0) and worst == 1.0
    got = np.asarray([[1, 0, 1, 1]], np.uint8)          # a pixel without support is set
    assert mref.compare(got, ref, v, S) == (1, 0.0, 1)
    assert mref.band(v, S) == (3, 1)
