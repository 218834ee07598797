"""Training augmentation: parameters and label geometry on the host, pixels on the GPU (SURVEY.md A14 defaults, N2).

Upstream's defaults for the reference's train call (/root/reference/BscanBased/yolo_seg_train.py:12): mosaic 1.0
(off for the last `close_mosaic` = 10 epochs), RandomPerspective(degrees 0, translate 0.1, scale 0.5, shear 0,
perspective 0), HSV (0.015, 0.7, 0.4), fliplr 0.5.  The letterboxed uint8 cache of the split lives in HBM; one launch
of `m355_augment` (csrc/augment.hip) composes the mosaic canvas, warps it bilinearly with border 114, applies the HSV
gains and the flip and writes the network input batch.  The polygons go through the same forward matrix here, are
clipped to the image (Sutherland-Hodgman) and filtered like upstream's `box_candidates` (>= 2 px wide and high).

The rest of upstream's chain -- `degrees`, `shear`, `perspective`, `flipud`, `mixup`, `copy_paste`, all 0.0 by default -- is
built the same way: the host draws a full 3x3 matrix, a copy-paste list and a second (mixup) layer,
and one launch of `m355_augment_ex` (csrc/augment_ex.hip) renders them.  With all six at 0 nothing here draws a random
number it did not draw before and `render` calls `m355_augment` as before.

Draw order of one output image (an option at 0 draws nothing):
  layer 0:  mosaic gate; [3 partner indices, xc, yc];  copy-paste gate;
            matrix: perspective x, perspective y, angle, scale, shear x, shear y, translate x, translate y
  mixup:    gate; [partner index, r ~ Beta(32, 32), then layer 1 drawn like layer 0]
  image:    flipud gate, fliplr gate, three HSV gains
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._capi import AUG_MAX_PASTE, AUG_MAX_POLY_VERTS, AugExParams, AugParams, AugPoly, check, lib
from .dataset import SegDataset, overlap_mask

HYP = dict(mosaic=1.0, scale=0.5, translate=0.1, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, fliplr=0.5,
           degrees=0.0, shear=0.0, perspective=0.0, flipud=0.0, mixup=0.0, copy_paste=0.0)
EX_OPTIONS = ("degrees", "shear", "perspective", "flipud", "mixup", "copy_paste")    # any of them > 0: m355_augment_ex renders
PASTE_MAX_IOA = 0.30          # a mirrored instance covering this share of an original one (or more) is not pasted


def check_hyp(hyp: Dict) -> None:
    """Ranges of the six options of EX_OPTIONS (upstream's): ValueError on a violation."""
    for k in EX_OPTIONS:
        v = hyp.get(k, 0.0)
        try:                                                   # any real scalar (numpy, 0-d tensor), not only int / float
            ok = not isinstance(v, (bool, str)) and math.isfinite(float(v))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{k}={v!r} must be a finite number")
    if not 0.0 <= hyp.get("perspective", 0.0) <= 0.001:
        raise ValueError(f"perspective={hyp['perspective']} must be in [0, 0.001]")
    for k in ("flipud", "mixup", "copy_paste"):
        if not 0.0 <= hyp.get(k, 0.0) <= 1.0:
            raise ValueError(f"{k}={hyp[k]} is a probability: it must be in [0, 1]")
    for k in ("degrees", "shear"):
        if hyp.get(k, 0.0) < 0.0:
            raise ValueError(f"{k}={hyp[k]} must be >= 0")


def clip_polygon(poly: np.ndarray, w: float, h: float) -> np.ndarray:
    """Sutherland-Hodgman clip of an (n,2) polygon to [0,w] x [0,h]; returns (m,2), m may be 0."""
    def clip_edge(pts, axis, bound, keep_less):
        out = []
        n = len(pts)
        for i in range(n):
            a, b = pts[i], pts[(i + 1) % n]
            ina = a[axis] <= bound if keep_less else a[axis] >= bound
            inb = b[axis] <= bound if keep_less else b[axis] >= bound
            if ina:
                out.append(a)
            if ina != inb:
                t = (bound - a[axis]) / (b[axis] - a[axis])
                out.append(a + t * (b - a))
        return out
    pts = [p for p in np.asarray(poly, np.float64)]
    for axis, bound, less in ((0, 0.0, False), (0, float(w), True), (1, 0.0, False), (1, float(h), True)):
        if not pts:
            break
        pts = clip_edge(pts, axis, bound, less)
    return np.asarray(pts, np.float64).reshape(-1, 2)


def random_perspective(rng, out_hw: Tuple[int, int], canvas_hw: Tuple[int, int], scale: float, translate: float,
                       degrees: float = 0.0, shear: float = 0.0, perspective: float = 0.0) -> np.ndarray:
    """Forward 3x3 matrix canvas -> output, upstream's M = T S R P C: C centres the canvas; P[2,0], P[2,1] ~ U(-perspective,
    perspective); R rotates by a ~ U(-degrees, degrees) degrees about the origin and scales by s ~ U(1-scale, 1+scale); S shears
    by tan of U(-shear, shear) degrees in x and in y; T moves the centre to U(0.5 - translate, 0.5 + translate) of the output.
    Draws in this order: P (two), a, s, S (two), T (two); degrees, shear or perspective at 0 draws nothing and leaves its
    factor out of the product, which is then the scale + translate matrix of the default options, bit for bit."""
    H, W = out_hw
    cc = np.eye(3)
    cc[0, 2], cc[1, 2] = -canvas_hw[1] / 2.0, -canvas_hw[0] / 2.0
    pm = None
    if perspective > 0:
        pm = np.eye(3)
        pm[2, 0] = rng.uniform(-perspective, perspective)
        pm[2, 1] = rng.uniform(-perspective, perspective)
    a = math.radians(rng.uniform(-degrees, degrees)) if degrees > 0 else None
    s = rng.uniform(1.0 - scale, 1.0 + scale)
    r = np.diag([s, s, 1.0])
    if a is not None:
        r[0, 0] = r[1, 1] = s * math.cos(a)
        r[0, 1] = s * math.sin(a)
        r[1, 0] = -s * math.sin(a)
    sm = None
    if shear > 0:
        sm = np.eye(3)
        sm[0, 1] = math.tan(math.radians(rng.uniform(-shear, shear)))
        sm[1, 0] = math.tan(math.radians(rng.uniform(-shear, shear)))
    t = np.eye(3)
    t[0, 2] = rng.uniform(0.5 - translate, 0.5 + translate) * W
    t[1, 2] = rng.uniform(0.5 - translate, 0.5 + translate) * H
    m = t
    for f in (sm, r, pm, cc):
        if f is not None:
            m = m @ f
    return m


def warp_points(m: np.ndarray, pts: np.ndarray) -> Optional[np.ndarray]:
    """(n,2) points through the 3x3 matrix, with the perspective divide when its last row is not (0, 0, 1).  None when a point
    lies on, behind or within 1e-6 of the horizon of the matrix (w <= 1e-6, where the divide is meaningless): such a polygon
    has no image."""
    q = pts @ m[:2, :2].T + m[:2, 2]
    if m[2, 0] != 0.0 or m[2, 1] != 0.0 or m[2, 2] != 1.0:
        w = pts @ m[2, :2] + m[2, 2]
        if (w <= 1e-6).any():
            return None
        q = q / w[:, None]
    return q


def _box(poly: np.ndarray) -> Tuple[float, float, float, float]:
    return float(poly[:, 0].min()), float(poly[:, 1].min()), float(poly[:, 0].max()), float(poly[:, 1].max())


def select_copy_paste(polys: Sequence[np.ndarray], canvas_w: float, p: float) -> List[int]:
    """Upstream's CopyPaste in flip mode, on boxes: mirror every instance left-right on the canvas (x -> canvas_w - x); the
    ratio of a mirrored instance against an original one is the area of the intersection of their boxes over the ORIGINAL box's
    area; a mirrored instance is eligible when that ratio is < 0.30 against every original; the eligible ones are ordered by
    their largest ratio, ascending (ties in instance order), and the first round(p * n_eligible) are taken (Python's round,
    as upstream).  Returns the indices of the instances whose mirror is pasted."""
    if not len(polys):
        return []
    boxes = np.array([_box(q) for q in polys], np.float64)
    mir = boxes.copy()
    mir[:, 0], mir[:, 2] = canvas_w - boxes[:, 2], canvas_w - boxes[:, 0]
    iw = (np.minimum(mir[:, None, 2], boxes[None, :, 2]) - np.maximum(mir[:, None, 0], boxes[None, :, 0])).clip(0)
    ih = (np.minimum(mir[:, None, 3], boxes[None, :, 3]) - np.maximum(mir[:, None, 1], boxes[None, :, 1])).clip(0)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    inter = iw * ih
    worst = np.divide(inter, area[None, :], out=np.zeros_like(inter), where=area[None, :] > 0).max(1)
    eligible = [int(i) for i in np.argsort(worst, kind="stable") if worst[i] < PASTE_MAX_IOA]
    return eligible[:int(round(p * len(eligible)))]


class Augmenter:
    def __init__(self, ds: SegDataset, device: torch.device, seed: int = 0, **hyp):
        unknown = [k for k in hyp if k not in HYP]
        if unknown:
            raise TypeError(f"unknown augmentation options {unknown}")
        self.ds, self.dev = ds, device
        self.hyp = {**HYP, **hyp}
        check_hyp(self.hyp)
        self.ex = any(self.hyp[k] > 0 for k in EX_OPTIONS)
        self.rng = np.random.default_rng(seed)
        self.cache = torch.from_numpy(ds.images).to(device)          # uint8 (N,H,W,3), resident for the whole run
        self.launches = {"m355_augment": 0, "m355_augment_ex": 0}
        self._work: Optional[torch.Tensor] = None                    # device copy of the m355_augment_ex tables
        self._host = None                                            # the host tables of the last m355_augment_ex call
        self._copied = None                                          # event behind that call

    def _layer(self, i: int, mosaic_on: bool) -> dict:
        """Random parameters of one layer: sources, mosaic centre, copy-paste list, matrix; `canvas` holds its instances
        (class, polygon in canvas coordinates), the pasted ones last."""
        H, W = self.ds.imgsz
        hy, rng, n = self.hyp, self.rng, len(self.ds)
        mosaic = bool(mosaic_on and rng.random() < hy["mosaic"])
        if mosaic:
            src = [int(i)] + [int(v) for v in rng.integers(0, n, 3)]
            xc, yc = int(rng.uniform(0.5 * W, 1.5 * W)), int(rng.uniform(0.5 * H, 1.5 * H))
            offs = [(xc - W, yc - H), (xc, yc - H), (xc - W, yc), (xc, yc)]
            ch, cw = 2 * H, 2 * W
        else:
            src, xc, yc, offs = [int(i)] * 4, 0, 0, [(0, 0)]
            ch, cw = H, W
        canvas = []
        for k, (ox, oy) in enumerate(offs):
            for c, poly in self.ds.labels[src[k]]:
                if mosaic:                                           # the part of the source visible on the canvas
                    poly = clip_polygon(poly + np.array([ox, oy], np.float64), 2 * W, 2 * H)
                    if len(poly) < 3:
                        continue
                canvas.append((c, poly))
        paste = []
        if hy["copy_paste"] > 0 and rng.random() < hy["copy_paste"]:
            picks = select_copy_paste([q for _, q in canvas], cw, hy["copy_paste"])
            picks = [j for j in picks if len(canvas[j][1]) <= AUG_MAX_POLY_VERTS][:AUG_MAX_PASTE]   # the kernel's caps
            for j in picks:
                c, q = canvas[j]
                paste.append(np.stack((cw - q[:, 0], q[:, 1]), 1))
                canvas.append((c, paste[-1]))
        m = random_perspective(rng, (H, W), (ch, cw), hy["scale"], hy["translate"], hy["degrees"], hy["shear"], hy["perspective"])
        return dict(src=src, xc=xc, yc=yc, m=m, mosaic=mosaic, paste=paste, canvas=canvas)

    def plan(self, indices: Sequence[int], mosaic_on: bool = True) -> List[dict]:
        """Random parameters + transformed labels of one batch (host).  A plan is its layer 0 (src, xc, yc, m, mosaic, paste)
        plus flip, flipud, gains, inst (the labels of both layers in output pixels) and, under mixup, mix = r and layer1."""
        H, W = self.ds.imgsz
        hy, rng, n = self.hyp, self.rng, len(self.ds)
        out = []
        for i in indices:
            layers = [self._layer(int(i), mosaic_on)]
            mix = 1.0
            if hy["mixup"] > 0 and rng.random() < hy["mixup"]:
                partner = int(rng.integers(0, n))
                mix = float(rng.beta(32.0, 32.0))
                layers.append(self._layer(partner, mosaic_on))
            flipud = bool(hy["flipud"] > 0 and rng.random() < hy["flipud"])
            flip = bool(rng.random() < hy["fliplr"])
            gains = rng.uniform(-1, 1, 3) * np.array([hy["hsv_h"], hy["hsv_s"], hy["hsv_v"]]) + 1.0
            inst = []
            for lay in layers:
                m = lay["m"]
                for c, poly in lay.pop("canvas"):
                    q = warp_points(m, poly)
                    if q is None:
                        continue
                    q = clip_polygon(q, W, H)
                    if len(q) < 3:
                        continue
                    if flip:
                        q = np.stack((W - q[:, 0], q[:, 1]), 1)
                    if flipud:
                        q = np.stack((q[:, 0], H - q[:, 1]), 1)
                    bw, bh = q[:, 0].max() - q[:, 0].min(), q[:, 1].max() - q[:, 1].min()
                    if bw < 2 or bh < 2:
                        continue
                    inst.append((c, q))
            p = dict(layers[0], flip=flip, flipud=flipud, gains=gains, inst=inst, mix=mix,
                     layer1=layers[1] if len(layers) == 2 else None)
            out.append(p)
        return out

    @staticmethod
    def _needs_ex(p: dict) -> bool:
        m = np.asarray(p["m"])
        return bool(p.get("flipud") or p.get("layer1") or p.get("paste") or m[2, 0] != 0 or m[2, 1] != 0 or m[2, 2] != 1)

    def render(self, plans: List[dict]) -> torch.Tensor:
        """One launch: uint8 (B,H,W,3) on the device.  m355_augment when the six options of EX_OPTIONS are all 0 and no plan
        asks for more (hand-made plans need not carry the new keys); m355_augment_ex otherwise."""
        if self.ex or any(self._needs_ex(p) for p in plans):
            return self.render_ex(plans)
        H, W = self.ds.imgsz
        B = len(plans)
        arr = (AugParams * B)()
        for b, p in enumerate(plans):
            minv = np.linalg.inv(p["m"])
            a = arr[b]
            for k in range(4):
                a.src[k] = p["src"][k]
            a.xc, a.yc = float(p["xc"]), float(p["yc"])
            for k, v in enumerate(minv[:2].reshape(-1)):
                a.minv[k] = float(v)
            a.hgain, a.sgain, a.vgain = (float(g) for g in p["gains"])
            a.flip, a.mosaic = int(p["flip"]), int(p["mosaic"])
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=self.dev)
        self.launches["m355_augment"] += 1
        check(lib.m355_augment(C.c_void_p(self.cache.data_ptr()), C.c_void_p(raw.data_ptr()), C.c_void_p(out.data_ptr()), B, H, W,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        out._keepalive = raw
        return out

    def ex_tables(self, plans: List[dict]):
        """The host arguments of m355_augment_ex for `plans`: (AugExParams[B], AugPoly[n_polys], float32 (n_verts, 2)).
        Affine matrices are inverted like `render` does and normalised to a last row of (0, 0, 1) exactly."""
        arr = (AugExParams * len(plans))()
        polys, verts, nv = [], [], 0
        for b, p in enumerate(plans):
            a = arr[b]
            layers = [p] + ([p["layer1"]] if p.get("layer1") else [])
            a.n_layers, a.mix = len(layers), float(p.get("mix", 1.0))
            a.hgain, a.sgain, a.vgain = (float(g) for g in p["gains"])
            a.flip, a.flipud = int(p["flip"]), int(bool(p.get("flipud")))
            for lay, L in zip(layers, a.layer):
                for k in range(4):
                    L.src[k] = lay["src"][k]
                L.xc, L.yc, L.mosaic = float(lay["xc"]), float(lay["yc"]), int(lay["mosaic"])
                m = np.asarray(lay["m"], np.float64)
                minv = np.linalg.inv(m)
                if m[2, 0] == 0 and m[2, 1] == 0:
                    minv = minv / minv[2, 2]
                    minv[2] = (0.0, 0.0, 1.0)
                for k, v in enumerate(minv.reshape(-1)):
                    L.minv[k] = float(v)
                paste = list(lay.get("paste") or [])
                if len(paste) > AUG_MAX_PASTE:
                    raise ValueError(f"a layer pastes at most {AUG_MAX_PASTE} polygons, got {len(paste)}")
                L.poly_first, L.poly_count = len(polys), len(paste)
                for q in paste:
                    q = np.asarray(q, np.float32).reshape(-1, 2)
                    polys.append((nv, len(q), int(math.floor(q[:, 0].min())), int(math.floor(q[:, 1].min())),
                                  int(math.ceil(q[:, 0].max())), int(math.ceil(q[:, 1].max()))))
                    verts.append(q)
                    nv += len(q)
        parr = (AugPoly * max(len(polys), 1))(*[AugPoly(*t) for t in polys])
        varr = np.ascontiguousarray(np.concatenate(verts) if verts else np.zeros((0, 2), np.float32), np.float32)
        return arr, parr, len(polys), varr

    def render_ex(self, plans: List[dict]) -> torch.Tensor:
        """One m355_augment_ex launch: uint8 (B,H,W,3) on the device."""
        H, W = self.ds.imgsz
        B = len(plans)
        arr, parr, n_polys, varr = self.ex_tables(plans)
        need = int(lib.m355_augment_ex_workspace_bytes(B, n_polys, len(varr)))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(max(need, 4096), dtype=torch.uint8, device=self.dev)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=self.dev)
        if self._copied is not None:                                 # the entry's contract: the previous call's host tables live
            self._copied.synchronize()                               # until the stream has passed its copies
        self._host = (arr, parr, varr)
        self.launches["m355_augment_ex"] += 1
        check(lib.m355_augment_ex(C.c_void_p(self.cache.data_ptr()), len(self.ds), arr, parr if n_polys else None, n_polys,
                                  varr.ctypes.data_as(C.POINTER(C.c_float)) if len(varr) else None, len(varr),
                                  C.c_void_p(self._work.data_ptr()), self._work.numel(), C.c_void_p(out.data_ptr()), B, H, W,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self._copied = torch.cuda.Event()
        self._copied.record()
        return out

    def batch(self, indices: Sequence[int], mosaic_on: bool = True, with_masks: bool = True) -> Dict:
        """Like SegDataset.batch (``with_masks`` included), with `img` already on the device."""
        H, W = self.ds.imgsz
        plans = self.plan(indices, mosaic_on)
        imgs = self.render(plans)
        bidx, cls, boxes = [], [], []
        masks = np.zeros((len(plans), H // 4, W // 4) if with_masks else (0,), np.uint8)
        if with_masks and any(len(p["inst"]) > 255 for p in plans):  # (a mosaic of four crowded images)
            masks = masks.astype(np.int32)
        for b, p in enumerate(plans):
            polys = [q for _, q in p["inst"]]
            if not polys:
                continue
            if with_masks:
                masks[b], order = overlap_mask(polys, (H, W))
            else:
                order = range(len(polys))
            for j in order:
                q = polys[j]
                x1, y1, x2, y2 = q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()
                bidx.append(b)
                cls.append(p["inst"][j][0])
                boxes.append([(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H])
        out = {"img": imgs, "batch_idx": np.asarray(bidx, np.float32), "cls": np.asarray(cls, np.float32),
               "bboxes": np.asarray(boxes, np.float32).reshape(-1, 4), "plans": plans}
        if with_masks:
            out["masks"] = masks
        return out
