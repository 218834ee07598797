"""Python host wrapper of the libmi355yolo engine (PyTorch-ROCm tensors as device memory / streams).

Stands where ``ultralytics.nn.tasks.SegmentationModel`` + ``SegmentationPredictor.postprocess`` stand
upstream (call site /root/reference/BscanBased/yolo8_seg_predict.py:8): the
arithmetic is in the HIP kernels behind the C-ABI, this file only owns buffers and argument plumbing.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import ConvInfo, LetterboxImage, ModelDesc, OpInfo, check, lib
from .preprocess import scale_boxes_to_original
from .spec import V9C, ConvSpec, conv_specs, fold_bn, is_detect, is_v5u, is_v8det, is_y11


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def scale_code(scale: str) -> int:
    """m355_model_desc.scale of a scale tag: 'n'..'x' (yolov8-seg), 'c' (yolov9c-seg), ('5' << 8) | n/s/m (YOLOv5u),
    ('1' << 8) | n/s/m (YOLO11), ('8' << 8) | n/s/m/l/x (YOLOv8 detect)."""
    if scale == V9C:
        return ord("c")
    if is_v5u(scale):
        return (ord("5") << 8) | ord(scale[1])
    if is_y11(scale):
        return (ord("1") << 8) | ord(scale[2])
    if is_v8det(scale):
        return (ord("8") << 8) | ord(scale[1])
    return ord(scale)


class SegEngine:
    """One engine per device.  Not thread-safe (one handle, one caller).  Serves the segmentation graphs (nm = 32 mask
    coefficients, prototypes) and the YOLOv5u, YOLO11 and YOLOv8 detection graphs (nm = 0: no prototypes, no masks)."""

    def __init__(self, scale: str = "s", nc: int = 1, imgsz: Tuple[int, int] = (640, 640),
                 max_batch: int = 32, device: int = 0, keep_raw: bool = True):
        """keep_raw: also write the raw head maps (`raw_head()`); the predict path and bench.py pass False — the head
        output convs decode their rows in their own epilogue and the raw maps are a parity / debugging output."""
        if not torch.cuda.is_available():
            raise RuntimeError("libmi355yolo needs a gfx950 GPU; there is no CPU fallback")
        self.device = torch.device("cuda", device)
        self.scale, self.nc, self.imgsz, self.max_batch = scale, nc, tuple(imgsz), max_batch
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            desc = ModelDesc(scale_code(scale), nc, imgsz[0], imgsz[1], max_batch)
            check(lib.m355_create(C.byref(desc), C.byref(self._h)))
            check(lib.m355_set_keep_raw(self._h, int(keep_raw)), self._h)
        self.num_anchors = lib.m355_num_anchors(self._h)
        self.pred_width = lib.m355_pred_width(self._h)
        ph, pw = C.c_int(), C.c_int()
        check(lib.m355_proto_hw(self._h, C.byref(ph), C.byref(pw)), self._h)
        self.proto_hw = (ph.value, pw.value)
        self.nm = self.pred_width - 4 - nc      # 32 mask coefficients, or 0 for a detection graph
        self.flops_per_image = lib.m355_flops_per_image(self._h)
        self.workspace_bytes = lib.m355_workspace_bytes(self._h)
        self.specs: List[ConvSpec] = conv_specs(scale, nc)
        self._check_graph()
        self._lb_host: Optional[torch.Tensor] = None     # pinned staging of letterbox(): the raw sources, one after the other
        self._lb_dev: Optional[torch.Tensor] = None      # its device copy
        self._lb_copied: Optional[torch.cuda.Event] = None   # the last upload has left the staging buffer
        self._lb_done: Optional[torch.cuda.Event] = None     # the last kernel has read the device copy

    @staticmethod
    def proto_is_composed(scale: str) -> bool:
        """True when the engine runs Proto's ConvTranspose + 3x3 conv as four composed 2x2 phase convolutions
        (graph.hip build_segment_head: prototype width a multiple of 64 and M355_NO_PROTOFUSE unset)."""
        import math
        import os
        from .spec import SCALES
        if scale == V9C:
            return "M355_NO_PROTOFUSE" not in os.environ      # 256 prototype channels
        if is_detect(scale):
            return False                                      # no Proto at all
        _, width, maxc = SCALES[scale]
        npr = int(math.ceil(min(256, maxc) * width / 8) * 8)
        return npr % 64 == 0 and "M355_NO_PROTOFUSE" not in os.environ

    # ------------------------------------------------------------------ graph / weights
    def conv_infos(self) -> List[ConvInfo]:
        out = []
        for i in range(lib.m355_num_convs(self._h)):
            ci = ConvInfo()
            check(lib.m355_get_conv_info(self._h, i, C.byref(ci)), self._h)
            out.append(ci)
        return out

    def _check_graph(self) -> None:
        infos = self.conv_infos()
        if len(infos) != len(self.specs):
            raise RuntimeError(f"engine reports {len(infos)} convs, host spec has {len(self.specs)}")
        for ci, s in zip(infos, self.specs):
            got = (ci.name.decode(), ci.cin, ci.cout, ci.k, ci.stride, bool(ci.has_bn), bool(ci.transposed), ci.groups)
            want = (s.name, s.cin, s.cout, s.k, s.stride, s.has_bn, s.transposed, s.groups)
            if got != want:
                raise RuntimeError(f"engine/host graph mismatch: {got} vs {want}")

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Fold BN on the host (A4) and hand fp32 weights to the engine, which packs them to fp16."""
        with torch.cuda.device(self.device):
            for i, s in enumerate(self.specs):
                w, b = fold_bn(sd, s)
                if tuple(w.shape) != s.weight_shape or b.numel() != s.cout:
                    raise ValueError(f"{s.name}: weight shape {tuple(w.shape)} != {s.weight_shape}")
                check(lib.m355_set_conv_weights(self._h, i, _ptr(w), _ptr(b)), self._h)

    # ------------------------------------------------------------------ forward / postprocess
    def letterbox(self, images: Sequence[np.ndarray], plan) -> torch.Tensor:
        """LetterBox on the device.  images: uint8 (h, w, 3) BGR arrays of any sizes; plan: what
        ``preprocess.letterbox_plan`` returned for their shapes (any net shape, not only this engine's).  Returns the uint8
        (n, net_h, net_w, 3) RGB batch ``forward`` takes, bit-identical to ``preprocess.letterbox`` of each image with the
        channels reversed.  The sources are packed into one pinned staging buffer and uploaded with one copy; staging and
        device buffer are kept and grown.  Asynchronous on the current stream; the images are only read."""
        table, (net_h, net_w) = plan
        n = len(images)
        if n < 1 or len(table) != n:
            raise ValueError(f"{n} images for a plan of {len(table)}")
        rows = (LetterboxImage * n)()
        srcs, total = [], 0
        for i, (im, (h, w, uh, uw, top, left)) in enumerate(zip(images, np.asarray(table).tolist())):
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.shape != (h, w, 3):
                raise ValueError(f"image {i}: expected a uint8 ndarray of shape {(h, w, 3)}")
            rows[i] = LetterboxImage(total, h, w, uh, uw, top, left)
            srcs.append(im)
            total += im.size
        with torch.cuda.device(self.device):
            if self._lb_host is None or self._lb_host.numel() < total:
                cap = (total + (1 << 22) - 1) >> 22 << 22
                if self._lb_done is not None:
                    self._lb_done.synchronize()          # nothing in flight reads the buffers that are let go
                self._lb_host = torch.empty((cap,), dtype=torch.uint8, pin_memory=True)
                self._lb_dev = torch.empty((cap,), dtype=torch.uint8, device=self.device)
                self._lb_copied, self._lb_done = torch.cuda.Event(), torch.cuda.Event()
            else:
                self._lb_copied.synchronize()            # the previous upload has read the staging buffer
                torch.cuda.current_stream().wait_event(self._lb_done)
            host = self._lb_host.numpy()
            for r, im in zip(rows, srcs):
                np.copyto(host[r.offset:r.offset + im.size].reshape(im.shape), im)
            self._lb_dev[:total].copy_(self._lb_host[:total], non_blocking=True)
            self._lb_copied.record()
            out = torch.empty((n, net_h, net_w, 3), dtype=torch.uint8, device=self.device)
            check(lib.m355_letterbox_u8(_ptr(self._lb_dev), rows, n, net_h, net_w, _ptr(out), _stream()))
            self._lb_done.record()
        return out

    def forward(self, images_u8_nhwc: torch.Tensor):
        """images: uint8 (B,H,W,3) on this device.  Returns preds f32 (B,A,4+nc+nm), protos f16 (B,h,w,32) (None when nm = 0)."""
        x = images_u8_nhwc
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or tuple(x.shape[1:3]) != self.imgsz:
            raise ValueError(f"expected uint8 (B,{self.imgsz[0]},{self.imgsz[1]},3), got {x.dtype} {tuple(x.shape)}")
        if not x.is_cuda or not x.is_contiguous():
            raise ValueError("input must be a contiguous CUDA tensor")
        B = x.shape[0]
        preds = torch.empty((B, self.num_anchors, self.pred_width), dtype=torch.float32, device=x.device)
        protos = None
        if self.nm:
            protos = torch.empty((B, self.proto_hw[0], self.proto_hw[1], self.nm), dtype=torch.float16, device=x.device)
        check(lib.m355_forward(self._h, _ptr(x), B, _ptr(preds), _ptr(protos), _stream()), self._h)
        return preds, protos

    def raw_head(self, batch: int) -> torch.Tensor:
        """Copy of the raw head maps (B,A,64+nc+32) f32 of the last forward (A13 layout)."""
        p, w = C.c_void_p(), C.c_int()
        check(lib.m355_get_raw_head(self._h, C.byref(p), C.byref(w)), self._h)
        out = torch.empty((batch, self.num_anchors, w.value), dtype=torch.float32, device=self.device)
        check(lib.m355_copy_raw_head(self._h, batch, _ptr(out), _stream()), self._h)
        return out

    def postprocess(self, preds: torch.Tensor, protos: Optional[torch.Tensor], conf: float = 0.25,
                    iou: float = 0.7, max_det: int = 300, masks: bool = True, multi_label: bool = False, max_nms: int = 30000,
                    agnostic: bool = False, classes=None):
        """Batched NMS + mask assembly.  Returns dets f32 (B,max_det,6+nm), counts i32 (B),
        masks u8 (B,max_det,H,W) or None (always None for a detection graph).  Only rows < counts[b] are defined.
        ``multi_label`` (upstream's validator mode, nc > 1): every (anchor, class) pair above ``conf`` is a candidate.
        ``agnostic``: class-agnostic NMS.  ``classes`` (an int or a sequence of them, upstream's predict argument): keep only
        anchors whose argmax class is one of them (ids outside [0, nc) match nothing; an empty sequence keeps nothing)."""
        masks = masks and self.nm > 0
        if multi_label and (agnostic or classes is not None):
            raise ValueError("agnostic / classes are options of the predict NMS; the multi-label validator NMS does not take them")
        if multi_label and self.nc > 1:
            return self._postprocess_multilabel(preds, protos, conf, iou, max_det, masks, max_nms)
        B = preds.shape[0]
        dets = torch.empty((B, max_det, 6 + self.nm), dtype=torch.float32, device=preds.device)
        counts = torch.empty((B,), dtype=torch.int32, device=preds.device)
        m = None
        if masks:
            m = torch.empty((B, max_det, self.imgsz[0], self.imgsz[1]), dtype=torch.uint8, device=preds.device)
        if not agnostic and classes is None:
            check(lib.m355_postprocess(self._h, _ptr(preds), _ptr(protos), B, conf, iou, max_det, _ptr(dets),
                                       _ptr(counts), _ptr(m), _stream()), self._h)
        else:
            cmask = class_mask(classes, self.nc, preds.device)
            check(lib.m355_postprocess_ex(self._h, _ptr(preds), _ptr(protos), B, conf, iou, max_det, int(bool(agnostic)),
                                          _ptr(cmask), _ptr(dets), _ptr(counts), _ptr(m), _stream()), self._h)
        return dets, counts, m

    def postprocess_native(self, preds: torch.Tensor, protos: torch.Tensor, orig_shapes: Sequence[Tuple[int, int]],
                           conf: float = 0.25, iou: float = 0.7, max_det: int = 300, agnostic: bool = False, classes=None):
        """NMS, then every detection's mask at its image's ORIGINAL resolution (upstream ``process_mask_native``, what
        predict(retina_masks=True) returns).  ``orig_shapes``: (h0, w0) of each image, letterboxed to this engine's imgsz.
        Returns (dets f32 (B,max_det,38) on the device, counts (list of int), boxes (per image f32 ndarray (n,4) in original
        pixels: ``scale_boxes_to_original`` of the rows, the boxes Results reports and the masks are cropped to), masks (per
        image uint8 (n,h0,w0) device tensors, views of one buffer of sum n*h0*w0 bytes allocated once the counts are known))."""
        if self.nm == 0:
            raise ValueError("a detection engine has no masks")
        B = preds.shape[0]
        shapes = [(int(h), int(w)) for h, w in orig_shapes]
        if len(shapes) != B:
            raise ValueError(f"{len(shapes)} original shapes for a batch of {B}")
        dets, counts, _ = self.postprocess(preds, protos, conf, iou, max_det, masks=False, agnostic=agnostic, classes=classes)
        counts_h = counts.cpu().tolist()
        rows = dets[..., :4].cpu().numpy()
        boxes = np.zeros((B, max_det, 4), np.float32)
        out_boxes = []
        for b, n in enumerate(counts_h):
            bx = scale_boxes_to_original(rows[b, :n], self.imgsz, shapes[b])
            boxes[b, :n] = bx
            out_boxes.append(bx)
        offsets = np.zeros(B + 1, np.int64)
        offsets[1:] = np.cumsum([n * h * w for n, (h, w) in zip(counts_h, shapes)])
        hw = np.ascontiguousarray(np.asarray(shapes, np.int32).reshape(B, 2))
        buf = torch.empty((int(offsets[-1]),), dtype=torch.uint8, device=preds.device)
        d_boxes = torch.from_numpy(boxes).to(preds.device)
        check(lib.m355_proto_masks_native(_ptr(dets), _ptr(counts), _ptr(protos), B, max_det, self.proto_hw[0],
                                          self.proto_hw[1], hw.ctypes.data_as(C.c_void_p), _ptr(d_boxes),
                                          offsets.ctypes.data_as(C.c_void_p), _ptr(buf) if buf.numel() else None, _stream()))
        masks = [buf[int(offsets[b]):int(offsets[b + 1])].view(counts_h[b], *shapes[b]) for b in range(B)]
        return dets, counts_h, out_boxes, masks

    def _postprocess_multilabel(self, preds, protos, conf, iou, max_det, masks, max_nms):
        """upstream's ``non_max_suppression(multi_label=True)``: class offsets make the classes independent, so it is one
        single-class NMS launch per class (the kernel and its bit-exact IoU arithmetic unchanged), the per-class survivors
        merged in score order and cut at ``max_det``.  ``max_nms``: scores below an image's max_nms-th largest candidate
        are masked out first (upstream keeps the top ``max_nms`` candidates of an image before the NMS)."""
        B, A, _ = preds.shape
        nc, nm = self.nc, self.nm
        sc = preds[..., 4:4 + nc]
        if A * nc > max_nms:
            kth = sc.reshape(B, A * nc).topk(max_nms, dim=1).values[:, -1]                    # (B,)
            sc = torch.where(sc >= kth[:, None, None], sc, torch.zeros_like(sc))
        all_d, all_valid = [], []
        for c in range(nc):
            pc = torch.cat((preds[..., :4], sc[..., c:c + 1], preds[..., 4 + nc:]), -1).contiguous()
            d = torch.empty((B, max_det, 6 + nm), dtype=torch.float32, device=preds.device)
            n = torch.empty((B,), dtype=torch.int32, device=preds.device)
            check(lib.m355_nms(_ptr(pc), B, A, 1, nm, conf, iou, max_det, _ptr(d), _ptr(n), _stream()))
            d[..., 5] = float(c)
            all_d.append(d)
            all_valid.append(torch.arange(max_det, device=preds.device)[None, :] < n[:, None])
        d = torch.cat(all_d, 1)                                                              # (B, nc * max_det, 6 + nm)
        valid = torch.cat(all_valid, 1)
        key = torch.where(valid, d[..., 4], torch.full_like(d[..., 4], -1.0))
        order = key.argsort(dim=1, descending=True, stable=True)[:, :max_det]
        dets = d.gather(1, order[..., None].expand(B, max_det, 6 + nm)).contiguous()
        counts = valid.sum(1).clamp_max(max_det).to(torch.int32)
        m = None
        if masks:
            m = torch.empty((B, max_det, self.imgsz[0], self.imgsz[1]), dtype=torch.uint8, device=preds.device)
            check(lib.m355_proto_masks(_ptr(dets), _ptr(counts), _ptr(protos), B, max_det, self.proto_hw[0], self.proto_hw[1],
                                       self.imgsz[0], self.imgsz[1], _ptr(m), _stream()))
        return dets, counts, m

    # ------------------------------------------------------------------ measurement hooks
    def op_infos(self) -> List[dict]:
        out = []
        for i in range(lib.m355_num_ops(self._h)):
            oi = OpInfo()
            check(lib.m355_get_op_info(self._h, i, C.byref(oi)), self._h)
            out.append(dict(kernel=oi.kernel.decode(), layer=oi.layer.decode(), flops=oi.flops_per_image,
                            bytes=oi.bytes_per_image, weight_bytes=oi.weight_bytes))
        return out

    def set_profiling(self, enable: bool) -> None:
        check(lib.m355_set_profiling(self._h, int(enable)), self._h)

    def collect_op_times(self):
        """Per-op (sum of milliseconds, launches) since profiling was enabled (HIP events on the launch stream)."""
        n = lib.m355_num_ops(self._h)
        ms = (C.c_double * n)()
        cnt = (C.c_long * n)()
        check(lib.m355_collect_op_times(self._h, ms, cnt), self._h)
        return list(ms), list(cnt)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.m355_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def class_mask(classes, nc: int, device) -> Optional[torch.Tensor]:
    """Device bitmask (ceil(nc/32) words, bit c % 32 of word c // 32) of a ``classes`` argument: None (every class), an int
    or a sequence of ints.  Ids outside [0, nc) set no bit."""
    if classes is None:
        return None
    ids = [classes] if isinstance(classes, (int, np.integer)) or (torch.is_tensor(classes) and classes.dim() == 0) \
        else list(classes)
    words = np.zeros((nc + 31) // 32, np.uint32)
    for c in ids:
        c = int(c)
        if 0 <= c < nc:
            words[c >> 5] |= np.uint32(1 << (c & 31))
    return torch.from_numpy(words.view(np.int32)).to(device)


def version() -> str:
    return _capi.version()
