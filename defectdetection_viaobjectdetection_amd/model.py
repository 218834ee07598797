"""``YOLO`` -- the model facade the reference scripts call, backed by the libmi355yolo engine.

Mirrors the surface of ``ultralytics.YOLO`` as exercised by the reference:
  ``YOLO("....yaml")`` / ``YOLO("....pt")``            /root/reference/BscanBased/yolo_seg_train.py:7-8,
                                                       yolo8_seg_predict.py:5
  ``model.predict(path, save=True)`` / ``model(path, conf=..)``   yolo8_seg_predict.py:8, yolo_detector.py:40
  ``model.names``                                      yolo_detector.py:51
  ``model.train(data=, epochs=, imgsz=, project=, name=, device=)``   yolo_seg_train.py:12-19
Nothing is ever downloaded: a model given by NAME that is not a local file raises a clear offline error.
All network arithmetic runs in the HIP kernels behind the C-ABI; there is no CPU fallback.
"""
from __future__ import annotations

import math
import os
import re
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .preprocess import expand_sources, letterbox, letterbox_plan, scale_boxes_to_original
from .results import Results
from .spec import SCALES, V9C, conv_specs, count_parameters, init_state_dict, is_detect, is_v8det, state_dict_keys

_YAML_RE = re.compile(r"^yolov8([nsmlx])?-seg\.ya?ml$")
_V8DET_RE = re.compile(r"^yolov8([nsmlx])?\.ya?ml$")
_V9C_RE = re.compile(r"^yolov9c-seg\.ya?ml$")
_V5U_RE = re.compile(r"^yolov5([nsmlx])u\.ya?ml$")
_Y11_RE = re.compile(r"^yolo11([nsmlx])\.ya?ml$")
CKPT_FORMAT = "mi355yolo-seg-v1"


class OfflineModelError(FileNotFoundError):
    pass


def _increment_dir(base: str) -> str:
    if not os.path.exists(base):
        return base
    i = 2
    while os.path.exists(f"{base}{i}"):
        i += 1
    return f"{base}{i}"


class YOLO:
    def __init__(self, model: str = "yolov8s-seg.yaml", task: Optional[str] = None, verbose: bool = False):
        self.task = "segment"
        self.ckpt_path: Optional[str] = None
        self.overrides: Dict = {}
        self._engines: Dict[Tuple[int, int, int], object] = {}
        self.train_args: Dict = {}
        name = os.path.basename(str(model))
        m = _YAML_RE.match(name)
        if m:
            self.scale = m.group(1) or "n"
            self.nc = 80
            self.names = {i: f"class{i}" for i in range(self.nc)}
            if os.path.isfile(model):
                self._read_yaml_overrides(model)
            self.state_dict = init_state_dict(self.scale, self.nc, seed=0)
        elif _V9C_RE.match(name):
            # the architecture the reference scripts literally name (/root/reference/BscanBased/yolo_seg_train.py:7)
            self.scale = V9C
            self.nc = 80
            self.names = {i: f"class{i}" for i in range(self.nc)}
            if os.path.isfile(model):
                self._read_yaml_overrides(model)
            self.state_dict = init_state_dict(self.scale, self.nc, seed=0)
        elif _V8DET_RE.match(name):
            # the detector the reference loads (signals/improved_multisignal/visualization/yolo_detector.py:20: yolov8n.pt)
            self.scale = "8" + (_V8DET_RE.match(name).group(1) or "n")
            self.task = "detect"
            self.nc = 80
            self.names = {i: f"class{i}" for i in range(self.nc)}
            if os.path.isfile(model):
                self._read_yaml_overrides(model)
            self.state_dict = init_state_dict(self.scale, self.nc, seed=0)
        elif _V5U_RE.match(name):
            # the detection family the reference retrains (/root/reference/BscanBased/yolo5s_retrain.py:6: yolov5su.pt)
            sc = _V5U_RE.match(name).group(1)
            if sc in "lx":
                raise NotImplementedError(f"'{name}': YOLOv5u scales l and x are not built (n, s and m are)")
            self.scale = "5" + sc
            self.task = "detect"
            self.nc = 80
            self.names = {i: f"class{i}" for i in range(self.nc)}
            if os.path.isfile(model):
                self._read_yaml_overrides(model)
            self.state_dict = init_state_dict(self.scale, self.nc, seed=0)
        elif _Y11_RE.match(name):
            # the detection family the reference trains (BscanBased/yolo/yolo_bbox_retrain.py: yolo11n)
            sc = _Y11_RE.match(name).group(1)
            if sc in "lx":
                raise NotImplementedError(f"'{name}': YOLO11 scales l and x are not built (n, s and m are)")
            self.scale = "11" + sc
            self.task = "detect"
            self.nc = 80
            self.names = {i: f"class{i}" for i in range(self.nc)}
            if os.path.isfile(model):
                self._read_yaml_overrides(model)
            self.state_dict = init_state_dict(self.scale, self.nc, seed=0)
        elif name.endswith((".yaml", ".yml")):
            raise NotImplementedError(
                f"architecture '{name}' is not built: this package implements the YOLOv8{{n,s,m,l,x}}-seg, YOLOv9c-seg, "
                "YOLOv8{n,s,m,l,x}, YOLOv5{n,s,m}u and YOLO11{n,s,m} (detection) graphs")
        elif name.endswith(".pt"):
            if not os.path.isfile(model):
                raise OfflineModelError(
                    f"'{model}' is not a local file.  Upstream would download weights by name; this build is offline "
                    "and never fetches.  Pass a path to a checkpoint written by this package (YOLO.save / .train).")
            self._load_checkpoint(model)
        else:
            raise ValueError(f"unsupported model specifier '{model}' (expected *.yaml or *.pt)")

    # ------------------------------------------------------------------ model state
    def _read_yaml_overrides(self, path: str) -> None:
        import yaml
        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
        if "nc" in cfg:
            self.set_classes(int(cfg["nc"]))

    def set_classes(self, nc: int, names: Optional[Dict[int, str]] = None) -> None:
        """Re-initialise the head for ``nc`` classes (what upstream does when data.yaml disagrees with the yaml)."""
        self.nc = nc
        self.names = dict(names) if names else {i: f"class{i}" for i in range(nc)}
        self.state_dict = init_state_dict(self.scale, nc, seed=0)
        self._drop_engines()

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        keys = state_dict_keys(self.scale, self.nc)
        missing = [k for k in keys if k not in sd]
        if missing:
            raise KeyError(f"state dict misses {len(missing)} keys, e.g. {missing[:3]}")
        for s in conv_specs(self.scale, self.nc):
            if s.rep:
                continue
            k = f"{s.name}.conv.weight" if s.has_bn else f"{s.name}.weight"
            if tuple(sd[k].shape) != s.weight_shape:
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != {s.weight_shape}")
        self.state_dict = {k: sd[k].detach().cpu().clone() for k in keys}
        self._drop_engines()

    def _load_checkpoint(self, path: str) -> None:
        import pickle
        ck = None
        try:
            ck = torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError:  # torch's weights-only loader met a class: not one of ours, maybe upstream's
            ck = None
        if not isinstance(ck, dict) or ck.get("format") != CKPT_FORMAT:
            # a checkpoint written by upstream Ultralytics: recover the tensors without its classes (upstream_ckpt.py)
            from .upstream_ckpt import load_upstream_checkpoint
            up = load_upstream_checkpoint(path)
            self.scale, self.nc, self.names = up["scale"], up["nc"], up["names"]
            self.train_args = up["train_args"]
            self.state_dict = up["state_dict"]
            self.ckpt_path = path
            self.task = "detect" if is_detect(self.scale) else "segment"
            return
        self.scale, self.nc = ck["scale"], int(ck["nc"])
        self.names = {int(k): v for k, v in ck["names"].items()}
        self.train_args = ck.get("train_args", {})
        self.state_dict = ck["model"]
        self.ckpt_path = path
        self.task = "detect" if is_detect(self.scale) else "segment"
        self._resume_state = ck.get("trainer")       # present in weights/last.pt: lets train(resume=True) continue

    def save(self, path: str, upstream: bool = False) -> str:
        """``upstream=True`` writes upstream Ultralytics' own checkpoint layout (a pickled ``SegmentationModel`` module
        graph, fp16, upstream_export.py) so that ``ultralytics.YOLO(path)`` of the real package can load it; the default
        is this package's plain state-dict format."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        if upstream:
            if is_detect(self.scale):
                raise NotImplementedError("upstream export of a detection model (YOLOv8, YOLOv5u, YOLO11) is not built")
            from .upstream_export import export_upstream_checkpoint
            return export_upstream_checkpoint(path, self.scale, self.nc, self.names, self.state_dict, self.train_args)
        torch.save({"format": CKPT_FORMAT, "scale": self.scale, "nc": self.nc, "names": self.names,
                    "train_args": self.train_args, "model": self.state_dict}, path)
        return path

    def info(self) -> Tuple[int, int]:
        n = count_parameters(self.state_dict)
        return len(conv_specs(self.scale, self.nc)), n

    def _drop_engines(self) -> None:
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def _engine(self, shape: Tuple[int, int], batch: int, device: int):
        from .engine import SegEngine  # loads libmi355yolo.so; raises loudly when it is missing
        key = (shape[0], shape[1], device)
        eng = self._engines.get(key)
        if eng is None or eng.max_batch < batch:
            if eng is not None:
                eng.close()
            eng = SegEngine(self.scale, self.nc, shape, max_batch=max(batch, 1), device=device, keep_raw=False)
            eng.load_state_dict(self.state_dict)
            self._engines[key] = eng
        return eng

    # ------------------------------------------------------------------ inference
    def predict(self, source=None, save: bool = False, imgsz=None, conf: float = 0.25, iou: float = 0.7,
                max_det: int = 300, device=0, verbose: bool = True, retina_masks: bool = False,
                project: Optional[str] = None, name: Optional[str] = None, batch: int = 32, classes=None,
                agnostic_nms: bool = False, **kwargs) -> List[Results]:
        """``retina_masks=True`` (segmentation models): masks at each image's original resolution (upstream
        ``process_mask_native``); a detection model accepts it and has no masks.  ``classes`` (int or sequence): keep only
        detections whose class is one of them.  ``agnostic_nms``: class-agnostic NMS."""
        if source is None:
            raise ValueError("source is required")
        retina = bool(retina_masks) and self.task == "segment"
        dev = int(device[0] if isinstance(device, (list, tuple)) else device)
        if imgsz is None:
            imgsz = self.train_args.get("imgsz", 640)  # D7: a checkpoint keeps its training size
        if isinstance(imgsz, int):
            imgsz = (imgsz, imgsz)
        imgsz = tuple(int(math.ceil(s / 32) * 32) for s in imgsz)
        t0 = time.perf_counter()
        imgs, paths = expand_sources(source)
        # auto=True (min-rectangle) letterbox like upstream's predictor for a single shape; mixed shapes pad to imgsz
        shapes = {im.shape[:2] for im in imgs}
        auto = len(shapes) == 1
        table, net_shape = letterbox_plan([im.shape[:2] for im in imgs], imgsz, auto)
        # the letterbox itself runs on the device (SegEngine.letterbox); M355_HOST_LETTERBOX=1 keeps the numpy one (the reference
        # the kernel is tested against), for A/B runs
        lb = [letterbox(im, imgsz, auto=auto) for im in imgs] if os.environ.get("M355_HOST_LETTERBOX") == "1" else None
        results: List[Results] = []
        save_dir = None
        if save:
            save_dir = _increment_dir(os.path.join(project or os.path.join("runs", self.task), name or "predict"))
            os.makedirs(save_dir, exist_ok=True)
        t_pre = (time.perf_counter() - t0) * 1e3 / len(imgs)
        for i0 in range(0, len(imgs), batch):
            chunk = imgs[i0:i0 + batch]
            eng = self._engine(net_shape, len(chunk), dev)
            with torch.cuda.device(eng.device):
                ta = time.perf_counter()
                if lb is None:
                    x = eng.letterbox(chunk, (table[i0:i0 + len(chunk)], net_shape))
                else:
                    x = torch.from_numpy(np.stack(lb[i0:i0 + len(chunk)])[:, :, :, ::-1].copy()).to(eng.device)  # BGR -> RGB, H2D
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                preds, protos = eng.forward(x)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if retina:
                    dets, counts_h, boxes_o, masks = eng.postprocess_native(
                        preds, protos, [im.shape[:2] for im in imgs[i0:i0 + len(chunk)]], conf, iou, max_det,
                        agnostic=agnostic_nms, classes=classes)
                    torch.cuda.synchronize()
                else:
                    dets, counts, masks = eng.postprocess(preds, protos, conf, iou, max_det, masks=True,
                                                          agnostic=agnostic_nms, classes=classes)
                    counts_h = None
                # the chunk's rows (and, where the host has not got them yet, its counts: exact in fp32) in one copy to the host
                rows_d = dets[:, :, :6].reshape(len(chunk), -1)
                if counts_h is None:
                    rows_d = torch.cat((rows_d, counts.to(torch.float32)[:, None]), 1)
                rows_h = rows_d.cpu().numpy()
                if counts_h is None:
                    counts_h = rows_h[:, -1].astype(np.int64).tolist()
                rows_h = rows_h[:, :max_det * 6].reshape(len(chunk), max_det, 6)
                t3 = time.perf_counter()
            for j, n in enumerate(counts_h):
                d = rows_h[j, :n].copy()
                orig = imgs[i0 + j]
                speed = {"preprocess": t_pre + (t1 - ta) * 1e3 / len(chunk), "inference": (t2 - t1) * 1e3 / len(chunk),
                         "postprocess": (t3 - t2) * 1e3 / len(chunk)}
                if retina:
                    # masks at the original resolution: Results sees a frame equal to the image (gain 1, pad 0)
                    d[:, :4] = boxes_o[j]
                    r = Results(orig, paths[i0 + j], self.names, torch.from_numpy(d), masks[j].cpu(), speed, orig.shape[:2])
                else:
                    d[:, :4] = scale_boxes_to_original(d[:, :4], net_shape, orig.shape[:2])
                    m = masks[j, :n].cpu() if masks is not None else None
                    r = Results(orig, paths[i0 + j], self.names, torch.from_numpy(d), m, speed, net_shape)
                if save_dir:
                    r.save_dir = save_dir
                    r.save(os.path.join(save_dir, os.path.splitext(os.path.basename(paths[i0 + j]))[0] + ".jpg"))
                if verbose:
                    print(f"image {i0 + j + 1}/{len(imgs)} {paths[i0 + j]}: {net_shape[0]}x{net_shape[1]} {r.verbose()}"
                          f"{speed['inference']:.1f}ms")
                results.append(r)
        if verbose and save_dir:
            print(f"Results saved to {save_dir}")
        return results

    __call__ = predict

    # ------------------------------------------------------------------ training
    def train(self, data: Optional[str] = None, epochs: int = 100, imgsz: int = 640, batch: int = 16,
              project: Optional[str] = None, name: Optional[str] = None, device=0, **kwargs):
        self._require_trainable("train")
        from .train import train as _train  # lazy: training pulls in the loss / dataset modules
        return _train(self, data=data, epochs=epochs, imgsz=imgsz, batch=batch, project=project, name=name,
                      device=device, **kwargs)

    def val(self, data: Optional[str] = None, imgsz: Optional[int] = None, batch: int = 16, device=0, **kwargs):
        self._require_trainable("val")
        from .train import validate as _validate
        return _validate(self, data=data, imgsz=imgsz, batch=batch, device=device, **kwargs)

    def _require_trainable(self, what: str) -> None:
        """The graphs TrainEngine builds: the segmentation families and YOLOv8 detect."""
        if self.task != "segment" and not is_v8det(self.scale):
            raise NotImplementedError(f"{what}() of a {self.task} model: detect training and validation (YOLOv5u, YOLO11) are not built "
                                      "yet; this package trains and validates the segmentation graphs and YOLOv8 detect only")
