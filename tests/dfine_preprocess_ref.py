"""numpy restatement of what RTDetrImageProcessorPil computes with its defaults (resize, BILINEAR, aspect not preserved; rescale;
no normalise, no pad), written from the description of the filter, not from the package under test: test infrastructure.

Pillow's 8-bit BILINEAR resize is a separable, antialiased fixed-point filter.  Per axis, scale = in / out, fs = max(scale, 1),
support = fs; output index xx has center = (xx + 0.5) * scale, taps [xmin, xmax) = [max(int(center - support + 0.5), 0),
min(int(center + support + 0.5), in)), tap x the weight 1 - |(x + xmin - center + 0.5) / fs| where that is below 1 (else 0); the
weights are summed in tap order, each divided by the sum (float64), then turned into int(w * 2**22 + 0.5).  A pass computes
clip((2**21 + sum k * pixel) >> 22, 0, 255) into uint8; horizontal first, then vertical on the uint8 result; a pass whose sizes
are equal is skipped.  Very tall, thin inputs (in_h / in_w of 125 and more, measured) run vertical first in Pillow: `in_domain`
keeps to aspect ratios within 64 : 1, where this restatement is Pillow's bytes.
"""
import numpy as np
import torch

PRECISION_BITS = 22
MAX_ASPECT = 64


def axis_tables(in_size: int, out_size: int):
    """(xmin (out,) int32, counts (out,) int32, coefficients (out, ksize) int32, zero behind a row's count)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(np.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int32)
    counts = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        w = [0.0] * n
        total = 0.0
        for x in range(n):
            a = abs((x + lo - center + 0.5) / fs)
            w[x] = 1.0 - a if a < 1.0 else 0.0
            total += w[x]
        for x in range(n):
            v = w[x] / total if total != 0.0 else w[x]
            coef[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5)
        xmin[xx], counts[xx] = lo, n
    return xmin, counts, coef


def _pass(img: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    """one pass along `axis` (0 = vertical, 1 = horizontal) of a uint8 (h, w, c) image"""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    xmin, counts, coef = axis_tables(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        n = int(counts[xx])
        k = coef[xx, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (k * src[xmin[xx]:xmin[xx] + n]).sum(0)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear_u8(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """uint8 (h, w, 3) -> uint8 (out_h, out_w, 3): horizontal pass, uint8, vertical pass"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    return np.ascontiguousarray(_pass(_pass(img, out_w, 1), out_h, 0))


def rescale_table(rescale_factor: float = 1 / 255) -> np.ndarray:
    """the 256 fp32 values a byte can become: float32(float64(b) * rescale_factor)"""
    return (np.arange(256, dtype=np.float64) * rescale_factor).astype(np.float32)


def preprocess(images, out_h: int, out_w: int, rescale_factor: float = 1 / 255) -> np.ndarray:
    """list of uint8 (h, w, 3) arrays -> (T, 3, out_h, out_w) float32"""
    table = rescale_table(rescale_factor)
    return np.stack([table[resize_bilinear_u8(np.asarray(im), out_h, out_w)].transpose(2, 0, 1) for im in images])


def in_domain(in_h: int, in_w: int) -> bool:
    """the shapes whose pass order is known to be horizontal-first: aspect ratio within 64 : 1 either way"""
    return in_h >= 1 and in_w >= 1 and in_h <= MAX_ASPECT * in_w and in_w <= MAX_ASPECT * in_h


# ---- the cases both test files run: name -> (uint8 (h, w, 3) image, (out_h, out_w)) -------------------------------------------------
def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def cases():
    return {
        "upscale": (noise(17, 23, 1), (32, 48)),
        "downscale_27_taps": (noise(400, 200, 2), (32, 32)),               # more than 5 taps on both axes
        "height_equal": (noise(32, 100, 3), (32, 48)),                     # the vertical pass is skipped
        "width_equal": (noise(100, 48, 4), (32, 48)),                      # the horizontal pass is skipped
        "both_equal": (noise(32, 48, 5), (32, 48)),                        # only the rescale runs
        "one_pixel": (noise(1, 1, 6), (32, 32)),
        "row_not_16_bytes": (noise(37, 53, 7), (32, 48)),                  # 159-byte rows
        "all_0": (np.zeros((20, 30, 3), np.uint8), (32, 48)),
        "all_255": (np.full((50, 90, 3), 255, np.uint8), (32, 48)),         # the rounding term and the clip at the top
        "checkerboard_down": (_checkerboard(50, 90), (32, 48)),
        "checkerboard_up": (_checkerboard(9, 14), (32, 48)),
        "frame_480x700_to_640": (noise(480, 700, 8), (640, 640)),
    }


# ---- the bound processor's fall-backs, shared by the host and the GPU tests ----------------------------------------------------------
def same_feature(a, b):
    """two BatchFeatures (or their parts): same type, keys, dtypes, devices and bits"""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if hasattr(a, "keys"):
        return hasattr(b, "keys") and list(a.keys()) == list(b.keys()) and all(same_feature(a[k], b[k]) for k in a.keys())
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_feature(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def fallback_calls():
    """name -> (processor kwargs, call kwargs, images): every condition that must reach the original method"""
    from PIL import Image
    img = cases()["row_not_16_bytes"][0]
    pil = Image.fromarray(img)
    size = {"height": 32, "width": 48}
    annotation = {"image_id": 7, "annotations": [{"bbox": [3.0, 4.0, 20.0, 10.0], "category_id": 1, "area": 200.0, "iscrowd": 0, "id": 1}]}
    return {
        "annotations": ({"size": size}, {"annotations": [annotation], "return_tensors": "pt"}, [pil]),
        "do_normalize": ({"size": size, "do_normalize": True}, {"return_tensors": "pt"}, [pil]),
        "do_normalize_at_the_call": ({"size": size}, {"return_tensors": "pt", "do_normalize": True}, [pil]),
        "return_tensors_np": ({"size": size}, {"return_tensors": "np"}, [pil]),
        "resample_bicubic": ({"size": size, "resample": Image.BICUBIC}, {"return_tensors": "pt"}, [pil]),
        "do_pad": ({"size": size, "do_pad": True}, {"return_tensors": "pt"}, [pil]),
        "mode_L": ({"size": size}, {"return_tensors": "pt"}, [pil.convert("L")]),
        "float_array": ({"size": size}, {"return_tensors": "pt", "do_rescale": False}, [img.astype(np.float32) / 255]),
        "outside_the_domain": ({"size": {"height": 32, "width": 32}}, {"return_tensors": "pt"}, [np.zeros((200, 2, 3), np.uint8) + 9]),
    }
