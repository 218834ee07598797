"""Parity of the HIP engine vs the CPU oracle across the configurations the reference / BASELINE.json name:
n / s / m scales, nc = 1 and 80 (multi-class NMS), imgsz 320 (what yolo_seg_train.py:15 uses) and non-square
inputs, batch sizes that do not fill a tile."""
import numpy as np
import pytest
import torch

from helpers import forward_and_postprocess_parity

pytestmark = pytest.mark.gpu


CASES = [
    # scale, nc, (h, w), batch
    ("n", 1, (640, 640), 3),
    ("m", 1, (640, 640), 2),
    ("s", 80, (320, 320), 5),
    ("n", 3, (320, 480), 1),
    ("s", 1, (320, 320), 7),
]


@pytest.mark.parametrize("scale,nc,shape,batch", CASES)
def test_forward_and_postprocess_parity(scale, nc, shape, batch, cuda_device):
    forward_and_postprocess_parity(scale, nc, shape, batch, cuda_device)
