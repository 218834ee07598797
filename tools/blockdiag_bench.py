"""Launch time of the block-diagonal head stage (csrc/conv3x3_planes.hip, block-diagonal single mode: cv2.l.1 + cv3.l.1 + cv4.l.1 of
a head level in one launch) through m355_conv3x3_blockdiag_fwd's diagnostic loop (M355_BNECK_REPS back-to-back launches), for the
launcher's own walk of the tiles (0) and the two it chooses from (1 single tiles, 2 whole slabs).
Usage: python tools/blockdiag_bench.py [batch] [H ...]        (default: 32 40 20)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from defectdetection_viaobjectdetection_amd import _capi  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
sizes = [int(v) for v in sys.argv[2:]] or [40, 20]
os.environ["M355_BNECK_REPS"] = "50"
WIDTHS = (64, 128, 32)
rng = np.random.default_rng(0)
ws = [rng.standard_normal((c, c, 3, 3)).astype(np.float32) * (2.0 / (9 * c)) ** 0.5 for c in WIDTHS]
bs = [rng.standard_normal(c).astype(np.float32) * 0.3 for c in WIDTHS]
widths = (C.c_int * 3)(*WIDTHS)
wp = (C.c_void_p * 3)(*[w.ctypes.data for w in ws])
bp = (C.c_void_p * 3)(*[b.ctypes.data for b in bs])
for H in sizes:
    x = torch.randn((B, H, H, 224), device="cuda").half()
    y = torch.empty_like(x)
    for walk in (0, 1, 2):
        sys.stderr.write(f"walk {walk}: ")
        sys.stderr.flush()
        _capi.check(_capi.lib.m355_conv3x3_blockdiag_fwd(C.c_void_p(x.data_ptr()), B, H, H, 224, 3, widths, widths, wp, bp,
                                                         C.c_void_p(y.data_ptr()), 224, walk, None))
