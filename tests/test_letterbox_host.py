"""Host side of the device letterbox: ``preprocess.letterbox_plan`` is ``letterbox_shape`` in table form, and
``m355_letterbox_u8`` is declared, exported, bound, and refuses every bad argument before any HIP call (so the refusals are
checked here, without a GPU, with a device pointer that is never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source shape, imgsz, auto)
CASES = [
    ((320, 320), (640, 640), True),       # the reference's case: a 320x320 B-scan at the default imgsz
    ((320, 320), (640, 640), False),
    ((1080, 1920), (640, 640), True),     # min-rectangle: 384 x 640
    ((1080, 1920), (640, 640), False),
    ((333, 517), (640, 640), True),       # odd sizes
    ((333, 517), (640, 640), False),
    ((1920, 1080), (640, 640), True),     # portrait
    ((517, 333), (320, 640), False),
    ((640, 640), (640, 640), True),       # already net-sized
    ((384, 640), (640, 640), True),
    ((100, 150), (640, 640), True),       # up-scale by a non-integer factor
    ((1, 320), (640, 640), False),
    ((320, 1), (640, 640), False),
]


@pytest.mark.parametrize("shape,imgsz,auto", CASES)
def test_plan_equals_letterbox_shape(shape, imgsz, auto):
    from defectdetection_viaobjectdetection_amd.preprocess import letterbox_plan, letterbox_shape
    table, net = letterbox_plan([shape], imgsz, auto)
    _, (uh, uw), (top, bottom, left, right), out = letterbox_shape(shape, imgsz, auto)
    assert table.dtype == np.int32 and table.shape == (1, 6)
    assert table[0].tolist() == [shape[0], shape[1], uh, uw, top, left]
    assert net == tuple(out) == (uh + top + bottom, uw + left + right)
    assert net[0] % 32 == 0 and net[1] % 32 == 0
    if not auto:
        assert net == imgsz


def test_plan_known_answers():
    from defectdetection_viaobjectdetection_amd.preprocess import letterbox_plan
    assert letterbox_plan([(1080, 1920)], (640, 640), True)[1] == (384, 640)
    t, net = letterbox_plan([(1080, 1920)], (640, 640), True)
    assert t[0].tolist() == [1080, 1920, 360, 640, 12, 0] and net == (384, 640)
    t, net = letterbox_plan([(320, 320)], (640, 640), True)
    assert t[0].tolist() == [320, 320, 640, 640, 0, 0] and net == (640, 640)


def test_plan_of_a_mixed_list():
    from defectdetection_viaobjectdetection_amd.preprocess import letterbox_plan, letterbox_shape
    shapes = [(320, 320), (1080, 1920), (333, 517), (1920, 1080), (640, 640), (1, 320)]
    table, net = letterbox_plan(shapes, (640, 640), False)
    assert net == (640, 640) and table.shape == (len(shapes), 6)
    for row, sh in zip(table.tolist(), shapes):
        _, (uh, uw), (top, _, left, _), out = letterbox_shape(sh, (640, 640), False)
        assert row == [sh[0], sh[1], uh, uw, top, left] and tuple(out) == net
    # the min-rectangle pad gives each shape a frame of its own: one batch cannot hold them
    with pytest.raises(ValueError):
        letterbox_plan(shapes, (640, 640), True)
    with pytest.raises(ValueError):
        letterbox_plan([], (640, 640), False)
    # 2000 x 1 at 640: the width rounds to 0 pixels (the host resize divides by it)
    with pytest.raises(ValueError):
        letterbox_plan([(2000, 1)], (640, 640), False)


def test_symbol_is_declared_exported_and_bound():
    from defectdetection_viaobjectdetection_amd import _capi
    header = open(os.path.join(ROOT, "include", "mi355yolo.h")).read()
    assert re.search(r"\bint\s+m355_letterbox_u8\s*\(", header) and "m355_letterbox_image" in header
    assert "m355_letterbox_u8" in _capi.SIGNATURES
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "m355_letterbox_u8")
    assert ctypes.sizeof(_capi.LetterboxImage) == 32   # int64 offset + six int32


def _call(rows, n=None, net=(640, 640), src=0x1000, out=0x2000, table=True):
    from defectdetection_viaobjectdetection_amd import _capi
    arr = (_capi.LetterboxImage * max(len(rows), 1))(*[_capi.LetterboxImage(*r) for r in rows])
    rc = _capi.lib.m355_letterbox_u8(ctypes.c_void_p(src), arr if table else None, len(rows) if n is None else n, net[0], net[1],
                                     ctypes.c_void_p(out), None)
    return rc, _capi.lib.m355_last_error(None)


def test_bad_arguments_are_refused_before_any_device_work():
    """The pointers are fake (never dereferenced): every refusal precedes the first HIP call, so it can be checked without a
    GPU.  A valid call is not made here -- it would launch."""
    ok = (0, 320, 320, 640, 640, 0, 0)            # offset, h, w, uh, uw, top, left
    second = (320 * 320 * 3, 100, 150, 427, 640, 106, 0)
    bad = {
        "null source": dict(rows=[ok], src=0),
        "null table": dict(rows=[ok], table=False),
        "null output": dict(rows=[ok], out=0),
        "n = 0": dict(rows=[ok], n=0),
        "n < 0": dict(rows=[ok], n=-3),
        "net_h not a multiple of 32": dict(rows=[ok], net=(650, 640)),
        "net_w not a multiple of 32": dict(rows=[ok], net=(640, 656)),
        "net_h = 0": dict(rows=[(0, 320, 320, 1, 1, 0, 0)], net=(0, 640)),
        "net_w < 0": dict(rows=[(0, 320, 320, 1, 1, 0, 0)], net=(640, -32)),
        "output not 16-byte aligned": dict(rows=[ok], out=0x2004),
        "h < 1": dict(rows=[(0, 0, 320, 640, 640, 0, 0)]),
        "w < 1": dict(rows=[(0, 320, -1, 640, 640, 0, 0)]),
        "uh < 1": dict(rows=[(0, 320, 320, 0, 640, 0, 0)]),
        "uw < 1": dict(rows=[(0, 320, 320, 640, 0, 0, 0)]),
        "window below the frame": dict(rows=[(0, 320, 320, 640, 640, 1, 0)]),
        "window right of the frame": dict(rows=[(0, 320, 320, 320, 320, 0, 321)]),
        "window taller than the frame": dict(rows=[(0, 320, 320, 672, 640, 0, 0)]),
        "negative top": dict(rows=[(0, 320, 320, 320, 320, -1, 0)]),
        "negative left": dict(rows=[(0, 320, 320, 320, 320, 0, -1)]),
        "negative offset": dict(rows=[(-1, 320, 320, 640, 640, 0, 0)]),
        "overlapping offsets": dict(rows=[ok, (320 * 320 * 3 - 1,) + second[1:]]),
        "misordered offsets": dict(rows=[(second[0] + 100 * 150 * 3,) + ok[1:], (0,) + second[1:]]),
        "bad second image": dict(rows=[ok, second[:3] + (0, 640, 106, 0)]),
    }
    for what, kw in bad.items():
        rc, err = _call(**kw)
        assert rc == -1, (what, rc)
        assert b"letterbox" in err, (what, err)
