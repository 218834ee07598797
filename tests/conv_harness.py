"""The guard-banded, per-element harness of the conv parity tests (a plain module: no fixtures, imports without a GPU).

A case is (B, H, W, cin, cout, k, stride, act, residual, fp32 output).  Its operands and its float64 reference come from
tests/conv_bound.py and are computed once per (case, seed key), shared by every tile id that runs the case, and never modified.
A launch reads x and the residual from between two bands of NaNs (a read outside them poisons the output) and writes into a
NaN-filled body between two bands of 0xA5 bytes (a write outside the body changes a byte; an element not written stays NaN).

judge() is the whole verdict of one accepted launch: finite, every element inside conv_bound's derived bound, the bands intact,
rel-L2 <= 1e-3, and a second launch with identical bits.
"""
import ctypes as C

import torch

import conv_bound as cb
import launch_ref as lr

GUARD = 4096            # bytes around the output
XGUARD = 32768          # fp16 NaNs around the input and the residual (more than a halo row of the widest case: 160 x 128 channels)
ERR_INVALID = -1        # M355_ERR_INVALID (include/mi355yolo.h)
REFUSED_TEXT = "conv launch failed: -1"

_REFS = {}


def out_hw(H, W, k, s):
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def reference(case, key=None, keep=True, hot=None):
    """(x, w, b, res, y64, tol) of a case.  `key` seeds the draw (default: the case itself).  `hot` is None or (name, mask): a
    (B, 1, H, W) bool mask of input pixels multiplied by 4 after the draw (the hot seams of tests/test_conv_seams_gpu.py), cached
    under its hashable name.  keep=False computes without caching (cases that run once and are large)."""
    ck = (case, case if key is None else key, None if hot is None else hot[0])
    if ck in _REFS:
        return _REFS[ck]
    B, H, W, cin, cout, k, s, act, use_res, f32 = case
    x, w, b, res = cb.draw_operands(ck[1], B, H, W, cin, cout, k, use_res, s)
    if hot is not None:
        x = torch.where(hot[1], x * 4, x)
    y64, z64, S = cb.conv_ref(x, w, b, k, s, act, res)
    tol = cb.conv_tol(y64, z64, S, cin * k * k, act, res, out_f32=f32)
    out = (x, w.contiguous(), b.contiguous(), res, y64, tol)
    if keep:
        _REFS[ck] = out
    return out


def banded_input(t_nchw, dev):
    """NHWC fp16 copy of t between two bands of XGUARD NaNs.  Returns (the allocation, the data pointer)."""
    flat = t_nchw.permute(0, 2, 3, 1).contiguous().to(torch.float16).reshape(-1)
    buf = torch.full((flat.numel() + 2 * XGUARD,), float("nan"), dtype=torch.float16)
    buf[XGUARD:XGUARD + flat.numel()] = flat
    d = buf.to(dev)
    return d, d.data_ptr() + 2 * XGUARD


def guarded_output(nbytes, dtype, dev):
    """A NaN-filled body of nbytes between two bands of GUARD bytes 0xA5.  Returns (the allocation, the body as a flat dtype view)."""
    raw = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    body = raw[GUARD:GUARD + nbytes].view(dtype)
    body.fill_(float("nan"))
    return raw, body


def guards_intact(raw, what):
    """Host copy of the body's bytes after asserting that no byte of either band changed."""
    h = raw.cpu()
    nbytes = h.numel() - 2 * GUARD
    assert bool((h[:GUARD] == 0xA5).all()) and bool((h[GUARD + nbytes:] == 0xA5).all()), f"{what}: a byte around the output changed"
    return h[GUARD:GUARD + nbytes]


def same_bits(a, b):
    """Two host tensors of one float dtype hold identical bits (NaN payloads included)."""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def launch(capi, case, tile, xp, rp, w, b, out_shape, dev):
    """One call of m355_conv2d_fwd into a fresh guard-banded, NaN-filled output.  Returns (rc, output (B, cout, Ho, Wo) on the host or
    None)."""
    B, H, W, cin, cout, k, s, act, use_res, f32 = case
    dt = torch.float32 if f32 else torch.float16
    n = B * out_shape[2] * out_shape[3] * cout
    raw, body = guarded_output(n * (4 if f32 else 2), dt, dev)
    rc = capi.lib.m355_conv2d_fwd(C.c_void_p(xp), B, H, W, cin, C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), cout, k, s, act,
                                  C.c_void_p(rp), C.c_void_p(body.data_ptr()), int(f32), tile,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = guards_intact(raw, f"tile {tile} {case}").view(dt)
    if rc != 0:
        assert bool(torch.isnan(got).all()), f"tile {tile} {case}: rc {rc} but the output was written"
        return rc, None
    return 0, got.reshape(B, out_shape[2], out_shape[3], cout).permute(0, 3, 1, 2)


def last_error(capi):
    return (capi.lib.m355_last_error(None) or b"").decode()


class NotLaunched(AssertionError):
    """m355_conv2d_fwd returned nonzero where the test lists only shapes its tile accepts (a refusal or a runtime error)."""


def judge(capi, case, tile, ops, dev, what=None):
    """The case through m355_conv2d_fwd on the forced tile, judged per element.  A nonzero rc fails.  Prints and returns
    (worst |err|/tol, its (image, channel, row, col), rel-L2)."""
    x, w, b, res, y64, tol = ops
    what = what or f"tile {tile} {case}"
    xd, xp = banded_input(x, dev)
    rd, rp = banded_input(res, dev) if res is not None else (None, 0)
    rc, got = launch(capi, case, tile, xp, rp, w, b, y64.shape, dev)
    if rc != 0:
        text = last_error(capi)
        e = NotLaunched(f"{what}: rc {rc}: {text!r}")
        e.refused = rc == ERR_INVALID and text == REFUSED_TEXT        # the launcher's predicate said no: nothing ran
        raise e
    worst, idx, bad = cb.worst_ratio(got, y64, tol)
    rel = cb.rel_l2(got, y64)
    print(f"{what}: accepted, worst |err|/tol {worst:.3f} at (image, channel, row, col) = {idx}, rel-L2 {rel:.2e}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (an element not written, or a read outside the input)"
    cb.check_elements(got, y64, tol, what)
    assert rel <= 1e-3, f"{what}: rel-L2 {rel}"
    rc2, got2 = launch(capi, case, tile, xp, rp, w, b, y64.shape, dev)
    assert rc2 == 0 and same_bits(got, got2), f"{what}: two runs differ"
    return worst, idx, rel


# ---- the other conv-family entries: any output between the same bands, judged with launch_ref.elem_bound
def judged_elementwise(got, ref, bound, what):
    """launch_ref.check_elementwise as an assertion: finite everywhere, no element beyond its bound.  Prints and returns the worst ratio."""
    ratio, rel, desc = lr.check_elementwise(got, ref, bound)
    print(f"{what}: worst |err|/bound {ratio:.3f}, rel-L2 {rel:.2e}; {desc}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (an element not written, or a read outside the input)"
    assert ratio <= 1.0, f"{what}: an element beyond its bound: {desc} (ratio {ratio:.3g})"
    return ratio
