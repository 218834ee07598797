"""Stamps live in the probe instance of a kernel (template parameter PROBE, csrc/device_prims.h), which a launcher starts only when a
stamp buffer or an ablation bit is set.  A stamped launch and a plain launch must compute the same bits, the stamped one must write
its stamp file, and the plain one must write none.

(a) the per-op entries in process: M355_STAMPS is read per call.
(b) the four engine-internal kernels (c2f_c32, conv3x3_s2c32, conv3x3_s2c64, proto_phase_wreg): their stamp switches have process
    lifetime, so one fresh child process runs the forward with the four set, and this process runs it with none.
No ablation bit is set anywhere: those runs are wrong by design and belong to the tools."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ != "__main__":
    import conv_harness as ch

    pytestmark = pytest.mark.gpu

CONV_STAMP_BYTES = (1 << 20) * 8          # m355_conv2d_fwd: a zeroed buffer of 2^20 uint64 (csrc/op_entries.hip)
SLAB_STAMP_BYTES = 256 * 4 * 8 * 2 * 8    # m355_bneck_pair_fwd, m355_conv3x3_blockdiag_fwd: 256 blocks x 4 waves x two records of 8 uint64

# rows of tests/test_ops_gpu.py::CONV_CASES (B, H, W, cin, cout, k, s, act, res, tile), one per kernel with a probe instance; the
# row-slab kernel through tile 33: the smallest stride-1 and stride-2 cases of tests/test_bneck_pair_gpu.py
CONV_ROWS = [
    ("conv_igemm 3x3", (2, 20, 20, 128, 128, 3, 1, 1, False, 1)),
    ("conv_igemm 1x1", (2, 20, 20, 64, 64, 1, 1, 0, False, 0)),
    ("halo 16", (2, 32, 32, 64, 64, 3, 1, 1, False, 16)),
    ("halo 17", (2, 32, 32, 128, 128, 3, 1, 1, True, 17)),
    ("halo 18", (2, 32, 32, 128, 128, 3, 1, 1, True, 18)),
    ("wide", (2, 32, 32, 128, 128, 3, 1, 1, True, 19)),
    ("slab", (2, 10, 10, 64, 64, 3, 1, 1, False, 25)),
    ("m32 27", (1, 8, 16, 64, 128, 3, 1, 1, False, 27)),
    ("m32 29", (1, 15, 30, 64, 72, 3, 1, 1, True, 29)),
    ("planes stride 1", (1, 13, 17, 128, 192, 3, 1, 1, True, 33)),
    ("planes stride 2", (1, 28, 44, 64, 192, 3, 2, 1, False, 33)),
]


def _h(a):
    return a.ctypes.data_as(C.c_void_p)


def _plain_stamped_plain(run, path, nbytes, what):
    """run() three times -- plain, with M355_STAMPS = path, plain again -- each returning a host tensor.  The three hold the same bits,
    the stamped call wrote `nbytes` with a non-zero record for block 0, the plain calls wrote nothing."""
    folder = os.path.dirname(path)
    assert "M355_STAMPS" not in os.environ
    first = run()
    assert os.listdir(folder) == [], f"{what}: a plain call wrote {os.listdir(folder)}"
    os.environ["M355_STAMPS"] = path
    try:
        stamped = run()
    finally:
        os.environ.pop("M355_STAMPS", None)
    assert os.listdir(folder) == [os.path.basename(path)]
    assert os.path.getsize(path) == nbytes, f"{what}: stamp file of {os.path.getsize(path)} bytes, the entry documents {nbytes}"
    rec = np.fromfile(path, dtype=np.uint64, count=8)
    assert rec.any(), f"{what}: the record of block 0 is zero"
    os.remove(path)
    last = run()
    assert os.listdir(folder) == [], f"{what}: a plain call after the stamped one wrote {os.listdir(folder)}"
    assert ch.same_bits(first, stamped), f"{what}: the stamped launch computed other bits"
    assert ch.same_bits(first, last), f"{what}: the plain launch after the stamped one computed other bits"
    assert bool(torch.isfinite(first).all()), f"{what}: non-finite output"


@pytest.mark.parametrize("name,row", CONV_ROWS, ids=[n for n, _ in CONV_ROWS])
def test_conv_entry_same_bits_stamped_and_plain(name, row, cuda_device, tmp_path):
    from defectdetection_viaobjectdetection_amd import _capi
    case, tile = row[:9] + (False,), row[9]
    x, w, b, res, y64, _ = ch.reference(case, key=row, keep=False)
    xd, xp = ch.banded_input(x, cuda_device)
    rd, rp = ch.banded_input(res, cuda_device) if res is not None else (None, 0)

    def run():
        rc, got = ch.launch(_capi, case, tile, xp, rp, w, b, y64.shape, cuda_device)     # (asserts the guard bands)
        assert rc == 0, f"{name}: rc {rc}: {ch.last_error(_capi)!r}"
        return got

    _plain_stamped_plain(run, str(tmp_path / "stamps.bin"), CONV_STAMP_BYTES, name)


def _guarded_call(cuda_device, n_out, call, what):
    """call(pointer of a NaN-filled fp16 body of n_out elements between guard bands) -> rc; returns the body on the host."""
    raw, body = ch.guarded_output(n_out * 2, torch.float16, cuda_device)
    rc = call(body.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}"
    return ch.guards_intact(raw, what).view(torch.float16).clone()


def test_bneck_pair_same_bits_stamped_and_plain(cuda_device, tmp_path):
    """The smallest pair case of tests/test_bneck_pair_gpu.py (its operands) through m355_bneck_pair_fwd."""
    from defectdetection_viaobjectdetection_amd import _capi
    B, H, W, Cc, shortcut = 1, 13, 37, 128, True
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cc)
    r16 = lambda t: t.half().float()
    x = (torch.randn((B, Cc, H, W), generator=g) * 0.8).half()
    wa = r16(torch.randn((Cc, Cc, 3, 3), generator=g) * (2.0 / (9 * Cc)) ** 0.5)
    wb = r16(torch.randn((Cc, Cc, 3, 3), generator=g) * (2.0 / (9 * Cc)) ** 0.5)
    ba, bb = (torch.randn(Cc, generator=g) * 0.3 for _ in range(2))
    arrs = [t.numpy().astype(np.float32).copy() for t in (wa, ba, wb, bb)]
    xd, xp = ch.banded_input(x.float(), cuda_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda yp: _capi.lib.m355_bneck_pair_fwd(C.c_void_p(xp), B, H, W, Cc, Cc, _h(arrs[0]), _h(arrs[1]), _h(arrs[2]), _h(arrs[3]),
                                                    int(shortcut), C.c_void_p(yp), Cc, st)
    _plain_stamped_plain(lambda: _guarded_call(cuda_device, B * H * W * Cc, call, "bneck pair"), str(tmp_path / "stamps.bin"),
                         SLAB_STAMP_BYTES, "bneck pair")


def test_blockdiag_same_bits_stamped_and_plain(cuda_device, tmp_path):
    """The smallest case of tests/test_planes_blockdiag_gpu.py (its operands) through m355_conv3x3_blockdiag_fwd."""
    from defectdetection_viaobjectdetection_amd import _capi
    widths_ = (64, 128, 32)
    B, H, W, walk = 2, 10, 13, 0
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    r16 = lambda t: t.half().float()
    Ct = sum(widths_)
    x = (torch.randn((B, Ct, H, W), generator=g) * 0.8).half()
    ws = [r16(torch.randn((c, c, 3, 3), generator=g) * (2.0 / (9 * c)) ** 0.5) for c in widths_]
    bs = [torch.randn(c, generator=g) * 0.3 for c in widths_]
    wn = [w.numpy().astype(np.float32).copy() for w in ws]
    bn = [b.numpy().astype(np.float32).copy() for b in bs]
    widths = (C.c_int * 3)(*widths_)
    wp = (C.c_void_p * 3)(*[w.ctypes.data for w in wn])
    bp = (C.c_void_p * 3)(*[b.ctypes.data for b in bn])
    xd, xp = ch.banded_input(x.float(), cuda_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda yp: _capi.lib.m355_conv3x3_blockdiag_fwd(C.c_void_p(xp), B, H, W, Ct, 3, widths, widths, wp, bp, C.c_void_p(yp), Ct, walk, st)
    _plain_stamped_plain(lambda: _guarded_call(cuda_device, B * H * W * Ct, call, "blockdiag"), str(tmp_path / "stamps.bin"),
                         SLAB_STAMP_BYTES, "blockdiag")


# ---- (b) the engine-internal kernels
# kernel label of the per-op record (what tools/op_table.py prints) -> the layer it must have taken, its stamp switch
ENGINE_KERNELS = {
    "c2f_c32<8x16px>": ("model.2.", "M355_C2F_STAMPS"),
    "conv3x3_s2c32<8x16px>+1x1": ("model.1", "M355_S2C32_STAMPS"),
    "conv3x3_s2c64<8x8px>+1x1": ("model.3", "M355_S2C64_STAMPS"),
    "proto_phase_wreg<8x16px>": ("model.22.proto", "M355_PROTOR_STAMPS"),
}


def _engine(size):
    """The s-seg engine at batch 1 with model.1 on the patch kernel itself: by default the stem joins that launch (conv_stem_c2.hip,
    a kernel without stamps), so the fusion pass is switched off for this engine (M355_NO_STEMFUSE, read at engine creation)."""
    from defectdetection_viaobjectdetection_amd.engine import SegEngine
    os.environ["M355_NO_STEMFUSE"] = "1"
    try:
        return SegEngine("s", 1, (size, size), max_batch=1)
    finally:
        os.environ.pop("M355_NO_STEMFUSE", None)


def _taken(eng):
    """Stamp switches of ENGINE_KERNELS whose kernel the plan took, for the layer named."""
    infos = eng.op_infos()
    return sorted(sw for k, (layer, sw) in ENGINE_KERNELS.items() if any(o["kernel"] == k and o["layer"].startswith(layer) for o in infos))


def _forward(eng, size, dev):
    from defectdetection_viaobjectdetection_amd.spec import synthetic_state_dict
    from defectdetection_viaobjectdetection_amd.synthetic import synthetic_bscans
    eng.load_state_dict(synthetic_state_dict("s", 1, seed=0))
    imgs = torch.from_numpy(synthetic_bscans(1, size, size, seed=6)).to(dev)
    _, protos = eng.forward(imgs)
    raw = eng.raw_head(1)
    torch.cuda.synchronize()
    return raw.cpu(), protos.cpu()


def _child(size, folder):
    """The forward in a process of its own, with the four stamp switches set by the parent."""
    sys.path.insert(0, ROOT)
    eng = _engine(size)
    assert _taken(eng) == sorted(sw for _, sw in ENGINE_KERNELS.values()), [(o["kernel"], o["layer"]) for o in eng.op_infos()]
    raw, protos = _forward(eng, size, torch.device("cuda", 0))
    eng.close()
    torch.save({"raw": raw, "protos": protos}, os.path.join(folder, "child.pt"))


def test_engine_kernels_same_bits_stamped_and_plain(cuda_device, tmp_path):
    every = sorted(sw for _, sw in ENGINE_KERNELS.values())
    # the smallest image size at which the plan takes all four: each needs its map to be a multiple of its tile, and model.3 joins
    # model.4.cv1 (the launch conv3x3_s2c64 takes) only where the tile heuristic gives its pixel count the 128-channel tile
    size, seen = None, {}
    for s in range(32, 2049, 32):
        eng = _engine(s)
        seen[s] = _taken(eng)
        eng.close()
        if seen[s] == every:
            size = s
            break
    assert size is not None, f"no image size up to 2048 routes model.1, model.2, model.3 and Proto to the four kernels: {seen}"
    print(f"image size {size}")
    env = dict(os.environ)
    for sw in every:
        assert sw not in env
        env[sw] = str(tmp_path / (sw + ".bin"))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), str(size), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    stamped = sorted(f for f in os.listdir(tmp_path) if f.endswith(".bin"))
    assert stamped == [sw + ".bin" for sw in every], stamped
    for f in stamped:
        rec = np.fromfile(str(tmp_path / f), dtype=np.uint64)
        assert rec.size >= 8 and rec[:8].any(), f"{f}: empty, or a zero record for wave 0 of block 0"
    child = torch.load(str(tmp_path / "child.pt"))
    eng = _engine(size)
    assert _taken(eng) == every       # a plan change fails here and does not pass vacuously
    raw, protos = _forward(eng, size, cuda_device)
    eng.close()
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".bin")) == stamped      # this process wrote none
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(protos.float()).all())
    assert ch.same_bits(raw, child["raw"]), "raw head output: the stamped forward computed other bits"
    assert ch.same_bits(protos, child["protos"]), "prototypes: the stamped forward computed other bits"


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
