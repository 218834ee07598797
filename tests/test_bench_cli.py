"""bench.py's command line: a plain run carries the headline figure alone, everything else it can measure sits behind
`--full`.  The option itself is checked on the host (`--help` ends before anything heavy is imported); the plain run's JSON
line on the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
BEHIND_FULL = ("roofline", "kernels", "c2f3x3", "forward_ms_per_step_events", "cpu_baseline", "train_step")


def test_full_is_an_option_and_off_by_default():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout
    with open(BENCH, encoding="utf-8") as f:
        text = f.read()
    assert 'add_argument("--full", action="store_true"' in text       # a flag: absent means off


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_nothing_behind_full(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1`: one JSON line with the headline keys, consistent with each other, none of
    the blocks that `--full` adds, and the five arrays of `--dump-outputs`."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    for key in HEADLINE:
        assert key in line, key
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "fp16"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = 32 images per step / the step period, both rounded (2 and 4 decimals) from the same elapsed time
    assert abs(line["value"] * line["ms_per_step"] / 32e3 - 1.0) < 1e-3
    assert not [k for k in BEHIND_FULL if k in line]
    assert sorted(os.listdir(tmp_path)) == ["counts.npy", "dets.npy", "masks.npy", "preds.npy", "protos.npy"]
