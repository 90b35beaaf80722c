"""bench.py's two kinds of run (-m gpu), each a child process on a small shape.  A plain run prints the headline fields and nothing that
needs a pass of its own; `--full` adds the reference parity, the roofline and per-kernel times, the one-stream and other-precision
sub-records (inference) and the gradient parity (fine-tune step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernel_ms_per_step", "one_stream", "parity", "parity_mode", "parity_mode_bf16x3", "bf16_mode",
             "gradient_parity", "cpu_baseline", "configs")


def bench_line(*args):
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    for k in HEADLINE:
        assert k in d, k
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    return d


def test_plain_inference_run_is_lean(cuda, tmp_path):
    d = bench_line("--blocks", "3", "--batch", "8", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["outputs_valid"] is True and d["config"]["streams"] == 2
    assert [k for k in FULL_ONLY if k in d] == []
    assert set(d["dump_outputs"]["arrays"]) == {"logp", "argmax"}
    assert np.load(tmp_path / "logp.npy").shape[0] == 8 * 3600 and np.load(tmp_path / "argmax.npy").shape == (8 * 3600,)


def test_full_inference_run_carries_the_extra_records(cuda):
    d = bench_line("--blocks", "3", "--batch", "8", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert d["outputs_valid"] is True
    assert d["roofline"]["launches_timed"] > 0 and d["roofline"]["achieved"] > 0
    assert d["kernel_ms_per_step"]["attention"] > 0
    assert d["one_stream"]["outputs_identical_to_two_streams"] is True
    assert d["parity"]["fixture"] == "g3_vits8_L3_r480" and d["parity"]["copies_identical"] is True
    for key in ("parity_mode", "parity_mode_bf16x3", "bf16_mode"):
        assert d[key]["value"] > 0 and d[key]["parity"]["fixture"] == "g3_vits8_L3_r480"
    assert "cpu_baseline" not in d and "configs" not in d      # --no-cpu-baseline; the other configs need the headline shape


def test_plain_finetune_run_is_lean(cuda):
    d = bench_line("--config", "finetune", "--batch", "2", "--steps", "2", "--warmup", "1")
    assert d["steps"] == 2 and np.isfinite(d["final_loss"])
    assert [k for k in FULL_ONLY if k in d] == []


def test_full_finetune_run_carries_the_extra_records(cuda):
    d = bench_line("--config", "finetune", "--batch", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert d["roofline"]["launches_timed"] > 0
    assert d["gradient_parity"]["tensors"] == 48
    assert d["cpu_baseline"] is None
