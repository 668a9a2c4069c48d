"""GPU: bench.py's plain run prints the headline line and nothing beyond it, `--dump-outputs` writes what its last
timed step computed (checked against the f64 oracle at the sampled positions), and `--full` adds the legs a plain
run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        *extra], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(ctx, oracle, tmp_path):
    import bench
    line = _bench("--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 7 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "single_queue" not in line and "device_copy_GBps" not in line["roofline"]
    y = np.load(tmp_path / "fir_out.npy")
    idx = np.load(tmp_path / "fir_out_index.npy")
    assert y.dtype == np.float32 and idx.dtype == np.float64 and y.shape == (idx.size, 2)
    assert y.nbytes + idx.nbytes <= 64 << 20
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < bench.STREAM
    # the last timed step is step warmup + steps - 1 = 8 of the rotation over 6 streams: stream 2 (seed 815 + 2)
    x = bench.synth_stream(815 + 2, bench.STREAM)
    truth = oracle.fir_direct_f64(bench.lowpass_taps(), x)[idx.astype(np.int64)]
    got = np.ascontiguousarray(y).view(np.complex64).reshape(-1)
    e = oracle.evm_db(got, truth)
    assert e <= -120.0, f"dumped FIR output EVM {e:.1f} dB"


def test_full_run_adds_its_legs(ctx):
    line = _bench("--full", "--no-cpu-baseline")
    assert line["steps"] == 7 and line["ms_per_step"] > 0
    assert line["single_queue"]["kernel_ms"] > 0
    for k in ("achieved_events", "device_copy_GBps", "per_dispatch_ms"):
        assert line["roofline"][k] > 0
