"""bench.py's plain run and `--dump-outputs`: the result line carries the headline only, and the files hold what the last
timed step computed (checked against the oracle on the one linear of the benchmark that holds synth weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_and_samples_large_arrays(tmp_path, monkeypatch):
    # importing bench sets a default for HSA_ENABLE_IPC_MODE_LEGACY; keep that out of this process's later tests
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    if "HSA_ENABLE_IPC_MODE_LEGACY" not in os.environ:
        monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY")
    import bench

    small = np.arange(12, dtype=np.float16).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / "a"), [("small", small)])
    got = np.load(tmp_path / "a" / "small.npy")
    assert got.dtype == np.float32 and got.shape == (3, 4) and np.array_equal(got, small.astype(np.float32))

    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 2 * 4 * 100)             # two arrays -> 100 elements each
    big = np.arange(1000, dtype=np.float64)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), [("big", big), ("small", small)])
    b, c = np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "c" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (100,) and np.array_equal(b, c)          # the same sample every time
    assert np.all(np.diff(b) >= 0) and set(b.tolist()) <= set(big.tolist())
    assert np.load(tmp_path / "b" / "small.npy").shape == (3, 4)


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_the_last_step(tmp_path):
    from oracle import c_oracle
    from sglang_awq_amd import synth

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--sets", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["unit"] == "GB/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    # value = algorithmic bytes of the step's two GEMVs (23,455,232 B each) over the wall time of one step
    assert out["ms_per_step"] > 0 and abs(out["value"] - 2 * 23_455_232 / (out["ms_per_step"] * 1e-3) / 1e9) <= 1e-3 * out["value"]
    for moved in ("roofline", "cpu_baseline", "prefill", "dequantize", "awq_gemm_op", "decode_7b_tp1"):
        assert moved not in out, moved                                    # these need --full

    assert sorted(os.listdir(tmp_path)) == ["y0_col.npy", "y1_row.npy"]
    y0, y1 = np.load(tmp_path / "y0_col.npy"), np.load(tmp_path / "y1_row.npy")
    assert y0.dtype == np.float32 and y0.shape == (1, 11008) and y1.shape == (1, 11008) and np.isfinite(y1).all()
    # with one weight set every step runs set 0, whose first linear holds synth weights: the benchmark's own oracle bar
    qw, s, qz = synth.make_awq_weights(4096, 11008, 128, "f16", "A", 1234)
    x = synth.make_activations(1, 4096, "f16", "A", 1234)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(exact), 2.0 ** -14))) - 10)
    assert np.all(np.abs(y0.astype(np.float64) - exact) <= 0.5 * ulp + 1e-3)

