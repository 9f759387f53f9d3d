"""bench.py's plain line and --dump-outputs: a plain run times exactly --steps steps and measures nothing beyond the headline; the
dump holds what the last timed step computed, bounded in size, and the same arguments give the same inputs run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixed_sample_caps_size_and_is_seeded():
    import bench
    rows = bench.DUMP_BYTES_PER_ARRAY // 16 + 1000
    t = torch.arange(rows * 2, dtype=torch.int64).view(rows, 2)
    a, b = bench.fixed_sample(t, np.float64), bench.fixed_sample(t, np.float64)
    assert a.dtype == np.float64 and a.nbytes <= bench.DUMP_BYTES_PER_ARRAY and a.shape[1] == 2
    assert np.array_equal(a, b)                                              # the same sample every time
    assert np.all(np.diff(a[:, 0]) > 0) and np.array_equal(a[:, 1], a[:, 0] + 1)   # whole rows, in order, no repeats
    small = torch.linspace(0, 1, 100)
    assert np.array_equal(bench.fixed_sample(small, np.float32), small.numpy())     # below the cap: all of it


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "8192",
           "--edges-per-k", "20000", "--deterministic"]
    recs, dumps = [], []
    for i in range(2):
        out = tmp_path / f"run{i}"
        run = subprocess.run(cmd + ["--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert run.returncode == 0, run.stderr[-2000:]
        recs.append(json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append({f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))})
    rec = recs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["timed_windows"]["n"] == 1
    assert abs(rec["value"] - 8192 / (rec["ms_per_step"] * 1e-3)) <= 1e-3 * rec["value"]
    # nothing beyond the headline without --full
    assert rec["roofline"] is None and not rec["kernel_class_ms_per_step"] and rec["model_step_only"] is None
    assert not {"cpu_baseline", "extra_points", "roofline_gather"} & set(rec)
    d = dumps[0]
    assert set(d) == {"bce", "recon", "logits", "batch_ids", "batch_weights", "params"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert d["logits"].shape == (8192,) and d["batch_ids"].shape == (8192, 5) and d["batch_weights"].shape == (8192,)
    assert np.isfinite(d["logits"]).all() and np.isfinite(d["params"]).all() and 0.0 < float(d["bce"][0]) < 5.0
    assert float(d["bce"][0]) == pytest.approx(rec["last_bce"], abs=1e-5)
    # same arguments, same inputs (and with the sorted embedding backward, the same results)
    assert np.array_equal(d["batch_ids"], dumps[1]["batch_ids"]) and np.array_equal(d["batch_weights"], dumps[1]["batch_weights"])
    for k in ("bce", "logits", "params"):
        np.testing.assert_allclose(d[k], dumps[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
