"""bench.py's command line on the GPU: a plain run (no --full) times exactly --steps steps,
leaves the CPU baseline, the host-inclusive rate and the legs out of the line, and
--dump-outputs writes the last step's op list and statistics as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.gpu, pytest.mark.late]


def test_plain_run_dumps_last_step(gpu, tmp_path):
    n = 64 << 20
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size-gib", str(n / 2**30), "--edit-ppm", "20", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert abs(d["value"] - 2 * n / (d["ms_per_step"] * 1e-3) / 2**30) <= 0.01 * d["value"]
    # the profiled launches are those of the 3 timed steps (the same launches in every step)
    assert d["kernels"] and all(v["launches"] % 3 == 0 for v in d["kernels"].values())
    assert d["cpu_baseline"] is None and d["host_inclusive"] is None and "c4" not in d and "c5" not in d
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["ops_a", "ops_b", "ops_kind", "stats"]
    assert all(v.dtype == np.float64 for v in got.values())
    kind, a, b = got["ops_kind"], got["ops_a"], got["ops_b"]
    assert kind.shape == a.shape == b.shape and set(np.unique(kind)) == {0.0, 1.0}
    assert int(b.sum()) == n  # the ops rebuild the whole source
    st = d["match_stats"]
    assert got["stats"].tolist() == [float(v) for v in st.values()]
    assert int((kind == 0).sum()) == st["copy_ops"] and int(b[kind == 1].sum()) == st["literal_bytes"]
    # Data ops carry source offsets: with no insertions each one starts where the ops before it end
    ends = np.concatenate([[0.0], np.cumsum(b)[:-1]])
    assert np.array_equal(a[kind == 1], ends[kind == 1])
