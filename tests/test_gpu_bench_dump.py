"""bench.py as the driver runs it, reduced: a plain `--gpus 1 --steps K --warmup W`
run in a process of its own times the K steps and nothing else (every other
leg's record is null without --full), and --dump-outputs writes the lists of
its last timed step: D.npy (float32) and I.npy (labels as float64).  The dumped
lists are the exact top-k of the benchmark's own inputs (corpus rows 0..N of
seed 1234, queries from row 50M of seed 5678) under the fp32 contract of
oracle/flat.mismatches (1e-5 relative), the tolerance smoke() holds the same
search to."""

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# more than one 256-query tile with a ragged last one, rows no multiple of a tile
N, D_, B, K = 20_011, 1536, 300, 10


def test_plain_bench_dumps_last_step_outputs(tmp_path):
    from vsearch.synth import synthetic_rows

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR")}
    env["MASTER_PORT"] = str(port)
    out = subprocess.run(
        ["timeout", "-k", "10", "100", sys.executable, "-u", os.path.join(ROOT, "bench.py"),
         "--gpus", "1", "--workload", "c2", "--ntotal", str(N), "--batch", str(B),
         "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")],
        capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "queries/s" and res["higher_is_better"] is True
    assert res["dtype"] == "fp32" and res["result_sane"] is True
    assert res["ms_per_step"] > 0
    # value is the timed steps' own rate (both rounded to 3 places in the line)
    assert res["value"] == pytest.approx(B / (res["ms_per_step"] / 1e3), rel=1e-2)
    for leg in ("batch1", "wide_k", "any_k", "cpu_baseline"):
        assert res[leg] is None, leg
    assert "clustered" not in res
    assert res.get("filter_verify", {}).get("exact_check") is None

    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["D.npy", "I.npy"]
    D, I = np.load(tmp_path / "dump" / "D.npy"), np.load(tmp_path / "dump" / "I.npy")
    assert D.dtype == np.float32 and I.dtype == np.float64
    assert D.shape == (B, K) and I.shape == (B, K)
    assert (I == np.floor(I)).all()
    xb = synthetic_rows(0, N, D_, seed=1234)
    xq = synthetic_rows(50_000_000, B, D_, seed=5678)
    Dr, Ir = flat.knn_exact(xb, xq, K, flat.METRIC_INNER_PRODUCT)
    bad = flat.mismatches(D, I.astype(np.int64), Dr, Ir, flat.METRIC_INNER_PRODUCT, xb, xq)
    assert not bad, bad[:3]
