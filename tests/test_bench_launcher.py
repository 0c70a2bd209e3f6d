"""bench.py's own rank launcher (the driver runs `python bench.py --gpus N`):
N fresh rank processes, one JSON line from rank 0, n_gpus = the world size the
collective saw and an all-gather head-count of every rank.  Rehearsed here
with --dry-run (gloo on CPU, no GPU, no kernel)."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 3])
def test_bench_launches_ranks_itself(world):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--dry-run",
         "--steps", "3", "--warmup", "1", "--batch", "64"],
        capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == world
    assert res["ranks_seen"] == world
    assert res["dry_run"] is True
    assert res["steps"] == 3 and res["warmup"] == 3 - 2
    assert res["value"] > 0


def test_bench_single_rank_no_launcher():
    """--gpus 1 runs in-process (no launcher) and still reports one rank."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["MASTER_PORT"] = "29533"
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "2",
         "--warmup", "0", "--batch", "8"],
        capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert res["n_gpus"] == 1 and res["ranks_seen"] == 1


def test_bench_options_full_and_dump_outputs():
    """--full is off by default and --dump-outputs takes a directory; --steps is
    the number of timed steps the line reports."""
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None
    assert a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_formats_and_budget(tmp_path):
    """Scores are stored as float32 and labels as float64, unchanged in value;
    past the budget the same seeded sample of rows is kept of every array and
    rows.npy names them, the same rows on every call."""
    import numpy as np
    import torch

    import bench

    D = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    I = torch.arange(12, dtype=torch.int64).reshape(4, 3) + (1 << 40)
    bench.dump_outputs(str(tmp_path / "a"), {"D": D, "I": I})
    Dn, In = np.load(tmp_path / "a" / "D.npy"), np.load(tmp_path / "a" / "I.npy")
    assert Dn.dtype == np.float32 and In.dtype == np.float64
    assert (Dn == D.numpy()).all() and (In.astype(np.int64) == I.numpy()).all()
    assert not (tmp_path / "a" / "rows.npy").exists()

    n = bench.DUMP_BUDGET_BYTES // (4 * 4 + 8) * 2  # twice the budget
    D = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4)
    I = torch.arange(n, dtype=torch.int64)
    total = 0
    for name in ("b", "c"):
        bench.dump_outputs(str(tmp_path / name), {"D": D, "I": I})
        total = sum(f.stat().st_size for f in (tmp_path / name).iterdir())
        assert total <= 64 * 10 ** 6
    rows = np.load(tmp_path / "b" / "rows.npy")
    assert (rows == np.load(tmp_path / "c" / "rows.npy")).all()
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    assert (np.load(tmp_path / "b" / "I.npy") == rows).all()
    assert (np.load(tmp_path / "b" / "D.npy")[:, 0] == D[:, 0].numpy()[rows.astype(np.int64)]).all()
