"""bench.py's command line: a plain run times its steps and prints the result line (the
evaluator, CPU baseline and cross-check legs stay out), `--dump-outputs DIR` writes the last
step's results as float64 .npy files, and `--full` adds the legs back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

INVALID = 0xFFFFFFFF


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-800:]
    return json.loads(lines[0])


def test_options_are_declared():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode == 2


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_results(gpu_ctx, tmp_path):
    """RMAT-12 ef16, k = 16, 2 timed steps: the result line's contract fields, none of the
    --full legs, and the dumped sequence, index, tree and parts equal the oracle's."""
    import oracle
    import sheep_amd
    out = str(tmp_path / "dump")
    d = run_bench("--scale", "12", "--k", "16", "--steps", "2", "--warmup", "1", "--dump-outputs", out)
    assert d["metric"] == "edges/s seq+tree+partition" and d["unit"] == "edges/s" and d["dtype"] == "u32"
    assert d["higher_is_better"] is True and d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["value"] > 0
    # value = records per second of a step; ms_per_step is rounded to 0.001 ms
    assert abs(1e3 * d["config"]["records"] / d["value"] - d["ms_per_step"]) <= 0.00051
    assert d["full"] is False and d["evaluator"] is None and "cpu_baseline" not in d
    assert not any(k.startswith("verified") for k in d)
    names = ["parts", "pos", "seq", "summary", "tree_parent", "tree_pst"]
    assert d["dumped_outputs"] == names and sorted(os.listdir(out)) == [n + ".npy" for n in names]
    got = {n: np.load(os.path.join(out, n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in got.values())

    r = sheep_amd.rmat_host(12, 16, 12)
    t, h = r[:, 0].astype(np.uint32), r[:, 1].astype(np.uint32)
    seq = oracle.sequence(t, h)
    parent, pst = oracle.build_tree(t, h, seq)
    parts, info = oracle.partition(parent, pst, seq, 16)
    assert np.array_equal(got["seq"], seq.astype(np.float64))
    assert np.array_equal(got["tree_parent"], parent.astype(np.float64))
    assert np.array_equal(got["tree_pst"], pst.astype(np.float64))
    assert np.array_equal(got["parts"], np.asarray(parts, np.int16).astype(np.float64))
    pos = np.full(len(got["pos"]), INVALID, dtype=np.float64)
    pos[seq] = np.arange(len(seq))
    assert np.array_equal(got["pos"], pos)
    assert got["summary"][0] == len(seq) == d["config"]["tree_nodes"] and got["summary"][1] == len(got["pos"])
    assert got["summary"][2] == info["created"] == d["config"]["created"]


@pytest.mark.gpu
def test_full_run_adds_the_legs(gpu_ctx):
    """--full: the evaluator's counts equal the oracle's, the merged tree of a 2-shard run is
    cross-checked, and the CPU baseline leg reports (a value where the reference harness is
    built and runs, the reason where it is not or does not)."""
    import oracle
    import sheep_amd
    d = run_bench("--full", "--scale", "12", "--k", "16", "--steps", "1", "--warmup", "0", "--eval-reps", "1",
                  "--shards", "2")
    assert d["full"] is True and d["steps"] == 1 and d["ms_per_step"] > 0
    assert d["verified_vs_pairwise_merges"] is True and d.get("verified_vs_whole_graph", True) is True
    r = sheep_amd.rmat_host(12, 16, 12)
    t, h = r[:, 0].astype(np.uint32), r[:, 1].astype(np.uint32)
    seq = oracle.sequence(t, h)
    parent, pst = oracle.build_tree(t, h, seq)
    parts, _ = oracle.partition(parent, pst, seq, 16)
    assert d["evaluator"]["ecv_down"] == oracle.evaluate(t, h, seq, parts)["ecv_down"]
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "reference" and cpu["unit"] == "edges/s"
    if cpu["value"] is None:
        # no reference harness or MPI on this host, or the harness cannot start here (its MPI
        # library is absent): the leg says which, and the run still exits 0
        assert "missing on this host" in cpu["sample"] or cpu["sample"].startswith("failed: "), cpu["sample"]
        assert cpu["cores"] == 0
    else:
        assert cpu["value"] > 0 and cpu["matches_gpu"]["seq"] and cpu["matches_gpu"]["tree"] \
            and cpu["matches_gpu"]["parts"]
