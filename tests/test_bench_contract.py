"""bench.py's output contract (the JSON line the driver parses) and its refusal to run without a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    env = dict(os.environ)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def test_bench_refuses_to_run_without_a_gpu():
    """No CPU fallback: on a machine without a GPU the bench exits with an error instead of timing anything else."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU")
    r = _run(["--steps", "1", "--warmup", "0", "--no-cpu-baseline"], timeout=300)
    assert r.returncode != 0
    assert "GPU" in (r.stderr + r.stdout)
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]       # no result line


@pytest.mark.gpu
def test_bench_line_carries_the_contract_fields():
    """One JSON line with BASELINE.json's metric, the roofline and cpu_baseline objects, the settle phase reported, and
    numbers that are consistent with each other (value = cells / time of a step; achieved = algorithmic bytes / kernel time)."""
    r = _run(["--gpus", "1", "--steps", "4", "--warmup", "1", "--settle-ms", "30", "--workload", "quad256_k1_fan", "--cpu-sample-rows", "8",
              "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "cells/s"
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] in ("weak", "strong") and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic"
    assert d["config"]["workload"] == "quad256_k1_fan" and "model" not in d["config"]
    assert d["settle"]["passes"] >= 1
    cells = d["config"]["cells"]
    assert abs(d["value"] - cells / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    ro = d["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-12 and 0.0 < ro["frac"] < 1.0
    assert abs(ro["achieved"] - ro["cells_per_launch"] * ro["algorithmic_bytes_per_cell"] / (ro["kernel_ms"] * 1e-3) / 1e9) <= 1e-6 * ro["achieved"]
    assert ro["kernel_ms"] <= d["ms_per_step"] * 1.05
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["unit"] == "cells/s" and cb["sample"]
    assert d["gpu_over_cpu"] > 10.0                                     # the north star's floor
    # counters are never replayed across builds: the line names its build, and `traffic` is that build's or null with the reason
    from proton_amd import _build
    assert d["build_stamp"] == _build.build_stamp() and ro["traffic_source"]
    assert ro["traffic"] is None or "counters of this build" in ro["traffic_source"]


@pytest.mark.gpu
def test_bench_mode_A_reports_the_matrix_assembly_span():
    """--mode A: operators + rhs + assembler<Mesh>'s own system directly in CSR, next to the CPU restatement's "Matrix assembly" span"""
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-ms", "20", "--workload", "quad256_k1_fan", "--mode", "A",
              "--cpu-sample-rows", "8", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["config"]["mode"] == "A" and d["stage_ms"]["fill"] > 0 and d["stage_ms"]["ops"] > 0
    ma = d["matrix_assembly"]
    assert ma["cpu_one_core"] > 0 and ma["gpu_over_cpu_one_core"] > 10.0 and abs(ma["value"] - d["value"]) < 1e-9 * d["value"]
    pk = d["roofline"]["per_kernel"]
    assert pk["fill"]["bytes"] > 0 and 0 < pk["fill"]["frac"] < 1


def test_dump_plan_stays_within_the_budget_and_is_fixed():
    """--dump-outputs: everything when it fits; otherwise a sample of distinct, sorted rows, the same in every run, the
    same rows for arrays with as many rows, and the files (headers included) within the budget"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    assert bench.dump_plan({"lc": (64, 14, 14), "rhs": (64, 6)}, bench.DUMP_BYTES) == {"lc": None, "rhs": None}
    shapes = {"lc": (1 << 20, 22, 22), "rhs": (1 << 20, 10), "csr_values": (488_000_000,), "empty": (0, 44, 44)}
    plan = bench.dump_plan(shapes, bench.DUMP_BYTES)
    again = bench.dump_plan(shapes, bench.DUMP_BYTES)
    written = 0
    for k, s in shapes.items():
        idx = plan[k]
        assert np.array_equal(idx, again[k]) and len(idx) <= s[0]
        if len(idx):
            assert idx.dtype == np.int64 and idx[0] >= 0 and idx[-1] < s[0] and (np.diff(idx) > 0).all()
        written += 256 + 8 * len(idx) * int(np.prod(s[1:]))
    assert np.array_equal(plan["lc"], plan["rhs"]) and len(plan["lc"]) > 1000 and len(plan["empty"]) == 0
    assert written <= bench.DUMP_BYTES == 64_000_000


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and leaves the CPU baseline out; --dump-outputs writes the last
    step's lc and rhs, float64 and within 64 MB, sampled at dump_plan's rows -- and those are the oracle's operators of those cells."""
    import numpy as np
    import oracle_lib
    sys.path.insert(0, ROOT)
    import bench
    out = tmp_path / "outputs"
    r = _run(["--gpus", "1", "--steps", "5", "--warmup", "1", "--settle-ms", "30", "--workload", "quad256_k1_fan",
              "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["cells"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["cpu_baseline"] is None and "gpu_over_cpu" not in d and d["same_step_one_gpu"] is None
    files = sorted(p.name for p in out.iterdir())
    assert files == ["lc.npy", "rhs.npy"]
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64_000_000
    N = 256
    di = oracle_lib.degrees(2, 1)
    plan = bench.dump_plan({"lc": (N * N, di.msize, di.msize), "rhs": (N * N, di.cbs)}, bench.DUMP_BYTES)
    lc, rhs = np.load(out / "lc.npy"), np.load(out / "rhs.npy")
    assert lc.dtype == rhs.dtype == np.float64
    assert lc.shape == (len(plan["lc"]), di.msize, di.msize) and rhs.shape == (len(plan["rhs"]), di.cbs)
    mp, points, ptids = oracle_lib.make_mesh(N, N)
    for i in np.linspace(0, len(plan["lc"]) - 1, 8).astype(int):
        c = int(plan["lc"][i])
        st, ref = oracle_lib.local_ops_batch(points, ptids, di, oracle_lib.QUAD_FAN, oracle_lib.STAB_NAIVE, first=c, n=1, fn=1, want=("lc",))
        assert st == 0
        assert np.abs(lc[i].T - ref["lc"][0]).max() <= 1e-12 * np.abs(ref["lc"][0]).max(), c
        assert np.abs(rhs[i] - ref["rhs"][0]).max() <= 1e-12 * np.abs(ref["rhs"][0]).max(), c
