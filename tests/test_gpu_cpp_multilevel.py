"""assembler::solve_condensed_fictdom of the C++ drop-in header with its trailing `coarse_levels` argument (proton_amd/host/hho.hpp):
tests/cpp/fictdom_multilevel_driver.cpp, compiled with g++ against the C ABI only, solves the face-only fictitious-domain system by
pa_conjugated_gradient_multilevel on the tables of pa_condensed_patches and pa_condensed_coarse (by side) and agrees with
fictdom_condensed_solve(patches="cell", coarse=H, coarse_levels=...) of the Python route: the same iteration count, the same
energy-norm error, the solution to 1e-12 relative."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (r"fictdom_multilevel N (\d+) k (\d+) r (\d+) H (\d+) levels (\d+) cut_cells (\d+) system (\d+) face_system (\d+) \(fbs (\d+)\) "
        r"cg_iters (\d+) CONVERGED energy_error ([0-9.e+-]+)")


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fictdom_multilevel_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fictdom_multilevel_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


def _run(driver, N, k, H, levels, dump):
    r = subprocess.run([driver, "-k", str(k), "-M", str(N), "-N", str(N), "-r", "4", "-H", str(H), "-L", levels, "-x", dump],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(LINE, r.stdout)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (N, k, 4, H), r.stdout
    print(r.stdout.strip())
    return int(m.group(10)), float(m.group(11)), np.fromfile(dump, dtype=np.float64)


def test_fictdom_multilevel_driver_agrees_with_the_python_route(driver, tmp_path):
    """`-f` at (20, 2), levels {2} + exact 4: CONVERGED at 1e-13, the energy-norm error of cuthho.xlsx within its 6 printed digits, the
    iteration count of the Python route and its solution to 1e-12 of the largest entry, with the smoothed level and without it (-L 0:
    the two-level solve of fictdom_coarse_driver); levels that are not nested are refused.  (No order between the two counts is
    asserted: the sum is additive, and on 20^2 cells a level at H = 2 below the exact H = 4 has nothing left to save -- 37 against 35
    on one MI355X run.)"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    import test_gpu_fictdom_condensed as F
    from proton_amd.batch import BatchAssembler
    N, k, ref = 20, 2, 9.30124e-5
    iters, energy, sol = _run(driver, N, k, 4, "2", str(tmp_path / "multi.bin"))
    iters0, energy0, _ = _run(driver, N, k, 4, "0", str(tmp_path / "two.bin"))
    assert abs(energy - ref) / ref < 6e-6 and abs(energy0 - ref) / ref < 6e-6
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    full, py_iters, reason = asm.fictdom_condensed_solve(k, 0, tol=1e-13, patches="cell", coarse=4, coarse_levels=(2,))
    two, py_iters0, _ = asm.fictdom_condensed_solve(k, 0, tol=1e-13, patches="cell", coarse=4)
    asm.synchronize()
    full = full.cpu().numpy()
    assert reason == 0 and py_iters == iters and py_iters0 == iters0
    assert sol.shape == full.shape and np.abs(sol - full).max() <= 1e-12 * np.abs(full).max()
    import oracle_lib as oracle
    py_energy = F.energy_error(oracle, oracle.CutMesh(N, refsteps=4), k, full)
    print("energy error: driver %.10e, Python route %.10e" % (energy, py_energy))
    assert abs(py_energy - energy) / energy < 6e-6           # (two implementations of the cut quadrature: the project's tolerance between them)
    r = subprocess.run([driver, "-k", str(k), "-M", str(N), "-N", str(N), "-r", "4", "-H", "4", "-L", "3"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 4 and "refused" in r.stdout
