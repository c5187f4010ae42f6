"""interface_assembler::solve_condensed of the C++ drop-in header with its trailing `coarse`, `coarse_parts` arguments
(proton_amd/host/cuthho.hpp): tests/cpp/interface_coarse_driver.cpp, compiled with g++ against the C ABI only, solves the interface
problem's face-only system by pa_conjugated_gradient_patch_coarse on the tables of pa_interface_condensed_patches and
pa_interface_condensed_coarse and agrees with interface_condensed_solve(patches="cell", coarse=H) of the Python route: the same
iteration count, the solution to 1e-12 relative, and fewer iterations than the same driver's with the patches alone."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (r"interface_coarse N (\d+) k (\d+) r (\d+) H (\d+) parts (\w+) cut_cells (\d+) system (\d+) face_system (\d+) cg_iters (\d+) "
        r"CONVERGED energy_error ([0-9.e+-]+)")


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "interface_coarse_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "interface_coarse_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


def _run(driver, N, k, H, parts, dump):
    r = subprocess.run([driver, "-k", str(k), "-M", str(N), "-N", str(N), "-r", "4", "-H", str(H), "-s", parts, "-t", "1e-13", "-x", dump],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(LINE, r.stdout)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)) == (N, k, 4, H, parts), r.stdout
    assert int(m.group(6)) > 0
    print(r.stdout.strip())
    return int(m.group(9)), float(m.group(10)), np.fromfile(dump, dtype=np.float64)


@pytest.mark.parametrize("N,k,ref", [(20, 2, 1.38029e-4), (32, 2, None)], ids=["20-k2", "32-k2"])
def test_interface_coarse_driver_agrees_with_the_python_route(driver, tmp_path, N, k, ref):
    """`-i` at (20, 2) and (32, 2), H = 4, both parts: CONVERGED at 1e-13, the iteration count of the Python route and its solution
    to 1e-12 of the largest entry; fewer iterations than H = 0 (the patches alone); at (20, 2) the energy-norm error of cuthho.xlsx
    within its 6 printed digits"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    iters0, energy0, _ = _run(driver, N, k, 0, "side", str(tmp_path / "patch.bin"))
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    for parts in ("side", "one"):
        iters, energy, sol = _run(driver, N, k, 4, parts, str(tmp_path / ("coarse_%s.bin" % parts)))
        assert iters < iters0
        if ref is not None:
            assert abs(energy - ref) / ref < 6e-6 and abs(energy0 - ref) / ref < 6e-6
        full, py_iters, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell", coarse=4, coarse_parts=parts)
        asm.synchronize()
        full = full.cpu().numpy()
        assert reason == 0 and py_iters == iters
        assert sol.shape == full.shape and np.abs(sol - full).max() <= 1e-12 * np.abs(full).max()
