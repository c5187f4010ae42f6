"""assembler::solve_condensed_fictdom of the C++ drop-in header with its trailing `patches` argument (proton_amd/host/hho.hpp):
tests/cpp/fictdom_patch_driver.cpp, compiled with g++ against the C ABI only, solves the face-only fictitious-domain system at
(20, 2) by pa_conjugated_gradient_patch on the tables of pa_condensed_patches and reproduces the F.D. table of
apps/cuthho/cuthho.xlsx in fewer iterations than the Jacobi solve of tests/cpp/fictdom_condensed_driver.cpp."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (r"fictdom_patch N (\d+) k (\d+) r (\d+) patches (\w+) cut_cells (\d+) system (\d+) face_system (\d+) \(fbs (\d+)\) cg_iters (\d+) "
        r"CONVERGED energy_error ([0-9.e+-]+)")
JACOBI_20_2 = 127                 # the device's Jacobi solve of the same system (README, tests/test_gpu_fictdom_condensed.py)


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fictdom_patch_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fictdom_patch_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("patches,most", [("cell", JACOBI_20_2 // 2), ("face", JACOBI_20_2)])
def test_fictdom_patch_driver_reproduces_xlsx(driver, patches, most):
    """`-f` at (20, 2): CONVERGED at 1e-13, the energy-norm error within the 6 printed digits, cell patches in at most half of
    Jacobi's 127 iterations"""
    N, k, ref = 20, 2, 9.30124e-5
    r = subprocess.run([driver, "-k", str(k), "-M", str(N), "-N", str(N), "-r", "4", "-p", patches], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(LINE, r.stdout)
    assert m and m.group(4) == patches and int(m.group(5)) > 0, r.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (N, k, 4)
    assert int(m.group(7)) == (k + 1) * 2 * N * (N - 1)
    print(r.stdout.strip())
    assert int(m.group(9)) <= most
    assert abs(float(m.group(10)) - ref) / ref < 6e-6, r.stdout
