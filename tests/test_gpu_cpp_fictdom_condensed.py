"""assembler::solve_condensed_fictdom of the C++ drop-in header (proton_amd/host/hho.hpp on a cuthho_poly_mesh of host/cuthho.hpp):
the fictitious-domain problem condensed to its face unknowns on the device (pa_fictdom_condensed_ops_batch, pa_condensed_csr_*),
solved by the device conjugate gradient and recovered (pa_fictdom_condensed_recover), compiled with g++ against the C ABI only,
reproduces the F.D. table of apps/cuthho/cuthho.xlsx."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (r"fictdom_condensed N (\d+) k (\d+) r (\d+) cut_cells (\d+) system (\d+) face_system (\d+) \(fbs (\d+)\) cg_iters (\d+) "
        r"CONVERGED energy_error ([0-9.e+-]+)")


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fictdom_condensed_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fictdom_condensed_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("k,N,ref", [(1, 20, 3.08508e-3), (2, 20, 9.30124e-5)])
def test_solve_condensed_fictdom_reproduces_xlsx(driver, k, N, ref):
    """`cuthho_square -k K -M N -N N -r 4 -f` with solve_condensed_fictdom in place of the loop (:883-900) and the solve (:915-919):
    CONVERGED at 1e-13, energy-norm error within the 6 printed digits"""
    r = subprocess.run([driver, "-k", str(k), "-M", str(N), "-N", str(N), "-r", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(LINE, r.stdout)
    assert m and int(m.group(4)) > 0, r.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (N, k, 4)
    cbs = (k + 3) * (k + 2) // 2
    assert int(m.group(5)) == int(m.group(6)) + cbs * N * N and int(m.group(6)) == (k + 1) * 2 * N * (N - 1)
    print(r.stdout.strip())
    assert abs(float(m.group(9)) - ref) / ref < 6e-6, r.stdout
