"""interface_assembler::solve_condensed of the C++ drop-in header (proton_amd/host/cuthho.hpp): the interface problem's operators,
the cells' static condensation, the face-only system, its conjugate gradient and the recovery of the cell unknowns on the device,
compiled with g++ against the C ABI only, reproduces the Interface table of apps/cuthho/cuthho.xlsx through take_local_data."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def interface_condensed_driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "interface_condensed_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "interface_condensed_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("k,N,ref", [(0, 10, 0.285023), (1, 20, 5.22389e-3), (2, 20, 1.38029e-4)])
def test_interface_solve_condensed_reproduces_xlsx(interface_condensed_driver, k, N, ref):
    """`cuthho_square -k K -M N -N N -r 4 -i` with solve_condensed in place of the loop and the solve (:1664-1743): threshold 1e-9,
    Jacobi; energy-norm error within the 6 printed digits"""
    r = subprocess.run([interface_condensed_driver, str(k), str(N), "4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"interface condensed N \d+ k \d+ r \d+ cut_cells (\d+) full_system (\d+) cg_iters \d+ energy_error ([0-9.e+-]+)",
                  r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout
    assert abs(float(m.group(3)) - ref) / ref < 6e-6, r.stdout
