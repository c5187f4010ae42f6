"""interface_assembler::assemble_all of the C++ drop-in header (proton_amd/host/cuthho.hpp): the interface problem's local
operators and its global system built directly in CSR on the device (pa_interface_csr_*), compiled with g++ against the C ABI
only and solved with the reference's conjugated_gradient, reproduces the Interface table of apps/cuthho/cuthho.xlsx."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def interface_batch_driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "interface_batch_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "interface_batch_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("k,N,ref", [(0, 10, 0.285023), (1, 10, 2.01456e-2), (2, 20, 1.38029e-4)])
def test_interface_assemble_all_reproduces_xlsx(interface_batch_driver, k, N, ref):
    """`cuthho_square -k K -M N -N N -r 4 -i` with assemble_all in place of the per-cell loop (:1664-1716): threshold 1e-9,
    Jacobi (:1737-1743); energy-norm error within the 6 printed digits"""
    r = subprocess.run([interface_batch_driver, str(k), str(N), "4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"interface N \d+ k \d+ r \d+ cut_cells (\d+) system (\d+) nnz (\d+) cg_iters \d+ energy_error ([0-9.e+-]+)", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout
    assert abs(float(m.group(4)) - ref) / ref < 6e-6, r.stdout
