"""interface_assembler::solve_condensed of the C++ drop-in header with its trailing `patches` argument (proton_amd/host/cuthho.hpp):
tests/cpp/interface_patch_driver.cpp, compiled with g++ against the C ABI only, solves the interface problem's face-only system at
(20, 2) by pa_conjugated_gradient_patch on the tables of pa_interface_condensed_patches and reproduces the Interface table of
apps/cuthho/cuthho.xlsx in a quarter of the iterations of its own Jacobi run."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = (r"interface_patch N (\d+) k (\d+) r (\d+) patches (\w+) cut_cells (\d+) system (\d+) face_system (\d+) cg_iters (\d+) "
        r"CONVERGED energy_error ([0-9.e+-]+)")
N, K, REF = 20, 2, 1.38029e-4


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "interface_patch_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "interface_patch_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


def run(driver, patches):
    r = subprocess.run([driver, "-k", str(K), "-M", str(N), "-N", str(N), "-r", "4", "-p", patches], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(LINE, r.stdout)
    assert m and m.group(4) == patches and int(m.group(5)) > 0, r.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (N, K, 4)
    print(r.stdout.strip())
    return int(m.group(7)), int(m.group(8)), float(m.group(9))


@pytest.fixture(scope="module")
def jacobi(driver):
    return run(driver, "jacobi")


@pytest.mark.parametrize("patches", ["cell", "face"])
def test_interface_patch_driver_reproduces_xlsx(driver, jacobi, patches):
    """`-i` at (20, 2), -r 4, threshold 1e-9 (:1737-1743): CONVERGED, the energy-norm error within the 6 printed digits, the same
    face system as the Jacobi run; cell patches in at most a quarter of that run's iterations (on the CPU twin at 1e-9: 317 to 57)"""
    rows, iters, err = run(driver, patches)
    assert rows == jacobi[0] and abs(jacobi[2] - REF) / REF < 6e-6
    assert abs(err - REF) / REF < 6e-6
    if patches == "cell":
        assert 4 * iters <= jacobi[1]
    else:
        assert iters < jacobi[1]
