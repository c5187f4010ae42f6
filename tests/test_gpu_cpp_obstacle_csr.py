"""obstacle_assembler<Mesh>::assemble_all_csr of the C++ drop-in header (proton_amd/host/hho.hpp): the obstacle system directly in
CSR (pa_obstacle_csr_assemble), compiled with g++ against the C ABI only, against assemble_all + finalize on a second assembler
of the same mesh and active set."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def obstacle_csr_driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "obstacle_csr_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "obstacle_csr_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("fd", [0, 1])
def test_assemble_all_csr_equals_assemble_all(obstacle_csr_driver, fd):
    """N = 8, the active set the disc r < 0.7: the same row pointers and column indices, values and right-hand side equal with =="""
    r = subprocess.run([obstacle_csr_driver, str(fd), "8"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert re.search(r"same_pattern 1 same_values 1 same_rhs 1", r.stdout), r.stdout
