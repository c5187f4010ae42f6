"""assembler<Mesh>::assemble_all_fused of the C++ drop-in header (proton_amd/host/hho.hpp): the global system written from
the local-operator kernel's on-chip image (pa_assembler_csr_assemble), compiled with g++ against the C ABI only, against
assemble_all on a second assembler of the same mesh."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fused_assembly_driver():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fused_assembly_driver")
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fused_assembly_driver.cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("cd,fd", [(2, 1), (3, 2)])
def test_assemble_all_fused_equals_assemble_all(fused_assembly_driver, cd, fd):
    """N = 8: the same row pointers and column indices; per row the largest |difference of values| over the row's largest
    |value|, and the same for the right-hand side, below 1e-11 (the two paths form lc in different kernel instances)"""
    r = subprocess.run([fused_assembly_driver, str(cd), str(fd), "8"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    m = re.search(r"same_pattern (\d) values_err ([0-9.e+-]+) rhs_err ([0-9.e+-]+)", r.stdout)
    assert m and m.group(1) == "1", r.stdout
    assert float(m.group(2)) < 1e-11 and float(m.group(3)) < 1e-11, r.stdout
