"""assembler::assemble_all_fictdom of the C++ drop-in header (proton_amd/host/hho.hpp on a cuthho_poly_mesh of host/cuthho.hpp): the
fictitious-domain problem's global system written in one pass on the device (pa_fictdom_csr_assemble), compiled with g++ against
the C ABI only and solved with the header's conjugated_gradient, reproduces the F.D. table of apps/cuthho/cuthho.xlsx and numbers
the system as the per-cell driver does."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = r"fictdom N (\d+) k (\d+) r (\d+) cut_cells (\d+) system (\d+) cg_iters (\d+) energy_error ([0-9.e+-]+)"


def _compile(name):
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module")
def fictdom_batch_driver():
    return _compile("fictdom_batch_driver")


@pytest.fixture(scope="module")
def cuthho_driver():
    return _compile("cuthho_driver")


@pytest.mark.parametrize("k,N,ref", [(0, 10, 0.188501), (1, 20, 3.08508e-3), (2, 20, 9.30124e-5)])
def test_fictdom_assemble_all_reproduces_xlsx(fictdom_batch_driver, cuthho_driver, k, N, ref):
    """`cuthho_square -k K -M N -N N -r 4 -f` with assemble_all_fictdom in place of the per-cell loop (:883-900) and the device
    conjugated_gradient: energy-norm error within the 6 printed digits, the system size of cuthho_driver -f"""
    flags = ["-k", str(k), "-M", str(N), "-N", str(N), "-r", "4"]
    r = subprocess.run([fictdom_batch_driver] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(LINE, r.stdout)
    assert m and int(m.group(4)) > 0, r.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (N, k, 4)
    print(r.stdout.strip())
    assert abs(float(m.group(7)) - ref) / ref < 6e-6, r.stdout
    p = subprocess.run([cuthho_driver] + flags + ["-f"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    mp = re.search(LINE, p.stdout)
    assert mp, p.stdout
    assert int(m.group(5)) == int(mp.group(5)) and int(m.group(4)) == int(mp.group(4)), (r.stdout, p.stdout)
