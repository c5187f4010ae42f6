"""solve_obstacle of the C++ drop-in header (proton_amd/host/hho.hpp): the active-set loop of obstacle.cpp:117-197 as one call to
pa_obstacle_solve, in a driver shaped like the reference's apps/obstacle and compiled with g++ against the C ABI only, against
obstacle_driver (the same loop on the host, batched operators) and apps/obstacle/results/convergence.txt."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = r"N (\d+) degree (\d+) iterations (\d+) error ([0-9.e+-]+) converged (\d)"


def build(name):
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
           "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module")
def drivers():
    return build("obstacle_solve_driver"), build("obstacle_driver")


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    m = re.search(LINE, r.stdout)
    assert m, r.stdout
    return int(m.group(3)), float(m.group(4)), int(m.group(5))


@pytest.mark.parametrize("k,N,ref", [(0, 8, 2.26205), (1, 16, 0.0588187)])
def test_solve_obstacle_driver(drivers, k, N, ref):
    """the energy error within 5e-6 of convergence.txt, converged, and as many systems solved as obstacle_driver ... batched"""
    solve_driver, host_driver = drivers
    iters, err, converged = run([solve_driver, str(k), str(N)])
    iters_host, err_host, converged_host = run([host_driver, str(k), str(N), "batched"])
    assert converged == 1 and converged_host == 1
    assert abs(err - ref) / ref < 5e-6
    assert iters == iters_host
