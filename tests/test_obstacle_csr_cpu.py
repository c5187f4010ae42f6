"""The obstacle system's direct CSR entry (pa_obstacle_csr_assemble) without a GPU: the header, the ctypes symbol list and the
built library agree on the export, a NULL context is refused, and the driver of assemble_all_csr compiles against the C ABI alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pa_obstacle_csr_assemble"


def test_header_binding_and_library_agree_on_the_new_export():
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    # declared once, with fifteen parameters, behind a comment that cites the reference and states the contract
    assert len(re.findall(r"\b" + NAME + r"\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))) == 1
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + NAME + r"\(([^;]*)\);", h, flags=re.S)
    assert m, "declaration with its comment"
    comment, params = m.group(1), re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    assert len(params.split(",")) == 15
    assert re.search(r"hho\.hpp:609-695", comment) and ":746-750" in comment and re.search(r"obstacle\.cpp:147-158", comment)
    assert "BIT-IDENTICAL" in comment
    assert capi.EXPORTS.count(NAME) == 1
    fn = getattr(capi.lib(), NAME)
    assert len(fn.argtypes) == 15
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert len(re.findall(r" T " + NAME + r"$", out, flags=re.M)) == 1


def test_a_null_context_is_refused():
    from proton_amd import capi
    di, _ = capi.degree_info(0, 1)
    st = capi.lib().pa_obstacle_csr_assemble(None, di, None, None, None, None, None, None, None, 0, None, None, None, None, None)
    assert st != 0 and st == 1                                  # PA_ERR_INVALID_ARG, not a dereference


def test_the_driver_of_assemble_all_csr_compiles_against_the_c_abi():
    """tests/cpp/obstacle_csr_driver.cpp needs nothing but proton_amd/host/hho.hpp, a C++17 compiler and the C ABI"""
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "obstacle_csr_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "obstacle_csr_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
