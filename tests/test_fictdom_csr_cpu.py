"""The fictitious-domain assembly entry (pa_fictdom_csr_assemble) without a GPU: the header, the ctypes symbol list and the built
library agree on the export, and a NULL context is refused."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pa_fictdom_csr_assemble"


def test_header_binding_and_library_agree_on_the_new_export():
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    assert int(re.search(r"#define PA_ABI_VERSION (\d+)", h).group(1)) == 5          # an added export is compatible
    # declared once, with eleven parameters, behind a comment that cites the reference and states the contract
    assert len(re.findall(r"\b" + NAME + r"\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))) == 1
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + NAME + r"\(([^;]*)\);", h, flags=re.S)
    assert m, "declaration with its comment"
    comment, params = m.group(1), re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    assert len(params.split(",")) == 11
    assert re.search(r"hho\.hpp:344-406", comment) and re.search(r"hho\.hpp:451-455", comment)
    assert re.search(r"cuthho_square\.cpp:881-905", comment) and "BIT-IDENTICAL" in comment
    assert capi.EXPORTS.count(NAME) == 1
    fn = getattr(capi.lib(), NAME)
    assert len(fn.argtypes) == 11
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert len(re.findall(r" T " + NAME + r"$", out, flags=re.M)) == 1
    # a NULL context is refused, not dereferenced: PA_ERR_INVALID_ARG
    assert fn(None, 1, capi.LOC_NEGATIVE, None, None, None, None, None, None, None, None) == 1


def test_drop_in_header_offers_the_batched_fictitious_domain_assembly():
    """tests/cpp/fictdom_batch_driver.cpp compiles against proton_amd/host/cuthho.hpp and the C ABI alone (no HIP headers)"""
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "fictdom_batch_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "fictdom_batch_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
