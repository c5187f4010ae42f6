"""The condensed fictitious-domain entries (pa_fictdom_condensed_ops_batch, pa_fictdom_condensed_recover) without a GPU: header,
ctypes symbol list and built library agree on the exports and each cites the reference; the 50-digit judge of
tests/fictdom_condensed_judge.py, which the GPU tests hold the kernels to, passes a longdouble elimination and rejects a
plain-double one on the oracle's own cut matrices; the drop-in header's new member compiles against the C ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import fictdom_condensed_judge as judge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pa_fictdom_condensed_ops_batch": 9, "pa_fictdom_condensed_recover": 9}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_binding_and_library_agree_on_the_new_exports(name):
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    assert len(re.findall(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))) == 1
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(([^;]*)\);", h, flags=re.S)
    assert m, "declaration with its comment"
    comment, params = m.group(1), re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    assert len(params.split(",")) == NAMES[name]
    # the assembly loop, the solve and take_local_data of the -f driver
    assert re.search(r"cuthho_square\.cpp:881-905", comment) and re.search(r":915-919", comment) and re.search(r":959-962", comment)
    # declared next to pa_fictdom_csr_assemble: after it, before the interface problem's section
    assert h.index("int pa_fictdom_csr_assemble(") < h.index("int " + name + "(") < h.index("pa_interface_params;")
    assert capi.EXPORTS.count(name) == 1
    fn = getattr(capi.lib(), name)
    assert len(fn.argtypes) == NAMES[name]
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert len(re.findall(r" T " + name + r"$", out, flags=re.M)) == 1
    # a NULL context is refused, not dereferenced: PA_ERR_INVALID_ARG
    assert fn(None, 1, capi.LOC_NEGATIVE, *([None] * (NAMES[name] - 3))) == 1


def test_kernel_file_is_built_and_holds_the_two_kernels():
    """the unit is built, and the cut cells' elimination and recovery are stated once: in the header both units include"""
    from proton_amd import _build
    csrc = os.path.join(ROOT, "proton_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    assert '"fictdom_condensed"' in open(_build.__file__).read()
    units = ("fictdom_condensed.hip", "interface_condensed.hip")
    # each problem keeps a recovery kernel of its own for its addressing
    assert "void fdcond_recover_kernel(" in text["fictdom_condensed.hip"] and "void ifcond_recover_kernel(" in text["interface_condensed.hip"]
    for f in units:
        s = text[f]
        assert "int ifd_cholesky(" not in s and "struct IfdAr<true>" not in s and '#include "ifd_dense.hpp"' in s
        # each unit launches the shared records kernel and calls the shared recovery; it defines neither
        assert "ifd_records_kernel<" in s and "ifd_recover_cell<" in s
        assert "void ifd_records_kernel(" not in s and "*ifd_recover_cell(" not in s
    # the factorization, the forward substitution over the NC columns, the Schur / g product loop and the two triangular sweeps:
    # one distinctive token of each, once under csrc/, and that in the header
    for token in ("int ifd_cholesky(", "void ifd_records_kernel(", "*ifd_recover_cell(",
                  "for (int c = lane; c < NC; c += 64)",
                  "Ar::mul(W[i * N + k], W[j * N + k])", "Ar::mul(W[i * N + k], W[NF * N + k])",
                  "Ar::mul(A[lane * N + j], b[j])", "Ar::mul(A[j * N + lane], b[j])"):
        assert [f for f in text if token in text[f]] == ["ifd_dense.hpp"] and text["ifd_dense.hpp"].count(token) == 1, token
    # no more than six kernels in the two units and their header: records, recovery of either problem, info remap, masked
    # right-hand side, copy
    assert sum(len(re.findall(r"__global__", text[f])) for f in units + ("ifd_dense.hpp",)) <= 6


def cut_matrices(oracle, N, k):
    """the oracle's cut operators of the circle's cut cells -> (lc [ncut, M, M], f [ncut, cbs], cbs)"""
    from cuthho_driver import oracle_cut_provider
    msh = oracle.CutMesh(N, refsteps=4)
    di = oracle.degrees(k + 1, k)
    local = oracle_cut_provider(msh, di)
    cut = [c for c in range(msh.nc) if msh.cell_loc[c] == oracle.CUT_ON_INTERFACE]
    return np.array([local[c][0] for c in cut]), np.array([local[c][1] for c in cut]), di.cbs


def worst(lcs, fs, n, dtype):
    w = 0.0
    for c in range(len(lcs)):
        S_ref, g_ref = judge.exact_record(lcs[c], fs[c], n)
        S, g = judge.eliminate(lcs[c], fs[c], n, dtype)
        w = max(w, judge.record_error(S, g, S_ref, g_ref))
    return w


def test_judge_passes_a_longdouble_elimination(oracle):
    """(20, 1): 52 cut cells, cond(A_TT) to 4.4e4; longdouble carries 11 bits more than double"""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.fail("numpy.longdouble is no wider than double here: the test needs the x87 extended format")
    lcs, fs, n = cut_matrices(oracle, 20, 1)
    assert len(lcs) == 52
    w = worst(lcs, fs, n, np.longdouble)
    print("longdouble elimination at (20, 1): worst record-relative error %.3e" % w)
    assert w <= judge.RECORD_GATE


def test_judge_rejects_a_plain_double_elimination(oracle):
    """(32, 2), the planted defect: 92 cut cells, cond(A_TT) to 1.2e8; plain double loses up to 7 digits"""
    lcs, fs, n = cut_matrices(oracle, 32, 2)
    assert len(lcs) == 92
    w = worst(lcs, fs, n, np.float64)
    print("plain-double elimination at (32, 2): worst record-relative error %.3e" % w)
    assert w > 1e-12


def test_judge_recovery_agrees_with_its_records():
    """u_T of exact_recover satisfies A_TT u_T + A_TF u_F = f on a well-conditioned matrix, and S u_F - g is the face residual"""
    rng = np.random.default_rng(5)
    n, NF = 6, 8
    B = rng.standard_normal((n + NF, n + NF))
    lc = B @ B.T + (n + NF) * np.eye(n + NF)
    f, uF = rng.standard_normal(n), rng.standard_normal(NF)
    uT = judge.exact_recover(lc, f, uF, n)
    assert np.abs(lc[:n, :n] @ uT + lc[:n, n:] @ uF - f).max() <= 1e-13 * np.abs(lc).max()
    S, g = judge.exact_record(lc, f, n)
    Sf = np.zeros((NF, NF))
    for j in range(NF):
        for i in range(j + 1):
            Sf[i, j] = Sf[j, i] = S[j * (j + 1) // 2 + i]
    assert np.abs(Sf @ uF - g - (lc[:n, n:].T @ uT + np.triu(lc[n:, n:]) @ uF + np.triu(lc[n:, n:], 1).T @ uF)).max() <= 1e-12 * np.abs(lc).max()


def test_drop_in_header_offers_the_condensed_fictitious_domain_solve():
    """tests/cpp/fictdom_condensed_driver.cpp compiles against proton_amd/host/cuthho.hpp and the C ABI alone (no HIP headers)"""
    assert "solve_condensed_fictdom" in open(os.path.join(ROOT, "proton_amd", "host", "hho.hpp")).read()
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "fictdom_condensed_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "fictdom_condensed_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
