"""The fused assembly entry (pa_assembler_csr_assemble) without a GPU: the header, the ctypes symbol list and the built
library agree on the export, and the assembling-mode instances of the local-operator kernel exist and keep the project's
"no instance may spill" rule (proton_amd/_build.py)."""
import concurrent.futures
import ctypes as C
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pa_assembler_csr_assemble"


def test_header_binding_and_library_agree_on_the_new_export():
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    assert int(re.search(r"#define PA_ABI_VERSION (\d+)", h).group(1)) == 5
    assert capi.lib().pa_abi_version() == 5
    # declared once, with the ten parameters of the issue, behind a comment that cites the reference and states the contract
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + NAME + r"\(([^;]*)\);", h, flags=re.S)
    assert m, "declaration with its comment"
    comment, params = m.group(1), re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    assert len(params.split(",")) == 10
    assert re.search(r"hho\.hpp:\d+", comment) and "BIT-IDENTICAL" in comment
    assert capi.EXPORTS.count(NAME) == 1
    fn = getattr(capi.lib(), NAME)
    assert len(fn.argtypes) == 10
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + NAME + r"$", out, flags=re.M)
    # a NULL context or a NULL values pointer is refused, not dereferenced
    assert fn(None, capi.DegreeInfo(2, 1, 2), 0, 2, None, None, None, None, None, None) == 1


# (cell degree, face degree, quadrature, min lanes) of the BASELINE.json configurations, and the stabilization / lanes-per-cell
# of the instance each one runs (the list of tests/test_build_cpu.py)
BASELINE_INSTANCES = [
    ((2, 1, 0, 16), (2, 16)),      # convergence_test / 1024^2 k=1: fancy
    ((3, 2, 0, 32), (2, 32)),      # north-star 1024^2 k=2: fancy
    ((4, 3, 0, 32), (2, 32)),      # 2048^2 k=3: fancy
    ((0, 1, 0, 16), (2, 16)),      # obstacle pair: dense fancy
    ((2, 1, 1, 16), (1, 16)),      # cuthho k=1: fan quadrature, naive
    ((3, 2, 1, 32), (1, 32)),      # cuthho k=2
]


def test_assembling_mode_instances_exist_and_do_not_spill():
    """tools/spills.py names the fourth mode and reports one `asm` instance per baseline configuration.  k = 1 and k = 2: no
    spilled register, no scratch.  k = 3 ((4, 3) tensor, fancy, 32 lanes): what the `cond` instance of that configuration
    shows before this mode was added -- 237 VGPRs, 0 spilled, 0 bytes of scratch -- so 0 / 0 here as well."""
    spec = importlib.util.spec_from_file_location("pa_spills", os.path.join(ROOT, "tools", "spills.py"))
    sp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sp)
    with concurrent.futures.ThreadPoolExecutor(max_workers=6) as ex:
        results = list(ex.map(sp.one, [c for c, _ in BASELINE_INSTANCES]))
    for (cfg, (stab, lanes)), rows in zip(BASELINE_INSTANCES, results):
        hit = [r for r in rows if r[0] == (cfg[0], cfg[1], cfg[2], stab, lanes) and r[1] == "asm"]
        assert len(hit) == 1, (cfg, rows)
        _, _, vgpr, spilled, scratch = hit[0]
        assert spilled == 0 and scratch == 0, (cfg, hit[0])
        # the mode rides on the condensed mode's instance: one of each, and the condensed one is still there
        assert len([r for r in rows if r[0] == hit[0][0] and r[1] == "cond"]) == 1
