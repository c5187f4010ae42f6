#!/usr/bin/env python3
"""Register footprint of every local-operator kernel instance (compiled to assembly with the flags _build.py uses):
name, VGPRs, spilled VGPRs, scratch bytes.  A spill in the store phase costs a vmcnt(0) wait per reload.
    python tools/spills.py                          the local-operator instances
    python tools/spills.py interface_csr [...]      every kernel of csrc/<unit>.hip instead
    python tools/spills.py --isa-hash               sha256 of every instance's device listing (to prove a refactor changed no code)"""
import concurrent.futures, hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from proton_amd import _build as B

def listing(cfg):
    cd, fd, q, gmin = cfg
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        cmd = [B.hipcc()] + B.FLAGS + ["-DPA_CD=%d" % cd, "-DPA_FD=%d" % fd, "-DPA_QUAD=%d" % q, "-DPA_GMIN=%d" % gmin] + \
            B.PER_CONFIG_FLAGS.get((cd, fd, q), []) + ["--cuda-device-only", "-S", "-o", out, os.path.join(B.CSRC, "hho_inst.hip")]
        subprocess.run(cmd, check=True, capture_output=True)
        return open(out).read()

def isa_hash(cfg):
    """of the listing without the lines of the __hip_cuid_ symbol, which is derived from the source PATH"""
    return hashlib.sha256("".join(l for l in listing(cfg).splitlines(True) if "__hip_cuid_" not in l).encode()).hexdigest()[:16]

def one(cfg):
    txt = listing(cfg)
    rows = []
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt):
        name = m.group(1)
        t = re.search(r"CfgILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi\d+EEE(Li\d)?", name)
        kind = "pre" if "cell_pre" in name else "small" if "hho_small" in name else {"Li0": "lc", "Li1": "split", "Li2": "cond", "Li3": "asm"}[t.group(6)]
        rows.append((tuple(int(x) for x in t.groups()[:5]), kind, int(m.group(3)), int(m.group(4)), int(m.group(2))))
    return rows

def unit(name):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([B.hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", "-o", out, os.path.join(B.CSRC, name + ".hip")],
                       check=True, capture_output=True)
        txt = open(out).read()
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt):
        kernel = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        kernel = kernel.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "rocprim" not in kernel:
            print("%-20s %-60s vgpr %3d spilled %3d scratch %4d" % (name, kernel, int(m.group(3)), int(m.group(4)), int(m.group(2))))


if __name__ == "__main__":
    if sys.argv[1:] == ["--isa-hash"]:
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            for cfg, h in zip(B.configs(), ex.map(isa_hash, B.configs())):
                print("cd=%d fd=%d quad=%d %s" % (*cfg[:3], h))
        sys.exit(0)
    if len(sys.argv) > 1:
        for name in sys.argv[1:]:
            unit(name)
        sys.exit(0)
    bad = 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        for rows in ex.map(one, B.configs()):
            for cfg, kind, vg, sp, scr in sorted(rows):
                flag = "  <-- spills" if sp or scr else ""
                bad += bool(sp or scr)
                print("cd=%d fd=%d quad=%d stab=%d G=%-2d %-5s vgpr %3d spilled %3d scratch %4d%s" % (*cfg, kind, vg, sp, scr, flag))
    print("instances with spills:", bad)
