"""The condensed face-only systems solved on the device by the conjugate gradient with the cell patches and (a) one exactly solved
hat level, pa_conjugated_gradient_patch_coarse -- the two-level routes, the yardstick -- or (b) smoothed hat levels below an exact
one, pa_conjugated_gradient_multilevel, in one process: plain Poisson (a random right-hand side, tolerance 1e-9, one part), the
fictitious-domain problem (cuthho_square -f, 1e-13, hats split by side) and, up to 512^2, the interface problem (cuthho_square -i,
1e-9, one part and by side, kappa = (1, 1) and (1, 1e4)).  Each system is assembled once.  A route is (levels, exact H); after one
warm-up solve of each route the solves run in alternating repetitions and the medians are reported: iterations, seconds to the
tolerance -- the route's tables (built inside the timed span, the table cap raised for the smoothed levels' and put back) and the
solve's own set-up (patch factors, every level's transpose and diagonal, the exact level's factor) included --, time per iteration
(seconds / (iterations + 1): the loop runs one update more than it counts).  On their own, with HIP events: the set-up of the
route's levels (pa_smoothed_level_setup of each, pa_coarse_precond_factor of the exact one) and the bytes held while the solve
runs (patch factors, tables, transposes, D^-1, the exact factor, scratch).  A route whose exact table the entry refuses (more than
4096 columns) is reported as refused.  The divergence test is set far out (1e10), as tools/coarse_pcg_timing.py has it.
    python tools/multilevel_pcg_timing.py [N,N,...] [k] [reps] [max_iter]                   (default 512,1024 2 5 50000)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from coarse_pcg_timing import fictdom_system, poisson_system, timed_once  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402

DIV = 1e10
NEG = pa.capi.LOC_NEGATIVE
ROUTES = (((), 16), ((), 32), ((4, 8), 16), ((2, 4, 8), 16), ((2, 4, 8, 16), 32))
INTERFACE_MAX_N = 512


def route_name(levels, exact):
    return ("smoothed {%s} + exact %d" % (", ".join(map(str, levels)), exact)) if levels else "two-level, exact %d" % exact


def problems(asm, N, k):
    """-> (name, tolerance, system, patches, table(H)) one after the other; a system lives until the next one is asked for"""
    cd = k + 1
    rp, ci, va, b = poisson_system(asm, N, k)
    yield "Poisson", 1e-9, (rp, ci, va, b), asm.condensed_patches(cd, k, "cell"), lambda H: asm.condensed_coarse(cd, k, H, "one")
    rp, ci, va, b = fictdom_system(asm, N, k)
    yield ("fictitious domain, by side", 1e-13, (rp, ci, va, b), asm.condensed_patches(cd, k, "cell"),
           lambda H: asm.condensed_coarse(cd, k, H, "side", NEG))
    if N > INTERFACE_MAX_N:
        return
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    for kappa_2 in (1.0, 1e4):
        ops = asm.interface_local_ops(k, kappa=(1.0, kappa_2))
        rec = asm.interface_condensed_ops(k, ops)
        del ops
        rp, ci = asm.interface_condensed_csr_pattern(k)
        va, b = asm.interface_condensed_csr_fill(k, rec, g)
        del rec
        cell = asm.interface_condensed_patches(k, "cell")
        for parts in ("one", "side"):
            yield ("interface kappa (1, %g), %s" % (kappa_2, parts), 1e-9, (rp, ci, va, b), cell,
                   lambda H, parts=parts: asm.interface_condensed_coarse(k, H, parts))


def build_tables(asm, table, levels, exact):
    cap = asm.ctx.coarse_table_cap
    asm.ctx.set_coarse_table_cap(pa.capi.SMOOTHED_MAX_NODES)
    try:
        lv = [table(H) for H in levels]
    finally:
        asm.ctx.set_coarse_table_cap(cap)
    return lv, table(exact)


def solve(asm, system, cell, table, levels, exact, tol, max_iter):
    rp, ci, va, b = system
    asm.synchronize()
    t0 = time.perf_counter()
    lv, ex = build_tables(asm, table, levels, exact)
    if levels:
        x, reason, iters, rr = asm.conjugated_gradient_multilevel(rp, ci, va, b, cell, lv, ex, tol=tol, div=DIV, max_iter=max_iter)
    else:
        x, reason, iters, rr = asm.conjugated_gradient_patch_coarse(rp, ci, va, b, cell, ex, tol=tol, div=DIV, max_iter=max_iter)
    asm.synchronize()
    return time.perf_counter() - t0, iters, reason, rr


def setup_and_bytes(asm, system, cell, table, levels, exact, reps):
    rp, ci, va, _ = system
    lv, ex = build_tables(asm, table, levels, exact)
    held = lambda tb: tb[0].numel() * 8 + tb[1].numel() * 12

    def once():
        out = [asm.smoothed_level_setup(rp, ci, va, tb) for tb in lv]
        return out, asm.coarse_precond_factor(rp, ci, va, ex)
    pres, pre = once()
    asm.synchronize()
    ms = statistics.median(timed_once(once) for _ in range(max(reps, 3)))
    pc = asm.patch_precond_factor(rp, ci, va, cell)
    total = 8 * pc["sizes"].factor_doubles + 4 * pc["sizes"].slot_ints + pc["sizes"].scratch_bytes
    total += held(ex) + pre["sizes"].pt_bytes + 8 * pre["sizes"].factor_doubles + pre["sizes"].scratch_bytes
    for tb, p in zip(lv, pres):
        total += held(tb) + p["sizes"].pt_bytes + 8 * p["sizes"].dinv_doubles + p["sizes"].scratch_bytes
    return ms, int(total), [tb[3] for tb in lv], ex[3]


def main():
    a = sys.argv[1:]
    Ns = [int(x) for x in (a[0] if a else "512,1024").split(",")]
    k = int(a[1]) if len(a) > 1 else 2
    reps = int(a[2]) if len(a) > 2 else 5
    max_iter = int(a[3]) if len(a) > 3 else 50000
    med = statistics.median
    asm = BatchAssembler(0)
    out = {"k": k, "reps": reps, "max_iter": max_iter, "divergence_threshold": DIV, "device": torch.cuda.get_device_name(0), "runs": []}
    for N in Ns:
        for name, tol, system, cell, table in problems(asm, N, k):
            print("\n%s, %d^2 cells, k = %d, tolerance %g: %d rows, %d patches" % (name, N, k, tol, system[3].numel(), cell[0].numel() - 1), flush=True)
            live = []
            for levels, exact in ROUTES:
                try:
                    solve(asm, system, cell, table, levels, exact, tol, max_iter)                 # warm-up, and whether the route is served
                    live.append((levels, exact))
                except pa.capi.ProtonAmdError as e:
                    print("  %-36s refused: %s" % (route_name(levels, exact), str(e).split(": ", 1)[-1]), flush=True)
            runs = {r: [] for r in live}
            for _ in range(reps):
                for r in live:
                    runs[r].append(solve(asm, system, cell, table, r[0], r[1], tol, max_iter))
            best = None
            for levels, exact in live:
                rs = runs[(levels, exact)]
                sec, iters = med(x[0] for x in rs), rs[0][1]
                ms, held, ncs, nce = setup_and_bytes(asm, system, cell, table, levels, exact, reps)
                if not levels and (best is None or sec < best):
                    best = sec
                assert all(x[1] == iters and x[2] == rs[0][2] for x in rs)                          # the same bits from call to call
                print("  %-36s %6d iterations (exit %d, rr %.2e) %8.4f s  %7.3f ms/iteration  set-up %7.2f ms  %7.1f MB held  columns %s + %d%s"
                      % (route_name(levels, exact), iters, rs[0][2], rs[0][3], sec, 1e3 * sec / (iters + 1), ms, held / 1e6,
                         "/".join(map(str, ncs)) or "-", nce, ("  %.2f x the best two-level route" % (best / sec)) if levels and best else ""),
                      flush=True)
                out["runs"].append({"problem": name, "N": N, "tol": tol, "levels": list(levels), "exact": exact, "iterations": iters,
                                    "exit": rs[0][2], "seconds": sec, "ms_per_iteration": 1e3 * sec / (iters + 1), "setup_ms": ms,
                                    "bytes_held": held, "level_columns": ncs, "exact_columns": nce})
            del system, cell, table
    print("\n" + json.dumps(out))


if __name__ == "__main__":
    main()
