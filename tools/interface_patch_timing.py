"""The condensed interface system (cuthho_square -i, face unknowns only) solved on the device by the conjugate gradient with three
preconditioners, in one process: the point Jacobi of pa_conjugated_gradient, and pa_conjugated_gradient_patch with one patch per
face ("face": both blocks of a cut face) and one patch per uncut cell and per side of a cut cell ("cell";
pa_interface_condensed_patches).  The protocol is that of tools/patch_pcg_timing.py: the system is assembled once
(pa_interface_condensed_ops_batch + pa_interface_condensed_csr_fill); after one warm-up solve of each, the three solves run in
alternating repetitions and the medians are reported: iterations, time to the tolerance, time per iteration (time / (iterations + 1):
the loop runs one update more than it counts), and on their own, with HIP events, the one-off factorisation (validation, slots,
Cholesky and inverse of every patch) and one application of the preconditioner.  The solve's time includes its own factorisation.
The divergence test is set far out (1e10) and the cap is 50000 iterations, as tools/interface_condensed_timing.py has them: its
committed Jacobi solve (profiles/interface_condensed_timing_512_k2.txt) is what the Jacobi line of this run is set beside.
    python tools/interface_patch_timing.py [N] [k] [reps] [tol] [max_iter]          (default 512 2 5 1e-9 50000)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402

DIV = 1e10
KINDS = ("jacobi", "face", "cell")
COMMITTED = {(512, 2, 1e-9): (9099, 3.193)}          # profiles/interface_condensed_timing_512_k2.txt: iterations, seconds


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    tol = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-9
    max_iter = int(sys.argv[5]) if len(sys.argv) > 5 else 50000
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    rec = asm.interface_condensed_ops(k, ops)
    del ops
    rp, ci = asm.interface_condensed_csr_pattern(k)
    va, b = asm.interface_condensed_csr_fill(k, rec, g)
    tables = {kind: asm.interface_condensed_patches(k, kind) for kind in KINDS[1:]}
    asm.synchronize()

    def solve(kind):
        asm.synchronize()
        t0 = time.perf_counter()
        if kind == "jacobi":
            x, reason, iters, rr = asm.conjugated_gradient(rp, ci, va, b, tol=tol, div=DIV, max_iter=max_iter, precond=True)
        else:
            x, reason, iters, rr = asm.conjugated_gradient_patch(rp, ci, va, b, tables[kind], tol=tol, div=DIV, max_iter=max_iter)
        asm.synchronize()
        return x, reason, iters, rr, time.perf_counter() - t0

    runs = {kind: [] for kind in KINDS}
    sols = {}
    for kind in KINDS:                                 # warm-up
        sols[kind] = solve(kind)[0]
    for _ in range(reps):
        for kind in KINDS:
            runs[kind].append(solve(kind)[1:])
    med = statistics.median
    res = {"N": N, "k": k, "cells": asm.ncells, "cut_cells": asm.ncut, "rows": b.numel(), "nnz": va.numel(), "reps": reps, "tol": tol,
           "max_iter": max_iter, "divergence_threshold": DIV, "solves": {}}
    print("interface %dx%d k=%d, face-only system: %d cells (%d cut), %d rows, %d nnz (%.0f MB of values and column indices); CG tolerance %g, "
          "cap %d; medians of %d alternating repetitions" % (N, N, k, asm.ncells, asm.ncut, b.numel(), va.numel(), va.numel() * 12 / 1e6, tol,
                                                           max_iter, reps))
    for kind in KINDS:
        reason, iters, rr = runs[kind][0][:3]
        assert all(r[:2] == (reason, iters) for r in runs[kind])
        t = med(r[3] for r in runs[kind])
        entry = {"exit_reason": reason, "iterations": iters, "relative_residual": rr, "time_s": t, "ms_per_iteration": 1e3 * t / (iters + 1)}
        line = "  %-6s: %s %5d iterations, %.3f s, %.3f ms per iteration" % (
            kind, "converged in" if reason == 0 else "NOT converged (exit %d) after" % reason, iters, t, entry["ms_per_iteration"])
        if kind == "jacobi":
            was = COMMITTED.get((N, k, tol))
            if was:
                entry["committed_iterations"], entry["committed_time_s"] = was
                line += "; committed (profiles/interface_condensed_timing_512_k2.txt): %d iterations, %.3f s" % was
        else:
            ptr, rows = tables[kind]
            pre = asm.patch_precond_factor(rp, ci, va, tables[kind])
            asm.synchronize()
            t_factor = med(timed_once(lambda: asm.patch_precond_factor(rp, ci, va, tables[kind])) for _ in range(max(reps, 5)))
            z = torch.empty_like(b)
            asm.patch_precond_apply(pre, b, z)
            t_apply = med(timed_once(lambda: asm.patch_precond_apply(pre, b, z)) for _ in range(max(reps, 5) * 4))
            t_tables = med(timed_once(lambda: asm.interface_condensed_patches(k, kind)) for _ in range(max(reps, 5)))
            sz = pre["sizes"]
            jac = res["solves"]["jacobi"]
            entry.update({"patches": ptr.numel() - 1, "entries": rows.numel(), "max_patch_rows": sz.max_patch_rows,
                          "lanes_per_patch": sz.lanes_per_patch, "tables_ms": t_tables, "factor_ms": t_factor, "apply_ms": t_apply,
                          "factor_bytes": 8 * sz.factor_doubles, "slot_bytes": 4 * sz.slot_ints, "scratch_bytes": sz.scratch_bytes,
                          "failed_patches": pre["failed"], "iterations_saved": jac["iterations"] / max(iters, 1),
                          "speedup_over_jacobi": jac["time_s"] / t,
                          "max_abs_diff_to_jacobi_rel": float((sols[kind] - sols["jacobi"]).abs().max() / sols["jacobi"].abs().max())})
            line += "; %.2f x fewer iterations, %.2f x %s in seconds than Jacobi; %d patches of up to %d rows (%d lanes each), tables %.3f ms, " \
                    "factor %.3f ms once (with the allocation of its buffers), apply %.3f ms, factors %.1f MB, slots %.1f MB, scratch %.1f MB; " \
                    "solution against Jacobi's %.2e" % (
                        entry["iterations_saved"], max(entry["speedup_over_jacobi"], 1 / entry["speedup_over_jacobi"]),
                        "faster" if entry["speedup_over_jacobi"] >= 1 else "SLOWER", entry["patches"], sz.max_patch_rows, sz.lanes_per_patch,
                        t_tables, t_factor, t_apply, entry["factor_bytes"] / 1e6, entry["slot_bytes"] / 1e6, sz.scratch_bytes / 1e6,
                        entry["max_abs_diff_to_jacobi_rel"])
        res["solves"][kind] = entry
        print(line)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
