"""The interface problem (cuthho_square -i) solved through its face-only system against the full system, on the device, with HIP
events after a warm-up.  Full: pa_interface_csr_fill (cell + face unknowns).  Condensed: the records (pa_interface_condensed_ops_batch:
uncut cells in double, cut cells in double-double) + pa_interface_condensed_csr_fill, then pa_interface_condensed_recover after the
solve.  Both systems go to pa_conjugated_gradient with Jacobi to the same tolerance.  The divergence test is set far out (1e10
instead of the reference's 100, which the Jacobi-PCG residual of the 512 x 512 systems crosses in its first iterations): the
tool measures the iterations to the tolerance.  A tolerance of 0 skips the two solves (the recovery is then timed on the condensed
right-hand side in place of a solution): the kernel timings alone, in seconds.
    python tools/interface_condensed_timing.py [N] [k] [reps] [tol]          (default 512 2 10 1e-9)"""
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


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def cg(asm, rp, ci, va, b, tol, max_iter):
    asm.synchronize()
    t0 = time.perf_counter()
    x, reason, iters, relres = asm.conjugated_gradient(rp, ci, va, b, tol=tol, div=DIV, max_iter=max_iter, precond=True)
    asm.synchronize()
    return x, {"converged": reason == 0, "exit_reason": reason, "iterations": iters, "relative_residual": relres,
               "time_s": time.perf_counter() - t0}


def cg_text(r, max_iter):
    if r is None:
        return "no solve"
    if r["converged"]:
        return "CG converged in %d iterations, %.3f s, relative residual %.3e" % (r["iterations"], r["time_s"], r["relative_residual"])
    why = "max_iter %d reached" % max_iter if r["exit_reason"] == 2 else "exit reason %d" % r["exit_reason"]
    return "CG NOT converged (%s) after %d iterations, %.3f s, relative residual %.3e: no time to the tolerance" % (
        why, r["iterations"], r["time_s"], r["relative_residual"])


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    tol = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-9
    max_iter = 50000
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    info = asm.ctx.interface_info(k)
    qi = asm.ctx.interface_condensed_query(k)
    asm.synchronize()

    # full system
    rp, ci = asm.interface_csr_pattern(k)
    va = torch.empty(ci.numel(), dtype=torch.float64, device=asm.device)
    RH = torch.empty(info.system_size, dtype=torch.float64, device=asm.device)
    asm.interface_csr_fill(k, ops, g, va, RH)
    t_full_fill = timed(lambda: asm.interface_csr_fill(k, ops, g, va, RH), reps)
    full_nnz = ci.numel()

    # condensed system
    crp, cci = asm.interface_condensed_csr_pattern(k)
    cva = torch.empty(max(qi.nnz, 1), dtype=torch.float64, device=asm.device)
    cRH = torch.empty(max(qi.system_size, 1), dtype=torch.float64, device=asm.device)
    rec = asm.interface_condensed_ops(k, ops)
    asm.interface_condensed_csr_fill(k, rec, g, cva, cRH)
    asm.synchronize()
    t_rec = timed(lambda: asm.interface_condensed_ops(k, ops), reps)
    t_cfill = timed(lambda: asm.interface_condensed_csr_fill(k, rec, g, cva, cRH), reps)
    t_both = timed(lambda: asm.interface_condensed_csr_fill(k, asm.interface_condensed_ops(k, ops), g, cva, cRH), reps)
    info_bad = int((rec["info"] != 0).sum()) + int((rec["info_cut"] != 0).sum())

    solve = tol > 0
    xF, cg_cond = cg(asm, crp, cci, cva[:qi.nnz], cRH[:qi.system_size], tol, max_iter) if solve else (cRH[:qi.system_size].clone(), None)
    asm.interface_condensed_recover(k, ops, xF, g)
    t_recover = timed(lambda: asm.interface_condensed_recover(k, ops, xF, g), reps)
    full_x = asm.interface_condensed_recover(k, ops, xF, g)
    del rec, crp, cci, cva, cRH
    torch.cuda.empty_cache()
    x, cg_full = cg(asm, rp, ci, va, RH, tol, max_iter) if solve else (None, None)
    asm.synchronize()
    # the two solutions are compared only if both reached the tolerance (an unconverged iterate says nothing about the recovery)
    diff = float((full_x - x).abs().max()) / float(x.abs().max()) if solve and cg_full["converged"] and cg_cond["converged"] else None

    res = {"N": N, "k": k, "cells": asm.ncells, "cut_cells": asm.ncut, "reps": reps, "tol": tol, "divergence_threshold": DIV,
           "full": {"rows": info.system_size, "nnz": full_nnz, "fill_ms": statistics.median(t_full_fill), "cg": cg_full},
           "condensed": {"rows": qi.system_size, "nnz": qi.nnz, "records_ms": statistics.median(t_rec),
                         "fill_ms": statistics.median(t_cfill), "records_plus_fill_ms": statistics.median(t_both),
                         "recover_ms": statistics.median(t_recover), "nonzero_info": info_bad, "cg": cg_cond},
           "max_abs_diff_of_solutions_rel": diff}
    print("interface %dx%d k=%d: %d cells (%d cut), CG tolerance %g with Jacobi" % (N, N, k, asm.ncells, asm.ncut, tol))
    print("  full:      %d rows, %d nnz; fill %.3f ms; %s" % (info.system_size, full_nnz, res["full"]["fill_ms"], cg_text(cg_full, max_iter)))
    print("  condensed: %d rows, %d nnz; records %.3f ms + fill %.3f ms (together %.3f ms); recovery %.3f ms; %s" %
          (qi.system_size, qi.nnz, res["condensed"]["records_ms"], res["condensed"]["fill_ms"], res["condensed"]["records_plus_fill_ms"],
           res["condensed"]["recover_ms"], cg_text(cg_cond, max_iter)))
    if diff is not None:
        print("  recovered full vector against the full system's CG solution: max |dx| / max |x| = %.3e" % diff)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
