"""The fictitious-domain problem (cuthho_square -f) solved through its face-only system against the full system, on the device, in
one process, with HIP events after a warm-up; the two assemblies are timed in alternating repetitions and the medians reported.
Full: pa_fictdom_csr_assemble (cell + face unknowns).  Condensed: the records (pa_fictdom_condensed_ops_batch: uncut cells from the
fused condensed pass, cut cells in double-double) + pa_condensed_csr_fill, then pa_fictdom_condensed_recover after the solve.  Both
systems go to pa_conjugated_gradient with Jacobi at the -f driver's threshold, under an iteration cap so that the full system
cannot run away.  The divergence test is set far out (1e10 instead of the reference's 100), as tools/interface_condensed_timing.py
does: the tool measures the iterations to the tolerance.  A tolerance of 0 skips the two solves (the recovery is then timed on the
condensed right-hand side in place of a solution).
    python tools/fictdom_condensed_timing.py [N] [k] [reps] [tol] [max_iter]          (default 512 2 10 1e-13 20000)"""
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
NEG = pa.capi.LOC_NEGATIVE


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, reps):
    """one repetition = every function once, in turn -> the list of times of each"""
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            out[i].append(timed_once(fn))
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
    why = "iteration cap %d reached" % max_iter if r["exit_reason"] == 2 else "exit reason %d" % r["exit_reason"]
    return "CG NOT converged (%s) after %d iterations, %.3f s, relative residual %.3e: no time to the tolerance" % (
        why, r["iterations"], r["time_s"], r["relative_residual"])


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    tol = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-13
    max_iter = int(sys.argv[5]) if len(sys.argv) > 5 else 20000
    cd = k + 1
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    f64 = dict(dtype=torch.float64, device=asm.device)
    rhs = torch.empty((asm.ncells, (cd + 1) * (cd + 2) // 2), **f64)
    asm.ctx.cut_uncut_rhs(cd, NEG, pa.capi.FN_SIN_SIN_RHS, rhs.data_ptr())
    cut = asm.cut_local_ops(k, NEG, want=("lc", "rhs"))
    asm.synchronize()

    # both systems once (warm-up: tables, scratch), into buffers the timed calls reuse
    rp, ci = asm.assembler_csr_pattern(cd, k)
    full = asm.fictdom_csr_scatter(k, NEG, rhs, g, cut["lc"], cut["rhs"])
    va, RH = full["values"], full["RHS"]
    crp, cci = asm.condensed_csr_pattern(cd, k)
    rec = asm.fictdom_condensed_records(k, NEG, rhs, cut["lc"], cut["rhs"])
    cva, cRH = asm.condensed_csr_fill(cd, k, rec["cond"], g)
    asm.synchronize()
    info_bad = int((rec["info"] != 0).sum()) + int((rec["info_cut"] != 0).sum())

    def full_assemble():
        asm.fictdom_csr_scatter(k, NEG, rhs, g, cut["lc"], cut["rhs"], values=va, RHS=RH)

    def records():
        asm.fictdom_condensed_records(k, NEG, rhs, cut["lc"], cut["rhs"], out=rec["cond"])

    def fill():
        asm.condensed_csr_fill(cd, k, rec["cond"], g, values=cva, rhs=cRH)

    def records_and_fill():
        records()
        fill()

    t_full, t_both, t_rec, t_fill = alternating([full_assemble, records_and_fill, records, fill], reps)

    solve = tol > 0
    xF, cg_cond = cg(asm, crp, cci, cva, cRH, tol, max_iter) if solve else (cRH.clone(), None)
    out = asm.fictdom_condensed_recover(k, xF, NEG, rhs, cut["lc"], cut["rhs"], g)
    t_recover = alternating([lambda: asm.fictdom_condensed_recover(k, xF, NEG, rhs, cut["lc"], cut["rhs"], g, full=out)], reps)[0]
    x, cg_full = cg(asm, rp, ci, va, RH, tol, max_iter) if solve else (None, None)
    asm.synchronize()
    # the two solutions are compared only if both reached the tolerance (an unconverged iterate says nothing about the recovery)
    diff = float((out - x).abs().max()) / float(x.abs().max()) if solve and cg_full["converged"] and cg_cond["converged"] else None

    med = statistics.median
    res = {"N": N, "k": k, "cells": asm.ncells, "cut_cells": asm.ncut, "reps": reps, "tol": tol, "max_iter": max_iter,
           "divergence_threshold": DIV,
           "full": {"rows": RH.numel(), "nnz": va.numel(), "assemble_ms": med(t_full), "cg": cg_full},
           "condensed": {"rows": cRH.numel(), "nnz": cva.numel(), "records_ms": med(t_rec), "fill_ms": med(t_fill),
                         "records_plus_fill_ms": med(t_both), "recover_ms": med(t_recover), "nonzero_info": info_bad, "cg": cg_cond},
           "max_abs_diff_of_solutions_rel": diff}
    print("fictitious domain %dx%d k=%d: %d cells (%d cut), CG tolerance %g with Jacobi, iteration cap %d; medians of %d alternating repetitions"
          % (N, N, k, asm.ncells, asm.ncut, tol, max_iter, reps))
    print("  full:      %d rows, %d nnz; pa_fictdom_csr_assemble %.3f ms; %s" % (RH.numel(), va.numel(), med(t_full), cg_text(cg_full, max_iter)))
    print("  condensed: %d rows, %d nnz; records %.3f ms + fill %.3f ms (together %.3f ms); recovery %.3f ms; nonzero infos %d; %s" %
          (cRH.numel(), cva.numel(), med(t_rec), med(t_fill), med(t_both), med(t_recover), info_bad, cg_text(cg_cond, max_iter)))
    if diff is not None:
        print("  recovered full vector against the full system's CG solution: max |dx| / max |x| = %.3e" % diff)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
