"""Timing of the "Matrix assembly" span of the fictitious-domain driver (cuthho_square.cpp:881-905) on the device, two paths on
identical input in one process, alternating, with HIP events after a warm-up and a settle phase:
  two-step: pa_local_ops_batch(FAN, NAIVE) (lc of every cell to HBM) + pa_cut_uncut_rhs_batch + pa_cut_local_ops_batch + pa_cut_merge
            + pa_assembler_csr_fill (lc read back, gathered);
  fused:    pa_cut_uncut_rhs_batch + pa_cut_local_ops_batch + pa_fictdom_csr_assemble with d_lc = NULL (values written from the
            operator kernel's on-chip image, the cut cells' matrices through the same scatter).
The preprocessing and the pattern are built once, outside both.  Before timing, values and RHS of the two paths are compared.
    python tools/fictdom_csr_timing.py [N] [reps] [k]          (default 512 15 2; circle of radius 0.35, 4 refinement steps)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402

WHERE = pa.capi.LOC_NEGATIVE
RHS_FN, BCS_FN = pa.capi.FN_SIN_SIN_RHS, pa.capi.FN_SIN_SIN_SOL


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    cd, fd = k + 1, k
    asm = BatchAssembler(0)
    ncut = asm.cut_preprocess(N, radius=0.35, refsteps=4)
    di, _ = pa.capi.degree_info(cd, fd)
    sz = pa.capi.sizes_for(di, pa.QUAD_FAN)
    nc, ctx, ls = asm.ncells, asm.ctx, asm.level_set
    g = asm.dirichlet_data(fd, BCS_FN)
    rowptr, colind = asm.assembler_csr_pattern(cd, fd)
    f64 = dict(dtype=torch.float64, device=asm.device)
    nnz, nrows = colind.numel(), rowptr.numel() - 1
    lc = torch.empty((nc, sz.msize, sz.msize), **f64)
    rhs = torch.empty((nc, sz.cbs), **f64)
    cut_lc = torch.empty((max(ncut, 1), sz.msize, sz.msize), **f64)
    cut_rhs = torch.empty((max(ncut, 1), sz.cbs), **f64)
    va_a, RHS_a = torch.empty(nnz, **f64), torch.empty(nrows, **f64)
    va_b, RHS_b = torch.empty(nnz, **f64), torch.empty(nrows, **f64)

    def rhs_and_cut():                                    # common to both paths
        ctx.cut_uncut_rhs(cd, WHERE, RHS_FN, rhs.data_ptr())
        ctx.cut_local_ops(fd, ls, WHERE, RHS_FN, BCS_FN, lc=cut_lc.data_ptr(), rhs=cut_rhs.data_ptr())

    def two_step():
        ctx.local_ops(di, pa.QUAD_FAN, pa.STAB_NAIVE, 0, nc, lc=lc.data_ptr())
        rhs_and_cut()
        ctx.cut_merge(fd, WHERE, cut_lc.data_ptr(), cut_rhs.data_ptr(), lc.data_ptr(), rhs.data_ptr())
        ctx.assembler_csr_fill(di, lc.data_ptr(), rhs.data_ptr(), g.data_ptr(), va_a.data_ptr(), RHS_a.data_ptr())

    def fused():
        rhs_and_cut()
        ctx.fictdom_csr_assemble(fd, WHERE, rhs.data_ptr(), g.data_ptr(), cut_lc.data_ptr(), cut_rhs.data_ptr(), va_b.data_ptr(),
                                 RHS_b.data_ptr(), None, None)

    two_step(); fused()                                   # warm-up: code objects, the context's record buffer, the cut lists, the scatter table
    asm.synchronize()
    equal_v, equal_r = bool(torch.equal(va_a, va_b)), bool(torch.equal(RHS_a, RHS_b))
    dv = float((va_a - va_b).abs().max()) / float(va_a.abs().max())
    dr = float((RHS_a - RHS_b).abs().max()) / max(float(RHS_a.abs().max()), 1e-300)
    t_end = time.perf_counter() + 1.0                     # settle: a second of the alternating work before the first timed repeat
    while time.perf_counter() < t_end:
        two_step(); fused()
        asm.synchronize()
    ta, tb = [], []
    for _ in range(reps):                                 # alternating: both paths see the same clocks and the same neighbours
        ta.append(timed_once(two_step))
        tb.append(timed_once(fused))
    ma, mb = statistics.median(ta), statistics.median(tb)
    res = {"N": N, "k": k, "cells": nc, "cut_cells": ncut, "nrows": nrows, "nnz": nnz, "reps": reps,
           "two_step_ms": ma, "two_step_min_ms": min(ta), "two_step_max_ms": max(ta),
           "fused_ms": mb, "fused_min_ms": min(tb), "fused_max_ms": max(tb), "fused_over_two_step": mb / ma,
           "lc_buffer_bytes": 8 * nc * sz.msize * sz.msize, "values_bit_identical": equal_v, "RHS_bit_identical": equal_r,
           "values_rel_diff": dv, "RHS_rel_diff": dr}
    print("%dx%d k=%d (%d cells, %d cut, %d rows, %d nnz): two-step %.3f ms (min %.3f, max %.3f)  fused %.3f ms (min %.3f, max %.3f)  fused / two-step %.3f"
          % (N, N, k, nc, ncut, nrows, nnz, ma, min(ta), max(ta), mb, min(tb), max(tb), mb / ma))
    print("  lc buffer the fused path does not need: %.2f GB; values bit-identical: %s, RHS bit-identical: %s (largest relative difference %.2e / %.2e)"
          % (res["lc_buffer_bytes"] / 1e9, equal_v, equal_r, dv, dr))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
