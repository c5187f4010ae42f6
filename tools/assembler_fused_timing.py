"""Timing of the "Matrix assembly" span (convergence_test.cpp:201-217) of the uncondensed system on the device, two paths on identical
input in one process, alternating, with HIP events after a warm-up and a settle phase:
  two-step: pa_local_ops_batch (lc to HBM) + pa_cell_rhs_batch + pa_assembler_csr_fill (lc read back, gathered);
  fused:    pa_cell_rhs_batch + pa_assembler_csr_assemble with d_lc = NULL (values written from the kernel's on-chip image).
The pattern is built once, outside both.  Before timing, values and RHS of the two paths are compared.
    python tools/assembler_fused_timing.py [N] [reps] [k ...]          (default 1024 15 2 1 3; tensor quadrature, fancy stabilization)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def one_degree(asm, N, k, reps):
    cd, fd = k + 1, k
    quad, stab = pa.QUAD_TENSOR, pa.STAB_FANCY
    di, _ = pa.capi.degree_info(cd, fd)
    sz = pa.capi.sizes_for(di, quad)
    asm.generate_mesh(N, N)
    nc = asm.ncells
    g = asm.dirichlet_data(fd, pa.capi.FN_SIN_SIN_SOL)
    rowptr, colind = asm.assembler_csr_pattern(cd, fd)
    f64 = dict(dtype=torch.float64, device=asm.device)
    nnz, nrows = colind.numel(), rowptr.numel() - 1
    lc = torch.empty((nc, sz.msize, sz.msize), **f64)
    rhs = torch.empty((nc, sz.cbs), **f64)
    va_a, RHS_a = torch.empty(nnz, **f64), torch.empty(nrows, **f64)
    va_b, RHS_b = torch.empty(nnz, **f64), torch.empty(nrows, **f64)
    ctx = asm.ctx

    def cell_rhs():
        ctx.cell_rhs(cd, 0, quad, pa.capi.FN_SIN_SIN_RHS, 0, nc, rhs.data_ptr())

    def two_step():
        ctx.local_ops(di, quad, stab, 0, nc, lc=lc.data_ptr())
        cell_rhs()
        ctx.assembler_csr_fill(di, lc.data_ptr(), rhs.data_ptr(), g.data_ptr(), va_a.data_ptr(), RHS_a.data_ptr())

    def fused():
        cell_rhs()
        ctx.assembler_csr_assemble(di, quad, stab, rhs.data_ptr(), g.data_ptr(), va_b.data_ptr(), RHS_b.data_ptr(), None, None)

    two_step(); fused()                                   # warm-up: code objects, the context's record buffer, the scatter table
    asm.synchronize()
    scale = float(va_a.abs().max())
    dv = float((va_a - va_b).abs().max()) / scale
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
    res = {"N": N, "k": k, "cells": nc, "nrows": nrows, "nnz": nnz, "reps": reps,
           "two_step_ms": ma, "two_step_min_ms": min(ta), "two_step_max_ms": max(ta),
           "fused_ms": mb, "fused_min_ms": min(tb), "fused_max_ms": max(tb), "fused_over_two_step": mb / ma,
           "lc_buffer_bytes": 8 * nc * sz.msize * sz.msize, "values_rel_diff": dv, "RHS_rel_diff": dr}
    print("%dx%d k=%d (%d cells, %d rows, %d nnz): two-step %.3f ms (min %.3f, max %.3f)  fused %.3f ms (min %.3f, max %.3f)  fused / two-step %.3f"
          % (N, N, k, nc, nrows, nnz, ma, min(ta), max(ta), mb, min(tb), max(tb), mb / ma))
    print("  lc buffer the fused path does not need: %.2f GB; values differ by %.2e, RHS by %.2e (relative to the largest entry)"
          % (res["lc_buffer_bytes"] / 1e9, dv, dr))
    print(json.dumps(res), flush=True)
    del lc, va_a, va_b, RHS_a, RHS_b
    torch.cuda.empty_cache()


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    ks = [int(a) for a in sys.argv[3:]] or [2, 1, 3]
    asm = BatchAssembler(0)
    for k in ks:
        one_degree(asm, N, k, reps)


if __name__ == "__main__":
    main()
