"""Timing of one assembly of the obstacle problem's global system (obstacle_assembler::assemble for every cell + finalize,
hho.hpp:609-695, :746-750: the span obstacle.cpp:147-158 repeats in every active-set iteration) on the device, two routes on
identical input in one process, alternating, with HIP events after a warm-up and a settle phase:
  triplets: pa_obstacle_triplets_batch (msize^2 + 1 slots per cell) + pa_csr_from_triplets (sort and reduce) + the scatter-add of
            the per-row right-hand-side sums (on the device here, torch index_add_; the C++ header downloads them and scatters
            on the host, which costs more);
  direct:   pa_obstacle_csr_assemble (row pointers, column indices, values and right-hand side in CSR, no triplets, no sort).
Setup: N x N cells on [-1,1]^2, pair (0, k), the active set the contact disc r < 0.7 of obstacle.cpp at the barycentres.  The
local operators, right-hand sides, boundary data and the tables of the active set are built once, outside both.  Before timing,
the outputs of the two routes are compared.
    python tools/obstacle_csr_timing.py [N] [reps] [k]          (default 512 25 1)"""
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


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    asm = BatchAssembler(0)
    asm.generate_mesh(N, N, (-1.0, -1.0), (1.0, 1.0))
    ctx, nc = asm.ctx, asm.ncells
    di = pa.capi.DegreeInfo(0, k, k + 1)
    ms = 1 + 4 * (k + 1)
    lc = asm.local_ops(0, k, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
    rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
    g = asm.dirichlet_data(k, pa.capi.FN_OBSTACLE_SOL)
    x = -1.0 + (torch.arange(N, dtype=torch.float64, device=asm.device) + 0.5) * 2.0 / N
    in_A = ((x[None, :] ** 2 + x[:, None] ** 2).sqrt() < 0.7).reshape(-1).to(torch.uint8).contiguous()
    gamma = torch.zeros(nc, dtype=torch.float64, device=asm.device)          # obstacle_fun = 0 (obstacle.cpp:113)
    A_ct, B_ct, num_I, num_A = asm.obstacle_tables(in_A)
    info = ctx.assembler_csr_query(di)
    nrows, cap = info.nrows, info.nnz
    i32, i64, f64 = (dict(dtype=t, device=asm.device) for t in (torch.int32, torch.int64, torch.float64))
    slots = nc * (ms * ms + 1)
    # triplet route: the slots, and CSR buffers of the same worst-case capacity
    rows, cols, vals = torch.empty(slots, **i32), torch.empty(slots, **i32), torch.empty(slots, **f64)
    rr, rv = torch.empty(nc * ms, **i32), torch.empty(nc * ms, **f64)
    rp_a, ci_a, va_a = torch.empty(nrows + 1, **i64), torch.empty(slots, **i32), torch.empty(slots, **f64)
    RHS_a = torch.empty(nrows + 1, **f64)                                    # the last entry takes the Dirichlet rows' zeros
    # direct route: buffers of pa_assembler_csr_query's sizes
    rp_b, ci_b, va_b, RHS_b = torch.empty(nrows + 1, **i64), torch.empty(cap, **i32), torch.empty(cap, **f64), torch.empty(nrows, **f64)
    nnz = [0, 0]

    def triplets():
        ctx.obstacle_triplets(di, 0, nc, lc.data_ptr(), rhs.data_ptr(), g.data_ptr(), gamma.data_ptr(), in_A.data_ptr(), A_ct.data_ptr(),
                              B_ct.data_ptr(), num_I, rows.data_ptr(), cols.data_ptr(), vals.data_ptr(), rr.data_ptr(), rv.data_ptr())
        nnz[0] = ctx.csr_from_triplets(slots, rows.data_ptr(), cols.data_ptr(), vals.data_ptr(), nrows, rp_a.data_ptr(), ci_a.data_ptr(),
                                       va_a.data_ptr())
        RHS_a.zero_()
        RHS_a.index_add_(0, torch.where(rr >= 0, rr, nrows).long(), rv)

    def direct():
        nnz[1] = ctx.obstacle_csr_assemble(di, lc.data_ptr(), rhs.data_ptr(), g.data_ptr(), gamma.data_ptr(), in_A.data_ptr(),
                                           A_ct.data_ptr(), B_ct.data_ptr(), num_I, rp_b.data_ptr(), ci_b.data_ptr(), va_b.data_ptr(),
                                           RHS_b.data_ptr())

    triplets(); direct()                                  # warm-up: code objects, the context's adjacency tables
    asm.synchronize()
    same = {"nnz": nnz[0] == nnz[1], "rowptr": bool(torch.equal(rp_a, rp_b)),
            "colind": bool(torch.equal(ci_a[:nnz[0]], ci_b[:nnz[1]])), "values": bool(torch.equal(va_a[:nnz[0]], va_b[:nnz[1]]))}
    # the device scatter adds a row's two sums in arrival order: compared to rounding, not bit for bit (the tests compare the
    # cell-order sum bit for bit)
    drhs = float((RHS_a[:nrows] - RHS_b).abs().max()) / max(float(RHS_b.abs().max()), 1e-300)
    t_end = time.perf_counter() + 1.0                     # settle: a second of the alternating work before the first timed repeat
    while time.perf_counter() < t_end:
        triplets(); direct()
        asm.synchronize()
    ta, tb = [], []
    for _ in range(reps):                                 # alternating: both routes see the same clocks and the same neighbours
        ta.append(timed_once(triplets))
        tb.append(timed_once(direct))
    ma, mb = statistics.median(ta), statistics.median(tb)
    res = {"N": N, "k": k, "cells": nc, "active_cells": num_A, "nrows": nrows, "nnz": nnz[1], "nnz_capacity": cap, "slots": slots,
           "reps": reps, "triplets_ms": ma, "triplets_min_ms": min(ta), "triplets_max_ms": max(ta),
           "direct_ms": mb, "direct_min_ms": min(tb), "direct_max_ms": max(tb), "direct_over_triplets": mb / ma,
           "triplet_buffer_bytes": 16 * slots, "bit_identical": same, "RHS_rel_diff": drhs}
    print("%dx%d pair (0,%d) (%d cells, %d active, %d rows, %d nnz): triplets %.3f ms (min %.3f, max %.3f)  direct %.3f ms (min %.3f, max %.3f)  direct / triplets %.3f"
          % (N, N, k, nc, num_A, nrows, nnz[1], ma, min(ta), max(ta), mb, min(tb), max(tb), mb / ma))
    print("  triplet slots the direct route does not need: %d (%.2f GB of rows, cols and vals); nnz / rowptr / colind / values bit-identical: %s / %s / %s / %s; largest relative difference of the right-hand sides %.2e"
          % (slots, res["triplet_buffer_bytes"] / 1e9, same["nnz"], same["rowptr"], same["colind"], same["values"], drhs))
    print(json.dumps(res), flush=True)
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
