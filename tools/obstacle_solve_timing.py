"""Timing of one outer iteration of the obstacle problem's active-set loop (obstacle.cpp:119-193) behind the assembly, two routes
on identical input in one process, alternating, after a warm-up:
  host:   what tests/cpp/obstacle_driver.cpp does with the system of pa_obstacle_csr_assemble -- the CSR and the right-hand side
          to the host, the rows of the active cells set aside there, the remaining SPD block uploaded, pa_conjugated_gradient,
          the solution back, multipliers, expand_solution, the next active set and the stopping norm on the host (numpy,
          vectorised: the driver's loops in C++ are not faster than these);
  device: pa_obstacle_block_solve on the arrays where they are, pa_obstacle_expand_solution, pa_obstacle_active_set_update.
pa_obstacle_tables and pa_obstacle_csr_assemble open both routes and are inside both timings.  Each route is timed with the
conjugate gradient stopped after its first product (threshold = inf: the iteration's cost around the solver) and capped at a
small fixed max_iter.  Times are host clocks around work that ends in a stream synchronise (the host route is host work).
    python tools/obstacle_solve_timing.py [N] [reps] [k] [cap]          (default 512 9 1 20; the disc r < 0.7 active)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    cap = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    fbs = k + 1
    asm = BatchAssembler(0)
    asm.generate_mesh(N, N, (-1.0, -1.0), (1.0, 1.0))
    nc = asm.ncells
    nf = asm.assembler_info(0, k).nfaces_local
    lc = asm.local_ops(0, k, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
    rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
    g = asm.dirichlet_data(k, pa.capi.FN_OBSTACLE_SOL)
    x = -1.0 + (np.arange(N) + 0.5) * 2.0 / N
    X, Y = np.meshgrid(x, x)
    in_A_host = (np.sqrt(X * X + Y * Y) < 0.7).reshape(-1)
    in_A = torch.from_numpy(in_A_host.astype(np.uint8)).to(asm.device)
    gamma = torch.zeros(nc, dtype=torch.float64, device=asm.device)
    gamma_host = np.zeros(nc)
    alpha_prev = torch.zeros(nc + fbs * nf, dtype=torch.float64, device=asm.device)
    alpha_prev_host = np.zeros(nc + fbs * nf)
    face_compress = None
    out = {}

    def assemble():
        A_ct, B_ct, num_I, num_A = asm.obstacle_tables(in_A)
        return (A_ct, B_ct, num_I, num_A) + asm.obstacle_csr_assemble(k, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I)

    def device_route(tol, max_iter):
        A_ct, B_ct, num_I, num_A, rowptr, colind, values, RHS = assemble()
        sol, reason, iters, rr = asm.obstacle_block_solve(k, rowptr, colind, values, RHS, in_A, A_ct, B_ct, num_I, tol=tol, max_iter=max_iter)
        alpha, beta = asm.obstacle_expand_solution(0, k, sol, g, gamma, in_A, A_ct, B_ct, num_I, nf)
        nxt, n_next, changed, norm = asm.obstacle_active_set_update(k, alpha, beta, gamma, alpha_prev=alpha_prev, in_A_prev=in_A)
        asm.synchronize()
        out["device"] = (sol, alpha, beta, nxt, n_next, norm, iters)

    def host_route(tol, max_iter):
        A_ct, B_ct, num_I, num_A, rowptr, colind, values, RHS = assemble()
        rp, ci, va, b = rowptr.cpu().numpy(), colind.cpu().numpy(), values.cpu().numpy(), RHS.cpu().numpy()      # the CSR to the host
        n = b.shape[0]
        nk = n - num_A
        # the rows that hold a multiplier column are set aside (block_solve of obstacle_driver.cpp)
        has_mult = np.maximum.reduceat(ci >= nk, rp[:-1]) if ci.size else np.zeros(n, dtype=bool)
        kept = np.nonzero(~has_mult)[0]
        assert kept.shape[0] == nk
        lens = np.diff(rp)
        entry_kept = np.repeat(~has_mult, lens)
        krp = np.zeros(nk + 1, dtype=np.int64)
        np.cumsum(lens[kept], out=krp[1:])
        kci, kva, bk = ci[entry_kept], va[entry_kept], b[kept]
        dev = lambda a: torch.from_numpy(a).to(asm.device)                                                       # the block back up
        y, reason, iters, rr = asm.conjugated_gradient(dev(krp), dev(kci), dev(kva), dev(bk), tol=tol, max_iter=max_iter, precond=True)
        yh = y.cpu().numpy()
        sol = np.zeros(n)
        sol[:nk] = yh
        # multipliers: b_i - sum_j A_ij y_j over the active rows
        act = np.nonzero(has_mult)[0]
        entry_act = ~entry_kept
        cols_a, vals_a = ci[entry_act], va[entry_act]
        below = cols_a < nk
        prod = np.where(below, vals_a * yh[np.where(below, cols_a, 0)], 0.0)
        arp = np.zeros(act.shape[0] + 1, dtype=np.int64)
        np.cumsum(lens[act], out=arp[1:])
        sums = np.add.reduceat(prod, arp[:-1]) if act.size else np.zeros(0)
        sol[cols_a[~below]] = b[act] - sums
        # expand_solution (hho.hpp:698-744), the next active set (obstacle.cpp:133-142) and the norm (:193)
        A_ct_h, B_ct_h = out["tables"]
        alpha = np.empty(nc + fbs * nf)
        alpha[:nc] = np.where(in_A_host, gamma_host, sol[np.where(in_A_host, 0, A_ct_h)])
        beta = np.where(in_A_host, sol[np.where(in_A_host, nk + B_ct_h, 0)], 0.0)
        comp = face_compress
        fa = np.where(comp[:, None] >= 0, sol[num_I + np.maximum(comp, 0)[:, None] * fbs + np.arange(fbs)[None, :]], out["g_host"])
        alpha[nc:] = fa.reshape(-1)
        nxt = (beta + 1.0 * (alpha[:nc] - gamma_host)) < 0
        norm = float(np.linalg.norm(alpha_prev_host - alpha))
        out["host"] = (sol, alpha, beta, nxt, int(nxt.sum()), norm, iters)

    # set-up outside both timings: the face numbering and the tables on the host, as the driver holds them
    A_ct, B_ct, num_I, num_A = asm.obstacle_tables(in_A)
    out["tables"] = (A_ct.cpu().numpy().astype(np.int64), B_ct.cpu().numpy().astype(np.int64))
    out["g_host"] = g.cpu().numpy().reshape(nf, fbs)
    info = asm.ctx.assembler_csr_query(pa.capi.DegreeInfo(0, k, k + 1))
    # compressed numbering of the non-Dirichlet faces, read off expand_solution itself: a solution that holds its own index
    probe = torch.arange(info.nrows, dtype=torch.float64, device=asm.device)
    zero_g = torch.full_like(g, -1.0)
    pa_alpha, _ = asm.obstacle_expand_solution(0, k, probe, zero_g, gamma, torch.zeros_like(in_A), *asm.obstacle_tables(torch.zeros_like(in_A))[:3], nf)
    first = pa_alpha[nc:].cpu().numpy().reshape(nf, fbs)[:, 0]
    face_compress = np.where(first < 0, -1, np.rint((first - nc) / fbs).astype(np.int64))

    modes = {"first_product": (float("inf"), 0), "cap_%d" % cap: (0.0, cap)}
    res = {"N": N, "k": k, "cells": nc, "active_cells": int(in_A_host.sum()), "nrows": int(info.nrows), "reps": reps, "cap": cap}
    for name, (tol, max_iter) in modes.items():
        device_route(tol, max_iter); host_route(tol, max_iter)      # warm-up; and the two routes compute the same
        d, h = out["device"], out["host"]
        same_x = bool(np.array_equal(d[0].cpu().numpy()[:res["nrows"] - res["active_cells"]], h[0][:res["nrows"] - res["active_cells"]]))
        dmult = float(np.abs(d[0].cpu().numpy() - h[0]).max())
        dalpha = float(np.abs(d[1].cpu().numpy() - h[1]).max())
        same_set = bool(np.array_equal(d[3].cpu().numpy().astype(bool), h[3]))
        device_route(tol, max_iter); host_route(tol, max_iter)
        td, th = [], []
        for _ in range(reps):                                       # alternating: both routes see the same clocks and neighbours
            t0 = time.perf_counter(); device_route(tol, max_iter); td.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); host_route(tol, max_iter); th.append(1e3 * (time.perf_counter() - t0))
        md, mh = statistics.median(td), statistics.median(th)
        res[name] = {"device_ms": md, "device_min_ms": min(td), "device_max_ms": max(td), "host_ms": mh, "host_min_ms": min(th),
                     "host_max_ms": max(th), "device_over_host": md / mh, "cg_iterations": int(d[6]), "block_solution_bit_identical": same_x,
                     "largest_solution_difference": dmult, "largest_alpha_difference": dalpha, "same_next_active_set": same_set}
        print("%dx%d pair (0,%d) (%d cells, %d active, %d rows), %s (%d CG iterations): host route %.2f ms (min %.2f, max %.2f)  device route "
              "%.3f ms (min %.3f, max %.3f)  device / host %.4f" % (N, N, k, nc, res["active_cells"], res["nrows"], name, d[6], mh, min(th),
                                                                   max(th), md, min(td), max(td), md / mh))
        print("  block solution bit-identical: %s; largest difference of the solutions (multipliers) %.2e, of alpha %.2e; same next active "
              "set: %s" % (same_x, dmult, dalpha, same_set))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
