"""The condensed face-only systems solved on the device by the conjugate gradient with and without the Galerkin coarse level, in one
process: the fictitious-domain problem (cuthho_square -f, tolerance 1e-13, hats split by side of the interface) and plain Poisson
(tolerance 1e-9, one part, a random right-hand side), each with the point Jacobi of pa_conjugated_gradient, the cell patches of pa_conjugated_gradient_patch
(the yardstick) and pa_conjugated_gradient_patch_coarse at every H given.  Each system is assembled once; after one warm-up solve
of each configuration the solves run in alternating repetitions and the medians are reported: iterations, time to the tolerance
(the solve's own factorisations included), time per iteration (time / (iterations + 1): the loop runs one update more than it
counts).  On their own, with HIP events: the table (pa_condensed_coarse with its query), the set-up (pa_coarse_precond_factor:
transpose, Galerkin product, Cholesky, inverse -- one call; tools/coarse_pcg_timing.py setup ... under a kernel trace splits it by
kernel: coarse_pt_* + coarse_w_kernel + coarse_galerkin_kernel are the product, coarse_chol_column_kernel + coarse_inverse_kernel
the factor), one application, and the bytes held while the solve runs.  A configuration the entry refuses (more than 4096 columns)
is reported as refused.  The divergence test is set far out (1e10), as tools/patch_pcg_timing.py has it.
    python tools/coarse_pcg_timing.py [N] [k] [reps] [max_iter] [H,H,...]           (default 512 2 5 20000 8,16,32)
    python tools/coarse_pcg_timing.py setup [N] [k] [H,H,...]       one table + one factor per problem and H, nothing else"""
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


def fictdom_system(asm, N, k):
    cd = k + 1
    asm.cut_preprocess(N, refsteps=4)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    rhs = torch.empty((asm.ncells, (cd + 1) * (cd + 2) // 2), dtype=torch.float64, device=asm.device)
    asm.ctx.cut_uncut_rhs(cd, NEG, pa.capi.FN_SIN_SIN_RHS, rhs.data_ptr())
    cut = asm.cut_local_ops(k, NEG, want=("lc", "rhs"))
    rec = asm.fictdom_condensed_records(k, NEG, rhs, cut["lc"], cut["rhs"])
    rp, ci = asm.condensed_csr_pattern(cd, k)
    va, b = asm.condensed_csr_fill(cd, k, rec["cond"], g)
    return rp, ci, va, b


def poisson_system(asm, N, k):
    cd = k + 1
    asm.generate_mesh(N, N)
    rhs = asm.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS, pa.QUAD_TENSOR)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    rec = asm.condensed_ops(cd, k, pa.QUAD_TENSOR, pa.STAB_FANCY, rhs=rhs)
    rp, ci = asm.condensed_csr_pattern(cd, k)
    va, b = asm.condensed_csr_fill(cd, k, rec, g)
    # a random right-hand side (seed 1), as in the measurements the coarse level was proposed with: the assembled one is that of
    # sin(pi x) sin(pi y), close to an eigenvector of the matrix, and the Jacobi solve meets 1e-9 on it in 7 iterations
    import numpy as np
    b = torch.tensor(np.random.default_rng(1).standard_normal(b.numel())).to(asm.device)
    return rp, ci, va, b


PROBLEMS = (("fictitious domain", fictdom_system, "side", 1e-13), ("Poisson", poisson_system, "one", 1e-9))


def coarse_table(asm, k, H, parts):
    try:
        return asm.condensed_coarse(k + 1, k, H, parts, NEG)
    except pa.capi.ProtonAmdError as e:
        return str(e)


def setup_only(N, k, Hs):
    asm = BatchAssembler(0)
    for name, build, parts, _ in PROBLEMS:
        rp, ci, va, b = build(asm, N, k)
        for H in Hs:
            tb = coarse_table(asm, k, H, parts)
            if isinstance(tb, str):
                print("%s H = %d: refused (%s)" % (name, H, tb))
                continue
            pre = asm.coarse_precond_factor(rp, ci, va, tb)
            asm.synchronize()
            print("%s H = %d: %d columns, pivot %d" % (name, H, tb[3], pre["pivot"]))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "setup":
        a = sys.argv[2:]
        return setup_only(int(a[0]) if a else 512, int(a[1]) if len(a) > 1 else 2, [int(h) for h in (a[2] if len(a) > 2 else "8,16,32").split(",")])
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    max_iter = int(sys.argv[4]) if len(sys.argv) > 4 else 20000
    Hs = [int(h) for h in (sys.argv[5] if len(sys.argv) > 5 else "8,16,32").split(",")]
    cd = k + 1
    asm = BatchAssembler(0)
    med = statistics.median
    out = {"N": N, "k": k, "reps": reps, "max_iter": max_iter, "divergence_threshold": DIV, "problems": {}}
    for name, build, parts, tol in PROBLEMS:
        rp, ci, va, b = build(asm, N, k)
        cell = asm.condensed_patches(cd, k, "cell")
        tables = {H: coarse_table(asm, k, H, parts) for H in Hs}
        asm.synchronize()
        kinds = ["jacobi", "cell"] + ["cell + coarse H = %d" % H for H in Hs if not isinstance(tables[H], str)]
        by_kind = {"cell + coarse H = %d" % H: H for H in Hs}

        def solve(kind):
            asm.synchronize()
            t0 = time.perf_counter()
            if kind == "jacobi":
                x, reason, iters, rr = asm.conjugated_gradient(rp, ci, va, b, tol=tol, div=DIV, max_iter=max_iter, precond=True)
            elif kind == "cell":
                x, reason, iters, rr = asm.conjugated_gradient_patch(rp, ci, va, b, cell, tol=tol, div=DIV, max_iter=max_iter)
            else:
                x, reason, iters, rr = asm.conjugated_gradient_patch_coarse(rp, ci, va, b, cell, tables[by_kind[kind]], tol=tol, div=DIV,
                                                                            max_iter=max_iter)
            asm.synchronize()
            return x, reason, iters, rr, time.perf_counter() - t0

        sols = {kind: solve(kind)[0] for kind in kinds}                        # warm-up
        runs = {kind: [] for kind in kinds}
        for _ in range(reps):
            for kind in kinds:
                runs[kind].append(solve(kind)[1:])
        print("%s %dx%d k=%d, face-only system: %d rows, %d nnz; CG tolerance %g, cap %d; medians of %d alternating repetitions" %
              (name, N, N, k, b.numel(), va.numel(), tol, max_iter, reps))
        res = {"rows": b.numel(), "nnz": va.numel(), "tol": tol, "parts": parts, "solves": {}}
        pre_cell = asm.patch_precond_factor(rp, ci, va, cell)
        cell_bytes = 8 * pre_cell["sizes"].factor_doubles + 4 * pre_cell["sizes"].slot_ints + pre_cell["sizes"].scratch_bytes
        for H in Hs:
            if isinstance(tables[H], str):
                print("  cell + coarse H = %d: refused: %s" % (H, tables[H]))
                res["solves"]["cell + coarse H = %d" % H] = {"refused": tables[H]}
        for kind in kinds:
            reason, iters, rr = runs[kind][0][:3]
            assert all(r[:2] == (reason, iters) for r in runs[kind])
            t = med(r[3] for r in runs[kind])
            entry = {"exit_reason": reason, "iterations": iters, "relative_residual": rr, "time_s": t, "ms_per_iteration": 1e3 * t / (iters + 1)}
            line = "  %-22s: %s %5d iterations, %.3f s, %.3f ms per iteration (set-up included)" % (
                kind, "converged in" if reason == 0 else "NOT converged (exit %d) after" % reason, iters, t, entry["ms_per_iteration"])
            if kind == "cell":
                entry["bytes_held"] = cell_bytes
                line += "; %.1f MB held" % (cell_bytes / 1e6)
            if kind in by_kind:
                H = by_kind[kind]
                tb = tables[H]
                t_table = med(timed_once(lambda: asm.condensed_coarse(cd, k, H, parts, NEG)) for _ in range(max(reps, 5)))
                pre = asm.coarse_precond_factor(rp, ci, va, tb)
                asm.synchronize()
                t_setup = med(timed_once(lambda: asm.coarse_precond_factor(rp, ci, va, tb)) for _ in range(max(reps, 3)))
                z = torch.zeros_like(b)
                asm.coarse_precond_apply(pre, b, z)
                t_apply = med(timed_once(lambda: asm.coarse_precond_apply(pre, b, z)) for _ in range(max(reps, 5) * 4))
                sz = pre["sizes"]
                table_bytes = tb[0].numel() * 8 + tb[1].numel() * 12
                entry.update({"H": H, "ncoarse": tb[3], "entries": tb[1].numel(), "table_ms": t_table, "setup_ms": t_setup, "apply_ms": t_apply,
                              "table_bytes": table_bytes, "pt_bytes": sz.pt_bytes, "factor_bytes": 8 * sz.factor_doubles,
                              "scratch_bytes": sz.scratch_bytes, "bytes_held": cell_bytes + table_bytes + sz.pt_bytes + 8 * sz.factor_doubles +
                              sz.scratch_bytes, "pivot": pre["pivot"],
                              "max_abs_diff_to_cell_rel": float((sols[kind] - sols["cell"]).abs().max() / sols["cell"].abs().max())})
                line += ("; %d columns, table %.3f ms, Galerkin product + factor %.3f ms (one call, with the allocation of its buffers), apply %.3f ms; "
                         "table %.1f MB, transpose %.1f MB, factor %.1f MB, scratch %.1f MB (%.1f MB held with the patches'); solution against "
                         "the cell patches' %.2e" % (tb[3], t_table, t_setup, t_apply, table_bytes / 1e6, sz.pt_bytes / 1e6,
                                                     8 * sz.factor_doubles / 1e6, sz.scratch_bytes / 1e6, entry["bytes_held"] / 1e6,
                                                     entry["max_abs_diff_to_cell_rel"]))
            res["solves"][kind] = entry
            print(line)
        out["problems"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
