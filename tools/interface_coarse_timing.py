"""The condensed interface system (cuthho_square -i, face unknowns only) solved on the device by the conjugate gradient with and
without the Galerkin coarse level, in one process: the point Jacobi of pa_conjugated_gradient, the cell patches of
pa_conjugated_gradient_patch (the yardstick: profiles/interface_patch_timing_512_k2.txt has them at 3817 iterations / 1.80 s at 1e-9)
and pa_conjugated_gradient_patch_coarse with the cell patches and the table of pa_interface_condensed_coarse, by side ("side") at
H = 16, 32 (and 8, expected to be refused: more than 4096 columns) and in one part ("one") at H = 8, 16, 32.  For every kappa the
system is assembled once; for every tolerance, after one warm-up solve of each configuration, the solves run in alternating
repetitions and the medians are reported: iterations, seconds to the tolerance (the solve's own factorisations -- patches and coarse
matrix -- included, and the table's time added), time per iteration (seconds / (iterations + 1): the loop runs one update more than it
counts).  On their own, with HIP events: the table (pa_interface_condensed_coarse with its query), the set-up
(pa_coarse_precond_factor: transpose, Galerkin product, Cholesky, inverse -- one call) and the bytes held while the solve runs.
The divergence test is set far out (1e10) and the cap is 50000 iterations, as tools/interface_patch_timing.py has them.
    python tools/interface_coarse_timing.py [N] [k] [reps] [max_iter] [kappa_2,kappa_2,...] [tol,tol,...]
                                                                                  (default 512 2 5 50000 1,1e4 1e-9,1e-13)"""
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
COARSE = (("side", 8), ("side", 16), ("side", 32), ("one", 8), ("one", 16), ("one", 32))
COMMITTED = {(512, 2, 1.0, 1e-9): {"jacobi": (9099, 3.193), "cell": (3817, 1.80)}}       # profiles/interface_patch_timing_512_k2.txt


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def coarse_table(asm, k, H, parts):
    try:
        return asm.interface_condensed_coarse(k, H, parts)
    except pa.capi.ProtonAmdError as e:
        return str(e)


def main():
    a = sys.argv[1:]
    N = int(a[0]) if a else 512
    k = int(a[1]) if len(a) > 1 else 2
    reps = int(a[2]) if len(a) > 2 else 5
    max_iter = int(a[3]) if len(a) > 3 else 50000
    kappas = [float(x) for x in (a[4] if len(a) > 4 else "1,1e4").split(",")]
    tols = [float(x) for x in (a[5] if len(a) > 5 else "1e-9,1e-13").split(",")]
    med = statistics.median
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    out = {"N": N, "k": k, "reps": reps, "max_iter": max_iter, "divergence_threshold": DIV, "runs": []}
    for kappa_2 in kappas:
        ops = asm.interface_local_ops(k, kappa=(1.0, kappa_2))
        rec = asm.interface_condensed_ops(k, ops)
        del ops
        rp, ci = asm.interface_condensed_csr_pattern(k)
        va, b = asm.interface_condensed_csr_fill(k, rec, g)
        cell = asm.interface_condensed_patches(k, "cell")
        tables = {"cell + coarse %s H = %d" % c: coarse_table(asm, k, c[1], c[0]) for c in COARSE}
        asm.synchronize()
        kinds = ["jacobi", "cell"] + [kind for kind, tb in tables.items() if not isinstance(tb, str)]
        pre_cell = asm.patch_precond_factor(rp, ci, va, cell)
        cell_bytes = 8 * pre_cell["sizes"].factor_doubles + 4 * pre_cell["sizes"].slot_ints + pre_cell["sizes"].scratch_bytes
        del pre_cell
        setup = {}
        for c in COARSE:
            kind = "cell + coarse %s H = %d" % c
            tb = tables[kind]
            if isinstance(tb, str):
                continue
            t_table = med(timed_once(lambda: asm.interface_condensed_coarse(k, c[1], c[0])) for _ in range(max(reps, 5)))
            pre = asm.coarse_precond_factor(rp, ci, va, tb)
            asm.synchronize()
            t_setup = med(timed_once(lambda: asm.coarse_precond_factor(rp, ci, va, tb)) for _ in range(max(reps, 3)))
            sz = pre["sizes"]
            table_bytes = tb[0].numel() * 8 + tb[1].numel() * 12
            setup[kind] = {"parts": c[0], "H": c[1], "ncoarse": tb[3], "entries": tb[1].numel(), "table_ms": t_table, "setup_ms": t_setup,
                           "pivot": pre["pivot"],
                           "bytes_held": cell_bytes + table_bytes + sz.pt_bytes + 8 * sz.factor_doubles + sz.scratch_bytes}
            del pre

        def solve(kind, tol):
            asm.synchronize()
            t0 = time.perf_counter()
            if kind == "jacobi":
                x, reason, iters, rr = asm.conjugated_gradient(rp, ci, va, b, tol=tol, div=DIV, max_iter=max_iter, precond=True)
            elif kind == "cell":
                x, reason, iters, rr = asm.conjugated_gradient_patch(rp, ci, va, b, cell, tol=tol, div=DIV, max_iter=max_iter)
            else:
                x, reason, iters, rr = asm.conjugated_gradient_patch_coarse(rp, ci, va, b, cell, tables[kind], tol=tol, div=DIV, max_iter=max_iter)
            asm.synchronize()
            return x, reason, iters, rr, time.perf_counter() - t0

        for tol in tols:
            sols = {kind: solve(kind, tol)[0] for kind in kinds}                # warm-up
            runs = {kind: [] for kind in kinds}
            for _ in range(reps):
                for kind in kinds:
                    runs[kind].append(solve(kind, tol)[1:])
            print("interface %dx%d k=%d kappa (1, %g), face-only system: %d cells (%d cut), %d rows, %d nnz; CG tolerance %g, cap %d; medians of "
                  "%d alternating repetitions" % (N, N, k, kappa_2, asm.ncells, asm.ncut, b.numel(), va.numel(), tol, max_iter, reps))
            res = {"kappa": (1.0, kappa_2), "tol": tol, "rows": b.numel(), "nnz": va.numel(), "solves": {}}
            for kind, tb in tables.items():
                if isinstance(tb, str):
                    print("  %-27s: refused: %s" % (kind, tb))
                    res["solves"][kind] = {"refused": tb}
            for kind in kinds:
                reason, iters, rr = runs[kind][0][:3]
                assert all(r[:2] == (reason, iters) for r in runs[kind])
                t = med(r[3] for r in runs[kind])
                entry = {"exit_reason": reason, "iterations": iters, "relative_residual": rr, "solve_s": t}
                if kind in setup:
                    entry.update(setup[kind])
                    t += 1e-3 * entry["table_ms"]
                entry["time_s"], entry["ms_per_iteration"] = t, 1e3 * t / (iters + 1)
                line = "  %-27s: %s %5d iterations, %.3f s, %.3f ms per iteration" % (
                    kind, "converged in" if reason == 0 else "NOT converged (exit %d) after" % reason, iters, t, entry["ms_per_iteration"])
                was = COMMITTED.get((N, k, kappa_2, tol), {}).get(kind)
                if was:
                    entry["committed_iterations"], entry["committed_time_s"] = was
                    line += "; committed (profiles/interface_patch_timing_512_k2.txt): %d iterations, %.2f s" % was
                if kind == "cell":
                    entry["bytes_held"] = cell_bytes
                    line += "; %.1f MB held" % (cell_bytes / 1e6)
                if kind in setup:
                    yard = res["solves"]["cell"]
                    entry["speedup_over_cell"] = yard["time_s"] / t
                    entry["max_abs_diff_to_cell_rel"] = float((sols[kind] - sols["cell"]).abs().max() / sols["cell"].abs().max())
                    line += ("; %d columns, table %.3f ms, set-up %.3f ms (one call, with the allocation of its buffers; both in the seconds), "
                             "%.1f MB held with the patches'; %.2f x fewer iterations, %.2f x %s in seconds than the cell patches; solution "
                             "against theirs %.2e" % (entry["ncoarse"], entry["table_ms"], entry["setup_ms"], entry["bytes_held"] / 1e6,
                                                      yard["iterations"] / max(iters, 1),
                                                      max(entry["speedup_over_cell"], 1 / entry["speedup_over_cell"]),
                                                      "faster" if entry["speedup_over_cell"] >= 1 else "SLOWER", entry["max_abs_diff_to_cell_rel"]))
                res["solves"][kind] = entry
                print(line, flush=True)
            out["runs"].append(res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
