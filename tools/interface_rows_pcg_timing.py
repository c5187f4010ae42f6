#!/usr/bin/env python3
"""The interface problem's face-only system (cuthho_square -i) solved by row slabs with and without the two-level preconditioner:
pa_conjugated_gradient_rows (point Jacobi, the only solver that reached the slabs before) against
pa_conjugated_gradient_rows_patch_coarse with the slab tables of pa_interface_rows_patches / pa_interface_rows_coarse -- the cell
patches alone, the cell patches with the table by side at H = 16, and with the table in one part at H = 8 and 16 -- on one rank, and
on 2 and 4 gloo processes that SHARE the one GPU (host-staged transport and halo, proton_amd.partition, as tools/rows_pcg_timing.py).
512^2, k = 2, the assembled right-hand side, the driver's 1e-9; kappa = (1, 1) and once more with kappa = (1, 1e4).  The divergence
test is set far out (1e10) and the cap is 50000 iterations, as tools/interface_coarse_timing.py has them.  Medians of 5 alternating
repetitions on the slowest rank; the seconds of a route hold the whole call -- the factors, the exchange of P's rows, A_c and its
Cholesky factor live for the call -- AND the building of its slab tables (timed in every repetition).

On one rank the same process also runs the one-process path on a whole-mesh context: pa_conjugated_gradient (Jacobi) and
pa_conjugated_gradient_patch_coarse with pa_interface_condensed_patches / pa_interface_condensed_coarse, table building included --
what interface_condensed_solve(patches="cell", coarse=H) runs between its assembly and its recovery, the same kernels.

    python tools/interface_rows_pcg_timing.py [--N 512 --k 2 --reps 5 --worlds 1,2,4 --kappas 1,1e4]
                                              [--out profiles/interface_rows_pcg_timing_512_k2.txt]

Without RANK in the environment the script is the driver: every (kappa, world size) is one step, a fresh group of worker processes
of this file under torch.distributed.run, each step under its own `timeout -k 10`; the steps are chained as with &&: after a step
that fails, is killed or runs out of time nothing more is started.  Ranks that share a GPU take turns on it and talk through host
copies: the lines of 2 and 4 ranks measure the plumbing (three sums and one exchange per iteration), not scaling."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=512)
ap.add_argument("--k", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--worlds", default="1,2,4")
ap.add_argument("--kappas", default="1,1e4")
ap.add_argument("--kappa", type=float, default=1.0)        # (a worker's)
ap.add_argument("--port", type=int, default=29581)
ap.add_argument("--step-seconds", type=int, default=420)
ap.add_argument("--out", default=None)
args = ap.parse_args()

DIV, CAP = 1e10, 50000
ROUTES = (("cell", None), ("cell+side16", ("side", 16)), ("cell+one8", ("one", 8)), ("cell+one16", ("one", 16)))


def driver():
    head = ("tools/interface_rows_pcg_timing.py on one MI355X: the interface problem's face-only system of the %d^2 mesh, k = %d, the assembled\n"
            "right-hand side, relative residual %g, divergence test at %g, row-partitioned over the ranks.  jacobi = pa_conjugated_gradient_rows\n"
            "(the point Jacobi: the parent's path); cell = pa_conjugated_gradient_rows_patch_coarse with the slab's cell patches\n"
            "(pa_interface_rows_patches); cell+side16 / cell+one8 / cell+one16 = the same with the slab's rows of the coarse table by side at\n"
            "H = 16 / in one part at H = 8, 16 (pa_interface_rows_coarse).  Seconds: median of %d alternating repetitions on the slowest rank of\n"
            "the whole call, set-up included, plus the building of the route's slab tables (`tables`, in the seconds).  one-process = the same\n"
            "system on a whole-mesh context in the same process (ranks 1 only): pa_conjugated_gradient / pa_conjugated_gradient_patch_coarse\n"
            "with pa_interface_condensed_patches / _coarse, table building in the seconds: the same kernels.  2 and 4 ranks are gloo processes\n"
            "that SHARE the one GPU and move every sum and exchange through host copies: those lines measure the plumbing, not scaling.\n"
            % (args.N, args.k, args.tol, DIV, args.reps))
    lines = []

    def keep():
        if args.out:
            with open(args.out, "w") as f:
                f.write(head + "\n".join(lines) + "\n")
    for kappa in (float(x) for x in args.kappas.split(",")):
        for w in (int(x) for x in args.worlds.split(",")):
            cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                   "--nproc-per-node", str(w), "--master-addr", "127.0.0.1", "--master-port", str(args.port + w), os.path.abspath(__file__),
                   "--N", str(args.N), "--k", str(args.k), "--reps", str(args.reps), "--tol", repr(args.tol), "--kappa", repr(kappa)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            got = [ln[len("RESULT "):] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not got:            # as `&&`: nothing more is started on the GPU
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                keep()
                raise SystemExit("the step kappa (1, %g) on %d ranks ended with status %d: stopping" % (kappa, w, r.returncode))
            lines.extend(got)
            print("\n".join(got), flush=True)
            keep()


def worker():
    import torch
    import torch.distributed as dist
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    from proton_amd.partition import HostStagedCgTransport, HostStagedHalo, row_partition
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    N, k, kappa = args.N, args.k, (1.0, args.kappa)
    f64 = dict(dtype=torch.float64, device="cuda:0")
    a = BatchAssembler(0)
    a.cut_preprocess(N, refsteps=4, rows=row_partition(N, world, rank))
    ops = a.interface_local_ops(k, kappa=kappa)
    g = a.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    rec = a.interface_rows_ops(k, ops)
    del ops
    info = a.interface_rows_info(k)
    out = a.interface_rows_halo_pack(k, rec, g) if info.halo_send_doubles else None
    inn = torch.zeros(info.halo_recv_doubles, **f64) if info.halo_recv_doubles else None
    a.synchronize()
    HostStagedHalo(rank, world)(out, inn)
    rp, ci = a.interface_rows_csr_pattern(k)
    va, b = a.interface_rows_csr_fill(k, rec, g, halo_below=inn)
    del rec, out, inn
    a.synchronize()
    tp = HostStagedCgTransport(rank, world, a.ctx).struct if world > 1 else None
    kw = dict(tol=args.tol, div=DIV, max_iter=CAP)

    def tables(coarse):
        return a.interface_rows_patches(k, "cell"), (a.interface_rows_coarse(k, coarse[1], coarse[0]) if coarse else None)

    def jacobi():
        x = torch.zeros_like(b)
        return a.ctx.conjugated_gradient_rows(tp, info.row_begin, info.row_end, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), b.data_ptr(),
                                              x.data_ptr(), **kw), 0.0, 0

    def route(coarse):
        def run():
            a.synchronize()
            t0 = time.perf_counter()
            pt, tb = tables(coarse)
            a.synchronize()
            t_tab = time.perf_counter() - t0
            x = torch.zeros_like(b)
            res = a.conjugated_gradient_rows_patch_coarse(tp, info.row_begin, info.row_end, rp, ci, va, b, pt, tb, x=x, **kw)[1:]
            return res, t_tab, (tb[3] if tb else 0)
        return run
    configs = [("jacobi", jacobi)] + [(name, route(c)) for name, c in ROUTES]
    if world == 1:                                          # the one-process path, in the same process
        w = BatchAssembler(0)
        w.cut_preprocess(N, refsteps=4)
        wops = w.interface_local_ops(k, kappa=kappa)
        wg = w.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
        wrec = w.interface_condensed_ops(k, wops)
        del wops
        wrp, wci = w.interface_condensed_csr_pattern(k)
        wva, wb = w.interface_condensed_csr_fill(k, wrec, wg)
        del wrec
        w.synchronize()

        def one_jacobi():
            return w.conjugated_gradient(wrp, wci, wva, wb, precond=True, **kw)[1:], 0.0, 0

        def one_process(coarse):
            def run():
                w.synchronize()
                t0 = time.perf_counter()
                pt = w.interface_condensed_patches(k, "cell")
                tb = w.interface_condensed_coarse(k, coarse[1], coarse[0]) if coarse else None
                w.synchronize()
                t_tab = time.perf_counter() - t0
                if tb is None:
                    res = w.conjugated_gradient_patch(wrp, wci, wva, wb, pt, **kw)[1:]
                else:
                    res = w.conjugated_gradient_patch_coarse(wrp, wci, wva, wb, pt, tb, **kw)[1:]
                w.synchronize()
                return res, t_tab, (tb[3] if tb else 0)
            return run
        configs += [("one-process jacobi", one_jacobi)] + [("one-process " + name, one_process(c)) for name, c in ROUTES]
    times, tabs, res = {n: [] for n, _ in configs}, {n: [] for n, _ in configs}, {}
    for rep in range(args.reps + 1):                       # (the first round warms the kernels up and is dropped)
        for name, fn in configs:
            a.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            res[name], t_tab, nc = fn()
            a.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
                tabs[name].append(t_tab)
            res[name] = tuple(res[name]) + (nc,)
    med = torch.tensor([statistics.median(times[n]) for n, _ in configs] + [statistics.median(tabs[n]) for n, _ in configs] +
                       [min(times[n]) for n, _ in configs] + [max(times[n]) for n, _ in configs], dtype=torch.float64)
    dist.all_reduce(med, op=dist.ReduceOp.MAX)
    if rank == 0:
        nk = len(configs)
        base = float(med[0])
        for i, (name, _) in enumerate(configs):
            reason, iters, rr, nc = res[name]
            print("RESULT kappa (1, %g)  ranks %d  %-24s exit %d  iterations %5d  residual %.2e  seconds %.4f  (min %.4f, max %.4f; %.2f x jacobi rows)%s"
                  % (args.kappa, world, name, reason, iters, rr, float(med[i]), float(med[2 * nk + i]), float(med[3 * nk + i]), float(med[i]) / base,
                     "  tables %.4f s%s" % (float(med[nk + i]), ", ncoarse %d" % nc if nc else "") if "jacobi" not in name else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if "RANK" in os.environ:
        worker()
    else:
        driver()
