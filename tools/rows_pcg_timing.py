#!/usr/bin/env python3
"""The row-partitioned face-only Poisson solve with and without the two-level preconditioner: pa_conjugated_gradient_rows (point
Jacobi, the solver the rows path had) against pa_conjugated_gradient_rows_patch_coarse with the slab's cell patches, and with the
cell patches plus the coarse level of H -- on one rank, and on 2 and 4 gloo processes that SHARE the one GPU (host-staged transport,
proton_amd.partition, as tools/rehearse_solve_n.py).  512^2, k = 2, a random right-hand side, 1e-9.  Medians of 5 alternating
repetitions of the whole call, its set-up included (the factors, the exchange of P's rows, A_c and its Cholesky factor live for the
call); the slab tables are built once, outside (timed on their own).

    python tools/rows_pcg_timing.py [--N 512 --k 2 --H 16 --reps 5 --worlds 1,2,4] [--out profiles/rows_pcg_timing_512_k2.txt]

Without RANK in the environment the script is the driver: it starts one group of worker processes per world size (fresh processes
of this file under torch.distributed.run) and gathers what rank 0 of each prints.  Ranks that share a GPU take turns on it and talk
through host copies: the lines of 2 and 4 ranks measure the plumbing (three sums and one exchange per iteration), not scaling."""
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
ap.add_argument("--H", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--worlds", default="1,2,4")
ap.add_argument("--port", type=int, default=29561)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def driver():
    lines = []
    for w in (int(x) for x in args.worlds.split(",")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(w), "--master-addr", "127.0.0.1",
               "--master-port", str(args.port + w), os.path.abspath(__file__), "--N", str(args.N), "--k", str(args.k), "--H", str(args.H),
               "--reps", str(args.reps), "--tol", repr(args.tol)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        got = [ln[len("RESULT "):] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the run on %d ranks failed" % w)
        lines += got
        print("\n".join(got), flush=True)
    head = ("tools/rows_pcg_timing.py on one MI355X: the face-only Poisson system of the %d^2 mesh, pair (%d, %d), a random right-hand side,\n"
            "relative residual %g, row-partitioned over the ranks.  jacobi = pa_conjugated_gradient_rows (the point Jacobi, all the rows solver had before);\n"
            "cell = pa_conjugated_gradient_rows_patch_coarse with the slab's cell patches; cell+H = the same with the coarse level of\n"
            "H = %d.  Seconds: median of %d alternating repetitions of the whole call on the slowest rank, set-up included; tables: the\n"
            "slab tables built once (pa_condensed_rows_patches, pa_condensed_rows_coarse, queries included).  2 and 4 ranks are gloo\n"
            "processes that SHARE the one GPU and move every sum and exchange through host copies: those lines measure the plumbing,\n"
            "not scaling.\n" % (args.N, args.k + 1, args.k, args.tol, args.H, args.reps))
    if args.out:
        with open(args.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


def worker():
    import torch
    import torch.distributed as dist
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    from proton_amd.partition import HostStagedCgTransport, HostStagedHalo, row_partition
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    N, cd, fd, H = args.N, args.k + 1, args.k, args.H
    a = BatchAssembler(0)
    a.generate_mesh(N, N, rows=row_partition(N, world, rank))
    rhs = a.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS, pa.QUAD_TENSOR)
    g = a.dirichlet_data(fd, pa.capi.FN_SIN_SIN_SOL)
    rec = a.condensed_ops(cd, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, rhs=rhs)
    info = a.condensed_info(cd, fd)
    out = a.condensed_halo_pack(cd, fd, rec, g) if info.halo_cells else None
    inn = torch.zeros((N, info.halo_doubles), dtype=torch.float64, device=a.device) if info.has_below else None
    a.synchronize()
    HostStagedHalo(rank, world)(out, inn)
    rp, ci = a.condensed_csr_pattern(cd, fd)
    va, _ = a.condensed_csr_fill(cd, fd, rec, g, halo_below=inn)
    b = torch.randn(info.system_size, generator=torch.Generator().manual_seed(1), dtype=torch.float64)[info.row_begin:info.row_end].to(a.device)
    a.synchronize()
    t0 = time.perf_counter()
    cell = a.condensed_rows_patches(cd, fd, "cell")
    coarse = a.condensed_rows_coarse(cd, fd, H)
    a.synchronize()
    t_tables = time.perf_counter() - t0
    tp = HostStagedCgTransport(rank, world, a.ctx).struct if world > 1 else None
    kw = dict(tol=args.tol, max_iter=20000)

    def jacobi(x):
        return a.ctx.conjugated_gradient_rows(tp, info.row_begin, info.row_end, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), b.data_ptr(),
                                              x.data_ptr(), **kw)

    def patches(x):
        return a.conjugated_gradient_rows_patch_coarse(tp, info.row_begin, info.row_end, rp, ci, va, b, cell, None, x=x, **kw)[1:]

    def two_level(x):
        return a.conjugated_gradient_rows_patch_coarse(tp, info.row_begin, info.row_end, rp, ci, va, b, cell, coarse, x=x, **kw)[1:]
    configs = [("jacobi", jacobi), ("cell", patches), ("cell+H", two_level)]
    times, res = {n: [] for n, _ in configs}, {}
    for rep in range(args.reps + 1):                       # (the first round warms the kernels up and is dropped)
        for name, fn in configs:
            x = torch.zeros_like(b)
            a.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            res[name] = fn(x)
            a.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    med = torch.tensor([statistics.median(times[n]) for n, _ in configs] + [t_tables], dtype=torch.float64)
    dist.all_reduce(med, op=dist.ReduceOp.MAX)
    if rank == 0:
        base = float(med[0])
        for i, (name, _) in enumerate(configs):
            reason, iters, rr = res[name]
            print("RESULT ranks %d  %-7s exit %d  iterations %5d  residual %.2e  seconds %.4f  (%.2f x jacobi rows)%s" %
                  (world, name, reason, iters, rr, float(med[i]), float(med[i]) / base,
                   "  ncoarse %d, tables %.4f s" % (coarse[3], float(med[3])) if name == "cell+H" else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if "RANK" in os.environ:
        worker()
    else:
        driver()
