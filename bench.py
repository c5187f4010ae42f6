#!/usr/bin/env python3
"""bench.py -- cells assembled per second on an N x N quad mesh (BASELINE.json's metric).

A "step" is one pass of the hot path over the whole mesh, in one of three modes:

  L  local operators to HBM (the mode of BASELINE.md section 4 the headline is quoted on): for every cell
     lc = data + stab (make_hho_laplacian + stabilization, hho.hpp:32-237) and the cell right-hand side
     (make_rhs, utils.hpp:153-174); 8 msize^2 + 8 cbs + 80 algorithmic bytes per cell.
  C  condensed: cell right-hand sides, then the SAME local-operator pass with the static condensation fused behind it
     (no lc in HBM: per cell the packed Schur complement + condensed rhs), then the face-only global system assembled
     directly in CSR (values + right-hand side of the rows this rank owns); 16 (4 fbs)^2 + 8 (4 fbs) + 80 algorithmic
     bytes per cell (mode C).

  A  the reference's "Matrix assembly" span (cuthho_square.cpp:881-905, convergence_test.cpp:201-217) on one GPU: mode L's
     local operators and cell right-hand sides, the Dirichlet data, and assembler<Mesh>'s OWN global system (cell + face
     unknowns, hho.hpp:298-335, 344-406, 451-455) built directly in CSR from them (pa_assembler_csr_fill: values + RHS; the
     symbolic phase is setup) -- printed next to cpu_baseline.matrix_assembly.  `roofline` stays the local-operator kernel's.

  python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run)

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`, and the roofline of the
same timed steps).  --full adds what takes work of its own: the CPU baseline (cpu_baseline, gpu_over_cpu and mode A's
matrix_assembly) and, for N > 1, the same step on rank 0's GPU alone (same_step_one_gpu, exchange_checked).
--dump-outputs DIR writes what the last timed step computed (Pipeline.outputs) as DIR/<name>.npy, float64, at most
DUMP_BYTES in all: a larger output is cut to a fixed sample of its rows (dump_plan), the same in every run and build.

Defaults: N = 1 -> the north-star target, 1024 x 1024, k = 2 (hho_degree_info(3, 2)), tensor Gauss, fancy stabilization,
mode L.  N > 1 -> BASELINE.json's config 5, 2048 x 2048, k = 3, mode C, STRONG scaling: the cell rows are block-partitioned
over the ranks, every rank assembles the CSR rows of the faces it owns, and the one exchange of a step is the packed
top-face rows of each slab's top cell row, sent one slab up through the library's RCCL entry points (pa_comm_*).  The N > 1
step is the N = 1 step of the same mode plus that exchange: `--gpus 1 --workload quad2048_k3 --mode C` runs exactly the
N > 1 step minus the exchange, and every N > 1 line carries `same_step_one_gpu` (the whole mesh on rank 0's GPU alone,
same mode, same code) so that the scaling of like with like can be read off one run.

Inputs (the structured mesh) are generated on the device and are resident in HBM when the timed region starts.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = {
    # name: (N, cd, fd, quad, stab, domain lo, hi, rhs fn id, rhs dinc, source config)
    "quad1024_k2": dict(N=1024, cd=3, fd=2, quad="tensor", stab="fancy", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0,
                        note="north-star target: 1024x1024 quad_mesh, hho_degree_info(3,2), fancy stabilization"),
    "quad256_k1_fan": dict(N=256, cd=2, fd=1, quad="fan", stab="naive", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0,
                           note="configs[1]: cuthho_square -M 256 -N 256 -k 1 -f, uncut cells (fan quadrature, naive stabilization)"),
    "quad512_k2_fan": dict(N=512, cd=3, fd=2, quad="fan", stab="naive", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0,
                           note="configs[2] without the cut cells: 512x512 k=2 fan quadrature, naive stabilization"),
    "obstacle512_k1": dict(N=512, cd=0, fd=1, quad="tensor", stab="fancy", lo=(-1.0, -1.0), hi=(1.0, 1.0), fn=3, dinc=1,
                           note="configs[3]: apps/obstacle 512x512 k=1, hho_degree_info(0,1)"),
    "quad2048_k3": dict(N=2048, cd=4, fd=3, quad="tensor", stab="fancy", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0,
                        note="configs[4]: 2048x2048 k=3 Laplacian, hho_degree_info(4,3)"),
    "cuthho512_k2": dict(N=512, cd=3, fd=2, quad="fan", stab="naive", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0, cut=True,
                         note="configs[2]: cuthho_square -M 512 -N 512 -k 2 -f, circle r=0.35, -r 4, node displacement: "
                              "uncut cells (fan quadrature, naive stabilization) + cut cells (Nitsche operators), merged"),
    "cuthho512_k2_interface": dict(N=512, cd=3, fd=2, quad="fan", stab="naive", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0, cut=True,
                                   interface=(1.0, 1.0, 5.0),
                                   note="cuthho_square -M 512 -N 512 -k 2 -i (run_cuthho_interface, cuthho_square.cpp:1625-1846), kappa_1 = kappa_2 = 1, "
                                        "eta = 5: every cell's one-sided operators + the cut cells' two-sided operators (2 msize unknowns each); mode L"),
    "quad1024_k2_general": dict(N=1024, cd=3, fd=2, quad="tensor", stab="fancy", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0, perturb=0.1,
                                note="the headline on GENERAL quadrilaterals: interior nodes displaced by U(-0.1 h, 0.1 h) (the commented-out "
                                     "perturbation of convergence_test.cpp:176-187, numpy default_rng(12345)): no two cells are congruent, "
                                     "so nothing can be reused between cells"),
    "quad1024_k1": dict(N=1024, cd=2, fd=1, quad="tensor", stab="fancy", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0,
                        note="1024x1024 k=1"),
    "quad1024_k3": dict(N=1024, cd=4, fd=3, quad="tensor", stab="fancy", lo=(0.0, 0.0), hi=(1.0, 1.0), fn=1, dinc=0,
                        note="1024x1024 k=3"),
}

# BASELINE.json's metric string, verbatim; the achieved HBM GB/s it mentions is roofline.achieved
BASELINE_METRIC = 'cells assembled/sec (+ achieved HBM GB/s) on N×N quad mesh, k=1..3'
HBM_PEAK_GBS = 8000.0        # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6      # 256 CU x 4 SIMD x 16 FMA/clk x 2 x 2.4 GHz; v_mfma_f64_16x16x4_f64 measured at 64 clk = the same rate
FP64_SUSTAINED_TFLOPS = 62.7  # measured on the box (tools/probe/valu_rate.hip): a wave64 v_fma_f64 every 2.09 ns per SIMD = 1.91 GHz sustained
DUMP_BYTES = 64_000_000      # --dump-outputs: the most it writes, all files and ranks together
DUMP_SEED = 20251016


def dump_plan(shapes, budget):
    """--dump-outputs: which rows (first index) of each output to write, within `budget` bytes of float64 files in all.
    Every row when everything fits; otherwise the same fraction of every array's rows, one row drawn from each of that
    many equal strata by numpy default_rng(DUMP_SEED) -- sorted, distinct, and the same from run to run and build to build
    (arrays with as many rows get the same rows: lc and rhs of the same cells).
    shapes: {name: shape}.  Returns {name: None (every row) or an int64 index array}."""
    import numpy as np
    header = 256                                               # bytes of one .npy header, rounded up
    row_bytes = {k: 8 * int(np.prod(s[1:], dtype=np.int64)) for k, s in shapes.items()}
    total = sum(s[0] * row_bytes[k] for k, s in shapes.items())
    room = budget - header * len(shapes)
    if total <= room:
        return {k: None for k in shapes}
    frac = (room - sum(row_bytes.values())) / total              # (keeping at least one row of each costs at most one row more)
    plan = {}
    for k, s in shapes.items():
        rows = int(s[0])
        keep = min(rows, max(1, int(rows * frac))) if rows else 0
        edges = (np.arange(keep + 1, dtype=np.int64) * rows) // keep if keep else np.zeros(1, dtype=np.int64)
        rng = np.random.default_rng(DUMP_SEED)
        plan[k] = edges[:-1] + (rng.random(keep) * (edges[1:] - edges[:-1])).astype(np.int64)
    return plan


def dump_outputs(torch, outputs, directory, budget, suffix=""):
    """write {name: device tensor} as directory/<name><suffix>.npy (float64), sampled by dump_plan within `budget`"""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    plan = dump_plan({k: tuple(t.shape) for k, t in outputs.items()}, budget)
    for k, t in outputs.items():
        idx = plan[k]
        if idx is not None and len(idx) < t.shape[0]:
            t = t.reshape(t.shape[0], -1).index_select(0, torch.from_numpy(idx).to(t.device)).reshape((len(idx),) + tuple(t.shape[1:]))
        np.save(os.path.join(directory, k + suffix + ".npy"), t.to(torch.float64).cpu().numpy())


def reference_flops_per_cell(w):
    """EXACT FP64 operations per cell of the reference's algorithm (make_hho_laplacian + stabilization), counted by the
    instrumented restatement oracle/flopcount (every double add / mul / div / sqrt of hho_oracle.c) and frozen in
    oracle/flops_per_cell.json (tests/test_oracle_flops.py keeps the file honest)."""
    try:
        tab = json.load(open(os.path.join(ROOT, "oracle", "flops_per_cell.json")))["per_cell"]
        return tab["%d,%d,%s,%s" % (w["cd"], w["fd"], w["quad"], w["stab"])]["local_ops_flops"]
    except (OSError, KeyError):
        return None


def bytes_per_cell(mode, msize, cbs, fbs):
    """Algorithmic bytes per cell (BASELINE.md section 4 / SURVEY.md section 8d).
    L: lc written (8 msize^2) + cell rhs written (8 cbs) + 4 node coordinates (64) + 4 u32 ids (16).
    C: condensed face-face COO, 16 B per entry (16 (4 fbs)^2) + condensed rhs (8 * 4 fbs) + the same 80 bytes read."""
    if mode == "L":
        return 8 * msize * msize + 8 * cbs + 80
    if mode == "A":       # the dominant kernel of mode A is mode L's
        return 8 * msize * msize + 8 * cbs + 80
    return 16 * (4 * fbs) ** 2 + 8 * 4 * fbs + 80


def cpu_baseline_cut(w, target_seconds=15.0):
    """Oracle on a bounded sample of the cut workload: a smaller mesh of the same problem
    (the per-cell cost does not depend on N; the cut-cell fraction scales like 1/N)."""
    import oracle_lib
    import cuthho_driver
    N = min(w["N"], 384)            # ~5-10 s of single-thread work
    msh = oracle_lib.CutMesh(N, refsteps=4)
    di = oracle_lib.degrees(w["cd"], w["fd"])
    t0 = time.perf_counter()
    (cuthho_driver.oracle_interface_provider if w.get("interface") else cuthho_driver.oracle_cut_provider)(msh, di)
    dt = time.perf_counter() - t0
    ncut = int((msh.cell_loc == oracle_lib.CUT_ON_INTERFACE).sum())
    return {"value": msh.nc / dt, "unit": "cells/s", "cores": 1, "kind": "port",
            "sample": "%dx%d mesh of the same problem (%d cells, %d cut), %.1f s, oracle %s + uncut operators and rhs, single thread"
                      % (N, N, msh.nc, ncut, dt, "two-sided (interface)" if w.get("interface") else "cut")}


def perturbation(N, lo, hi, amount):
    """displacements of the interior nodes, U(-amount h, amount h), numpy default_rng(12345) -- the same
    array for the GPU mesh and for the CPU baseline's mesh"""
    import numpy as np
    rng = np.random.default_rng(12345)
    h = (hi[0] - lo[0]) / N
    d = rng.uniform(-amount * h, amount * h, size=((N + 1) * (N + 1), 2))
    ij = np.arange((N + 1) * (N + 1))
    i, j = ij % (N + 1), ij // (N + 1)
    d[~((i > 0) & (i < N) & (j > 0) & (j < N))] = 0.0
    return d


def general_quad_mesh(torch, N, lo, hi, amount, device):
    """The generator mesh (basic_mesh.hpp:230-298: points min + i h, cells {p, p+1, p+Nx+2, p+Nx+1})
    with displaced interior nodes, built directly as device arrays."""
    i = torch.arange(N + 1, dtype=torch.float64, device=device)
    hx, hy = (hi[0] - lo[0]) / N, (hi[1] - lo[1]) / N
    pts = torch.stack([(lo[0] + i * hx).repeat(N + 1), (lo[1] + i * hy).repeat_interleave(N + 1)], dim=1).contiguous()
    pts += torch.from_numpy(perturbation(N, lo, hi, amount)).to(device)
    ci = torch.arange(N, device=device, dtype=torch.int64)
    p0 = (ci.repeat_interleave(N) * (N + 1) + ci.repeat(N))                    # cell (i, j) -> j (Nx+1) + i, cell id = j Nx + i
    ptids = torch.stack([p0, p0 + 1, p0 + N + 2, p0 + N + 1], dim=1).to(torch.int32).contiguous()    # ids < 2^31: same bits as u32
    return pts, ptids


def workload_mesh(w):
    """host arrays of the workload's mesh for the CPU baseline (oracle side)"""
    import oracle_lib
    N = w["N"]
    mp, points, ptids = oracle_lib.make_mesh(N, N, w["lo"], w["hi"])
    if w.get("perturb"):
        points += perturbation(N, w["lo"], w["hi"], w["perturb"])
    return points, ptids


def cpu_baseline(w, sample_rows, target_seconds=6.0):
    """The oracle (CPU restatement of the reference's loop; oracle/hho_oracle.c, -O3 -mavx like the reference's Release
    build) on a bounded sample of the same workload: the first rows of the same mesh.  Two spans, each with one thread
    (the reference is single-threaded: the reference-equivalent number, `value`) and with every host core (OpenMP over
    cells): the per-cell operators + rhs alone, and the span the reference's drivers print as "Matrix assembly"
    (cuthho_square.cpp:881-905, obstacle.cpp:145-161: make_assembler, operators, rhs, assemble, finalize)."""
    import numpy as np
    import oracle_lib
    N = w["N"]
    di = oracle_lib.degrees(w["cd"], w["fd"])
    quad = oracle_lib.QUAD_TENSOR if w["quad"] == "tensor" else oracle_lib.QUAD_FAN
    stab = oracle_lib.STAB_FANCY if w["stab"] == "fancy" else oracle_lib.STAB_NAIVE
    cores = oracle_lib.max_threads()
    out = {"unit": "cells/s", "kind": "port", "cores": 1, "cores_all": cores}
    if w.get("perturb"):
        # general quadrilaterals: the oracle's assembly span works on the generator mesh; time the operators on the
        # displaced mesh through the batch entry point
        points, ptids = workload_mesh(w)
        L = oracle_lib.lib()
        ptids = np.ascontiguousarray(ptids, dtype=np.uint64)
        fn = L.hho_builtin_fn(w["fn"])

        def ops(n, nt):
            lc = np.zeros((n, di.msize, di.msize)); rhs = np.zeros((n, di.cbs))
            t0 = time.perf_counter()
            st = L.hho_local_ops_batch_mt(oracle_lib._dp(points), oracle_lib._u64p(ptids), 0, n, di, quad, stab, fn, None, w["dinc"],
                                          oracle_lib._dp(lc), oracle_lib._dp(rhs), nt)
            assert st == 0
            return n / (time.perf_counter() - t0)
        rate = ops(min(N * N, 4096), 1)
        rows = sample_rows if sample_rows > 0 else max(1, min(N, int(target_seconds * rate / N)))
        out["value"] = ops(rows * N, 1)
        out["value_all_cores"] = ops(min(N, rows * min(cores, 8)) * N, cores)
        out["sample"] = "first %d of %d cell rows of the same (displaced) mesh, operators + rhs, oracle/hho_oracle.c" % (rows, N)
        return out
    probe = oracle_lib.matrix_assembly_timed(N, di, quad, stab, (0, max(1, 4096 // N)), w["fn"], 2, w["dinc"], w["lo"], w["hi"], 1)
    rate = probe["cells"] / probe["seconds_assembly"]
    rows = sample_rows if sample_rows > 0 else max(1, min(N, int(target_seconds * rate / N)))
    one = oracle_lib.matrix_assembly_timed(N, di, quad, stab, (0, rows), w["fn"], 2, w["dinc"], w["lo"], w["hi"], 1)
    rows_all = max(rows, min(N, rows * min(cores, 8)))
    allc = oracle_lib.matrix_assembly_timed(N, di, quad, stab, (0, rows_all), w["fn"], 2, w["dinc"], w["lo"], w["hi"], cores)
    out.update({
        "value": one["cells"] / one["seconds_ops"],
        "value_all_cores": allc["cells"] / allc["seconds_ops"],
        "matrix_assembly": {"value": one["cells"] / one["seconds_assembly"], "value_all_cores": allc["cells"] / allc["seconds_assembly"],
                            "unit": "cells/s",
                            "what": "the span the reference prints as \"Matrix assembly\" (cuthho_square.cpp:881-905): make_assembler + "
                                    "per-cell operators + rhs + assembler.assemble + finalize (setFromTriplets)"},
        "sample": "a strip of %d (1 thread) / %d (%d threads, OpenMP over cells) of the mesh's %d cell rows, assembled as a mesh of its own "
                  "(same cells; tables, right-hand side and finalize at their per-cell cost): %.1f + %.1f s and %.1f + %.1f s; "
                  "`value` = per-cell operators + rhs, one thread (the reference is single-threaded); oracle/hho_oracle.c, gcc -O3 -mavx"
                  % (rows, rows_all, cores, N, one["seconds_ops"], one["seconds_assembly"], allc["seconds_ops"], allc["seconds_assembly"]),
    })
    return out


class Pipeline:
    """The step of one rank: its slab of the mesh, its buffers, the sequence of library calls of one pass."""

    def __init__(self, torch, pa, w, mode, rows, N, device_index, comm=None, host_exchange=None, gather=None):
        from proton_amd.batch import BatchAssembler
        self.torch, self.pa, self.w, self.mode, self.N = torch, pa, w, mode, N
        self.quad = pa.QUAD_TENSOR if w["quad"] == "tensor" else pa.QUAD_FAN
        self.stab = pa.STAB_FANCY if w["stab"] == "fancy" else pa.STAB_NAIVE
        self.di, _ = pa.degree_info(w["cd"], w["fd"])
        self.sz = pa.sizes_for(self.di, self.quad)
        self.asm = BatchAssembler(device_index)
        self.comm, self.host_exchange = comm, host_exchange
        # --exchange allgather: (world, largest nnz_owned, largest row count over the ranks) -- after the fill every rank gathers
        # every rank's CSR values and right-hand side (the north star's literal collective); None: the halo rows are all that travels
        self.gather = gather
        self.host_gather = None
        self._side = self._pin_out = self._pin_in = self._ev_pack = None
        asm, sz, dev = self.asm, self.sz, self.asm.device
        self.cut = bool(w.get("cut"))
        whole = rows is None or (rows[0] == 0 and rows[1] == N)
        if self.cut:
            # host preprocessing (the whole mesh on every rank, the context keeps its slab): outside the timed region
            asm.cut_preprocess(N, refsteps=4, rows=None if whole else rows)
            # (side-stream overlap of the cut cells' kernel, pa_context_set_cut_overlap: measured SLOWER here, 0.75 vs 0.69 ms
            # per step -- the persistent grid of the uncut cells' kernel holds the whole chip, the two only contend)
            asm.ctx.set_cut_overlap(bool(os.environ.get("PA_CUT_OVERLAP")))
        elif w.get("perturb") and whole and mode != "C":
            self.mesh_keep = general_quad_mesh(torch, N, w["lo"], w["hi"], w["perturb"], dev)     # caller-owned device arrays
            asm.ctx.mesh_attach_device(self.mesh_keep[0].data_ptr(), (N + 1) * (N + 1), self.mesh_keep[1].data_ptr(), N * N)
        elif w.get("perturb"):
            # the generator's numbering (closed-form faces: condensed mode, slabs) with the displaced coordinates: every rank
            # draws the same whole-mesh perturbation and keeps the node rows of its slab
            asm.generate_mesh(N, N, w["lo"], w["hi"], rows=rows)
            r0_, r1_ = (0, N) if rows is None else rows
            pts = general_quad_mesh(torch, N, w["lo"], w["hi"], w["perturb"], dev)[0][r0_ * (N + 1):(r1_ + 1) * (N + 1)].contiguous()
            asm.ctx.mesh_set_points(pts.data_ptr(), pts.shape[0])
            torch.cuda.synchronize()
        else:
            asm.generate_mesh(N, N, w["lo"], w["hi"], rows=rows)
        self.n = asm.ncells
        f64 = dict(dtype=torch.float64, device=dev)
        self.rhs = torch.empty((self.n, sz.cbs), **f64)
        if mode in ("L", "A"):
            self.lc = torch.empty((self.n, sz.msize, sz.msize), **f64)
            if mode == "A":
                self.ainfo = asm.ctx.assembler_csr_query(self.di)
                self.rowptr, self.colind = asm.assembler_csr_pattern(w["cd"], w["fd"])      # symbolic phase (setup)
                self.values = torch.empty(max(self.ainfo.nnz, 1), **f64)
                self.b = torch.empty(max(self.ainfo.nrows, 1), **f64)
                self.g = torch.empty((asm.assembler_info(w["cd"], w["fd"]).nfaces_local, sz.fbs), **f64)
            if self.cut and w.get("interface"):
                self.iparms = pa.capi.InterfaceParams(*w["interface"])
                self.cut_lc = torch.empty((max(asm.ncut, 1), 2 * sz.msize, 2 * sz.msize), **f64)
                self.cut_rhs = torch.empty((max(asm.ncut, 1), 2 * sz.cbs), **f64)
            elif self.cut:
                self.cut_lc = torch.empty((max(asm.ncut, 1), sz.msize, sz.msize), **f64)
                self.cut_rhs = torch.empty((max(asm.ncut, 1), sz.cbs), **f64)
        else:
            ci = self.ci = asm.ctx.condensed_query(self.di)
            self.rec = torch.empty((self.n, ci.cond_doubles), **f64)
            self.g = asm.dirichlet_data(w["fd"], 2)                       # boundary data: sin(pi x) sin(pi y) (setup)
            self.rowptr, self.colind = asm.condensed_csr_pattern(w["cd"], w["fd"])          # symbolic phase (setup)
            self.values = torch.empty(max(ci.nnz_owned, 1), **f64)
            self.b = torch.empty(max(ci.row_end - ci.row_begin, 1), **f64)
            self.halo_out = torch.empty((max(ci.halo_cells, 1), ci.halo_doubles), **f64)
            self.halo_in = torch.zeros((N, ci.halo_doubles), **f64) if ci.has_below else None
            if self.cut:
                nf_ = ci.nf
                self.cut_lc = torch.empty((max(asm.ncut, 1), sz.msize, sz.msize), **f64)
                self.cut_rhs = torch.empty((max(asm.ncut, 1), sz.cbs), **f64)
                self.cut_Sp = torch.empty((max(asm.ncut, 1), nf_ * (nf_ + 1) // 2), **f64)
                self.cut_g = torch.empty((max(asm.ncut, 1), nf_), **f64)
            if gather is not None:
                world_, max_nnz, max_rows = gather
                self.values = torch.zeros(max_nnz, **f64)          # (padded to the largest slab: all-gather wants equal counts)
                self.b = torch.zeros(max_rows, **f64)
                self.all_values = torch.empty(world_ * max_nnz, **f64)
                self.all_b = torch.empty(world_ * max_rows, **f64)
        self.ev = {}

    def _tick(self, i, name):
        if i is not None:
            e = self.torch.cuda.Event(enable_timing=True)
            e.record()
            self.ev.setdefault(i, []).append((name, e))

    def step(self, i=None):
        pa, asm, w, di, n = self.pa, self.asm, self.w, self.di, self.n
        if self.mode in ("L", "A"):
            self._tick(i, "start")
            if self.cut and w.get("interface"):
                # run_cuthho_interface's loop (cuthho_square.cpp:1666-1714): the cut cells' two-sided operators and right-hand sides
                # (2 msize unknowns), then every cell's one-sided ones; the assembler takes the cut cells' from the first array
                if asm.ncut:
                    asm.ctx.cut_interface_ops(w["fd"], asm.level_set, self.iparms, w["fn"], None, None, self.cut_lc.data_ptr(),
                                              self.cut_rhs.data_ptr(), None)
                self._tick(i, "cut")
                asm.ctx.cut_interface_uncut(w["fd"], self.iparms, w["fn"], self.lc.data_ptr(), None, None)
                self._tick(i, "ops")
                asm.ctx.cut_interface_uncut(w["fd"], self.iparms, w["fn"], None, self.rhs.data_ptr(), None)
                self._tick(i, "rhs")
                return
            if self.cut and asm.ncut:
                asm.ctx.cut_local_ops(w["fd"], asm.level_set, pa.capi.LOC_NEGATIVE, w["fn"], 2, None, None, None,
                                      self.cut_lc.data_ptr(), self.cut_rhs.data_ptr(), None)
                self._tick(i, "cut")
            asm.ctx.local_ops(di, self.quad, self.stab, 0, n, None, None, None, self.lc.data_ptr(), None)
            self._tick(i, "ops")
            if self.cut:      # the fictitious-domain driver's make_rhs: only the cells of the domain are integrated (cuthho_square.cpp:628-629)
                asm.ctx.cut_uncut_rhs(w["cd"], pa.capi.LOC_NEGATIVE, w["fn"], self.rhs.data_ptr())
            else:
                asm.ctx.cell_rhs(w["cd"], w["dinc"], self.quad, w["fn"], 0, n, self.rhs.data_ptr(), None)
            self._tick(i, "rhs")
            if self.cut and asm.ncut:
                asm.ctx.cut_merge(w["fd"], pa.capi.LOC_NEGATIVE, self.cut_lc.data_ptr(), self.cut_rhs.data_ptr(), self.lc.data_ptr(),
                                  self.rhs.data_ptr())
                self._tick(i, "merge")
            if self.mode == "A":
                # assembler.assemble's Dirichlet projection (hho.hpp:381-386) and the global system (:391-405, finalize :451-455)
                asm.ctx.dirichlet_data(w["fd"], 2, self.g.data_ptr())
                asm.ctx.assembler_csr_fill(di, self.lc.data_ptr(), self.rhs.data_ptr(), self.g.data_ptr(), self.values.data_ptr(),
                                           self.b.data_ptr())
                self._tick(i, "fill")
            return
        ci, N = self.ci, self.N
        self._tick(i, "start")
        if self.cut:
            # the cut cells first: operators (pa_cut_local_ops_batch), then the stand-alone condensation of their local matrices
            # into packed records; the fused pass below runs the uncut formulas on every cell, pa_cut_merge_condensed replaces
            # the cut cells' records before anything reads them (halo pack, fill)
            if asm.ncut:
                asm.ctx.cut_local_ops(w["fd"], asm.level_set, pa.capi.LOC_NEGATIVE, w["fn"], 2, None, None, None,
                                      self.cut_lc.data_ptr(), self.cut_rhs.data_ptr(), None)
                asm.ctx.static_condensation_packed(di, asm.ncut, self.cut_lc.data_ptr(), self.cut_rhs.data_ptr(),
                                                   self.cut_Sp.data_ptr(), self.cut_g.data_ptr(), None)
            self._tick(i, "cut")
            asm.ctx.cut_uncut_rhs(w["cd"], pa.capi.LOC_NEGATIVE, w["fn"], self.rhs.data_ptr())
            asm.ctx.cut_merge(w["fd"], pa.capi.LOC_NEGATIVE, None, self.cut_rhs.data_ptr(), None, self.rhs.data_ptr())     # zero outside the domain
        else:
            asm.ctx.cell_rhs(w["cd"], w["dinc"], self.quad, w["fn"], 0, n, self.rhs.data_ptr(), None)
        self._tick(i, "rhs")
        top = N if ci.halo_cells else 0
        nd = ci.cond_doubles
        if top:
            # the slab's top cell row first: its packed top-face rows travel one slab up while the rest is computed
            f0 = n - top
            asm.ctx.condensed_ops(di, self.quad, self.stab, f0, top, self.rhs[f0:].data_ptr(), self.rec[f0:].data_ptr(), None)
            if self.cut and asm.ncut:
                asm.ctx.cut_merge_condensed(w["fd"], self.cut_Sp.data_ptr(), self.cut_g.data_ptr(), self.rec.data_ptr())
            asm.ctx.condensed_halo_pack(di, self.rec.data_ptr(), self.g.data_ptr(), self.halo_out.data_ptr())
        self._exchange_start()
        asm.ctx.condensed_ops(di, self.quad, self.stab, 0, n - top, self.rhs.data_ptr(), self.rec.data_ptr(), None)
        self._tick(i, "ops")
        if self.cut and asm.ncut:
            asm.ctx.cut_merge_condensed(w["fd"], self.cut_Sp.data_ptr(), self.cut_g.data_ptr(), self.rec.data_ptr())
            self._tick(i, "merge")
        self._exchange_wait()
        self._tick(i, "exchange_wait")
        asm.ctx.condensed_csr_fill(di, self.rec.data_ptr(), self.g.data_ptr(), None if self.halo_in is None else self.halo_in.data_ptr(),
                                   self.values.data_ptr(), self.b.data_ptr())
        self._tick(i, "fill")
        if self.gather is not None:
            world_, max_nnz, max_rows = self.gather
            if self.comm is not None:
                self.comm.allgather_start(self.values.data_ptr(), self.all_values.data_ptr(), 8 * max_nnz)
                self.comm.wait()
                self.comm.allgather_start(self.b.data_ptr(), self.all_b.data_ptr(), 8 * max_rows)
                self.comm.wait()
            elif self.host_gather is not None:
                self.torch.cuda.current_stream().synchronize()
                self.host_gather(self.values, self.all_values, max_nnz)
                self.host_gather(self.b, self.all_b, max_rows)
            self._tick(i, "allgather")

    def _exchange_start(self):
        ci = self.ci
        if self.comm is not None:
            self.comm.halo_exchange_start(self.halo_out.data_ptr() if ci.halo_cells else None, int(ci.halo_cells) * ci.halo_doubles,
                                          None if self.halo_in is None else self.halo_in.data_ptr(),
                                          0 if self.halo_in is None else self.halo_in.numel())
        elif self.host_exchange is not None:
            # host-staged transport (rehearsal, or RCCL did not come up): like the RCCL path the exchange runs NEXT TO the
            # kernels of the other rows -- the packed rows are complete at this event; the copies and the gloo messages
            # happen in _exchange_wait, on a side stream, after the rest of the step's kernels have been launched
            self._ev_pack = self.torch.cuda.Event()
            self._ev_pack.record()

    def _exchange_wait(self):
        torch = self.torch
        if self.comm is not None:
            self.comm.wait()
        elif self.host_exchange is not None:
            ci = self.ci
            if self._side is None:
                self._side = torch.cuda.Stream()
                self._pin_out = torch.empty(self.halo_out.shape, dtype=self.halo_out.dtype).pin_memory() if ci.halo_cells else None
                self._pin_in = None if self.halo_in is None else torch.empty(self.halo_in.shape, dtype=self.halo_in.dtype).pin_memory()
            with torch.cuda.stream(self._side):
                self._side.wait_event(self._ev_pack)
                if self._pin_out is not None:
                    self._pin_out.copy_(self.halo_out, non_blocking=True)
                self._side.synchronize()
                self.host_exchange.exchange_host(self._pin_out, self._pin_in)
                if self._pin_in is not None and self.host_exchange.rank > 0:
                    self.halo_in.copy_(self._pin_in, non_blocking=True)
                ev_in = torch.cuda.Event()
                ev_in.record(self._side)
            torch.cuda.current_stream().wait_event(ev_in)

    def stage_ms(self, steps):
        """mean HIP-event time between the ticks of a step, per stage name"""
        acc = {}
        for i in range(steps):
            ticks = self.ev[i]
            for (a, ea), (b, eb) in zip(ticks[:-1], ticks[1:]):
                acc[b] = acc.get(b, 0.0) + ea.elapsed_time(eb)
        return {k: v / steps for k, v in acc.items()}

    def outputs(self):
        """what a caller of the step receives, by name, as the step leaves it in device memory (lc: one column-major
        matrix per cell, the library's layout) -- the arrays --dump-outputs writes"""
        asm = self.asm
        if self.mode in ("L", "A"):
            out = {"lc": self.lc, "rhs": self.rhs}
            if self.cut and self.w.get("interface"):
                out.update(cut_lc=self.cut_lc[:asm.ncut], cut_rhs=self.cut_rhs[:asm.ncut])     # the cut cells' two-sided operators
            if self.mode == "A":
                out.update(dirichlet=self.g, csr_values=self.values[:int(self.ainfo.nnz)], csr_rhs=self.b[:int(self.ainfo.nrows)])
            return out
        ci = self.ci
        out = {"rhs": self.rhs, "records": self.rec, "csr_values": self.values[:int(ci.nnz_owned)],
               "csr_rhs": self.b[:int(ci.row_end) - int(ci.row_begin)]}
        if self.gather is not None:
            out.update(all_csr_values=self.all_values, all_csr_rhs=self.all_b)
        return out

    def check(self):
        """the timed work produced finite, non-trivial results (not a cached / skipped pass)"""
        torch = self.torch
        if os.environ.get("PA_ABLATE"):      # (profiling-only stage ablation produces garbage on purpose)
            return
        probe = (self.lc if self.mode in ("L", "A") else self.rec)[:: max(1, self.n // 64)]
        assert bool(torch.isfinite(probe).all()) and float(probe.abs().max()) > 0.0
        if self.mode in ("C", "A"):
            v = self.values[:: max(1, self.values.numel() // 4096)]
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0.0 and bool(torch.isfinite(self.b).all())


def settle(torch, dist, world, fn, seconds):
    """Untimed passes of the step before the W warmup steps, about `seconds` of them: after idling the GPU runs the first
    ~20 ms of a burst of work at lower clocks (tools/steps_sweep.sh: the kernels of the headline step take 1.43 ms over the
    first 5 steps after 3 warmup steps, 1.24-1.30 ms from the 30th on), which with W = 3..5 and K = 20 would be a tenth of
    the timed region -- and made the HIP-event kernel time disagree with the rocprofv3 average over all launches.  The same
    number of passes on every rank (the step of several GPUs contains an exchange).  Returns the number of passes."""
    if seconds <= 0:
        return 0
    fn(None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(None)
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    n = torch.tensor([min(2000, max(1, int(seconds / one)))])
    if world > 1:
        dist.all_reduce(n, op=dist.ReduceOp.MAX)
    for _ in range(int(n[0])):
        fn(None)
    torch.cuda.synchronize()
    return int(n[0]) + 2


def timed(torch, dist, world, fn, steps, warmup, with_index=True):
    for _ in range(warmup):
        fn(None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i if with_index else None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="default: quad1024_k2 on one GPU, quad2048_k3 (BASELINE.json's config 5) on several")
    ap.add_argument("--mode", default=None, choices=["L", "C", "A"],
                    help="L: local operators + rhs to HBM (default on one GPU); C: condensed records + face-only CSR rows "
                         "(default on several GPUs: the mode with the exchange); A: the reference's \"Matrix assembly\" span -- L + "
                         "assembler<Mesh>'s own cell + face system directly in CSR (one GPU)")
    ap.add_argument("--backend", default=os.environ.get("PA_BENCH_BACKEND", "nccl"), choices=["nccl", "gloo"],
                    help="nccl = RCCL, one rank per GPU (what the driver runs); gloo = rehearsal of the N>1 code path with "
                         "several ranks sharing the visible GPU(s) and a host-staged exchange (numbers not comparable)")
    ap.add_argument("--exchange", default="halo", choices=["halo", "allgather"],
                    help="N>1, mode C.  halo (default): the packed top-face rows of each slab, one slab up, are all that travels.  allgather: "
                         "behind it the north star's literal collective -- every rank all-gathers every rank's CSR values and right-hand "
                         "side (pa_comm_allgather_start) and ends the step holding the whole face-only system")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements beyond the timed steps: the CPU baseline, and for N > 1 the same step on rank 0's GPU alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64, at most 64 MB in all; "
                         "a fixed sample of the rows of larger outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--rccl-timeout", type=float, default=180.0,
                    help="N>1: seconds to wait for the RCCL communicator before the step falls back to the host-staged exchange")
    ap.add_argument("--settle-ms", type=float, default=250.0,
                    help="untimed passes of the step before the warmup steps, in ms of GPU work (clock ramp after idle); 0 = none")
    ap.add_argument("--no-one-gpu-reference", action="store_true", help="N>1, with --full: skip the same step on rank 0's GPU alone")
    ap.add_argument("--cpu-sample-rows", type=int, default=0, help="cell rows timed by the CPU baseline (0 = auto)")
    args = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL across processes needs it on this pool
    import torch
    import torch.distributed as dist
    import proton_amd as pa
    from proton_amd.partition import row_partition

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus %d needs `python -m torch.distributed.run --nproc-per-node %d bench.py ...`"
                             % (args.gpus, args.gpus))
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    workload = args.workload or ("quad1024_k2" if world == 1 else "quad2048_k3")
    mode = args.mode or ("L" if world == 1 else "C")
    w = WORKLOADS[workload]
    N = w["N"]
    if w.get("interface") and mode != "L":
        raise SystemExit("the interface workload runs in mode L (the two-sided cells have 2 msize unknowns: no condensed form is built)")
    if (w.get("cut") or w.get("perturb")) and mode == "A":
        raise SystemExit("mode A runs on the generator mesh (assembler<Mesh>'s system of a fictitious-domain problem drops the cells outside the domain: not built)")
    if mode == "A" and world > 1:
        raise SystemExit("mode A (the reference's one-process \"Matrix assembly\" span) is single-GPU; several GPUs assemble the face-only system (mode C)")
    rehearsal = world > 1 and args.backend == "gloo"
    if rehearsal:
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    comm = None
    host_exchange = None
    rccl_error = None
    abandoned_thread = False
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # torch.distributed carries the bootstrap (RCCL unique id), the barriers and the max over ranks of the timings;
        # the exchange of the step itself goes through the library's own RCCL entry points (pa_comm_*)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()

    r0, r1 = row_partition(N, world, rank)
    gather = None
    if world > 1 and mode == "C" and args.exchange == "allgather":
        di_, _ = pa.degree_info(w["cd"], w["fd"])
        infos = [pa.capi.condensed_partition_info(N, N, row_partition(N, world, r), di_) for r in range(world)]
        gather = (world, None, max(int(i.row_end - i.row_begin) for i in infos))
    pipe = Pipeline(torch, pa, w, mode, (r0, r1), N, local_rank, gather=None)
    if gather is not None:
        # nnz of the owned rows is known after the symbolic phase: the largest over the ranks sizes the padded buffers
        mx = torch.tensor([int(pipe.ci.nnz_owned)])
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        gather = (world, int(mx[0]), gather[2])
        del pipe
        pipe = Pipeline(torch, pa, w, mode, (r0, r1), N, local_rank, gather=gather)
    if world > 1 and mode == "C":
        from proton_amd.partition import HostStagedHalo
        if not rehearsal:
            try:
                ids = [pa.capi.comm_unique_id() if rank == 0 else None]
            except Exception as e:       # noqa: BLE001  (reported in the JSON line, never silent)
                ids, rccl_error = [None], repr(e)
            dist.broadcast_object_list(ids, src=0)
            if ids[0] is not None:
                # ncclCommInitRank is collective and blocks: under a watchdog, so that a rendezvous that never completes
                # (interface selection, a rank that died) ends in the labelled host-staged transport, not in a hung bench
                import threading
                box = {}

                def create():
                    try:
                        box["comm"] = pa.capi.Comm(pipe.asm.ctx, world, rank, ids[0])
                    except Exception as e:   # noqa: BLE001
                        box["err"] = repr(e)
                th = threading.Thread(target=create, daemon=True)
                th.start()
                th.join(args.rccl_timeout)
                if th.is_alive():
                    rccl_error = "RCCL communicator creation did not return within %g s" % args.rccl_timeout
                    abandoned_thread = True
                else:
                    comm, rccl_error = box.get("comm"), box.get("err")
            else:
                rccl_error = rccl_error or "rank 0 could not create an RCCL unique id"
            # every rank must take the same transport: if RCCL did not come up on ALL of them the step's exchange goes
            # through host copies over gloo instead -- the same buffers, the same protocol, labelled as such in `config.exchange`
            ok = torch.tensor([0 if rccl_error else 1])
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok[0]) == 0:
                errs = [None] * world
                dist.all_gather_object(errs, rccl_error)
                rccl_error = "; ".join("rank %d: %s" % (r, e) for r, e in enumerate(errs) if e) or "unknown"
                if comm is not None:
                    comm.close()
                    comm = None
                rehearsal = True
            else:
                pipe.comm = comm
        if rehearsal:
            host_exchange = HostStagedHalo(rank, world)
            pipe.host_exchange = host_exchange
            if gather is not None:
                from proton_amd.partition import HostStagedAllgather
                pipe.host_gather = HostStagedAllgather(rank, world)
        dist.barrier()                                     # communicators exist before anything is timed

    n_settle = settle(torch, dist, world, pipe.step, args.settle_ms * 1e-3)
    elapsed = timed(torch, dist, world, pipe.step, args.steps, args.warmup)
    stages = pipe.stage_ms(args.steps)
    # the span the roofline's bytes are divided by.  L / A: the local-operator kernels (pre-pass + cooperative kernel; with the
    # cut cells also their kernel and the merge -- all cells' bytes are credited).  C: EVERY kernel of the step that moves the
    # mode's algorithmic bytes (cell rhs, operators + condensation, CSR fill): the bytes stand for the assembled face-face
    # system, which only exists after the fill.
    if mode == "C":
        kern_ms = stages["rhs"] + stages["ops"] + stages["fill"] + stages.get("cut", 0.0) + stages.get("merge", 0.0)
    else:
        kern_ms = stages["ops"] + stages.get("cut", 0.0) + stages.get("merge", 0.0)
    pipe.check()
    if args.dump_outputs:
        dump_outputs(torch, pipe.outputs(), args.dump_outputs, DUMP_BYTES // world, "" if world == 1 else "_rank%d" % rank)

    # N > 1, --full: the same step, same mode, same code, whole mesh, on rank 0's GPU alone (the other ranks wait): the
    # like-for-like one-GPU number of this run
    one_gpu = None
    exchange_checked = None
    if world > 1 and args.full and not args.no_one_gpu_reference:
        ref_sums = None
        if rank == 0:
            ref = Pipeline(torch, pa, w, mode, (0, N), N, local_rank)
            settle(torch, dist, 1, ref.step, args.settle_ms * 1e-3)
            t_ref = timed(torch, dist, 1, ref.step, max(3, args.steps // 4), 1)
            one_gpu = {"value": N * N / (t_ref / max(3, args.steps // 4)), "ms_per_step": t_ref / max(3, args.steps // 4) * 1e3}
            if mode == "C":
                ref_sums = [float(ref.values.sum()), float(ref.values.abs().sum()), float(ref.b.sum()), float(ref.b.abs().sum())]
            else:
                ref_sums = [float(ref.lc.sum()), float(ref.lc.abs().sum()), float(ref.rhs.sum()), float(ref.rhs.abs().sum())]
            del ref
        dist.barrier()
        if mode == "C":
            # the slabs' systems stacked are the whole-mesh system: the sums of the CSR values and of the right-hand side over
            # the ranks must be those of the one-GPU reference -- they are not if a slab's halo rows did not arrive
            loc = torch.tensor([float(pipe.values.sum()), float(pipe.values.abs().sum()), float(pipe.b.sum()), float(pipe.b.abs().sum())],
                               dtype=torch.float64)
            dist.all_reduce(loc, op=dist.ReduceOp.SUM)
            if gather is not None:
                # (the padding is zero: the gathered copy of ANY rank must sum to the same whole-mesh system)
                got = torch.tensor([float(pipe.all_values.sum()), float(pipe.all_values.abs().sum()), float(pipe.all_b.sum()),
                                    float(pipe.all_b.abs().sum())], dtype=torch.float64)
                worst = (got - loc).abs() / torch.tensor([max(abs(float(loc[1])), 1e-300)] * 2 + [max(abs(float(loc[3])), 1e-300)] * 2, dtype=torch.float64)
                dist.all_reduce(worst, op=dist.ReduceOp.MAX)
                gathered_ok = bool(float(worst.max()) <= 1e-9)
            if rank == 0:
                if gather is not None and not gathered_ok:
                    print("bench.py: a rank's all-gathered system does NOT sum to the ranks' systems (relative %r)" % worst.tolist(), file=sys.stderr, flush=True)
                exchange_checked = (gather is None or gathered_ok) and all(abs(a - r) <= 1e-9 * max(abs(ref_sums[1 if i < 2 else 3]), 1e-300) for i, (a, r) in enumerate(zip(loc.tolist(), ref_sums)))
                if not exchange_checked:      # reported in the line (and loudly here), not fatal: the timing is still a measurement
                    print("bench.py: the ranks' systems do NOT add up to the whole-mesh system: %r vs %r" % (loc.tolist(), ref_sums), file=sys.stderr, flush=True)

        if mode == "L":
            # no exchange in this mode; still: the slabs' local matrices and right-hand sides stacked are the whole mesh's
            # (a slab that mis-read its node rows, or lost its cut cells, shows here)
            loc = torch.tensor([float(pipe.lc.sum()), float(pipe.lc.abs().sum()), float(pipe.rhs.sum()), float(pipe.rhs.abs().sum())],
                               dtype=torch.float64)
            dist.all_reduce(loc, op=dist.ReduceOp.SUM)
            if rank == 0:
                exchange_checked = all(abs(a - r) <= 1e-9 * max(abs(ref_sums[1 if i < 2 else 3]), 1e-300) for i, (a, r) in enumerate(zip(loc.tolist(), ref_sums)))
                if not exchange_checked:
                    print("bench.py: the slabs' local matrices do NOT add up to the whole mesh's: %r vs %r" % (loc.tolist(), ref_sums), file=sys.stderr, flush=True)

    names = ("rhs", "ops", "exchange_wait", "fill", "allgather", "cut", "merge")
    t = torch.tensor([elapsed, kern_ms] + [stages.get(k, 0.0) for k in names], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed, kern_ms = float(t[0]), float(t[1])
    stage_max = {k: float(t[2 + i]) for i, k in enumerate(names) if k in stages}

    if rank == 0:
        sz, di, n_local = pipe.sz, pipe.di, pipe.n
        total_cells = N * N
        ms_per_step = elapsed / args.steps * 1e3
        value = total_cells / (elapsed / args.steps)
        bpc = bytes_per_cell(mode, sz.msize, sz.cbs, sz.fbs)
        li = pipe.asm.ctx.launch_info(di, pipe.quad, pipe.stab, n_local, condensed=(mode == "C"))
        achieved = n_local * bpc / (kern_ms * 1e-3) / 1e9
        # HBM bytes of the dominant kernels from the PMC counters.  They are collected in separate rocprofv3 --pmc passes
        # (tools/profile_round.sh), not in this run: an entry of profiles/pmc_traffic.json is emitted only for the BUILD it was
        # measured on (stamp = hash of csrc/ + flags, proton_amd/_build.py:build_stamp) -- otherwise null, with the reason.
        from proton_amd import _build as pa_build
        stamp = pa_build.build_stamp()
        traffic, traffic_reason = None, "no entry for %s|%s in profiles/pmc_traffic.json" % (workload, mode)
        tf = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tf):
            try:
                rec = json.load(open(tf)).get("%s|%s" % (workload, "L" if mode == "A" else mode))
                if rec and rec.get("n_gpus", 1) == world:
                    if rec.get("build_stamp") == stamp:
                        traffic, traffic_reason = rec["hbm_bytes_per_launch"], "counters of this build (%s)" % rec.get("source", "profiles/")
                    else:
                        traffic_reason = "the entry was measured on build %s, this is %s: re-run tools/profile_round.sh" % (rec.get("build_stamp"), stamp)
            except Exception as e:       # noqa: BLE001
                traffic, traffic_reason = None, "profiles/pmc_traffic.json unreadable: %r" % (e,)
        fl = reference_flops_per_cell(w)
        per_kernel = None
        if mode == "C":
            cd_ = pipe.ci.cond_doubles
            nnz_own = int(pipe.ci.nnz_owned)
            per_kernel = {
                "ops": {"ms": stage_max["ops"], "bytes": n_local * (8 * cd_ + 8 * sz.cbs + 80),
                        "what": "hho_local_ops<MODE_COND> + pre-pass: 80 B of mesh and 8 cbs of cell rhs read, the packed record (8 x %d B) written per cell" % cd_},
                "fill": {"ms": stage_max["fill"], "bytes": 8 * nnz_own + 8 * (int(pipe.ci.row_end) - int(pipe.ci.row_begin)) + n_local * 8 * cd_,
                         "what": "cond_fill + cond_rhs_rows: the records read once, the CSR values and right-hand side of the owned rows written"},
            }
        elif mode == "A":
            per_kernel = {
                "ops": {"ms": stage_max["ops"], "bytes": n_local * bpc, "what": "local operators (mode L's bytes)"},
                "fill": {"ms": stage_max["fill"], "bytes": n_local * 8 * sz.msize * sz.msize + 8 * int(pipe.ainfo.nnz) + 8 * int(pipe.ainfo.nrows),
                         "what": "dirichlet_data + asm_fill_cells + asm_fill_faces: lc read once, CSR values (nnz = %d) and RHS (%d rows) written"
                                 % (int(pipe.ainfo.nnz), int(pipe.ainfo.nrows))},
            }
        if per_kernel:
            for v in per_kernel.values():
                v["GB/s"] = v["bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else None
                v["frac"] = None if v["GB/s"] is None else v["GB/s"] / HBM_PEAK_GBS
        exch = "none"
        if world > 1 and mode == "C":
            exch = ("packed top-face rows of each slab's top cell row, one slab up (%d cells x %d doubles = %.2f MB per rank and step), %s"
                    % (N, pipe.ci.halo_doubles, N * pipe.ci.halo_doubles * 8 / 1e6,
                       ("host-staged gloo (NOT RCCL%s)" % ((": RCCL failed to initialise -- " + rccl_error) if rccl_error else ", --backend gloo rehearsal"))
                       if rehearsal else "RCCL send/recv through pa_comm_halo_exchange_start"))
            if gather is not None:
                exch += ("; THEN the north star's all-gather: every rank's CSR values (%d doubles, padded) and right-hand side (%d) to every rank "
                         "(%.2f GB received per rank and step), %s" % (gather[1], gather[2], (world - 1) * (gather[1] + gather[2]) * 8 / 1e9,
                                                                      "host-staged gloo" if rehearsal else "pa_comm_allgather_start (RCCL)"))
        res = {
            "metric": BASELINE_METRIC,
            "value": value, "unit": "cells/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True,
            "settle": {"passes": n_settle, "ms": args.settle_ms,
                       "what": "untimed passes of the same step BEFORE the W warmup steps (GPU clock ramp after idle, tools/steps_sweep.sh)"},
            "scaling": "strong" if world > 1 else "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload, "mode": mode,
                       "mesh": "%dx%d quad_mesh on [%g,%g]^2 (reference generator)" % (N, N, w["lo"][0], w["hi"][0]),
                       "hho_degree_info": [w["cd"], w["fd"]], "k": w["fd"], "quadrature": w["quad"], "stabilization": w["stab"],
                       "cells": total_cells, "msize": sz.msize,
                       "outputs": ("lc (msize^2 f64) + cell rhs per cell, to HBM" if mode == "L" else
                                   "lc + cell rhs per cell, Dirichlet data, then assembler<Mesh>'s global system in CSR: %d values + RHS of %d rows"
                                   % (int(pipe.ainfo.nnz), int(pipe.ainfo.nrows)) if mode == "A" else
                                   "cell rhs, packed condensed records (%d f64 per cell: upper triangle of the Schur complement + condensed rhs), "
                                   "CSR values + right-hand side of the face-only system's owned rows" % pipe.ci.cond_doubles),
                       "parallelism": "cell rows block-partitioned over %d GPU(s)" % world,
                       "exchange": exch, "note": w["note"]},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_reason,
                         "kernel": li.kernel_name.decode() + " + hho_cell_pre (its one-thread-per-cell pre-pass)",
                         "kernel_ms": kern_ms,
                         "kernel_ms_is": ("HIP events on the launch stream around the dominant kernel's launches of one step (pre-pass + cooperative "
                                          "kernel: the sum of their rocprofv3 averages; with cut cells also their kernel and the merge), mean over the "
                                          "timed steps, max over ranks") if mode != "C" else
                                         ("HIP events around EVERY kernel of the step that moves the mode's algorithmic bytes: cell rhs + operators with "
                                          "the condensation fused + CSR fill (stage_ms), mean over the timed steps, max over ranks"),
                         # the kernels of the step one by one, each with the bytes IT moves by construction (not the notional COO)
                         "per_kernel": per_kernel,
                         "algorithmic_bytes_per_cell": bpc, "cells_per_launch": n_local,
                         "lanes_per_cell": li.lanes_per_cell, "grid_blocks": li.grid_blocks,
                         "lds_bytes_per_block": li.lds_bytes_per_block},
            # the survey's second roof: the path is FP64-bound, not HBM-bound, for k >= 2.  Informational: the kernel executes
            # fewer flops than the reference's algorithm (cell integrals through moments, data + stab through one Z^T Z), so
            # this is reference work done per second, not an instruction-level utilisation.
            "roofline_fp64": None if fl is None else {
                "bound": "fp64", "achieved": n_local * fl / (kern_ms * 1e-3) / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": n_local * fl / (kern_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                "reference_flops_per_cell": fl,
                "peak_sustained_measured": FP64_SUSTAINED_TFLOPS,
                "frac_of_sustained": n_local * fl / (kern_ms * 1e-3) / 1e12 / FP64_SUSTAINED_TFLOPS,
                "source": "exact count of the instrumented CPU restatement (oracle/flopcount -> oracle/flops_per_cell.json)"},
            "stage_ms": stage_max,
            "build_stamp": stamp,
            # N > 1: how the step's exchange travelled, for the driver to read without parsing prose
            "transport": None if world == 1 or mode != "C" else ("host-staged" if rehearsal else "rccl"),
            "rccl_error": rccl_error,
            "kernel_only_cells_per_s": n_local * world / (kern_ms * 1e-3),
            "same_step_one_gpu": None if one_gpu is None else dict(one_gpu, unit="cells/s", speedup=value / one_gpu["value"],
                                                                   what="the identical step (mode %s, whole mesh) on rank 0's GPU alone" % mode),
            "exchange_checked": exchange_checked,      # N > 1: sums of the ranks' CSR values / right-hand sides == the one-GPU reference's
        }
        if args.full and not args.no_cpu_baseline:
            # the CPU loop in the same run at every N (rank 0's host cores; the other ranks wait at the barrier below)
            res["cpu_baseline"] = cpu_baseline_cut(w) if pipe.cut else cpu_baseline(w, args.cpu_sample_rows)
            res["gpu_over_cpu"] = value / res["cpu_baseline"]["value"]
            if mode == "A" and res["cpu_baseline"].get("matrix_assembly"):
                ma = res["cpu_baseline"]["matrix_assembly"]
                res["matrix_assembly"] = {"value": value, "unit": "cells/s", "ms_per_step": ms_per_step,
                                          "cpu_one_core": ma["value"], "cpu_all_cores": ma["value_all_cores"],
                                          "gpu_over_cpu_one_core": value / ma["value"], "gpu_over_cpu_all_cores": value / ma["value_all_cores"],
                                          "what": "the span the reference prints as \"Matrix assembly\": operators + rhs + assemble + finalize, "
                                                  "whole step of this line against the same span of the CPU restatement"}
        else:
            res["cpu_baseline"] = None
        print(json.dumps(res), flush=True)

    if comm is not None:
        comm.close()
    if world > 1:
        dist.barrier()
        if abandoned_thread:          # a thread is still inside RCCL: leave without running its teardown -- and not with rc 0:
            sys.stdout.flush()        # the line above is a measurement of the host-staged transport, the run itself did not go as asked
            os._exit(3)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
