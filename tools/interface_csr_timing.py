"""Timing of the interface problem's global system (cuthho_square -i, interface_assembler) on the device, with HIP events after a
warm-up: the sorted path (pa_interface_triplets_batch + pa_csr_from_triplets) against the direct CSR (pa_interface_csr_pattern once,
pa_interface_csr_fill per assembly).  The fill's algorithmic bytes: the local matrices it uses read once (uncut cells' lc, cut
cells' lc_cut), values and RHS written once.
    python tools/interface_csr_timing.py [N] [k] [reps]          (default 512 2 10)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    info = asm.ctx.interface_info(k)
    cbs = (k + 3) * (k + 2) // 2
    ms = cbs + 4 * (k + 1)
    asm.synchronize()

    def sorted_path():
        t = asm.interface_triplets(k, ops, g)
        r = torch.cat([t["rows"].reshape(-1), t["rows_cut"].reshape(-1)])
        c = torch.cat([t["cols"].reshape(-1), t["cols_cut"].reshape(-1)])
        v = torch.cat([t["vals"].reshape(-1), t["vals_cut"].reshape(-1)])
        return asm.csr_from_triplets(r, c, v, info.system_size)

    def triplets_only():
        asm.interface_triplets(k, ops, g)

    pattern_first = timed(lambda: asm.interface_csr_pattern(k), 1)[0]          # symbolic tables built here
    rowptr, colind = asm.interface_csr_pattern(k)
    values = torch.empty(colind.numel(), dtype=torch.float64, device=asm.device)
    RHS = torch.empty(info.system_size, dtype=torch.float64, device=asm.device)
    sorted_path(); asm.interface_csr_fill(k, ops, g, values, RHS)                   # warm-up
    asm.synchronize()
    t_sorted = timed(sorted_path, reps)
    t_trip = timed(triplets_only, reps)
    t_pattern = timed(lambda: asm.interface_csr_pattern(k), reps)
    t_fill = timed(lambda: asm.interface_csr_fill(k, ops, g, values, RHS), reps)
    ncut, nc = asm.ncut, asm.ncells
    lc_bytes = 8 * ((nc - ncut) * ms * ms + ncut * 4 * ms * ms)
    out_bytes = 8 * (colind.numel() + info.system_size)
    fill_ms = statistics.median(t_fill)
    res = {"N": N, "k": k, "cells": nc, "cut_cells": ncut, "nrows": info.system_size, "nnz": colind.numel(), "reps": reps,
           "sorted_path_ms": statistics.median(t_sorted), "of_which_triplets_ms": statistics.median(t_trip),
           "pattern_first_call_ms": pattern_first, "pattern_ms": statistics.median(t_pattern), "fill_ms": fill_ms,
           "fill_min_ms": min(t_fill), "fill_bytes": lc_bytes + out_bytes, "fill_lc_bytes": lc_bytes, "fill_out_bytes": out_bytes,
           "fill_GBps": (lc_bytes + out_bytes) / (fill_ms * 1e-3) / 1e9,
           "speedup_fill_vs_sorted": statistics.median(t_sorted) / fill_ms}
    print("interface %dx%d k=%d: %d cells (%d cut), %d rows, %d nnz" % (N, N, k, nc, ncut, info.system_size, colind.numel()))
    print("  sorted path (triplets + csr_from_triplets): %.2f ms (triplets alone %.2f ms)" % (res["sorted_path_ms"], res["of_which_triplets_ms"]))
    print("  direct pattern: %.2f ms first call (symbolic tables), %.2f ms after" % (pattern_first, res["pattern_ms"]))
    print("  direct fill: %.3f ms median, %.3f ms min; %.1f MB algorithmic -> %.0f GB/s" %
          (fill_ms, res["fill_min_ms"], res["fill_bytes"] / 1e6, res["fill_GBps"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
