"""The interface problem's face-only system by row slabs (pa_interface_rows_*) next to the whole-mesh path
(pa_interface_condensed_*), on ONE device: the slabs of R ranks assembled one after the other, each in its own context, the real
packed halo of the slab below handed to the next one; HIP events after a warm-up, medians in ms.  Per slab: the records, the halo
pack, the fill, the recovery (on the right-hand side in place of a solution: the kernel time alone).  No exchange and no solve are
timed: both need one GPU per rank.  The stacked values are compared with the whole mesh's.
    python tools/interface_rows_timing.py [N] [k] [slabs] [reps]          (default 512 2 8 10)"""
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
    return statistics.median(out)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    R = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    f64 = dict(dtype=torch.float64, device="cuda:0")

    w = BatchAssembler(0)
    w.cut_preprocess(N, refsteps=4)
    ops = w.interface_local_ops(k)
    g = w.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    qi = w.ctx.interface_condensed_query(k)
    rp, ci = w.interface_condensed_csr_pattern(k)
    va, RH = torch.empty(max(qi.nnz, 1), **f64), torch.empty(max(qi.system_size, 1), **f64)
    rec = w.interface_condensed_ops(k, ops)
    w.interface_condensed_csr_fill(k, rec, g, va, RH)
    w.synchronize()
    whole = {"rows": qi.system_size, "nnz": qi.nnz, "cut_cells": w.ncut,
             "records_ms": timed(lambda: w.interface_condensed_ops(k, ops), reps),
             "fill_ms": timed(lambda: w.interface_condensed_csr_fill(k, rec, g, va, RH), reps),
             "recover_ms": timed(lambda: w.interface_condensed_recover(k, ops, RH[:qi.system_size], g), reps)}
    del ops, rec
    torch.cuda.empty_cache()

    bounds = [r * N // R for r in range(R + 1)]
    slabs, halo, rows, nnz, same = [], None, 0, 0, True
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        a = BatchAssembler(0)
        a.cut_preprocess(N, refsteps=4, rows=(r0, r1))
        sops = a.interface_local_ops(k)
        sg = a.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
        i = a.interface_rows_info(k)
        n = i.row_end - i.row_begin
        srp, sci = a.interface_rows_csr_pattern(k)
        sva, sRH = torch.empty(max(i.nnz_owned, 1), **f64), torch.empty(max(n, 1), **f64)
        srec = a.interface_rows_ops(k, sops)
        a.interface_rows_csr_fill(k, srec, sg, halo, sva, sRH)
        out = torch.empty(max(i.halo_send_doubles, 1), **f64)
        a.interface_rows_halo_pack(k, srec, sg, out)
        a.synchronize()
        same = same and torch.equal(sva[:i.nnz_owned], va[nnz:nnz + i.nnz_owned]) and torch.equal(sRH[:n], RH[rows:rows + n]) and \
            torch.equal(srp + nnz, rp[rows:rows + n + 1]) and torch.equal(sci, ci[nnz:nnz + i.nnz_owned])
        xF = RH[i.row_begin:i.col_end].clone()
        slabs.append({"rows": [r0, r1], "cells": a.ncells, "cut_cells": a.ncut, "owned_rows": n, "nnz_owned": i.nnz_owned,
                      "halo_recv_doubles": i.halo_recv_doubles, "halo_send_doubles": i.halo_send_doubles,
                      "records_ms": timed(lambda: a.interface_rows_ops(k, sops), reps),
                      "halo_pack_ms": timed(lambda: a.interface_rows_halo_pack(k, srec, sg, out), reps),
                      "fill_ms": timed(lambda: a.interface_rows_csr_fill(k, srec, sg, halo, sva, sRH), reps),
                      "recover_ms": timed(lambda: a.interface_rows_recover(k, sops, xF, sg), reps)})
        halo = out[:i.halo_send_doubles].clone() if r1 < N else None
        rows, nnz = rows + n, nnz + i.nnz_owned
        del a, sops, srec, sva, sRH
        torch.cuda.empty_cache()
    same = same and rows == qi.system_size and nnz == qi.nnz

    res = {"N": N, "k": k, "slabs": R, "reps": reps, "whole": whole, "by_slab": slabs, "stacked_equals_whole_mesh": bool(same)}
    print("interface %dx%d k=%d: %d rows, %d nnz, %d cut cells; %d slabs one after the other on one device" %
          (N, N, k, qi.system_size, qi.nnz, whole["cut_cells"], R))
    print("  whole mesh: records %.3f ms, fill %.3f ms, recovery %.3f ms" % (whole["records_ms"], whole["fill_ms"], whole["recover_ms"]))
    for s in slabs:
        print("  rows %4d-%4d: %6d cells (%4d cut), %7d owned rows; records %.3f ms, halo pack %.3f ms (%d doubles up), fill %.3f ms, "
              "recovery %.3f ms" % (s["rows"][0], s["rows"][1], s["cells"], s["cut_cells"], s["owned_rows"], s["records_ms"],
                                    s["halo_pack_ms"], s["halo_send_doubles"], s["fill_ms"], s["recover_ms"]))
    for key in ("records_ms", "halo_pack_ms", "fill_ms", "recover_ms"):
        print("  %-13s slowest slab %.3f ms, sum over the slabs %.3f ms" % (key[:-3], max(s[key] for s in slabs), sum(s[key] for s in slabs)))
    print("  stacked slabs equal the whole-mesh CSR bit for bit: %s" % same)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
