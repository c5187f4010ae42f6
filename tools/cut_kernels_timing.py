"""The two cut-cell kernels on the circle of the cut workloads (refsteps 4), on the library PA_LIB names (default: the shipped
one), timed with HIP events after a warm-up: `reps` repetitions of each, median with min and max,
  per launch of pa_cut_local_ops_batch        cut_local_ops_kernel alone, outputs lc + rhs, 20 launches per repetition;
  per call of pa_cut_interface_ops_batch      cut_interface_kernel, the stabilization of both sides through cut_local_ops_kernel
                                              and the lc scatter, outputs lc + rhs + info, 10 calls per repetition.
One process per figure wanted, under a time limit of its own:
    timeout -k 10 300 python tools/cut_kernels_timing.py [N] [k] [reps]          (default 512 2 10)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import proton_amd as pa  # noqa: E402
from proton_amd.batch import BatchAssembler  # noqa: E402


def timed(fn, inner, reps):
    """-> ms per call of fn: `reps` figures, each `inner` calls between two events"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return out


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    asm = BatchAssembler(0)
    asm.cut_preprocess(N, refsteps=4)
    cut = asm.cut_local_ops(k, want=("lc", "rhs"))                       # warm-up: the quadrature lists of the negative side
    ops = asm.interface_local_ops(k, kappa=(1.0, 7.5))                   # ... of both sides, the context's scratch
    asm.synchronize()
    parms = pa.capi.InterfaceParams(1.0, 7.5, 5.0)

    def one_sided():
        asm.ctx.cut_local_ops(k, asm.level_set, pa.capi.LOC_NEGATIVE, pa.capi.FN_SIN_SIN_RHS, pa.capi.FN_SIN_SIN_SOL, None, None, None,
                              cut["lc"].data_ptr(), cut["rhs"].data_ptr(), None)

    def two_sided():
        asm.ctx.cut_interface_ops(k, asm.level_set, parms, pa.capi.FN_SIN_SIN_RHS, None, None, ops["lc_cut"].data_ptr(),
                                  ops["rhs_cut"].data_ptr(), ops["info_cut"].data_ptr())

    timed(one_sided, 20, 2)
    timed(two_sided, 10, 2)
    t1, t2 = timed(one_sided, 20, reps), timed(two_sided, 10, reps)
    asm.synchronize()
    med = statistics.median
    print("%dx%d k=%d: %d cut cells; %d repetitions (library %s)" % (N, N, k, asm.ncut, reps, pa.capi.LIB_PATH))
    print("  pa_cut_local_ops_batch (lc + rhs)    median %.4f ms per launch [min %.4f max %.4f]" % (med(t1), min(t1), max(t1)))
    print("  pa_cut_interface_ops_batch (lc, rhs) median %.4f ms per call   [min %.4f max %.4f]" % (med(t2), min(t2), max(t2)))
    print(json.dumps({"N": N, "k": k, "cut_cells": asm.ncut, "reps": reps,
                      "cut_local_ops_ms": {"median": med(t1), "min": min(t1), "max": max(t1)},
                      "cut_interface_ops_ms": {"median": med(t2), "min": min(t2), "max": max(t2)}}))


if __name__ == "__main__":
    main()
