// obstacle_rhs.hpp -- the per-(cell, local row) right-hand-side sum of obstacle_assembler::assemble (hho.hpp:676-679, :686), in a
// header of its own: hho_assembly.hpp (the triplet route, capi_obstacle.hip) and obstacle_csr.hip (the direct CSR route) include it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

// Right-hand-side sum of local row i of one cell (hho.hpp:676-679, :686): minus the dropped columns j (col[j] < 0) times what is
// known there -- gamma for the cell column of an active cell, the Dirichlet data dd[j] for a boundary face --, subtracted in
// column order from zero; the cell rows (i < cbs) add the cell's right-hand side last.  A: the cell's msize x msize operator,
// column-major; `assembled`: the row is pushed at all (not a Dirichlet face's); cell_rhs: the cell's cbs values or null.
// The ONE statement of this sum: obstacle_triplets_kernel and the direct CSR fill (obstacle_csr.hip) both call it, so that the
// compiler contracts the same products into the same fused multiply-adds on both routes.
__device__ __forceinline__ double obstacle_rhs_row(const double *A, int msize, int cbs, int i, bool assembled, const int32_t *col,
                                                   const double *dd, double gam, const double *cell_rhs)
{
    double s = 0.0;
    if (assembled)
        for (int j = 0; j < msize; ++j)
            if (col[j] < 0) s -= A[i + j * msize] * (j < cbs ? gam : dd[j]);    // :676-679
    if (i < cbs && cell_rhs != nullptr) s += cell_rhs[i];                        // :686
    return s;
}

}  // namespace pa
