// obstacle_csr.hpp -- host entry point of obstacle_csr.hip: obstacle_assembler's system (hho.hpp:609-695, :746-750) for cell
// degree 0, built directly in CSR from the tables of face_system.hpp (a FaceSystemView).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "face_system.hpp"

namespace pa {

struct ObstacleCsrArgs {
    // the mesh and the symbolic tables of the plain assembler's system (whole-mesh context, after asm_prepare)
    FaceSystemView v;
    uint64_t cell_nnz;                 // entries of all cell rows: asm_sizes(v, 1, fbs).cell_nnz
    // the active set
    const uint8_t *in_A;
    const int32_t *A_ct, *B_ct;
    uint64_t num_I, num_other;
    // one assembly
    const double *lc, *rhs, *g, *gamma;       // rhs, g may be null
    int64_t *rowptr;
    int32_t *colind;
    double *values, *RHS;                     // RHS may be null
};

// rowptr (ncells + fbs nown + 1), colind / values (the stored entries only) and RHS of the obstacle system; *removed receives
// the number of (non-Dirichlet face, active adjacent cell) pairs: the system stores the plain system's nnz - fbs * *removed
// entries.  Returns after the stream has drained; its temporaries are gone on every path out.
hipError_t obstacle_csr_assemble(hipStream_t stream, int fbs, const ObstacleCsrArgs &args, uint32_t *removed);

}  // namespace pa
