// obstacle_csr.hpp -- host entry point of obstacle_csr.hip: obstacle_assembler's system (hho.hpp:609-695, :746-750) for cell
// degree 0, built directly in CSR from the face adjacency tables of condensed.hpp and the prefix counts of assembler_csr.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "condensed.hpp"

namespace pa {

struct ObstacleCsrArgs {
    // the mesh and the symbolic tables of the plain assembler's system (whole-mesh context)
    const uint32_t *cell_faces;
    const int32_t *face_compress;
    const CondFace *faces;             // nown records
    const CondFaceLean *lean;
    const uint32_t *colprefix;         // nown + 1: column faces of the faces before q
    const uint32_t *cprefix;           // ncells + 1: non-Dirichlet faces of the cells before c
    const uint32_t *fprefix;           // nown + 1: cells of the faces before q
    uint32_t ncells, nown;
    uint64_t cell_nnz;                 // entries of all cell rows: ncells + fbs cprefix[ncells]
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
