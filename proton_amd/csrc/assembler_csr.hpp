// assembler_csr.hpp -- host entry points of assembler_csr.hip: the reference's own global system (cell + face unknowns,
// hho.hpp:252-463) in CSR, built from the face adjacency tables of condensed.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "condensed.hpp"
#include "hho_asm_scatter.hpp"

namespace pa {

// per cell the number of its non-Dirichlet faces (nfc, ncells + 1) and its exclusive prefix; per non-Dirichlet face the number of
// its cells (nfcell, nown + 1) and its exclusive prefix
hipError_t asm_build_tables(hipStream_t stream, const CondMesh &m, uint32_t ncells, uint32_t nown, const CondFaceLean *lean,
                            uint32_t *nfc, uint32_t *cprefix, uint32_t *nfcell, uint32_t *fprefix);
hipError_t asm_pattern(hipStream_t stream, const CondMesh &m, int cbs, int fbs, uint32_t ncells, uint32_t nown, uint64_t cell_nnz,
                       const CondFace *faces, const uint32_t *colprefix, const uint32_t *cprefix, const uint32_t *fprefix,
                       int64_t *rowptr, int32_t *colind);
hipError_t asm_fill(hipStream_t stream, const CondMesh &m, int cbs, int fbs, uint32_t ncells, uint32_t nown, uint64_t cell_nnz,
                    const CondFaceLean *lean, const uint32_t *colprefix, const uint32_t *cprefix, const uint32_t *fprefix,
                    const double *lc, const double *rhs, const double *g, double *values, double *RHS);
// the fused path (pa_assembler_csr_assemble): the per-cell scatter table of hho_asm_scatter.hpp (ncells records; whole-mesh contexts,
// where a face's compressed id is its position in `faces`), and the zeroing of the entries the scatter accumulates
hipError_t asm_build_scatter_table(hipStream_t stream, const CondMesh &m, uint32_t ncells, const CondFace *faces, const uint32_t *colprefix,
                                   const uint32_t *cprefix, const uint32_t *fprefix, AsmCellRec *out);
hipError_t asm_zero_accumulated(hipStream_t stream, int cbs, int fbs, uint32_t ncells, uint32_t nown, uint64_t cell_nnz,
                                const CondFace *faces, const uint32_t *colprefix, const uint32_t *fprefix, double *values, double *RHS);

}  // namespace pa
