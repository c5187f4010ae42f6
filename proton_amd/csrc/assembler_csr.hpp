// assembler_csr.hpp -- host entry points of assembler_csr.hip: the reference's own global system (cell + face unknowns,
// hho.hpp:252-463) in CSR, built from the face adjacency tables of condensed.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "condensed.hpp"
#include "device_buf.hpp"
#include "hho_asm_scatter.hpp"

namespace pa {

// direct CSR of the assembler's own system: non-Dirichlet faces per cell / cells per face and their exclusive prefixes (nfc, cprefix:
// ncells + 1; nfcell, fprefix: nown + 1), and per cell where the fused assembly's scatter writes (hho_asm_scatter.hpp); built on first
// use (asm_prepare)
struct AsmTables {
    DeviceBuf<uint32_t> nfc, cprefix, nfcell, fprefix;
    DeviceBuf<AsmCellRec> scatter;
    uint64_t cell_faces_total = 0, face_cells_total = 0;
    bool ready() const { return scatter.get() != nullptr; }
};

// fills t's counts and prefixes (allocated by the caller) from the view's mesh and lean records
hipError_t asm_build_tables(hipStream_t stream, const FaceSystemView &v, const AsmTables &t);
hipError_t asm_pattern(hipStream_t stream, const FaceSystemView &v, int cbs, int fbs, int64_t *rowptr, int32_t *colind);
hipError_t asm_fill(hipStream_t stream, const FaceSystemView &v, int cbs, int fbs, const double *lc, const double *rhs, const double *g,
                    double *values, double *RHS);
// the fused path (pa_assembler_csr_assemble): the per-cell scatter table of hho_asm_scatter.hpp (ncells records; whole-mesh contexts,
// where a face's compressed id is its position in `faces`), and the zeroing of the entries the scatter accumulates
hipError_t asm_build_scatter_table(hipStream_t stream, const FaceSystemView &v, AsmCellRec *out);
hipError_t asm_zero_accumulated(hipStream_t stream, const FaceSystemView &v, int cbs, int fbs, double *values, double *RHS);
// the fictitious-domain path (pa_fictdom_csr_assemble): the cut cells' operators (cut_lc ncut x msize^2 column-major, cut_rhs ncut x cbs
// or null = 0; cut_cells: their indices in the context) through asm_scatter_cell, for the pairs (face_deg + 1, face_deg), face_deg <= 2;
// lc_out (ncells x msize^2 or null) receives the cut cells' rows
hipError_t asm_cut_scatter(hipStream_t stream, int face_deg, const AsmScatterArgs &s, uint32_t ncut, const uint32_t *cut_cells,
                           const double *cut_lc, const double *cut_rhs, double *lc_out);

}  // namespace pa
