// interface_csr.hpp -- host entry points of interface_csr.hip: interface_assembler's global system (cuthho_square.cpp:1091-1443,
// cut cells and cut faces with two blocks of unknowns) in CSR, built from the tables of pa_cut_preprocess.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

// the cut mesh as the interface numbering sees it (the context's device copies; whole-mesh contexts only)
struct IfCsrMesh {
    const uint32_t *cell_faces;                 // ncells x 4 global face ids
    const int8_t *cell_loc, *face_loc;          // LOC_* of cut_host.hpp
    const int32_t *cut_index;                   // cell -> row of the cut batches, -1 for uncut cells
    const int32_t *cell_table, *face_table;     // first block of a cell / face (face_table -1: Dirichlet face)
    uint32_t ncells, nfaces;
    uint32_t num_all_cells, num_other_faces;    // cell blocks / face blocks (cut elements counted twice)
};

// A row group is one block of unknowns: a cell block (cbs rows) or a face block (fbs rows).  Every row of a group has the same
// columns, a sorted run of units (a unit is one whole block of columns).  `cell` lists the (at most two) cells that push rows
// into the group, lower id first; rcode[s] packs their local row bases (see ifc_code in interface_csr.hip).
struct IfGroup {
    uint64_t vstart;        // first CSR entry of the group's first row
    uint32_t ustart;        // first unit
    uint16_t nunits, R;     // units; entries per row
    int32_t cell[2];        // -1: none
    uint32_t rcode;         // local row bases of cell[0] (low 16 bits) and cell[1] (high 16 bits)
    uint32_t pad_;
};
struct IfUnit {
    int32_t gcol;           // first global column of the block
    uint16_t pos, width;    // position in the row, cbs or fbs
    uint32_t ccode;         // local column bases of cell[0] (low 16 bits) and cell[1] (high 16 bits)
};

// the symbolic tables of one (cut mesh, face degree), owned by the context
struct IfCsrTables {
    int face_deg = -1;
    uint64_t nrows = 0, nnz = 0;
    uint32_t ngroups = 0, nunits = 0;
    IfGroup *groups = nullptr;
    IfUnit *units = nullptr;
};

// builds *t (freeing what it holds first); on failure every allocation is released and *t is left empty
hipError_t ifcsr_build(hipStream_t stream, const IfCsrMesh &m, int face_deg, IfCsrTables *t);
void ifcsr_release(IfCsrTables *t);
hipError_t ifcsr_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind);
hipError_t ifcsr_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const double *lc, const double *rhs, const double *g,
                      const double *lc_cut, const double *rhs_cut, double *values, double *RHS);

}  // namespace pa
