// interface_csr.hpp -- host entry points of interface_csr.hip and interface_condensed.hip: interface_assembler's global system
// (cuthho_square.cpp:1091-1443, cut cells and cut faces with two blocks of unknowns) and its face-only system after static
// condensation, in CSR and as triplets, built from the tables of pa_cut_preprocess.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

constexpr int8_t IF_LOC_CUT = 2;                // LOC_CUT of cut_host.hpp

// the cut mesh as the interface numbering sees it (the context's device copies; whole-mesh contexts only)
struct IfCsrMesh {
    const uint32_t *cell_faces;                 // ncells x 4 global face ids
    const int8_t *cell_loc, *face_loc;          // LOC_* of cut_host.hpp
    const int32_t *cut_index;                   // cell -> row of the cut batches, -1 for uncut cells
    const int32_t *cell_table, *face_table;     // first block of a cell / face (face_table -1: Dirichlet face)
    uint32_t ncells, nfaces;
    uint32_t num_all_cells, num_other_faces;    // cell blocks / face blocks (cut elements counted twice)
};

struct IfDims {
    int cbs, fbs;
};
__host__ __device__ __forceinline__ IfDims if_dims(int face_deg) { return {(face_deg + 3) * (face_deg + 2) / 2, face_deg + 1}; }

// The numbering's index map (:1223-1234, :1291-1321): the global unknown of local unknown i of cell X, whose unknowns are
// [cell | faces] (uncut) or [cell-, cell+, faces-, faces+] (cut).  faces+ of a cut face is its second block, faces+ of an uncut
// face its only block (:1319).  -1 on a Dirichlet face; its entry of the boundary data (nfaces x fbs) goes to *bdof if given.
__device__ __forceinline__ int32_t if_global_index(const IfCsrMesh &m, IfDims d, size_t X, bool cut, int i, size_t *bdof = nullptr)
{
    const int ncd = cut ? 2 * d.cbs : d.cbs;
    if (i < ncd) return (int32_t)((uint64_t)m.cell_table[X] * d.cbs + i);
    const int u = i - ncd, side = u / (4 * d.fbs), lf = (u / d.fbs) % 4, k = u % d.fbs;
    const uint32_t f = m.cell_faces[4 * X + lf];
    const int32_t b = m.face_table[f];
    if (b < 0) {
        if (bdof != nullptr) *bdof = (size_t)f * d.fbs + k;
        return -1;
    }
    const int dup = (cut && side == 1 && m.face_loc[f] == IF_LOC_CUT) ? 1 : 0;
    return (int32_t)((uint64_t)m.num_all_cells * d.cbs + (uint64_t)(b + dup) * d.fbs + k);
}

// the same in the face-only numbering (the numbering without its cell blocks), of local face unknown j
__device__ __forceinline__ int32_t if_face_index(const IfCsrMesh &m, IfDims d, size_t X, bool cut, int j, size_t *bdof = nullptr)
{
    const int32_t gi = if_global_index(m, d, X, cut, (cut ? 2 : 1) * d.cbs + j, bdof);
    return gi < 0 ? -1 : gi - (int32_t)m.num_all_cells * d.cbs;
}

// 16-bit code of at most two local indices (ascending): count in bits 0-1, first in bits 2-8, second in bits 9-15
__host__ __device__ __forceinline__ uint32_t ifc_code1(int a) { return 1u | ((uint32_t)a << 2); }
__host__ __device__ __forceinline__ uint32_t ifc_code2(int a, int b) { return 2u | ((uint32_t)a << 2) | ((uint32_t)b << 9); }
__device__ __forceinline__ int ifc_count(uint32_t c) { return (int)(c & 3u); }
__device__ __forceinline__ int ifc_first(uint32_t c) { return (int)((c >> 2) & 127u); }
__device__ __forceinline__ int ifc_second(uint32_t c) { return (int)((c >> 9) & 127u); }

// A row group is one block of unknowns: a cell block (cbs rows) or a face block (fbs rows).  Every row of a group has the same
// columns, a sorted run of units (a unit is one whole block of columns): the cell units first (cell blocks come first in the
// numbering), then the face units, which are the row of the face-only system.  `cell` lists the (at most two) cells that push
// rows into the group, lower id first; rcode[s] packs their local row bases (see ifc_code above).
struct IfGroup {
    uint64_t vstart;        // first CSR entry of the group's first row
    uint32_t ustart;        // first unit
    uint16_t nunits, R;     // units; entries per row
    int32_t cell[2];        // -1: none
    uint32_t rcode;         // local row bases of cell[0] (low 16 bits) and cell[1] (high 16 bits)
    uint16_t fu0, fpos;     // first face unit (nunits: none) and its position in the row (R: none)
};
static_assert(sizeof(IfGroup) == 32, "IfGroup is two 16-byte loads");
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
    // the face-only (condensed) system of the same numbering: first entry of every face group's rows (num_other_faces + 1)
    // and the total
    uint64_t *cvstart = nullptr;
    uint64_t cnnz = 0;
};

// the local matrices and right-hand sides of the full system: uncut ncells x msize^2 / ncells x cbs (rows of cut cells unused),
// cut ncut x (2 msize)^2 / ncut x 2 cbs; column-major
struct IfLocalArgs {
    const double *lc, *rhs, *g, *lc_cut, *rhs_cut;      // g: nfaces x fbs Dirichlet data or null
};
// The records of the face-only system: uncut cells [S packed (ncells x nf(nf+1)/2) | g (ncells x nf)], cut cells
// [S (ncut x NF(NF+1)/2) | g (ncut x NF)], nf = 4 fbs, NF = 8 fbs; S the upper triangle of the Schur complement, column-packed.
struct IfCondArgs {
    const double *cond, *cond_cut;      // records
    const double *g;                    // nfaces x fbs Dirichlet data or null
    const uint32_t *cut_cells;          // ncut cell ids
    uint32_t ncut;
};
// The face-only system of ONE SLAB of cell rows (pa_interface_rows_*).  The mesh is the slab's extended range (interface_rows.hpp:
// the halo row below, then the slab's cells, numbered from the range's first blocks); the rows are those of the owned face
// blocks [q0, q0 + nq), shifted to start at 0; the columns are global.  A cell of the slab reads the slab's records, a halo cell
// the received halo [S of the nh halo cells | their g | S of their nhc cut cells | their g | nh x nf boundary values: the
// Dirichlet data of each halo cell's faces, zero where a face is not Dirichlet].
struct IfRowsArgs {
    const double *cond, *cond_cut;      // the slab's records
    const double *g;                    // Dirichlet data by the context's own face ids, or null
    const double *halo;                 // the halo received from the slab below; null on slab 0
    uint32_t ncells, ncut;              // the slab's cells and cut cells
    uint32_t nh, nhc;                   // halo cells and the cut cells among them
    uint32_t fshift;                    // extended id of the context's face 0
    uint32_t q0, nq;                    // the owned face blocks
    int32_t col0;                       // global column of the first owned row
    uint64_t v0, nnz;                   // cvstart of block q0; entries of the owned rows
};
// triplets in the reference's push order, n = msize (full) or nf (face-only) unknowns per uncut cell, N = 2 msize or NF per cut
// cell: uncut slots ncells x n^2 (cut cells: all -1), cut slots ncut x N^2; right-hand side slots ncells x n / ncut x N
struct IfTriplets {
    int32_t *rows, *cols; double *vals;
    int32_t *rows_cut, *cols_cut; double *vals_cut;
    int32_t *rhs_rows; double *rhs_vals;
    int32_t *rhs_rows_cut; double *rhs_vals_cut;
};

// builds *t (freeing what it holds first); on failure every allocation is released and *t is left empty
hipError_t ifcsr_build(hipStream_t stream, const IfCsrMesh &m, int face_deg, IfCsrTables *t);
void ifcsr_release(IfCsrTables *t);
// the full system (interface_csr.hip)
hipError_t ifcsr_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind);
hipError_t ifcsr_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfLocalArgs &a, double *values, double *RHS);
hipError_t ifcsr_triplets(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfLocalArgs &a, const IfTriplets &o);
// the face-only system: the same gather reading the records (interface_csr.hip)
hipError_t ifcond_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind);
hipError_t ifcond_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfCondArgs &a, double *values, double *RHS);
hipError_t ifcond_triplets(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const IfTriplets &o);
// the face-only system of a slab: the same gather again, rows local, columns global (interface_csr.hip)
hipError_t ifrows_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfRowsArgs &a, int64_t *rowptr, int32_t *colind);
hipError_t ifrows_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfRowsArgs &a, double *values, double *RHS);
// what a slab sends up: the records of its last ns cells (nsc of them cut, the last of its cut records) and the Dirichlet data
// of their faces, in the layout IfRowsArgs::halo describes; cell_faces / face_dir: the context's
hipError_t ifrows_halo_pack(hipStream_t stream, int face_deg, const uint32_t *cell_faces, const uint8_t *face_dir, uint32_t ncells,
                            uint32_t ncut, uint32_t ns, uint32_t nsc, const double *cond, const double *cond_cut, const double *g,
                            double *halo);

// ---- the dense per-cell work of the condensation (interface_condensed.hip) ------------------------------------------------
// the cut cells' records in double-double (one wavefront per cut cell); info[cc] = 200 + j + 1 for a failed pivot j, else 0
hipError_t ifcond_cut_records(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const double *lc_cut,
                              const double *rhs_cut, double *cond_cut, int32_t *info);
// the uncut cells' info of static_condensation_kernel (j + 1) in the same convention
hipError_t ifcond_info_remap(hipStream_t stream, size_t n, int32_t *info);
// u_T = A_TT^-1 (f_T - A_TF u_F) of every cell (cut cells in double-double) into the interface_assembler's full solution vector:
// cell blocks at cell_table, then xF
hipError_t ifcond_recover(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const double *lc,
                          const double *rhs, const double *lc_cut, const double *rhs_cut, const double *xF, double *full);

// ---- the patch tables of the face-only system for pa_patch_precond_* (patch_precond.hip) ----------------------------------
// Rows are values of if_face_index.  IF_PATCH_FACE: one patch per non-Dirichlet face, all rows of its blocks (a cut face: the
// negative block, then the positive).  IF_PATCH_CELL: one patch per uncut cell, and per side of a cut cell (negative first): the
// blocks if_face_index gives that side's local slots, in the face order bottom, right, top, left -- an uncut face of a cut cell
// only on the side it lies on.  Dirichlet faces are skipped; a cell or side without rows gives no patch.
constexpr int IF_PATCH_FACE = 0, IF_PATCH_CELL = 1;     // PA_PATCH_FACE, PA_PATCH_CELL
// counts the table (*npatches, *entries) and, with ptr given and *entries < 2^31, writes it (ptr *npatches + 1, rows *entries);
// waits for the stream
hipError_t ifcond_patches(hipStream_t stream, const IfCsrMesh &m, int face_deg, int kind, uint64_t *npatches, uint64_t *entries,
                          int64_t *ptr, int32_t *rows);
// The same for a slab of cell rows (pa_interface_rows_patches): m holds the slab's extended tables (interface_rows.hpp), whose
// first halo_cells cells are the row below and give no patch; of an item's blocks those within the owned range [q0, q1) stay, and
// block q gives the GLOBAL rows of block fb0 + q.  A patch that keeps no block is dropped; ptr starts at 0.
struct IfPatchRange {
    size_t item0;                               // the first item
    int32_t q0, q1;                             // the blocks that stay
    int64_t shift;                              // block q is block shift + q of the rows
};
hipError_t ifrows_patches(hipStream_t stream, const IfCsrMesh &m, uint32_t halo_cells, int32_t q0, int32_t q1, int64_t fb0, int face_deg,
                          int kind, uint64_t *npatches, uint64_t *entries, int64_t *ptr, int32_t *rows);

}  // namespace pa
