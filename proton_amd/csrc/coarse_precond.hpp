// coarse_precond.hpp -- host entry points of coarse_precond.hip: a Galerkin coarse level for the device conjugate gradient
//   z = (accumulate ? z : 0) + P (P^T A P)^-1 P^T r
// added to the patch sum of patch_precond.hpp in the conjugate gradient of solver_cg.hpp:63-144 (the solve of
// cuthho_square.cpp:915-919; the solver with both: rows_precond.hpp), and the coarse table of the face-only system: bilinear hats
// on every H-th mesh line.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "interface_csr.hpp"
#include "structured_mesh.hpp"

namespace pa {

constexpr int COARSE_MAX_ROW_ENTRIES = 4;  // PA_COARSE_MAX_ROW_ENTRIES
constexpr int COARSE_MAX_NODES = 4096;     // PA_COARSE_MAX_NODES
constexpr int COARSE_W_SLOTS = 16;         // (column, value) slots of a row of A P

// the coarse table P (n x ncoarse) in CSR: row i holds cols[ptr[i]] .. cols[ptr[i + 1] - 1], ascending, with vals
struct CoarseTable {
    size_t n, ncoarse;
    const int64_t *ptr;                    // n + 1
    const int32_t *cols;
    const double *vals;
};

// what one table needs.  pt: P^T in CSR as one buffer (row pointer, fine rows, values); the factor is the packed lower triangle of
// L^-1 (row i at i (i + 1) / 2); the scratch holds the coarse vectors of an apply in front and the build's work space behind
struct CoarseSizes {
    uint64_t entries;                      // ptr[n]
    uint64_t pt_bytes, factor_doubles, scratch_bytes;
};

// why a table was refused (0 = it was not); where a table breaks several rules the largest code is reported
enum { COARSE_OK = 0, COARSE_BAD_SIZE = 1, COARSE_BAD_VALUE = 2, COARSE_BAD_ORDER = 3, COARSE_BAD_INDEX = 4, COARSE_BAD_NODES = 5,
       COARSE_TOO_LARGE = 6, COARSE_W_OVERFLOW = 7, COARSE_BAD_LEVEL_NODES = 8 };
const char *coarse_refusal_text(int refusal);

// sizes of the table; checks ncoarse and ptr alone (ptr[0] = 0, every row of 0..4 entries).  Waits for the stream.
hipError_t coarse_query(hipStream_t stream, size_t n, size_t ncoarse, const int64_t *ptr, CoarseSizes *out, int *refusal);
// the columns and values of a table whose ptr has passed coarse_query: in range, ascending, finite.  Writes scratch only.  Waits.
hipError_t coarse_validate(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, void *scratch, int *refusal);
// the two checks alone, for a table of up to max_nodes columns (multilevel_precond.hip: a smoothed level has no dense matrix and no
// COARSE_MAX_NODES).  coarse_check_ptr: ncoarse and ptr as coarse_query, -> ptr[n]; coarse_check_rows: the columns and values as
// coarse_validate, with counts (ncoarse + 2: the rows that hold a column) and flags (4 int32) the caller's.  Both wait.
hipError_t coarse_check_ptr(hipStream_t stream, size_t n, size_t ncoarse, size_t max_nodes, const int64_t *ptr, uint64_t *entries,
                            int *refusal);
hipError_t coarse_check_rows(hipStream_t stream, const CoarseTable &t, uint32_t *counts, int32_t *flags, int *refusal);
// P^T, A_c = P^T A P (to coarse_matrix as well if not null), its Cholesky factor and the packed L^-1 of a validated table;
// *pivot = 0 or j + 1 for the first non-positive pivot j; *refusal: a row of A P beyond COARSE_W_SLOTS columns.  Waits.
hipError_t coarse_factor(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const CoarseTable &t,
                         const CoarseSizes &sz, void *pt, double *factor, void *scratch, double *coarse_matrix, int32_t *pivot,
                         int *refusal);
// z = (accumulate ? z : 0) + P L^-T L^-1 P^T r; part_rz (may be null): the partial sums of r . z per block of RB rows
void coarse_apply(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const void *pt, const double *factor, void *scratch,
                  int accumulate, const double *r, double *z, double *part_rz);

// ---- the same in stages, for a table that holds the rows [row0, row0 + n) of P on one rank of a row-partitioned system ----
// P for the `rows` rows from global row col0 on: the columns a rank's matrix rows read (its own rows and the ends of its neighbours')
struct CoarseWindow {
    int64_t col0;
    size_t rows;
    const int64_t *ptr;                    // rows + 1
    const int32_t *cols;
    const double *vals;
};
// coarse_factor up to the coarse matrix: P^T of the table's rows, W = A P with P from win (null: the table itself), and this
// table's addend P^T W in the scratch, both triangles.  After coarse_validate.  Waits for the stream before the last kernel.
hipError_t coarse_galerkin(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const CoarseTable &t,
                           const CoarseSizes &sz, const CoarseWindow *win, void *pt, void *scratch, int *refusal);
// the coarse matrix in the scratch: its lower triangle packed row by row into tri (ncoarse (ncoarse + 1) / 2 doubles), or (unpack)
// from tri into both triangles
void coarse_matrix_triangle(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, void *scratch, int unpack, double *tri);
// the rest of coarse_factor: Cholesky of the coarse matrix in the scratch and the packed L^-1.  Waits.
hipError_t coarse_cholesky(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, double *factor, void *scratch,
                           double *coarse_matrix, int32_t *pivot);
// the two halves of coarse_apply: -> P^T r of the table's rows (ncoarse doubles in the scratch, the caller may add the other
// ranks' to them in place), and the rest from those
double *coarse_restrict(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const void *pt, void *scratch, const double *r);
void coarse_correct(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const double *factor, void *scratch, int accumulate,
                    const double *r, double *z, double *part_rz);
// coarse_correct without its gather: -> u = L^-T L^-1 (P^T r) (ncoarse doubles in the scratch), for a caller that prolongs several
// levels in one pass (multilevel_precond.hpp)
const double *coarse_solve(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const double *factor, void *scratch);
// rows [first, first + count) of the table as 8 doubles each: four (column as double, value) pairs, padded with column -1
void coarse_rows_pack(hipStream_t stream, const CoarseTable &t, size_t first, size_t count, double *out);
// P for the window: need_lo packed rows below the table's own, need_hi above (a row ends at the first pair whose column is no
// column of the table); wptr: need_lo + n + need_hi + 1, wcols / wvals: entries + 4 (need_lo + need_hi)
void coarse_window_build(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, size_t need_lo, size_t need_hi,
                         const double *recv_lo, const double *recv_hi, int64_t *wptr, int32_t *wcols, double *wvals);

// ---- the coarse table of the face-only system of pa_condensed_csr_pattern (whole-mesh structured contexts) ----
// The mesh and what a face is: its two points (face_pts, point p = vertex (p % (Nx + 1), p / (Nx + 1))), its compressed id (-1
// Dirichlet) and, by side, its location (face_loc) against `where`.  ptr = null: the sizes only.  Waits for the stream.
struct CoarseMesh {
    StructuredMesh sm;
    uint32_t nfaces;
    const uint32_t *face_pts;
    const int32_t *face_compress;
    const int8_t *face_loc;                // null: one part
    int where;
};
// max_columns: the table is written only with 1 to max_columns columns (pa_context_set_coarse_table_cap; the counts are given
// either way)
hipError_t condensed_coarse(hipStream_t stream, const CoarseMesh &m, int fbs, int H, uint64_t max_columns, uint64_t *ncoarse,
                            uint64_t *entries, int64_t *ptr, int32_t *cols, double *vals);

// ---- rows [row_begin, row_end) of that table for a slab of the generator mesh, from the closed forms of structured_mesh.hpp: the
// slab owns the compressed faces [p0, p1); the columns are the whole mesh's, ptr starts at 0 ----
struct SlabCoarseMesh {
    StructuredMesh sm;
    int32_t p0, p1;
};
hipError_t condensed_rows_coarse(hipStream_t stream, const SlabCoarseMesh &m, int fbs, int H, uint64_t *ncoarse, uint64_t *entries,
                                 int64_t *ptr, int32_t *cols, double *vals);

// ---- the same hats on the face-only system of pa_interface_condensed_csr_pattern (interface_assembler's numbering: im) ----
// An uncut non-Dirichlet face owns block face_table[f], a cut one that block (negative side) and the next (positive side); both
// take the values of the face's end points.  by_side: an uncut face's block is in the part of its side, a cut face's blocks in
// parts 0 and 1.  A cut face on the Dirichlet boundary owns nothing: the pointers of its unowned block are written, equal.
struct IfCoarseMesh {
    IfCsrMesh im;
    StructuredMesh sm;
    const uint32_t *face_pts;
    int by_side;
};
hipError_t interface_condensed_coarse(hipStream_t stream, const IfCoarseMesh &m, int fbs, int H, uint64_t max_columns, uint64_t *ncoarse,
                                      uint64_t *entries, int64_t *ptr, int32_t *cols, double *vals);

// ---- rows [row_begin, row_end) of that table for a slab of the interface problem (pa_interface_rows_coarse) ----
// im: the slab's extended tables (interface_rows.hpp: its own faces and those of the cell row below), extended face f being
// global face face0 + f of sm's whole mesh, whose vertex indices the hats live on; the slab owns the extended blocks [q0, q1),
// row (q - q0) fbs + k of the table.  by_side: the columns that stay are decided by the whole mesh, from the tags every rank
// holds (face_loc_all, nfaces_all: device copy of the whole-mesh face_loc), never by the slab's own blocks: the same ncoarse and
// column ids on every slab.  ptr starts at 0.
struct IfRowsCoarseMesh {
    IfCsrMesh im;
    StructuredMesh sm;
    uint32_t face0;
    int32_t q0, q1;
    int by_side;
    const int8_t *face_loc_all;
    uint32_t nfaces_all;
};
hipError_t interface_rows_coarse(hipStream_t stream, const IfRowsCoarseMesh &m, int fbs, int H, uint64_t *ncoarse, uint64_t *entries,
                                 int64_t *ptr, int32_t *cols, double *vals);

}  // namespace pa
