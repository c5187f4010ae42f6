// patch_precond.hpp -- host entry points of patch_precond.hip: the additive Schwarz preconditioner over patches of rows
//   z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r
// for the conjugate gradient of solver_cg.hpp:63-144 in place of the point Jacobi (the solve of cuthho_square.cpp:915-919; the solver
// with it: rows_precond.hpp), and the patch tables of the face-only systems.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "structured_mesh.hpp"

namespace pa {

constexpr int PATCH_MAX_ROWS = 16;         // PA_PATCH_MAX_ROWS: 4 fbs at k = 3

// the patch table: patch p holds the rows rows[ptr[p]] .. rows[ptr[p + 1] - 1] of an n-row system.  row0: the system is the rows
// [row0, row0 + n) of a larger one (a rank's rows: CgRowsWindow, cg.hpp) and the table names them by their global indices; the
// matrix is stored from row 0 on with global columns, the vectors hold the n rows
struct PatchTable {
    size_t n, npatches;
    const int64_t *ptr;                    // npatches + 1
    const int32_t *rows;                   // ptr[npatches]
    int64_t row0 = 0;
};

// what one table needs.  lanes: the lanes that share a patch (4, 8 or 16: the smallest that holds max_rows); every patch's factor
// takes max_rows (max_rows + 1) / 2 doubles (the packed lower triangle of L^-1, row by row)
struct PatchSizes {
    uint64_t entries;                      // ptr[npatches]
    int32_t max_rows, lanes;
    uint64_t factor_doubles;               // npatches * max_rows (max_rows + 1) / 2
    uint64_t slot_ints;                    // n + 1 + entries: per row where its contributions sit in the patch-major buffer
    uint64_t scratch_bytes;                // the patch-major buffer and the counters of the build
};

// why a table was refused (0 = it was not).  Where the rows break several rules the largest code is reported: a repeated or
// misplaced index usually leaves the row it stands for uncovered, and the cause says more than the consequence
enum { PATCH_OK = 0, PATCH_BAD_SIZE = 1, PATCH_UNCOVERED_ROW = 2, PATCH_REPEATED_ROW = 3, PATCH_BAD_INDEX = 4, PATCH_TOO_LARGE = 5 };
const char *patch_refusal_text(int refusal);

// sizes of the table; checks ptr alone (ptr[0] = 0, every patch of 1..16 rows).  Waits for the stream.
hipError_t patch_query(hipStream_t stream, size_t n, size_t npatches, const int64_t *ptr, PatchSizes *out, int *refusal);
// validates the table (indices, repeats, cover) -- nothing but scratch is written unless it passes --, builds the row-to-slots
// table and factors every patch; info[p] = 0 or j + 1 for the first non-positive pivot j; *failed = patches with info != 0.
// Waits for the stream.
hipError_t patch_factor(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const PatchTable &t,
                        const PatchSizes &sz, double *factors, int32_t *slots, void *scratch, int32_t *info, int *refusal, size_t *failed);
// z = M r with the factors and slots of patch_factor; part_rz (may be null): the partial sums of r . z per block of RB rows
void patch_apply(hipStream_t stream, const PatchTable &t, const PatchSizes &sz, const double *factors, const int32_t *slots,
                 void *scratch, const double *r, double *z, double *part_rz);

// ---- the patch tables of the face-only system of pa_condensed_csr_pattern (whole-mesh contexts: compressed face q owns rows
// q fbs .. q fbs + fbs - 1) ----
// one patch per non-Dirichlet face; row0: the first row of the nfaces faces (a slab's: its row_begin)
void face_patches(hipStream_t stream, uint32_t nfaces, int fbs, int32_t row0, int64_t *ptr, int32_t *rows);
// flags[c] = cell c has a non-Dirichlet face (cprefix: non-Dirichlet faces of the cells before c, ncells + 1)
void cell_patch_flags(hipStream_t stream, uint32_t ncells, const uint32_t *cprefix, uint8_t *flags);
// one patch per flagged cell (index[c]: its patch, -1 none), rows in the cell's face order bottom, right, top, left
void cell_patches(hipStream_t stream, uint32_t ncells, uint32_t npatches, const uint32_t *cell_faces, const int32_t *face_compress,
                  const uint32_t *cprefix, const int32_t *index, int fbs, int64_t *ptr, int32_t *rows);

// ---- the cell patches of a slab of the generator mesh that owns the compressed faces [p0, p1): one patch per cell of the slab
// with an owned non-Dirichlet face, the global rows of those faces in the cell's face order.  ptr = null: the sizes only.  Waits.
hipError_t slab_cell_patches(hipStream_t stream, const StructuredMesh &sm, int32_t p0, int32_t p1, int fbs, uint64_t *npatches,
                             uint64_t *entries, int64_t *ptr, int32_t *rows);

}  // namespace pa
