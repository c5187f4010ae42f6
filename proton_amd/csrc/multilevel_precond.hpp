// multilevel_precond.hpp -- host entry points of multilevel_precond.hip: a SMOOTHED coarse level for the device conjugate gradient
//   z = (accumulate ? z : 0) + P diag(P^T A P)^-1 P^T r
// next to the patch sum of patch_precond.hpp and the exactly solved level of coarse_precond.hpp in the conjugate gradient of
// solver_cg.hpp:63-144 (the solve of cuthho_square.cpp:915-919 on the face-only system): the additive multilevel form on nested hat
// spaces.  The table is coarse_precond.hpp's CoarseTable with its row rules; there is no dense matrix, so ncoarse runs up to
// SMOOTHED_MAX_NODES.  The solver with all three kinds of level: rows_precond.hpp (conjugated_gradient_multilevel).
//
// The order of every sum is part of the contract.  A column's sum (of P^T r, and of d_j) runs over the column's entries by fine
// row ascending: entry e of the column goes to slot e mod 64, every slot adds its entries in ascending order (fused multiply-add),
// and the 64 slots are added by the xor tree 32, 16, 8, 4, 2, 1.  The kernels give a column to a wavefront (a slot per lane) or to a
// quarter of one (four slots per lane, the tree's first two steps inside the lane), chosen on the host by the mean column length:
// the bits do not depend on the choice.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "coarse_precond.hpp"

namespace pa {

constexpr size_t SMOOTHED_MAX_NODES = (size_t)1 << 24;     // PA_SMOOTHED_MAX_NODES
constexpr int MULTILEVEL_MAX_TABLES = 9;                   // PA_MULTILEVEL_MAX_LEVELS smoothed levels and the exact one

// what one level needs.  pt: P^T in CSR as one buffer (row pointer, fine rows ascending within a row, values); the scratch holds the
// coarse vector of an apply in front and the set-up's work space (the sort of the entries by column) behind
struct SmoothedSizes {
    uint64_t entries;                      // ptr[n]
    uint64_t pt_bytes, dinv_doubles, scratch_bytes;
    uint64_t work_bytes;                   // of the scratch: the sort's and the scan's own temporaries
    int lanes;                             // 16 or 64: the lanes that share a column
};

// sizes of the table; checks ncoarse (1 .. SMOOTHED_MAX_NODES) and ptr alone, as coarse_query.  Waits for the stream.
hipError_t smoothed_query(hipStream_t stream, size_t n, size_t ncoarse, const int64_t *ptr, SmoothedSizes *out, int *refusal);
// the columns and values of a table whose ptr has passed smoothed_query, with coarse_validate's kernels.  Writes scratch only.  Waits.
hipError_t smoothed_validate(hipStream_t stream, const CoarseTable &t, const SmoothedSizes &sz, void *scratch, int *refusal);
// P^T (a stable radix sort of the entries by column: linear in the entries, fine rows ascending) and dinv_j = 1 / d_j,
// d_j = sum_i P_ij (sum_k A_ik P_kj), of a validated table.  *column = 0, or j + 1 for the first column whose d_j is not a positive
// finite number (an empty column is one): dinv is then not written.  Waits.
hipError_t smoothed_setup(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const CoarseTable &t,
                          const SmoothedSizes &sz, void *pt, double *dinv, void *scratch, int32_t *column);
// -> u = D^-1 P^T r (ncoarse doubles in the scratch)
const double *smoothed_restrict(hipStream_t stream, const CoarseTable &t, const SmoothedSizes &sz, const void *pt, const double *dinv,
                                void *scratch, const double *r);
// z = (accumulate ? z : 0) + P u of smoothed_restrict, a row's terms added in entry order; part_rz (may be null): the partial sums
// of r . z per block of RB rows
void smoothed_apply(hipStream_t stream, const CoarseTable &t, const SmoothedSizes &sz, const void *pt, const double *dinv, void *scratch,
                    int accumulate, const double *r, double *z, double *part_rz);

// ---- the prolongations of several levels in one pass over z: z_i += sum over the tables in their order, a table's terms in entry
// order onto the running sum -- the bits of one accumulating apply after the other --, and the block partials of r . z
struct ProlongTables {
    int count;
    const int64_t *ptr[MULTILEVEL_MAX_TABLES];
    const int32_t *cols[MULTILEVEL_MAX_TABLES];
    const double *vals[MULTILEVEL_MAX_TABLES];
    const double *u[MULTILEVEL_MAX_TABLES];
};
void multilevel_prolong(hipStream_t stream, size_t n, const ProlongTables &tables, const double *r, double *z, double *part_rz);

}  // namespace pa
