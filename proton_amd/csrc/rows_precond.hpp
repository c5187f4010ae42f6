// rows_precond.hpp -- host entry points of rows_precond.hip: the conjugate gradient of solver_cg.hpp:63-144 with the patches of
// patch_precond.hpp and the Galerkin coarse level of coarse_precond.hpp, on one rank and on a row-partitioned system with both
// partitioned by rows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cg.hpp"
#include "coarse_precond.hpp"

namespace pa {

// ---- one rank: z = (patch sum), and z = (patch sum) + (coarse term) ----
// status: 0 solved (see exit_reason), 1 table refused (*refusal), 2 a patch is not positive definite; x is written only with 0
hipError_t conjugated_gradient_patch(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                                     const double *b, double *x, size_t npatches, const int64_t *patch_ptr, const int32_t *patch_rows,
                                     double convergence_threshold, double divergence_threshold, size_t max_iter, int *exit_reason,
                                     size_t *iterations, double *relative_residual, int *status, int *refusal);
// status: 0 solved (see exit_reason), 1 patch table refused, 2 a patch is not positive definite, 3 coarse table refused
// (*refusal: its code), 4 the coarse matrix is not positive definite (*pivot); x is written only with 0.  A refused table of either
// level is reported before a patch that is not positive definite.
hipError_t conjugated_gradient_patch_coarse(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind,
                                            const double *values, const double *b, double *x, size_t npatches, const int64_t *patch_ptr,
                                            const int32_t *patch_rows, size_t ncoarse, const int64_t *p_ptr, const int32_t *p_cols,
                                            const double *p_vals, double convergence_threshold, double divergence_threshold,
                                            size_t max_iter, int *exit_reason, size_t *iterations, double *relative_residual, int *status,
                                            int *refusal, int32_t *pivot);

// ---- one rank: z = (patch sum) + the smoothed levels in their order (multilevel_precond.hpp) + (coarse term of `exact`, may be null) ----
// status: those of conjugated_gradient_patch_coarse, and 5: the table of smoothed level `level` was refused (*refusal), 6: column
// pivot - 1 of smoothed level `level` has no positive finite d_j.  The order: the patch table, every level's table, the exact
// table; then a patch, a level, the exact level that is not positive definite.  x is written only with status 0.  nlevels = 0: the
// call is conjugated_gradient_patch_coarse (exact = null: conjugated_gradient_patch) itself.
struct MultilevelReport {
    int status = 0, refusal = 0, level = -1;
    int32_t pivot = 0;
};
hipError_t conjugated_gradient_multilevel(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                                          const double *b, double *x, size_t npatches, const int64_t *patch_ptr, const int32_t *patch_rows,
                                          int nlevels, const CoarseTable *levels, const CoarseTable *exact, double convergence_threshold,
                                          double divergence_threshold, size_t max_iter, int *exit_reason, size_t *iterations,
                                          double *relative_residual, MultilevelReport *report);

// ---- a row-partitioned system ----
// what this rank's status 5 or 6 was about: level 1 the patches, 2 the coarse level; refusal: the code of patch_refusal_text /
// coarse_refusal_text (status 5); pivot: j + 1 for the first non-positive pivot j of the coarse matrix (status 6, level 2)
struct RowsPrecondReport {
    int level = 0, refusal = 0;
    int32_t pivot = 0;
};

// conjugated_gradient_rows (cg.hpp: its arguments, results and statuses) with z = (patch sum) + (coarse term).  The patch table
// holds GLOBAL row indices within [row_begin, row_end); p_ptr / p_cols / p_vals are the rank's own rows of P (p_ptr from 0,
// global coarse columns), ncoarse the same on every rank, 0 = patches only.  Statuses beyond conjugated_gradient_rows': 5 a table
// of this rank was refused, 6 a patch of this rank or the coarse matrix is not positive definite (*report says which); x is
// written only with status 0.  Without a transport, from row 0 and with whole tables the call is conjugated_gradient_patch_coarse
// (ncoarse = 0: conjugated_gradient_patch) bit for bit.
hipError_t conjugated_gradient_rows_patch_coarse(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end,
                                                 const int64_t *rowptr, const int32_t *colind, const double *values, const double *b,
                                                 double *x, size_t npatches, const int64_t *patch_ptr, const int32_t *patch_rows,
                                                 size_t ncoarse, const int64_t *p_ptr, const int32_t *p_cols, const double *p_vals,
                                                 double convergence_threshold, double divergence_threshold, size_t max_iter,
                                                 int *exit_reason, size_t *iterations, double *relative_residual, int *transport_status,
                                                 RowsPrecondReport *report);

}  // namespace pa
