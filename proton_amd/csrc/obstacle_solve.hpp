// obstacle_solve.hpp -- host entry points of obstacle_solve.hip: the solve of obstacle_assembler's system (the SparseLU of
// obstacle.cpp:170-175) on the device, in place on the CSR arrays of obstacle_csr.hpp, and the active-set update of
// obstacle.cpp:133-142 with the stopping norm of :193.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cg.hpp"

namespace pa {

// what the update leaves on the device and the host reads back: three scalars
struct ObstacleUpdateResult {
    double step2;                      // sum of (alpha_prev - alpha)^2 over the whole vector
    uint64_t num_A, changed;
};

// Device memory of the two entry points for systems of up to `rows` rows and updates of up to `blocks` blocks: the vectors of
// the conjugate gradient, the row map, the right-hand side of the SPD block, the partial sums of the update.
struct ObstacleSolveWorkspace {
    CgWorkspace cg;
    size_t rows = 0, blocks = 0;
    int32_t *rowmap = nullptr;
    double *bk = nullptr, *part_step = nullptr;
    uint32_t *part_count = nullptr;    // 2 per block: active cells, changed flags
    ObstacleUpdateResult *result = nullptr;
};
// leaves the workspace empty when it fails
hipError_t obstacle_workspace_reserve(ObstacleSolveWorkspace *ws, size_t rows, size_t update_elements);
void obstacle_workspace_release(ObstacleSolveWorkspace *ws);

struct ObstacleBlockArgs {
    uint32_t ncells;
    uint64_t nrows, num_I;             // nrows = ncells + fbs (non-Dirichlet faces); nk = nrows - (ncells - num_I)
    const int64_t *rowptr;
    const int32_t *colind;
    const double *values, *RHS;
    const uint8_t *in_A;
    const int32_t *A_ct, *B_ct;
    double *x;                         // nrows: the SPD block's solution at [0, nk), the multipliers behind it
};

// x = A^-1 RHS.  The kept rows (inactive cells in A_ct order, then the face rows) against the columns below nk are solved by
// conjugated_gradient_one_rank through a row map, in place; every active cell's row then gives its multiplier.  ws: NULL = a
// workspace of this call's own.  Returns after the stream has drained.
hipError_t obstacle_block_solve(hipStream_t stream, const ObstacleBlockArgs &args, ObstacleSolveWorkspace *ws,
                                double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                                int *exit_reason, size_t *iterations, double *relative_residual);

struct ObstacleUpdateArgs {
    uint32_t ncells;
    uint64_t nalpha;                   // ncells + fbs nfaces
    double c;
    const double *alpha, *beta, *gamma;
    const double *alpha_prev;          // may be null: zeros
    const uint8_t *in_A_prev;          // may be null: no cell active; may equal in_A
    uint8_t *in_A;
};

// in_A[i] = beta[i] + c (alpha[i] - gamma[i]) < 0 with every operation rounded on its own, the counts and the squared step.
// Returns after the stream has drained.
hipError_t obstacle_active_set_update(hipStream_t stream, const ObstacleUpdateArgs &args, ObstacleSolveWorkspace *ws,
                                      ObstacleUpdateResult *out);

// p[i] = v, i < n (beta = 1 at the start of the loop, obstacle.cpp:99)
hipError_t obstacle_fill(hipStream_t stream, double *p, size_t n, double v);

}  // namespace pa
