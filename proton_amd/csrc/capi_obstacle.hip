// capi_obstacle.hip -- the C ABI of the obstacle problem: the active-set tables, obstacle_assembler's triplets and its system
// directly in CSR, the block solve, the active-set update, and the whole loop on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "context.hpp"
#include "device_tmp.hpp"
#include "hho_assembly.hpp"
#include "obstacle_csr.hpp"
#include "obstacle_solve.hpp"
#include "scan.hpp"

int pa_obstacle_tables(pa_context *ctx, const uint8_t *d_in_A, int32_t *d_A_ct, int32_t *d_B_ct, size_t *num_I,
                       size_t *num_A)
{
    if (!ctx || !d_in_A || !d_A_ct || !d_B_ct) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->mesh.ptids) return PA_ERR_NO_MESH;
    const uint32_t n = (uint32_t)ctx->mesh.ncells;
    const uint32_t nblocks = (n + pa::SCAN_TILE - 1) / pa::SCAN_TILE;
    uint32_t *d_counts = nullptr;
    PA_HIP(ctx, hipMalloc(&d_counts, (nblocks + 1) * sizeof(uint32_t)));
    hipLaunchKernelGGL(pa::active_count_kernel, dim3(nblocks), dim3(pa::SCAN_BLOCK), 0, ctx->stream, d_in_A, n, d_counts);
    hipLaunchKernelGGL(pa::active_block_scan_kernel, dim3(1), dim3(pa::SCAN_BLOCK), 0, ctx->stream, d_counts, nblocks);
    hipLaunchKernelGGL(pa::active_tables_kernel, dim3(nblocks), dim3(pa::SCAN_BLOCK), 0, ctx->stream, d_in_A, n, d_counts,
                       d_A_ct, d_B_ct);
    uint32_t total = 0;
    hipError_t e = hipMemcpyAsync(&total, d_counts + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_counts);
    PA_HIP(ctx, e);
    if (num_A) *num_A = total;
    if (num_I) *num_I = n - total;
    return PA_OK;
}

int pa_obstacle_triplets_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n, const double *d_lc,
                               const double *d_rhs, const double *d_g, const double *d_gamma, const uint8_t *d_in_A,
                               const int32_t *d_A_ct, const int32_t *d_B_ct, size_t num_I, int32_t *d_rows,
                               int32_t *d_cols, double *d_vals, int32_t *d_rhs_rows, double *d_rhs_vals)
{
    if (!ctx || !d_lc || !d_gamma || !d_in_A || !d_A_ct || !d_B_ct || !d_rows || !d_cols || !d_vals || !d_rhs_rows ||
        !d_rhs_vals)
        return PA_ERR_INVALID_ARG;
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (!whole_mesh(ctx)) { ctx->last_error = "obstacle assembler needs the whole mesh on the context"; return PA_ERR_INVALID_ARG; }
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first || num_I > ctx->mesh.ncells) return PA_ERR_INVALID_ARG;
    pa_assembler_info info;
    pa_assembler_query(ctx, di, &info);
    if (info.system_size >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;
    if (n == 0) return PA_OK;
    pa::ObstacleArgs o;
    pa::TripletArgs &a = o.t;
    a.cell_faces = ctx->faces.cell_faces.get(); a.face_dir = ctx->faces.face_dir.get(); a.face_compress = ctx->faces.face_compress.get();
    a.g = d_g; a.lc = d_lc; a.rhs = d_rhs; a.first = first; a.n = n;
    a.cell_base = 0; a.ncells_global = ctx->mesh.ncells_global;
    a.cbs = pa::P2(di.cell_deg); a.fbs = di.face_deg + 1;
    a.rows = d_rows; a.cols = d_cols; a.vals = d_vals; a.rhs_rows = d_rhs_rows; a.rhs_vals = d_rhs_vals;
    o.in_A = d_in_A; o.A_ct = d_A_ct; o.B_ct = d_B_ct; o.gamma = d_gamma; o.num_I = num_I; o.num_other = ctx->faces.num_other_faces;
    const int msize = a.cbs + 4 * a.fbs;
    const size_t shmem = msize * sizeof(double) + 2 * msize * sizeof(int32_t);
    const size_t resident = (size_t)ctx->num_cus * 8;
    const int grid = (int)(n < resident ? n : resident);
    hipLaunchKernelGGL(pa::obstacle_triplets_kernel, dim3(grid), dim3(256), shmem, ctx->stream, o);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_obstacle_expand_solution(pa_context *ctx, pa_degree_info di, const double *d_solution, const double *d_g,
                                const double *d_gamma, const uint8_t *d_in_A, const int32_t *d_A_ct,
                                const int32_t *d_B_ct, size_t num_I, double *d_alpha, double *d_beta)
{
    if (!ctx || !d_solution || !d_gamma || !d_in_A || !d_A_ct || !d_B_ct || !d_alpha || !d_beta) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (!whole_mesh(ctx)) { ctx->last_error = "obstacle assembler needs the whole mesh on the context"; return PA_ERR_INVALID_ARG; }
    pa::ExpandArgs a;
    a.in_A = d_in_A; a.face_dir = ctx->faces.face_dir.get(); a.A_ct = d_A_ct; a.B_ct = d_B_ct; a.face_compress = ctx->faces.face_compress.get();
    a.solution = d_solution; a.g = d_g; a.gamma = d_gamma;
    a.ncells = ctx->mesh.ncells; a.nfaces = ctx->faces.nfaces_local; a.num_I = num_I; a.num_other = ctx->faces.num_other_faces;
    a.cbs = pa::P2(di.cell_deg); a.fbs = di.face_deg + 1; a.alpha = d_alpha; a.beta = d_beta;
    const uint64_t total = a.ncells * a.cbs + a.nfaces * a.fbs;
    hipLaunchKernelGGL(pa::obstacle_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, a);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

// ---- obstacle_assembler's system (cell degree 0) directly in CSR: obstacle_csr.hip -----------------------------------
int pa_obstacle_csr_assemble(pa_context *ctx, pa_degree_info di, const double *d_lc, const double *d_rhs, const double *d_g,
                             const double *d_gamma, const uint8_t *d_in_A, const int32_t *d_A_ct, const int32_t *d_B_ct, size_t num_I,
                             int64_t *d_rowptr, int32_t *d_colind, double *d_values, double *d_RHS, size_t *nnz)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    // every refusal comes before the first launch that touches an output buffer
    if (!d_lc || !d_gamma || !d_in_A || !d_A_ct || !d_B_ct || !d_rowptr || !d_colind || !d_values || !nnz) {
        ctx->last_error = "pa_obstacle_csr_assemble: only d_rhs, d_g and d_RHS may be NULL";
        return PA_ERR_INVALID_ARG;
    }
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (di.cell_deg != 0) {
        ctx->last_error = "pa_obstacle_csr_assemble: the direct path covers cell degree 0 (cbs = 1, obstacle.cpp:51); the overlapping "
                          "cell rows of hho.hpp:631 for cbs > 1 stay with pa_obstacle_triplets_batch + pa_csr_from_triplets";
        return PA_ERR_INVALID_DEGREE;
    }
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (!whole_mesh(ctx)) { ctx->last_error = "obstacle assembler needs the whole mesh on the context"; return PA_ERR_INVALID_ARG; }
    const int fbs = di.face_deg + 1;
    if (num_I > ctx->mesh.ncells || ctx->mesh.ncells + (uint64_t)fbs * ctx->faces.num_other_faces >= ((uint64_t)1 << 31)) {      // int32 column ids
        ctx->last_error = "pa_obstacle_csr_assemble: num_I beyond the cells of the mesh, or 2^31 rows and more";
        return PA_ERR_INVALID_ARG;
    }
    const int st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    pa::ObstacleCsrArgs a;
    a.v = face_system_view(ctx);
    const pa::AsmSizes plain = pa::asm_sizes(a.v, 1, fbs);
    a.cell_nnz = plain.cell_nnz;
    a.in_A = d_in_A; a.A_ct = d_A_ct; a.B_ct = d_B_ct; a.num_I = num_I; a.num_other = ctx->faces.num_other_faces;
    a.lc = d_lc; a.rhs = d_rhs; a.g = d_g; a.gamma = d_gamma;
    a.rowptr = d_rowptr; a.colind = d_colind; a.values = d_values; a.RHS = d_RHS;
    uint32_t removed = 0;
    PA_HIP(ctx, pa::obstacle_csr_assemble(ctx->stream, fbs, a, &removed));
    *nnz = (size_t)(plain.nnz - (uint64_t)fbs * removed);
    return PA_OK;
}

// ---- the solve of that system and the active-set loop around it: obstacle_solve.hip -----------------------------------------
// the refusals the three entry points share with pa_obstacle_csr_assemble; PA_OK = go on
static int obstacle_solve_refusals(pa_context *ctx, pa_degree_info di, const char *who)
{
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (di.cell_deg != 0) {
        ctx->last_error = std::string(who) + ": cell degree 0 only (cbs = 1, obstacle.cpp:51), as pa_obstacle_csr_assemble";
        return PA_ERR_INVALID_DEGREE;
    }
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (!whole_mesh(ctx)) { ctx->last_error = "obstacle assembler needs the whole mesh on the context"; return PA_ERR_INVALID_ARG; }
    if (ctx->mesh.ncells + (uint64_t)(di.face_deg + 1) * ctx->faces.num_other_faces >= ((uint64_t)1 << 31)) {
        ctx->last_error = std::string(who) + ": 2^31 rows and more";
        return PA_ERR_INVALID_ARG;
    }
    return PA_OK;
}

static pa::ObstacleBlockArgs obstacle_block_args(const pa_context *ctx, pa_degree_info di, const int64_t *d_rowptr, const int32_t *d_colind,
                                                 const double *d_values, const double *d_RHS, const uint8_t *d_in_A, const int32_t *d_A_ct,
                                                 const int32_t *d_B_ct, size_t num_I, double *d_x)
{
    pa::ObstacleBlockArgs a;
    a.ncells = (uint32_t)ctx->mesh.ncells; a.nrows = ctx->mesh.ncells + (uint64_t)(di.face_deg + 1) * ctx->faces.num_other_faces; a.num_I = num_I;
    a.rowptr = d_rowptr; a.colind = d_colind; a.values = d_values; a.RHS = d_RHS;
    a.in_A = d_in_A; a.A_ct = d_A_ct; a.B_ct = d_B_ct; a.x = d_x;
    return a;
}

int pa_obstacle_block_solve(pa_context *ctx, pa_degree_info di, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                            const double *d_RHS, const uint8_t *d_in_A, const int32_t *d_A_ct, const int32_t *d_B_ct, size_t num_I,
                            double convergence_threshold, double divergence_threshold, size_t max_iter, int apply_preconditioner,
                            double *d_x, int32_t *exit_reason, size_t *iterations, double *relative_residual)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    if (!d_rowptr || !d_colind || !d_values || !d_RHS || !d_in_A || !d_A_ct || !d_B_ct || !d_x) {
        ctx->last_error = "pa_obstacle_block_solve: only exit_reason, iterations and relative_residual may be NULL";
        return PA_ERR_INVALID_ARG;
    }
    (void)hipSetDevice(ctx->device);
    const int st = obstacle_solve_refusals(ctx, di, "pa_obstacle_block_solve");
    if (st != PA_OK) return st;
    if (num_I > ctx->mesh.ncells) { ctx->last_error = "pa_obstacle_block_solve: num_I beyond the cells of the mesh"; return PA_ERR_INVALID_ARG; }
    int reason = 0;
    PA_HIP(ctx, pa::obstacle_block_solve(ctx->stream, obstacle_block_args(ctx, di, d_rowptr, d_colind, d_values, d_RHS, d_in_A, d_A_ct, d_B_ct,
                                                                          num_I, d_x),
                                         nullptr, convergence_threshold, divergence_threshold, max_iter, apply_preconditioner, &reason,
                                         iterations, relative_residual));
    if (exit_reason) *exit_reason = reason;
    return PA_OK;
}

static pa::ObstacleUpdateArgs obstacle_update_args(const pa_context *ctx, pa_degree_info di, double c, const double *d_alpha,
                                                   const double *d_beta, const double *d_gamma, const double *d_alpha_prev,
                                                   const uint8_t *d_in_A_prev, uint8_t *d_in_A)
{
    pa::ObstacleUpdateArgs a;
    a.ncells = (uint32_t)ctx->mesh.ncells; a.nalpha = ctx->mesh.ncells + (uint64_t)(di.face_deg + 1) * ctx->faces.nfaces_local; a.c = c;
    a.alpha = d_alpha; a.beta = d_beta; a.gamma = d_gamma; a.alpha_prev = d_alpha_prev; a.in_A_prev = d_in_A_prev; a.in_A = d_in_A;
    return a;
}

int pa_obstacle_active_set_update(pa_context *ctx, pa_degree_info di, double c, const double *d_alpha, const double *d_beta,
                                  const double *d_gamma, const double *d_alpha_prev, const uint8_t *d_in_A_prev, uint8_t *d_in_A,
                                  size_t *num_A, size_t *changed, double *step_norm)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    if (!d_alpha || !d_beta || !d_gamma || !d_in_A) {
        ctx->last_error = "pa_obstacle_active_set_update: d_alpha, d_beta, d_gamma and d_in_A are required";
        return PA_ERR_INVALID_ARG;
    }
    (void)hipSetDevice(ctx->device);
    const int st = obstacle_solve_refusals(ctx, di, "pa_obstacle_active_set_update");
    if (st != PA_OK) return st;
    pa::ObstacleUpdateResult r{0.0, 0, 0};
    PA_HIP(ctx, pa::obstacle_active_set_update(ctx->stream, obstacle_update_args(ctx, di, c, d_alpha, d_beta, d_gamma, d_alpha_prev,
                                                                                d_in_A_prev, d_in_A), nullptr, &r));
    if (num_A) *num_A = (size_t)r.num_A;
    if (changed) *changed = (size_t)r.changed;
    if (step_norm) *step_norm = sqrt(r.step2);
    return PA_OK;
}

namespace {
// The workspace of pa_obstacle_solve's loop.  Declared after the loop's DeviceTmp, so that on every path out of the function,
// the refusals of an iteration included, the stream has drained before anything the loop's kernels may be using is freed.
struct ObstacleLoopScope {
    hipStream_t stream;
    pa::ObstacleSolveWorkspace ws;
    ~ObstacleLoopScope()
    {
        (void)hipStreamSynchronize(stream);
        pa::obstacle_workspace_release(&ws);
    }
};
}  // namespace

int pa_obstacle_solve(pa_context *ctx, pa_degree_info di, const double *d_lc, const double *d_rhs, const double *d_g, const double *d_gamma,
                      const pa_obstacle_solve_params *params, double *d_alpha, double *d_beta, uint8_t *d_in_A, pa_obstacle_solve_info *info,
                      size_t *num_A_history, size_t *cg_iterations_history)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    // every refusal comes before the first launch that touches an output buffer
    if (!d_lc || !d_gamma || !params || !d_alpha || !d_beta || !d_in_A || !info) {
        ctx->last_error = "pa_obstacle_solve: only d_rhs, d_g and the two history arrays may be NULL";
        return PA_ERR_INVALID_ARG;
    }
    if (params->max_outer == 0) { ctx->last_error = "pa_obstacle_solve: max_outer = 0 solves nothing"; return PA_ERR_INVALID_ARG; }
    (void)hipSetDevice(ctx->device);
    int st = obstacle_solve_refusals(ctx, di, "pa_obstacle_solve");
    if (st != PA_OK) return st;
    pa_assembler_csr_info csr;
    st = pa_assembler_csr_query(ctx, di, &csr);
    if (st != PA_OK) return st;
    const size_t nc = ctx->mesh.ncells, fbs = (size_t)di.face_deg + 1, nrows = (size_t)csr.nrows, nalpha = nc + fbs * ctx->faces.nfaces_local;

    pa::DeviceTmp tmp(ctx->stream);
    ObstacleLoopScope buf{ctx->stream, {}};
    int64_t *rowptr = nullptr;
    int32_t *colind = nullptr, *A_ct = nullptr, *B_ct = nullptr;
    double *values = nullptr, *RHS = nullptr, *x = nullptr, *alpha[2] = {nullptr, nullptr}, *beta[2] = {nullptr, nullptr};
    uint8_t *flags[2] = {nullptr, nullptr};
    bool held = tmp.alloc(&rowptr, nrows + 1) && tmp.alloc(&colind, (size_t)csr.nnz) && tmp.alloc(&values, (size_t)csr.nnz) &&
                tmp.alloc(&RHS, nrows) && tmp.alloc(&x, nrows) && tmp.alloc(&A_ct, nc) && tmp.alloc(&B_ct, nc);
    for (int i = 0; i < 2; ++i) held = held && tmp.alloc(&alpha[i], nalpha) && tmp.alloc(&beta[i], nc) && tmp.alloc(&flags[i], nc);
    PA_HIP(ctx, tmp.error());
    PA_HIP(ctx, pa::obstacle_workspace_reserve(&buf.ws, nrows, nalpha));

    // alpha = 0, beta = 1 (obstacle.cpp:98-99) and the first active set (:133-142)
    PA_HIP(ctx, hipMemsetAsync(alpha[0], 0, nalpha * sizeof(double), ctx->stream));
    PA_HIP(ctx, pa::obstacle_fill(ctx->stream, beta[0], nc, 1.0));
    pa::ObstacleUpdateResult upd{0.0, 0, 0};
    PA_HIP(ctx, pa::obstacle_active_set_update(ctx->stream, obstacle_update_args(ctx, di, params->c, alpha[0], beta[0], d_gamma, nullptr,
                                                                                nullptr, flags[0]), &buf.ws, &upd));
    pa_obstacle_solve_info out{0, 0, 0.0, 0, 0};
    int cur = 0, fl = 0;                                   // alpha[cur] / beta[cur]: the last completed iteration; flags[fl]: its system's
    while (out.outer_iterations < params->max_outer) {
        size_t num_I = 0, num_A = 0, nnz = 0;
        st = pa_obstacle_tables(ctx, flags[fl], A_ct, B_ct, &num_I, &num_A);
        if (st != PA_OK) return st;
        st = pa_obstacle_csr_assemble(ctx, di, d_lc, d_rhs, d_g, d_gamma, flags[fl], A_ct, B_ct, num_I, rowptr, colind, values, RHS, &nnz);
        if (st != PA_OK) return st;
        const size_t nk = nrows - num_A;
        int reason = 0;
        size_t iters = 0;
        PA_HIP(ctx, pa::obstacle_block_solve(ctx->stream, obstacle_block_args(ctx, di, rowptr, colind, values, RHS, flags[fl], A_ct, B_ct, num_I, x),
                                             &buf.ws, params->cg_convergence_threshold, params->cg_divergence_threshold,
                                             params->cg_max_iter ? params->cg_max_iter : 20 * nk, params->apply_preconditioner, &reason,
                                             &iters, nullptr));
        if (num_A_history) num_A_history[out.outer_iterations] = num_A;
        if (cg_iterations_history) cg_iterations_history[out.outer_iterations] = iters;
        out.outer_iterations++;
        out.cg_iterations += iters;
        out.cg_exit_reason = reason;
        if (reason != 0) break;                            // alpha[cur] / beta[cur] stay those of the last completed iteration
        st = pa_obstacle_expand_solution(ctx, di, x, d_g, d_gamma, flags[fl], A_ct, B_ct, num_I, alpha[1 - cur], beta[1 - cur]);
        if (st != PA_OK) return st;
        // the step of this iteration (:193) and the active set of the next (:133-142) in one pass
        PA_HIP(ctx, pa::obstacle_active_set_update(ctx->stream, obstacle_update_args(ctx, di, params->c, alpha[1 - cur], beta[1 - cur], d_gamma,
                                                                                    alpha[cur], flags[fl], flags[1 - fl]), &buf.ws, &upd));
        cur = 1 - cur;
        out.last_step_norm = sqrt(upd.step2);
        if (out.last_step_norm < params->outer_tol) { out.converged = 1; break; }
        if (out.outer_iterations < params->max_outer) fl = 1 - fl;      // (after the last system its own flags are the result)
    }
    PA_HIP(ctx, hipMemcpyAsync(d_alpha, alpha[cur], nalpha * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    PA_HIP(ctx, hipMemcpyAsync(d_beta, beta[cur], nc * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    PA_HIP(ctx, hipMemcpyAsync(d_in_A, flags[fl], nc * sizeof(uint8_t), hipMemcpyDeviceToDevice, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *info = out;
    return PA_OK;
}
