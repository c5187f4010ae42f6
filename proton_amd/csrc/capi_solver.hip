// capi_solver.hip -- the C ABI of the device solvers: the conjugate gradient on one rank and on row slabs, the patch
// preconditioner and the Galerkin coarse level with the solvers that use them (rows_precond.hip), and the tables of both levels
// for the face-only system of an uncut mesh, whole (pa_condensed_patches, pa_condensed_coarse) or by slab (pa_condensed_rows_*).
// What every entry point of a kind repeats is stated once in front: the transport handed on, the status of a row-partitioned
// solve mapped to the return code, the messages of a refused table and of a matrix that is not positive definite.
#include <hip/hip_runtime.h>

#include <string>

#include "cg.hpp"
#include "coarse_precond.hpp"
#include "context.hpp"
#include "device_tmp.hpp"
#include "multilevel_precond.hpp"
#include "patch_precond.hpp"
#include "rows_precond.hpp"
#include "scan.hpp"

// ---- stated once ------------------------------------------------------------------------------------------------------------------
static int patch_refused(pa_context *ctx, const char *who, int refusal)
{
    ctx->last_error = std::string(who) + ": " + pa::patch_refusal_text(refusal);
    return PA_ERR_INVALID_ARG;
}

static int coarse_refused(pa_context *ctx, const char *who, int refusal)
{
    ctx->last_error = std::string(who) + ": " + pa::coarse_refusal_text(refusal);
    return PA_ERR_INVALID_ARG;
}

// `what`: which matrix, and where to look
static int patch_not_spd(pa_context *ctx, const char *who, const char *what)
{
    ctx->last_error = std::string(who) + ": a patch matrix " + what;
    return PA_ERR_NOT_SPD;
}

static int coarse_not_spd(pa_context *ctx, const char *who, int32_t pivot)
{
    ctx->last_error = std::string(who) + ": the coarse matrix is not positive definite (pivot " + std::to_string(pivot - 1) + ")";
    return PA_ERR_NOT_SPD;
}

// level < 0: the one level of the call
static int level_not_spd(pa_context *ctx, const char *who, int level, int32_t column)
{
    ctx->last_error = std::string(who) + ": the diagonal of P^T A P is not positive (column " + std::to_string(column - 1) +
                      (level >= 0 ? ", smoothed level " + std::to_string(level) + ")" : std::string(")"));
    return PA_ERR_NOT_SPD;
}

// the caller's transport as the solvers take it; false: a callback is missing
static bool transport_in(const pa_cg_transport *transport, pa::CgTransport *tp)
{
    *tp = pa::CgTransport{};
    if (!transport) return true;
    if (!transport->allreduce_sum || !transport->halo || !transport->neighbour_counts) return false;
    tp->user = transport->user; tp->allreduce_sum = transport->allreduce_sum; tp->halo = transport->halo;
    tp->neighbour_counts = transport->neighbour_counts;
    return true;
}

// what a row-partitioned solve returns for the statuses conjugated_gradient_rows knows (cg.hpp), after its outputs have been handed on
static int rows_solve_result(pa_context *ctx, const char *who, hipError_t he, int reason, int tstat, int32_t *exit_reason,
                             int32_t *transport_status)
{
    if (exit_reason) *exit_reason = reason;
    if (transport_status) *transport_status = tstat;
    if (he != hipSuccess) { ctx->last_error = std::string(who) + ": " + hipGetErrorString(he); return PA_ERR_HIP; }
    if (tstat == 3) ctx->last_error = std::string(who) + ": another rank failed; every rank left the solve at the same reduction";
    return (tstat == 1 || tstat == 3) ? PA_ERR_COMM : (tstat == 2 ? PA_ERR_INVALID_ARG : PA_OK);
}

// ---- the conjugate gradient: solver.hip ------------------------------------------------------------------------------------------
int pa_conjugated_gradient(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                           const double *d_b, double *d_x, double convergence_threshold, double divergence_threshold,
                           size_t max_iter, int apply_preconditioner, int32_t *exit_reason, size_t *iterations,
                           double *relative_residual)
{
    if (!ctx || !d_rowptr || (nrows && (!d_colind || !d_values || !d_b || !d_x))) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    int reason = 0;
    PA_HIP(ctx, pa::conjugated_gradient(ctx->stream, nrows, d_rowptr, d_colind, d_values, d_b, d_x, convergence_threshold,
                                        divergence_threshold, max_iter, apply_preconditioner, &reason, iterations, relative_residual));
    if (exit_reason) *exit_reason = reason;
    return PA_OK;
}

int pa_conjugated_gradient_rows(pa_context *ctx, const pa_cg_transport *transport, int64_t row_begin, int64_t row_end,
                                const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values, const double *d_b, double *d_x,
                                double convergence_threshold, double divergence_threshold, size_t max_iter, int apply_preconditioner,
                                int32_t *exit_reason, size_t *iterations, double *relative_residual, int32_t *transport_status)
{
    if (!ctx || !d_rowptr || row_end < row_begin) return PA_ERR_INVALID_ARG;
    if (row_end > row_begin && (!d_colind || !d_values || !d_b || !d_x)) return PA_ERR_INVALID_ARG;
    pa::CgTransport tp;
    if (!transport_in(transport, &tp)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    int reason = 0, tstat = 0;
    const hipError_t he = pa::conjugated_gradient_rows(ctx->stream, transport ? &tp : nullptr, row_begin, row_end, d_rowptr, d_colind, d_values,
                                                       d_b, d_x, convergence_threshold, divergence_threshold, max_iter, apply_preconditioner,
                                                       &reason, iterations, relative_residual, &tstat);
    return rows_solve_result(ctx, "pa_conjugated_gradient_rows", he, reason, tstat, exit_reason, transport_status);
}

// ---- the patch preconditioner (patch_precond.hip), the conjugate gradient with it (rows_precond.hip) and its whole-mesh tables ----
static void patch_info_out(const pa::PatchSizes &sz, pa_patch_precond_info *out)
{
    out->entries = sz.entries; out->max_patch_rows = sz.max_rows; out->lanes_per_patch = sz.lanes;
    out->factor_doubles = sz.factor_doubles; out->slot_ints = sz.slot_ints; out->scratch_bytes = sz.scratch_bytes;
}

int pa_patch_precond_query(pa_context *ctx, size_t nrows, size_t npatches, const int64_t *d_patch_ptr, pa_patch_precond_info *out)
{
    if (!ctx || !d_patch_ptr || !out) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::PatchSizes sz;
    int refusal = 0;
    PA_HIP(ctx, pa::patch_query(ctx->stream, nrows, npatches, d_patch_ptr, &sz, &refusal));
    if (refusal) return patch_refused(ctx, "pa_patch_precond_query", refusal);
    patch_info_out(sz, out);
    return PA_OK;
}

int pa_patch_precond_factor(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                            size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows, double *d_factors,
                            int32_t *d_slots, void *d_scratch, int32_t *d_info, size_t *failed_patches)
{
    if (!ctx || !d_rowptr || !d_patch_ptr || !d_slots || !d_scratch) return PA_ERR_INVALID_ARG;
    if (npatches && (!d_colind || !d_values || !d_patch_rows || !d_factors || !d_info)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::PatchSizes sz;
    int refusal = 0;
    PA_HIP(ctx, pa::patch_query(ctx->stream, nrows, npatches, d_patch_ptr, &sz, &refusal));
    if (refusal) return patch_refused(ctx, "pa_patch_precond_factor", refusal);
    size_t failed = 0;
    const pa::PatchTable t{nrows, npatches, d_patch_ptr, d_patch_rows};
    PA_HIP(ctx, pa::patch_factor(ctx->stream, d_rowptr, d_colind, d_values, t, sz, d_factors, d_slots, d_scratch, d_info, &refusal, &failed));
    if (refusal) return patch_refused(ctx, "pa_patch_precond_factor", refusal);
    if (failed_patches) *failed_patches = failed;
    return failed ? PA_ERR_NOT_SPD : PA_OK;
}

int pa_patch_precond_apply(pa_context *ctx, size_t nrows, size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                           const double *d_factors, const int32_t *d_slots, void *d_scratch, const double *d_r, double *d_z)
{
    if (!ctx || !d_patch_ptr || !d_slots || !d_scratch) return PA_ERR_INVALID_ARG;
    if (nrows && (!d_patch_rows || !d_factors || !d_r || !d_z)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::PatchSizes sz;
    int refusal = 0;
    PA_HIP(ctx, pa::patch_query(ctx->stream, nrows, npatches, d_patch_ptr, &sz, &refusal));
    if (refusal) return patch_refused(ctx, "pa_patch_precond_apply", refusal);
    const pa::PatchTable t{nrows, npatches, d_patch_ptr, d_patch_rows};
    pa::patch_apply(ctx->stream, t, sz, d_factors, d_slots, d_scratch, d_r, d_z, nullptr);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_conjugated_gradient_patch(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                                 const double *d_b, double *d_x, size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                                 double convergence_threshold, double divergence_threshold, size_t max_iter, int32_t *exit_reason,
                                 size_t *iterations, double *relative_residual)
{
    if (!ctx || !d_rowptr || (nrows && (!d_colind || !d_values || !d_b || !d_x || !d_patch_ptr || !d_patch_rows))) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    int reason = 0, status = 0, refusal = 0;
    PA_HIP(ctx, pa::conjugated_gradient_patch(ctx->stream, nrows, d_rowptr, d_colind, d_values, d_b, d_x, npatches, d_patch_ptr, d_patch_rows,
                                              convergence_threshold, divergence_threshold, max_iter, &reason, iterations, relative_residual,
                                              &status, &refusal));
    if (status == 1) return patch_refused(ctx, "pa_conjugated_gradient_patch", refusal);
    if (status == 2) return patch_not_spd(ctx, "pa_conjugated_gradient_patch", "is not positive definite (pa_patch_precond_factor says which)");
    if (exit_reason) *exit_reason = reason;
    return PA_OK;
}

// the cells with a non-Dirichlet face: their count and (index given) per cell its rank among them, -1 none
static int cell_patch_index(pa_context *ctx, pa::DeviceTmp &tmp, uint32_t *count, int32_t **index)
{
    const uint32_t nc = (uint32_t)ctx->mesh.ncells;
    uint8_t *flags = nullptr;
    uint32_t *counts = nullptr;
    int32_t *unused = nullptr, *idx = nullptr;
    if (!tmp.alloc(&flags, nc) || !tmp.alloc(&counts, (size_t)pa::scan_tiles(nc) + 1) || !tmp.alloc(&unused, nc) || !tmp.alloc(&idx, nc))
        PA_HIP(ctx, tmp.error());
    pa::cell_patch_flags(ctx->stream, nc, ctx->asmb.cprefix.get(), flags);
    *count = 0;
    if (nc && !tmp.ok(pa::scan_flags(ctx->stream, flags, nc, counts, unused, idx, count))) PA_HIP(ctx, tmp.error());
    if (index) *index = idx;
    return PA_OK;
}

int pa_condensed_patches_query(pa_context *ctx, pa_degree_info di, int kind, size_t *npatches, size_t *entries)
{
    if (!ctx || !npatches || !entries || !degree_ok(di) || (kind != PA_PATCH_FACE && kind != PA_PATCH_CELL)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const int st = asm_prepare(ctx);                     // whole-mesh contexts only, as pa_assembler_csr_fill
    if (st != PA_OK) return st;
    const pa::FaceSystemView v = face_system_view(ctx);
    const size_t fbs = (size_t)di.face_deg + 1;
    if (kind == PA_PATCH_FACE) { *npatches = v.nown; *entries = fbs * v.nown; return PA_OK; }
    pa::DeviceTmp tmp(ctx->stream);
    uint32_t count = 0;
    const int sc = cell_patch_index(ctx, tmp, &count, nullptr);
    if (sc != PA_OK) return sc;
    *npatches = count;
    *entries = fbs * v.cell_faces_total;                 // cprefix[ncells] of face_system.hpp
    return PA_OK;
}

int pa_condensed_patches(pa_context *ctx, pa_degree_info di, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows)
{
    if (!ctx || !d_patch_ptr || !degree_ok(di) || (kind != PA_PATCH_FACE && kind != PA_PATCH_CELL)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const int st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    const pa::FaceSystemView v = face_system_view(ctx);
    const int fbs = di.face_deg + 1;
    if ((uint64_t)fbs * v.cell_faces_total >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // int32 slots
    if (v.nown && !d_patch_rows) return PA_ERR_INVALID_ARG;
    if (kind == PA_PATCH_FACE) {
        pa::face_patches(ctx->stream, v.nown, fbs, 0, d_patch_ptr, d_patch_rows);
        PA_HIP(ctx, hipGetLastError());
        return PA_OK;
    }
    pa::DeviceTmp tmp(ctx->stream);
    uint32_t count = 0;
    int32_t *index = nullptr;
    const int sc = cell_patch_index(ctx, tmp, &count, &index);
    if (sc != PA_OK) return sc;
    pa::cell_patches(ctx->stream, v.ncells, count, v.cell_faces, v.face_compress, v.cprefix, index, fbs, d_patch_ptr, d_patch_rows);
    PA_HIP(ctx, hipGetLastError());
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the index lives until the kernel has read it
    return PA_OK;
}

// ---- the Galerkin coarse level (coarse_precond.hip) and the conjugate gradient with both levels (rows_precond.hip) -----------------
int pa_coarse_precond_query(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, pa_coarse_precond_info *out)
{
    if (!ctx || !d_p_ptr || !out) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::CoarseSizes sz;
    int refusal = 0;
    PA_HIP(ctx, pa::coarse_query(ctx->stream, nrows, ncoarse, d_p_ptr, &sz, &refusal));
    if (refusal) return coarse_refused(ctx, "pa_coarse_precond_query", refusal);
    out->entries = sz.entries; out->pt_bytes = sz.pt_bytes; out->factor_doubles = sz.factor_doubles; out->scratch_bytes = sz.scratch_bytes;
    return PA_OK;
}

int pa_coarse_precond_factor(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                             size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals, void *d_pt,
                             double *d_factor, void *d_scratch, double *d_coarse_matrix, int32_t *pivot)
{
    if (!ctx || !d_rowptr || !d_p_ptr || !d_pt || !d_factor || !d_scratch) return PA_ERR_INVALID_ARG;
    if (nrows && (!d_colind || !d_values || !d_p_cols || !d_p_vals)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::CoarseSizes sz;
    int refusal = 0;
    PA_HIP(ctx, pa::coarse_query(ctx->stream, nrows, ncoarse, d_p_ptr, &sz, &refusal));
    if (refusal) return coarse_refused(ctx, "pa_coarse_precond_factor", refusal);
    const pa::CoarseTable t{nrows, ncoarse, d_p_ptr, d_p_cols, d_p_vals};
    PA_HIP(ctx, pa::coarse_validate(ctx->stream, t, sz, d_scratch, &refusal));
    if (refusal) return coarse_refused(ctx, "pa_coarse_precond_factor", refusal);
    int32_t piv = 0;
    PA_HIP(ctx, pa::coarse_factor(ctx->stream, d_rowptr, d_colind, d_values, t, sz, d_pt, d_factor, d_scratch, d_coarse_matrix, &piv, &refusal));
    if (refusal) return coarse_refused(ctx, "pa_coarse_precond_factor", refusal);
    if (pivot) *pivot = piv;
    return piv ? coarse_not_spd(ctx, "pa_coarse_precond_factor", piv) : PA_OK;
}

int pa_coarse_precond_apply(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols,
                            const double *d_p_vals, const void *d_pt, const double *d_factor, void *d_scratch, int accumulate,
                            const double *d_r, double *d_z)
{
    if (!ctx || !d_p_ptr || !d_pt || !d_factor || !d_scratch) return PA_ERR_INVALID_ARG;
    if (nrows && (!d_p_cols || !d_p_vals || !d_r || !d_z)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::CoarseSizes sz;
    int refusal = 0;
    PA_HIP(ctx, pa::coarse_query(ctx->stream, nrows, ncoarse, d_p_ptr, &sz, &refusal));
    if (refusal) return coarse_refused(ctx, "pa_coarse_precond_apply", refusal);
    const pa::CoarseTable t{nrows, ncoarse, d_p_ptr, d_p_cols, d_p_vals};
    pa::coarse_apply(ctx->stream, t, sz, d_pt, d_factor, d_scratch, accumulate, d_r, d_z, nullptr);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_conjugated_gradient_patch_coarse(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind,
                                        const double *d_values, const double *d_b, double *d_x, size_t npatches,
                                        const int64_t *d_patch_ptr, const int32_t *d_patch_rows, size_t ncoarse, const int64_t *d_p_ptr,
                                        const int32_t *d_p_cols, const double *d_p_vals, double convergence_threshold,
                                        double divergence_threshold, size_t max_iter, int32_t *exit_reason, size_t *iterations,
                                        double *relative_residual)
{
    if (!ctx || !d_rowptr || (nrows && (!d_colind || !d_values || !d_b || !d_x || !d_patch_ptr || !d_patch_rows || !d_p_ptr || !d_p_cols ||
                                        !d_p_vals)))
        return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    int reason = 0, status = 0, refusal = 0;
    int32_t pivot = 0;
    PA_HIP(ctx, pa::conjugated_gradient_patch_coarse(ctx->stream, nrows, d_rowptr, d_colind, d_values, d_b, d_x, npatches, d_patch_ptr,
                                                     d_patch_rows, ncoarse, d_p_ptr, d_p_cols, d_p_vals, convergence_threshold,
                                                     divergence_threshold, max_iter, &reason, iterations, relative_residual, &status,
                                                     &refusal, &pivot));
    if (status == 1) return patch_refused(ctx, "pa_conjugated_gradient_patch_coarse", refusal);
    if (status == 3) return coarse_refused(ctx, "pa_conjugated_gradient_patch_coarse", refusal);
    if (status == 2) return patch_not_spd(ctx, "pa_conjugated_gradient_patch_coarse", "is not positive definite (pa_patch_precond_factor says which)");
    if (status == 4) return coarse_not_spd(ctx, "pa_conjugated_gradient_patch_coarse", pivot);
    if (exit_reason) *exit_reason = reason;
    return PA_OK;
}

// ---- a smoothed level (multilevel_precond.hip) and the conjugate gradient with patches, smoothed levels and an exact level ---------
static int smoothed_sizes(pa_context *ctx, const char *who, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, pa::SmoothedSizes *sz)
{
    int refusal = 0;
    PA_HIP(ctx, pa::smoothed_query(ctx->stream, nrows, ncoarse, d_p_ptr, sz, &refusal));
    return refusal ? coarse_refused(ctx, who, refusal) : PA_OK;
}

int pa_smoothed_level_query(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, pa_smoothed_level_info *out)
{
    if (!ctx || !d_p_ptr || !out) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::SmoothedSizes sz;
    const int st = smoothed_sizes(ctx, "pa_smoothed_level_query", nrows, ncoarse, d_p_ptr, &sz);
    if (st != PA_OK) return st;
    out->entries = sz.entries; out->pt_bytes = sz.pt_bytes; out->dinv_doubles = sz.dinv_doubles; out->scratch_bytes = sz.scratch_bytes;
    out->lanes_per_column = sz.lanes;
    return PA_OK;
}

int pa_smoothed_level_setup(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                            size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals, void *d_pt,
                            double *d_dinv, void *d_scratch, int32_t *column)
{
    if (!ctx || !d_rowptr || !d_p_ptr || !d_pt || !d_dinv || !d_scratch) return PA_ERR_INVALID_ARG;
    if (nrows && (!d_colind || !d_values || !d_p_cols || !d_p_vals)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const char *who = "pa_smoothed_level_setup";
    pa::SmoothedSizes sz;
    const int st = smoothed_sizes(ctx, who, nrows, ncoarse, d_p_ptr, &sz);
    if (st != PA_OK) return st;
    const pa::CoarseTable t{nrows, ncoarse, d_p_ptr, d_p_cols, d_p_vals};
    int refusal = 0;
    PA_HIP(ctx, pa::smoothed_validate(ctx->stream, t, sz, d_scratch, &refusal));
    if (refusal) return coarse_refused(ctx, who, refusal);
    int32_t col = 0;
    PA_HIP(ctx, pa::smoothed_setup(ctx->stream, d_rowptr, d_colind, d_values, t, sz, d_pt, d_dinv, d_scratch, &col));
    if (column) *column = col;
    return col ? level_not_spd(ctx, who, -1, col) : PA_OK;
}

int pa_smoothed_level_apply(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols,
                            const double *d_p_vals, const void *d_pt, const double *d_dinv, void *d_scratch, int accumulate,
                            const double *d_r, double *d_z)
{
    if (!ctx || !d_p_ptr || !d_pt || !d_dinv || !d_scratch) return PA_ERR_INVALID_ARG;
    if (nrows && (!d_p_cols || !d_p_vals || !d_r || !d_z)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    pa::SmoothedSizes sz;
    const int st = smoothed_sizes(ctx, "pa_smoothed_level_apply", nrows, ncoarse, d_p_ptr, &sz);
    if (st != PA_OK) return st;
    const pa::CoarseTable t{nrows, ncoarse, d_p_ptr, d_p_cols, d_p_vals};
    pa::smoothed_apply(ctx->stream, t, sz, d_pt, d_dinv, d_scratch, accumulate, d_r, d_z, nullptr);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_conjugated_gradient_multilevel(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                                      const double *d_b, double *d_x, size_t npatches, const int64_t *d_patch_ptr,
                                      const int32_t *d_patch_rows, size_t nlevels, const pa_coarse_table *levels,
                                      const pa_coarse_table *exact, double convergence_threshold, double divergence_threshold,
                                      size_t max_iter, int32_t *exit_reason, size_t *iterations, double *relative_residual)
{
    if (!ctx || !d_rowptr || nlevels > (size_t)PA_MULTILEVEL_MAX_LEVELS || (nlevels && !levels)) return PA_ERR_INVALID_ARG;
    if (nrows && (!d_colind || !d_values || !d_b || !d_x || !d_patch_ptr || !d_patch_rows)) return PA_ERR_INVALID_ARG;
    pa::CoarseTable lt[PA_MULTILEVEL_MAX_LEVELS], et{};
    for (size_t k = 0; k <= nlevels; ++k) {
        const pa_coarse_table *t = k < nlevels ? &levels[k] : exact;
        if (!t) continue;
        if (nrows && (!t->d_p_ptr || !t->d_p_cols || !t->d_p_vals)) return PA_ERR_INVALID_ARG;
        (k < nlevels ? lt[k] : et) = pa::CoarseTable{nrows, t->ncoarse, t->d_p_ptr, t->d_p_cols, t->d_p_vals};
    }
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const char *who = "pa_conjugated_gradient_multilevel";
    int reason = 0;
    pa::MultilevelReport rep;
    PA_HIP(ctx, pa::conjugated_gradient_multilevel(ctx->stream, nrows, d_rowptr, d_colind, d_values, d_b, d_x, npatches, d_patch_ptr, d_patch_rows,
                                                   (int)nlevels, lt, exact ? &et : nullptr, convergence_threshold, divergence_threshold, max_iter,
                                                   &reason, iterations, relative_residual, &rep));
    switch (rep.status) {
    case 1: return patch_refused(ctx, who, rep.refusal);
    case 2: return patch_not_spd(ctx, who, "is not positive definite (pa_patch_precond_factor says which)");
    case 3: return coarse_refused(ctx, who, rep.refusal);
    case 4: return coarse_not_spd(ctx, who, rep.pivot);
    case 5: {
        const int st = coarse_refused(ctx, who, rep.refusal);
        ctx->last_error += " (smoothed level " + std::to_string(rep.level) + ")";
        return st;
    }
    case 6: return level_not_spd(ctx, who, rep.level, rep.pivot);
    default: break;
    }
    if (exit_reason) *exit_reason = reason;
    return PA_OK;
}

// ---- both levels on the row-partitioned system (rows_precond.hip), the tables of a slab, and the whole-mesh coarse table -----------
int pa_conjugated_gradient_rows_patch_coarse(pa_context *ctx, const pa_cg_transport *transport, int64_t row_begin, int64_t row_end,
                                             const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values, const double *d_b,
                                             double *d_x, size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                                             size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals,
                                             double convergence_threshold, double divergence_threshold, size_t max_iter,
                                             int32_t *exit_reason, size_t *iterations, double *relative_residual, int32_t *transport_status)
{
    if (!ctx || !d_rowptr || row_end < row_begin || row_end >= ((int64_t)1 << 31)) return PA_ERR_INVALID_ARG;
    if (row_end > row_begin && (!d_colind || !d_values || !d_b || !d_x || !d_patch_ptr || !d_patch_rows)) return PA_ERR_INVALID_ARG;
    if (ncoarse && (!d_p_ptr || !d_p_cols || !d_p_vals)) return PA_ERR_INVALID_ARG;
    pa::CgTransport tp;
    if (!transport_in(transport, &tp)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    int reason = 0, tstat = 0;
    pa::RowsPrecondReport rep;
    const hipError_t he = pa::conjugated_gradient_rows_patch_coarse(ctx->stream, transport ? &tp : nullptr, row_begin, row_end, d_rowptr, d_colind,
                                                                    d_values, d_b, d_x, npatches, d_patch_ptr, d_patch_rows, ncoarse, d_p_ptr,
                                                                    d_p_cols, d_p_vals, convergence_threshold, divergence_threshold, max_iter,
                                                                    &reason, iterations, relative_residual, &tstat, &rep);
    const char *who = "pa_conjugated_gradient_rows_patch_coarse";
    const int st = rows_solve_result(ctx, who, he, reason, tstat, exit_reason, transport_status);
    if (he != hipSuccess || tstat < 5) return st;
    if (tstat == 5) return rep.level == 1 ? patch_refused(ctx, who, rep.refusal) : coarse_refused(ctx, who, rep.refusal);
    return rep.level == 1 ? patch_not_spd(ctx, who, "of this rank is not positive definite") : coarse_not_spd(ctx, who, rep.pivot);
}

// a slab of the generator mesh and the compressed faces [p0, p1) it owns (cond_prepare); a whole mesh is the slab of all rows
static int slab_of(pa_context *ctx, pa_degree_info di, const char *who, pa::StructuredMesh *sm, int32_t *p0, int32_t *p1)
{
    if (!degree_ok(di)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (!ctx->faces.structured) { ctx->last_error = std::string(who) + ": the mesh of pa_mesh_generate only"; return PA_ERR_INVALID_ARG; }
    const int st = cond_prepare(ctx);
    if (st != PA_OK) return st;
    if ((uint64_t)(di.face_deg + 1) * ctx->faces.num_other_faces >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // int32 rows
    *sm = ctx->faces.sm; *p0 = ctx->cond.p0; *p1 = ctx->cond.p0 + (int32_t)ctx->cond.nown;
    return PA_OK;
}

static int rows_patches(pa_context *ctx, pa_degree_info di, int kind, const char *who, size_t *npatches, size_t *entries, int64_t *d_patch_ptr,
                        int32_t *d_patch_rows)
{
    if (kind != PA_PATCH_FACE && kind != PA_PATCH_CELL) return PA_ERR_INVALID_ARG;
    pa::StructuredMesh sm;
    int32_t p0 = 0, p1 = 0;
    const int st = slab_of(ctx, di, who, &sm, &p0, &p1);
    if (st != PA_OK) return st;
    const int fbs = di.face_deg + 1;
    uint64_t np = (uint64_t)(p1 - p0), ne = np * fbs;
    if (kind == PA_PATCH_FACE) {
        if (d_patch_ptr) {
            pa::face_patches(ctx->stream, (uint32_t)np, fbs, p0 * fbs, d_patch_ptr, d_patch_rows);
            PA_HIP(ctx, hipGetLastError());
        }
    } else PA_HIP(ctx, pa::slab_cell_patches(ctx->stream, sm, p0, p1, fbs, &np, &ne, d_patch_ptr, d_patch_rows));
    if (npatches) *npatches = (size_t)np;
    if (entries) *entries = (size_t)ne;
    return PA_OK;
}

int pa_condensed_rows_patches_query(pa_context *ctx, pa_degree_info di, int kind, size_t *npatches, size_t *entries)
{
    if (!ctx || !npatches || !entries) return PA_ERR_INVALID_ARG;
    return rows_patches(ctx, di, kind, "pa_condensed_rows_patches_query", npatches, entries, nullptr, nullptr);
}

int pa_condensed_rows_patches(pa_context *ctx, pa_degree_info di, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows)
{
    if (!ctx || !d_patch_ptr || !d_patch_rows) return PA_ERR_INVALID_ARG;
    return rows_patches(ctx, di, kind, "pa_condensed_rows_patches", nullptr, nullptr, d_patch_ptr, d_patch_rows);
}

static int rows_coarse(pa_context *ctx, pa_degree_info di, int H, int parts, const char *who, size_t *ncoarse, size_t *entries,
                       int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    if (H < 1) return PA_ERR_INVALID_ARG;
    if (parts != PA_COARSE_ONE) { ctx->last_error = std::string(who) + ": PA_COARSE_ONE only (the parts of a cut mesh are a whole-mesh table's)"; return PA_ERR_INVALID_ARG; }
    pa::SlabCoarseMesh m;
    const int st = slab_of(ctx, di, who, &m.sm, &m.p0, &m.p1);
    if (st != PA_OK) return st;
    uint64_t nc = 0, ne = 0;
    PA_HIP(ctx, pa::condensed_rows_coarse(ctx->stream, m, di.face_deg + 1, H, &nc, &ne, d_p_ptr, d_p_cols, d_p_vals));
    if (nc < 1 || nc > (uint64_t)PA_COARSE_MAX_NODES) return coarse_count_refused(ctx, who, H, nc);
    if (ncoarse) *ncoarse = (size_t)nc;
    if (entries) *entries = (size_t)ne;
    return PA_OK;
}

int pa_condensed_rows_coarse_query(pa_context *ctx, pa_degree_info di, int H, int parts, size_t *ncoarse, size_t *entries)
{
    if (!ctx || !ncoarse || !entries) return PA_ERR_INVALID_ARG;
    return rows_coarse(ctx, di, H, parts, "pa_condensed_rows_coarse_query", ncoarse, entries, nullptr, nullptr, nullptr);
}

int pa_condensed_rows_coarse(pa_context *ctx, pa_degree_info di, int H, int parts, int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    if (!ctx || !d_p_ptr || !d_p_cols || !d_p_vals) return PA_ERR_INVALID_ARG;
    return rows_coarse(ctx, di, H, parts, "pa_condensed_rows_coarse", nullptr, nullptr, d_p_ptr, d_p_cols, d_p_vals);
}

// the refusals of the two pa_condensed_coarse entries and the mesh they read
static int coarse_mesh(pa_context *ctx, pa_degree_info di, int H, int parts, int where, pa::CoarseMesh *m)
{
    if (!degree_ok(di) || H < 1 || (parts != PA_COARSE_ONE && parts != PA_COARSE_BY_SIDE)) return PA_ERR_INVALID_ARG;
    if (parts == PA_COARSE_BY_SIDE && where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const int st = asm_prepare(ctx);                     // whole-mesh contexts only, as pa_condensed_patches
    if (st != PA_OK) return st;
    if (!ctx->faces.structured) { ctx->last_error = "pa_condensed_coarse: the mesh of pa_mesh_generate / pa_cut_preprocess only"; return PA_ERR_INVALID_ARG; }
    if (parts == PA_COARSE_BY_SIDE && (!ctx->cut.host || !ctx->cut.face_loc.get())) return PA_ERR_NO_MESH;
    PA_HIP(ctx, join_side_stream(ctx));
    m->sm = ctx->faces.sm; m->nfaces = (uint32_t)ctx->faces.nfaces_local;
    m->face_pts = ctx->faces.face_pts.get(); m->face_compress = ctx->faces.face_compress.get();
    m->face_loc = parts == PA_COARSE_BY_SIDE ? ctx->cut.face_loc.get() : nullptr; m->where = where;
    return PA_OK;
}

int coarse_count_refused(pa_context *ctx, const char *who, int H, uint64_t ncoarse, uint64_t max_columns)
{
    ctx->last_error = std::string(who) + ": H = " + std::to_string(H) + " gives " + std::to_string(ncoarse) +
                      " coarse columns; 1 to " + std::to_string(max_columns) + " are served";
    return PA_ERR_INVALID_ARG;
}

int pa_condensed_coarse_query(pa_context *ctx, pa_degree_info di, int H, int parts, int where, size_t *ncoarse, size_t *entries)
{
    if (!ctx || !ncoarse || !entries) return PA_ERR_INVALID_ARG;
    pa::CoarseMesh m;
    const int st = coarse_mesh(ctx, di, H, parts, where, &m);
    if (st != PA_OK) return st;
    uint64_t nc = 0, ne = 0;
    const uint64_t cap = ctx->coarse_table_cap;
    PA_HIP(ctx, pa::condensed_coarse(ctx->stream, m, di.face_deg + 1, H, cap, &nc, &ne, nullptr, nullptr, nullptr));
    if (nc < 1 || nc > cap) return coarse_count_refused(ctx, "pa_condensed_coarse_query", H, nc, cap);
    *ncoarse = (size_t)nc;
    *entries = (size_t)ne;
    return PA_OK;
}

int pa_condensed_coarse(pa_context *ctx, pa_degree_info di, int H, int parts, int where, int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    if (!ctx || !d_p_ptr || !d_p_cols || !d_p_vals) return PA_ERR_INVALID_ARG;
    pa::CoarseMesh m;
    const int st = coarse_mesh(ctx, di, H, parts, where, &m);
    if (st != PA_OK) return st;
    uint64_t nc = 0, ne = 0;
    const uint64_t cap = ctx->coarse_table_cap;
    PA_HIP(ctx, pa::condensed_coarse(ctx->stream, m, di.face_deg + 1, H, cap, &nc, &ne, d_p_ptr, d_p_cols, d_p_vals));
    if (nc < 1 || nc > cap) return coarse_count_refused(ctx, "pa_condensed_coarse", H, nc, cap);
    return PA_OK;
}
