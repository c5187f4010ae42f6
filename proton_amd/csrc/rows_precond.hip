// rows_precond.hip -- the order in which the two levels of patch_precond.hip and coarse_precond.hip are called: the conjugate
// gradient of solver_cg.hpp:63-144 (the solve of cuthho_square.cpp:915-919 on the face-only system) with
//   z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r + P (P^T A P)^-1 P^T r
// on one rank (conjugated_gradient_patch: the first term alone; conjugated_gradient_patch_coarse) and on a ROW-PARTITIONED system
// (conjugated_gradient_rows_patch_coarse), where every rank holds the rows [row_begin, row_end) of A (global columns), its own
// patches and its own rows of P.
//
// There is no kernel and no loop here: the iterations are solver.hip's (conjugated_gradient_one_rank,
// conjugated_gradient_rows_stored), the kernels are those of the two levels, and this file is the order of the calls.
//   TwoLevel: both tables, what they need on the device, and the local set-up every front end shares (prepare): the patch table
//             judged and factored, then the coarse table judged.  A refusal of either table wins over a failed patch pivot, which
//             prepare only counts; the front ends map its result to their own statuses.  apply: the patch sum, then the coarse term.
//   one rank: prepare, coarse_factor, the one-rank loop with TwoLevel's apply.
//   patches:  on a rank a patch lies inside the rank's rows, so its block R_p A R_p^T lies inside the rank's rows and their own
//             columns: the level needs no communication.  The table names global rows (PatchTable::row0), the matrix is read through
//             the window view: storage row r - row_begin, global columns.
//   set-up:   the rows of P for the two ends of the window come from the neighbours through the transport's halo callback, 8 doubles
//             a row; W = A_r P_window (16 slots a row), the rank's addend P_r^T W of A_c in the fixed order of the one-rank product;
//             the lower triangle is summed over the ranks and mirrored, so A_c is the same bits on every rank, and every rank
//             factors it.
//   apply:    patch sum (local), P_r^T r (local), its sum over the ranks, the two packed triangular products (redundant), the
//             gather added onto the patch sum with the block partials of r . z.
//   levels:   conjugated_gradient_multilevel adds the smoothed levels of multilevel_precond.hip between the two: the tables judged in
//             the order patches, levels, exact level, then the matrices in the same order, and an apply whose gathers share one pass
//             over z.  Without a smoothed level it is the two-level solver itself.  One rank only.
// Every exit of the row-partitioned solve is collective (solver.hip): a local failure -- a refused table (5), a matrix that is not
// positive definite (6), a callback (1), HIP (4) -- is a flag behind the next sum, and nobody iterates unless everybody can.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cg.hpp"
#include "coarse_precond.hpp"
#include "device_tmp.hpp"
#include "multilevel_precond.hpp"
#include "patch_precond.hpp"
#include "rows_precond.hpp"

namespace pa {

namespace {

constexpr size_t SUM_PIECE = (size_t)1 << 20;      // doubles of A_c's triangle per sum over the ranks (the callback counts in int)

struct TwoLevel {
    PatchTable pt;
    CoarseTable ct;                        // ncoarse = 0 after prepare(coarse = false): patches only
    PatchSizes psz = PatchSizes();
    CoarseSizes csz = CoarseSizes();
    double *factors = nullptr, *cfactor = nullptr;
    int32_t *slots = nullptr, *info = nullptr;
    char *pscratch = nullptr, *cpt = nullptr, *cscratch = nullptr;
    // what prepare found: the level whose table was refused (1 the patches, 2 the coarse level, 0 neither) with the refusal's code,
    // and the patches whose pivot failed -- to be reported only where no table was refused
    int level = 0, refusal = 0;
    size_t failed = 0;

    bool refused(int lv) { level = refusal ? lv : 0; return refusal != 0; }

    // the local set-up: the patch table judged and factored (a system without rows has none), then -- coarse -- the coarse table
    // judged.  Returns at the first refusal.  The temporaries are tmp's.
    hipError_t prepare(hipStream_t stream, DeviceTmp &tmp, const int64_t *rowptr, const int32_t *colind, const double *values, bool coarse)
    {
        const hipError_t e = prepare_patches(stream, tmp, rowptr, colind, values);
        if (e != hipSuccess || level || !coarse) return e;
        return prepare_coarse(stream, tmp);
    }

    // its two halves (the multilevel solver judges its smoothed levels between them)
    hipError_t prepare_patches(hipStream_t stream, DeviceTmp &tmp, const int64_t *rowptr, const int32_t *colind, const double *values)
    {
        hipError_t e = hipSuccess;
        if (pt.n) {
            e = patch_query(stream, pt.n, pt.npatches, pt.ptr, &psz, &refusal);
            if (e != hipSuccess || refused(1)) return e;
            if (!tmp.alloc(&factors, (size_t)psz.factor_doubles + 1) || !tmp.alloc(&slots, (size_t)psz.slot_ints) ||
                !tmp.alloc(&info, pt.npatches + 1) || !tmp.alloc(&pscratch, (size_t)psz.scratch_bytes))
                return tmp.error();
            e = patch_factor(stream, rowptr, colind, values, pt, psz, factors, slots, pscratch, info, &refusal, &failed);
            if (e != hipSuccess || refused(1)) return e;
        }
        return hipSuccess;
    }

    hipError_t prepare_coarse(hipStream_t stream, DeviceTmp &tmp)
    {
        hipError_t e = coarse_query(stream, ct.n, ct.ncoarse, ct.ptr, &csz, &refusal);
        if (e != hipSuccess || refused(2)) return e;
        if (!tmp.alloc(&cpt, (size_t)csz.pt_bytes) || !tmp.alloc(&cfactor, (size_t)csz.factor_doubles) ||
            !tmp.alloc(&cscratch, (size_t)csz.scratch_bytes))
            return tmp.error();
        e = coarse_validate(stream, ct, csz, cscratch, &refusal);
        if (e != hipSuccess || refused(2)) return e;
        return hipSuccess;
    }
};

// z = M^-1 r of a prepared and factored TwoLevel: the patch sum, and the coarse term onto it where there is one (the block partials
// of r . z come from whichever kernel writes z last)
void two_level_apply(void *user, hipStream_t stream, const double *r, double *z, double *part_rz)
{
    const TwoLevel &l = *(const TwoLevel *)user;
    patch_apply(stream, l.pt, l.psz, l.factors, l.slots, l.pscratch, r, z, l.ct.ncoarse ? nullptr : part_rz);
    if (l.ct.ncoarse) coarse_apply(stream, l.ct, l.csz, l.cpt, l.cfactor, l.cscratch, 1, r, z, part_rz);
}

// both one-rank solvers.  coarse = false: the patches alone, status 0 .. 2
hipError_t conjugated_gradient_two_level(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                                         const double *b, double *x, const PatchTable &pt, bool coarse, const CoarseTable &ct,
                                         double convergence_threshold, double divergence_threshold, size_t max_iter, int *exit_reason,
                                         size_t *iterations, double *relative_residual, int *status, int *refusal, int32_t *pivot)
{
    *status = 0;
    *refusal = 0;
    *pivot = 0;
    size_t iter = 0;
    int reason = 0;
    double rr = 0.0;
    if (n) {
        DeviceTmp tmp(stream);
        TwoLevel l;
        l.pt = pt;
        l.ct = coarse ? ct : CoarseTable{n, 0, nullptr, nullptr, nullptr};
        double *z = nullptr;
        if (!tmp.alloc(&z, n)) return tmp.error();
        hipError_t e = l.prepare(stream, tmp, rowptr, colind, values, coarse);
        if (e != hipSuccess) return e;
        *refusal = l.refusal;
        if (l.level) { *status = l.level == 1 ? 1 : 3; return hipSuccess; }
        if (l.failed) { *status = 2; return hipSuccess; }
        if (coarse) {
            e = coarse_factor(stream, rowptr, colind, values, l.ct, l.csz, l.cpt, l.cfactor, l.cscratch, nullptr, pivot, refusal);
            if (e != hipSuccess) return e;
            if (*refusal) { *status = 3; return hipSuccess; }
            if (*pivot) { *status = 4; return hipSuccess; }
        }
        const CgPreconditioner pre{&l, two_level_apply, z};
        e = conjugated_gradient_one_rank(stream, n, CgCsr{rowptr, colind, values, nullptr}, &pre, nullptr, b, x, convergence_threshold,
                                         divergence_threshold, max_iter, 0, &reason, &iter, &rr);
        if (e != hipSuccess) return e;
    }
    if (exit_reason) *exit_reason = reason;
    if (iterations) *iterations = iter;
    if (relative_residual) *relative_residual = rr;
    return hipSuccess;
}

// ---- the additive multilevel form: TwoLevel's patches and exactly solved level with smoothed levels between them -------------------
struct Multilevel {
    TwoLevel two;                          // (ct.ncoarse = 0: no exact level)
    int nlevels = 0;
    CoarseTable lt[MULTILEVEL_MAX_TABLES];
    SmoothedSizes lsz[MULTILEVEL_MAX_TABLES];
    char *lpt[MULTILEVEL_MAX_TABLES], *lscratch[MULTILEVEL_MAX_TABLES];
    double *ldinv[MULTILEVEL_MAX_TABLES];
};

// z = M^-1 r: the patch sum, every level's coarse vector (u_l = D_l^-1 P_l^T r, then the exact level's L^-T L^-1 P_c^T r), and one
// pass over z that adds the gathers in the order levels 0, 1, .., exact and leaves the block partials of r . z
void multilevel_apply(void *user, hipStream_t stream, const double *r, double *z, double *part_rz)
{
    const Multilevel &m = *(const Multilevel *)user;
    const TwoLevel &l = m.two;
    patch_apply(stream, l.pt, l.psz, l.factors, l.slots, l.pscratch, r, z, nullptr);
    ProlongTables tb{};
    for (int k = 0; k < m.nlevels; ++k) {
        tb.ptr[tb.count] = m.lt[k].ptr; tb.cols[tb.count] = m.lt[k].cols; tb.vals[tb.count] = m.lt[k].vals;
        tb.u[tb.count++] = smoothed_restrict(stream, m.lt[k], m.lsz[k], m.lpt[k], m.ldinv[k], m.lscratch[k], r);
    }
    if (l.ct.ncoarse) {
        coarse_restrict(stream, l.ct, l.csz, l.cpt, l.cscratch, r);
        tb.ptr[tb.count] = l.ct.ptr; tb.cols[tb.count] = l.ct.cols; tb.vals[tb.count] = l.ct.vals;
        tb.u[tb.count++] = coarse_solve(stream, l.ct, l.csz, l.cfactor, l.cscratch);
    }
    multilevel_prolong(stream, l.pt.n, tb, r, z, part_rz);
}

struct RowsPrecond {
    DeviceTmp *tmp;
    TwoLevel lv;
    std::vector<double> host;              // what goes through allreduce_sum
    RowsPrecondReport rep;
};

template <class T> bool take(RowsPrecond &p, CgRowsFail *fail, T **q, size_t count)
{
    return p.tmp->alloc(q, count) || fail->hip_ok(p.tmp->error());
}

// the local part
void rows_prepare(void *user, hipStream_t stream, const CgRowsSystem &s, CgRowsFail *fail)
{
    RowsPrecond &p = *(RowsPrecond *)user;
    TwoLevel &l = p.lv;
    if (!fail->hip_ok(l.prepare(stream, *p.tmp, s.rowptr, s.colind, s.values, l.ct.ncoarse != 0))) return;
    if (l.level) { p.rep.level = l.level; p.rep.refusal = l.refusal; fail->status = 5; }
    else if (l.failed) { p.rep.level = 1; fail->status = 6; }
}

// host doubles summed over the ranks in place, the rank's flag behind them -> 0, or the status every rank leaves with
int rows_sum(const CgTransport *tp, double *vals, size_t count, const CgRowsFail *fail)
{
    vals[count] = fail->status ? 1.0 : 0.0;
    if (tp->allreduce_sum(tp->user, vals, (int)(count + 1)) != 0) return fail->status ? fail->status : 1;
    return vals[count] > 0.0 ? (fail->status ? fail->status : 3) : 0;
}

// the collective part: A_c, the same bits on every rank, and its factor
int rows_setup(void *user, hipStream_t stream, const CgRowsSystem &s, CgRowsFail *fail)
{
    RowsPrecond &p = *(RowsPrecond *)user;
    TwoLevel &l = p.lv;
    if (!l.ct.ncoarse) return 0;
    const CgTransport *tp = s.tp;
    const size_t n = l.ct.n, nc = l.ct.ncoarse, ntri = nc * (nc + 1) / 2;
    const size_t need_lo = (size_t)s.need_lo, need_hi = (size_t)s.need_hi, give_lo = (size_t)s.give_lo, give_hi = (size_t)s.give_hi;
    int refusal = 0;
    CoarseWindow win{};
    if (tp) {
        // P for the window: my first and last rows to the neighbours, theirs into the two ends.  (Rows that never arrive -- a
        // neighbour whose exchange failed -- read as empty: all bits set is no column.)
        double *send_lo = nullptr, *send_hi = nullptr, *recv_lo = nullptr, *recv_hi = nullptr, *wvals = nullptr;
        int64_t *wptr = nullptr;
        int32_t *wcols = nullptr;
        const size_t wentries = (size_t)l.csz.entries + COARSE_MAX_ROW_ENTRIES * (need_lo + need_hi);
        if (!fail->status)
            (void)(take(p, fail, &send_lo, 8 * give_lo) && take(p, fail, &send_hi, 8 * give_hi) && take(p, fail, &recv_lo, 8 * need_lo) &&
                   take(p, fail, &recv_hi, 8 * need_hi) && take(p, fail, &wptr, need_lo + n + need_hi + 1) &&
                   take(p, fail, &wcols, wentries) && take(p, fail, &wvals, wentries));
        if (!fail->status)
            (void)(fail->hip_ok(hipMemsetAsync(recv_lo, 0xff, need_lo ? 64 * need_lo : 8, stream)) &&
                   fail->hip_ok(hipMemsetAsync(recv_hi, 0xff, need_hi ? 64 * need_hi : 8, stream)));
        if (!fail->status) {
            coarse_rows_pack(stream, l.ct, 0, give_lo, send_lo);
            coarse_rows_pack(stream, l.ct, n - give_hi, give_hi, send_hi);
            if (tp->halo(tp->user, send_lo, 8 * give_lo, send_hi, 8 * give_hi, recv_lo, 8 * need_lo, recv_hi, 8 * need_hi, (void *)stream) != 0)
                fail->status = 1;
        }
        if (!fail->status) {
            coarse_window_build(stream, l.ct, l.csz, need_lo, need_hi, recv_lo, recv_hi, wptr, wcols, wvals);
            win = CoarseWindow{s.row_begin - s.need_lo, need_lo + n + need_hi, wptr, wcols, wvals};
        }
    }
    if (!fail->status && fail->hip_ok(coarse_galerkin(stream, s.rowptr, s.colind, s.values, l.ct, l.csz, tp ? &win : nullptr, l.cpt,
                                                      l.cscratch, &refusal)) && refusal) {
        p.rep.level = 2; p.rep.refusal = refusal; fail->status = 5;
    }
    if (tp) {
        // the lower triangle over the ranks, in pieces; then both triangles from it: exactly symmetric, identical everywhere
        double *tri = nullptr;
        std::vector<double> h(ntri, 0.0), piece(std::min(ntri, SUM_PIECE) + 1);
        if (!fail->status && take(p, fail, &tri, ntri)) {
            coarse_matrix_triangle(stream, l.ct, l.csz, l.cscratch, 0, tri);
            (void)(fail->hip_ok(hipMemcpyAsync(h.data(), tri, ntri * 8, hipMemcpyDeviceToHost, stream)) && fail->hip_ok(hipStreamSynchronize(stream)));
        }
        for (size_t off = 0; off < ntri; off += SUM_PIECE) {
            const size_t m = std::min(SUM_PIECE, ntri - off);
            std::copy(h.begin() + off, h.begin() + off + m, piece.begin());
            if (fail->status) std::fill(piece.begin(), piece.begin() + m, 0.0);
            const int st = rows_sum(tp, piece.data(), m, fail);
            if (st) return st;
            std::copy(piece.begin(), piece.begin() + m, h.begin() + off);
        }
        if (fail->hip_ok(hipMemcpyAsync(tri, h.data(), ntri * 8, hipMemcpyHostToDevice, stream)) && fail->hip_ok(hipStreamSynchronize(stream)))
            coarse_matrix_triangle(stream, l.ct, l.csz, l.cscratch, 1, tri);
    }
    if (!fail->status && fail->hip_ok(coarse_cholesky(stream, l.ct, l.csz, l.cfactor, l.cscratch, nullptr, &p.rep.pivot)) && p.rep.pivot) {
        p.rep.level = 2; fail->status = 6;       // (the same pivot on every rank: they factor the same bits)
    }
    p.host.assign(nc + 1, 0.0);
    if (!tp) return fail->status;
    double flag[2] = {0.0, 0.0};
    return rows_sum(tp, flag, 0, fail);
}

// TwoLevel's apply in its stages, the sum of the restrictions over the ranks between the two halves of the coarse term
int rows_apply(void *user, hipStream_t stream, const CgRowsSystem &s, const double *r, double *z, double *part_rz, CgRowsFail *fail)
{
    RowsPrecond &p = *(RowsPrecond *)user;
    const TwoLevel &l = p.lv;
    const CgTransport *tp = s.tp;
    const size_t n = l.pt.n, nc = l.ct.ncoarse;
    if (!fail->status) {
        if (n) patch_apply(stream, l.pt, l.psz, l.factors, l.slots, l.pscratch, r, z, nc ? nullptr : part_rz);
        else (void)fail->hip_ok(hipMemsetAsync(part_rz, 0, 8, stream));      // (no rows: the one block's partial is zero)
    }
    if (!nc) return 0;
    double *rc = nullptr;
    if (!fail->status) rc = coarse_restrict(stream, l.ct, l.csz, l.cpt, l.cscratch, r);
    if (tp) {
        std::fill(p.host.begin(), p.host.end(), 0.0);
        if (!fail->status)
            (void)(fail->hip_ok(hipMemcpyAsync(p.host.data(), rc, nc * 8, hipMemcpyDeviceToHost, stream)) && fail->hip_ok(hipStreamSynchronize(stream)));
        if (fail->status) std::fill(p.host.begin(), p.host.end(), 0.0);
        const int st = rows_sum(tp, p.host.data(), nc, fail);
        if (st) return st;
        (void)fail->hip_ok(hipMemcpyAsync(rc, p.host.data(), nc * 8, hipMemcpyHostToDevice, stream));
    }
    if (!fail->status && n) coarse_correct(stream, l.ct, l.csz, l.cfactor, l.cscratch, 1, r, z, part_rz);
    return 0;
}

}  // namespace

hipError_t conjugated_gradient_patch(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                                     const double *b, double *x, size_t npatches, const int64_t *patch_ptr, const int32_t *patch_rows,
                                     double convergence_threshold, double divergence_threshold, size_t max_iter, int *exit_reason,
                                     size_t *iterations, double *relative_residual, int *status, int *refusal)
{
    int32_t pivot = 0;
    return conjugated_gradient_two_level(stream, n, rowptr, colind, values, b, x, PatchTable{n, npatches, patch_ptr, patch_rows}, false,
                                         CoarseTable{}, convergence_threshold, divergence_threshold, max_iter, exit_reason, iterations,
                                         relative_residual, status, refusal, &pivot);
}

hipError_t conjugated_gradient_patch_coarse(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind,
                                            const double *values, const double *b, double *x, size_t npatches, const int64_t *patch_ptr,
                                            const int32_t *patch_rows, size_t ncoarse, const int64_t *p_ptr, const int32_t *p_cols,
                                            const double *p_vals, double convergence_threshold, double divergence_threshold,
                                            size_t max_iter, int *exit_reason, size_t *iterations, double *relative_residual, int *status,
                                            int *refusal, int32_t *pivot)
{
    return conjugated_gradient_two_level(stream, n, rowptr, colind, values, b, x, PatchTable{n, npatches, patch_ptr, patch_rows}, true,
                                         CoarseTable{n, ncoarse, p_ptr, p_cols, p_vals}, convergence_threshold, divergence_threshold,
                                         max_iter, exit_reason, iterations, relative_residual, status, refusal, pivot);
}

hipError_t conjugated_gradient_multilevel(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                                          const double *b, double *x, size_t npatches, const int64_t *patch_ptr, const int32_t *patch_rows,
                                          int nlevels, const CoarseTable *levels, const CoarseTable *exact, double convergence_threshold,
                                          double divergence_threshold, size_t max_iter, int *exit_reason, size_t *iterations,
                                          double *relative_residual, MultilevelReport *report)
{
    *report = MultilevelReport();
    const PatchTable pt{n, npatches, patch_ptr, patch_rows};
    if (nlevels == 0) {                    // the two-level solvers themselves: their launches, their bits
        const hipError_t e = conjugated_gradient_two_level(stream, n, rowptr, colind, values, b, x, pt, exact != nullptr,
                                                           exact ? *exact : CoarseTable{}, convergence_threshold, divergence_threshold, max_iter,
                                                           exit_reason, iterations, relative_residual, &report->status, &report->refusal,
                                                           &report->pivot);
        report->level = -1;
        return e;
    }
    size_t iter = 0;
    int reason = 0;
    double rr = 0.0;
    if (n) {
        DeviceTmp tmp(stream);
        Multilevel m;
        TwoLevel &l = m.two;
        l.pt = pt;
        l.ct = exact ? *exact : CoarseTable{n, 0, nullptr, nullptr, nullptr};
        m.nlevels = nlevels;
        double *z = nullptr;
        if (!tmp.alloc(&z, n)) return tmp.error();
        // the tables, in their order: patches, levels, exact
        hipError_t e = l.prepare_patches(stream, tmp, rowptr, colind, values);
        if (e != hipSuccess) return e;
        if (l.level) { report->status = 1; report->refusal = l.refusal; return hipSuccess; }
        for (int k = 0; k < nlevels; ++k) {
            m.lt[k] = levels[k];
            report->level = k;
            e = smoothed_query(stream, n, levels[k].ncoarse, levels[k].ptr, &m.lsz[k], &report->refusal);
            if (e != hipSuccess) return e;
            if (report->refusal) { report->status = 5; return hipSuccess; }
            if (!tmp.alloc(&m.lpt[k], (size_t)m.lsz[k].pt_bytes) || !tmp.alloc(&m.ldinv[k], (size_t)m.lsz[k].dinv_doubles) ||
                !tmp.alloc(&m.lscratch[k], (size_t)m.lsz[k].scratch_bytes))
                return tmp.error();
            e = smoothed_validate(stream, m.lt[k], m.lsz[k], m.lscratch[k], &report->refusal);
            if (e != hipSuccess) return e;
            if (report->refusal) { report->status = 5; return hipSuccess; }
        }
        report->level = -1;
        if (exact) {
            e = l.prepare_coarse(stream, tmp);
            if (e != hipSuccess) return e;
            if (l.level) { report->status = 3; report->refusal = l.refusal; return hipSuccess; }
        }
        // the matrices, in the same order.  (Every level's validation left its counts in the level's own scratch.)
        if (l.failed) { report->status = 2; return hipSuccess; }
        for (int k = 0; k < nlevels; ++k) {
            e = smoothed_setup(stream, rowptr, colind, values, m.lt[k], m.lsz[k], m.lpt[k], m.ldinv[k], m.lscratch[k], &report->pivot);
            if (e != hipSuccess) return e;
            if (report->pivot) { report->status = 6; report->level = k; return hipSuccess; }
        }
        if (exact) {
            e = coarse_factor(stream, rowptr, colind, values, l.ct, l.csz, l.cpt, l.cfactor, l.cscratch, nullptr, &report->pivot, &report->refusal);
            if (e != hipSuccess) return e;
            if (report->refusal) { report->status = 3; return hipSuccess; }
            if (report->pivot) { report->status = 4; return hipSuccess; }
        }
        const CgPreconditioner pre{&m, multilevel_apply, z};
        e = conjugated_gradient_one_rank(stream, n, CgCsr{rowptr, colind, values, nullptr}, &pre, nullptr, b, x, convergence_threshold,
                                         divergence_threshold, max_iter, 0, &reason, &iter, &rr);
        if (e != hipSuccess) return e;
    }
    if (exit_reason) *exit_reason = reason;
    if (iterations) *iterations = iter;
    if (relative_residual) *relative_residual = rr;
    return hipSuccess;
}

hipError_t conjugated_gradient_rows_patch_coarse(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end,
                                                 const int64_t *rowptr, const int32_t *colind, const double *values, const double *b,
                                                 double *x, size_t npatches, const int64_t *patch_ptr, const int32_t *patch_rows,
                                                 size_t ncoarse, const int64_t *p_ptr, const int32_t *p_cols, const double *p_vals,
                                                 double convergence_threshold, double divergence_threshold, size_t max_iter,
                                                 int *exit_reason, size_t *iterations, double *relative_residual, int *transport_status,
                                                 RowsPrecondReport *report)
{
    const size_t n = (size_t)(row_end - row_begin);
    DeviceTmp tmp(stream);
    RowsPrecond p;
    p.tmp = &tmp;
    p.lv.pt = PatchTable{n, npatches, patch_ptr, patch_rows, row_begin};
    p.lv.ct = CoarseTable{n, ncoarse, p_ptr, p_cols, p_vals};
    double *z = nullptr;
    if (!tmp.alloc(&z, n)) return tmp.error();
    const CgRowsPreconditioner pre{&p, rows_prepare, rows_setup, rows_apply, z};
    const hipError_t e = conjugated_gradient_rows_stored(stream, tp, row_begin, row_end, rowptr, colind, values, &pre, b, x,
                                                         convergence_threshold, divergence_threshold, max_iter, exit_reason, iterations,
                                                         relative_residual, transport_status);
    if (report) *report = p.rep;
    return e;
}

}  // namespace pa
