// capi_local_ops.hip -- the C ABI's hot path (kernel selection, the local-operator passes over the cells) and the per-cell work
// next to it: right-hand sides, projections, quadrature points, boundary data, static condensation.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "context.hpp"
#include "hho_assembly.hpp"
#include "hho_aux.hpp"

#ifndef PA_PIECE_CELLS
#define PA_PIECE_CELLS ((size_t)192 * 1024)
#endif

// ---- the hot path -------------------------------------------------------------------------
static int pick_lanes(int cd, int fd, int quad)
{
    const int gmin = min_lanes(cd, fd, quad);
    if (gmin == 0) return 0;
    int lanes = gmin;                                   // fewest lanes per cell = most cells per wavefront
#ifdef PA_TUNING      // profiling / A-B builds only (proton_amd/_build.py, PA_BUILD_TAG): the shipped library reads no knob
    if (const char *env = std::getenv("PA_LANES_PER_CELL")) {
        const int v = std::atoi(env);
        if ((v == 16 || v == 32 || v == 64) && v >= gmin) lanes = v;
    }
#endif
    return lanes;
}

int select_kernel(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t n, const pa::KernelEntry **entry, int *grid,
                  bool cond)
{
    pa_sizes sz;
    const int st = pa_sizes_for(di, quad_kind, &sz);
    if (st != PA_OK) return st;
    if (stab_kind < PA_STAB_NONE || stab_kind > PA_STAB_FANCY) return PA_ERR_INVALID_ARG;
    const int lanes = pick_lanes(di.cell_deg, di.face_deg, quad_kind);
    const pa::KernelEntry *e = lanes ? find_kernel(di.cell_deg, di.face_deg, quad_kind, stab_kind, lanes) : nullptr;
    if (!e || (cond && !e->launch_cond)) return PA_ERR_INVALID_DEGREE;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cond ? e->func_cond : e->func, 64,
                                                     cond ? e->lds_bytes_cond : e->lds_bytes) != hipSuccess || per_cu < 1)
        per_cu = 1;
    // A persistent grid of exactly waves_per_simd x 4 blocks per CU: when the compiler needs fewer registers than
    // the launch bound allows the hardware could hold more, and more was measured to be slower (msize 9: +24 %)
    const int waves = cond ? e->waves_per_simd_cond : e->waves_per_simd;
    if (per_cu > 4 * waves) per_cu = 4 * waves;
#ifdef PA_TUNING
    if (const char *env = std::getenv("PA_BLOCKS_PER_CU")) {
        const int v = std::atoi(env);
        if (v > 0) per_cu = v;
    }
#endif
    const size_t cpb = 64 / lanes;
    size_t blocks = (n + cpb - 1) / cpb;
    const size_t resident = (size_t)per_cu * (size_t)ctx->num_cus;
    if (blocks > resident) blocks = resident;            // persistent: every block loops over its share of cells
    if (blocks == 0) blocks = 1;
    *entry = e;
    *grid = (int)blocks;
    return PA_OK;
}

int run_local_ops(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t first, size_t n, const LocalOpsOut &o)
{
    double *d_oper = o.oper, *d_data = o.data, *d_stab = o.stab, *d_lc = o.lc;
    int32_t *d_info = o.info;
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->mesh.points) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const pa::KernelEntry *e = nullptr;
    int grid = 0;
    const int st = select_kernel(ctx, di, quad_kind, stab_kind, n, &e, &grid, o.cond);
    if (st != PA_OK) return st;
    if (o.assemble && !e->launch_asm) return PA_ERR_INVALID_DEGREE;
    if (n == 0) return PA_OK;
    uint32_t ablate = 0;
#ifdef PA_TUNING      // stage ablation produces garbage operators on purpose: never in the shipped library
    if (const char *env = std::getenv("PA_ABLATE")) ablate = (uint32_t)std::strtoul(env, nullptr, 0);
#endif
    const bool split = !o.cond && (d_data != nullptr || d_stab != nullptr);
    // msize <= 9 and nothing but lc (and info) asked for: the thread-per-cell kernel of hho_small.hpp -- one launch, no record
    if (e->launch_small && !o.cond && !split && d_oper == nullptr && d_lc != nullptr && ablate == 0) {
        pa::SmallOpsArgs sa;
        sa.tab = ctx->tab.get(); sa.points = ctx->mesh.points; sa.ptids = ctx->mesh.ptids;
        sa.first = first; sa.n = n; sa.lc = d_lc; sa.info = d_info;
        PA_HIP(ctx, e->launch_small(sa, ctx->stream));
        return PA_OK;
    }
    // The cooperative kernel takes the per-cell head from the pre-pass and runs in pieces of at most `piece` cells: pre-pass
    // of a piece into the context's record buffer, then the cooperative kernel over the same cells (same stream).
    size_t piece = n;
    size_t cap_bytes = ctx->records.cap_bytes;                            // (pa_context_set_record_cap; default 4 GiB)
    const size_t per_cell = (size_t)e->pre_doubles * sizeof(double);
    size_t max_cells = (cap_bytes / per_cell) & ~(size_t)4095;
    // Pieces of at most PA_PIECE_CELLS cells by default: the records of a piece (134 MB at k = 2, 255 MB at k = 3) are then
    // still in the Infinity Cache when the cooperative kernel reads them, and the next piece's overwrite them there --
    // measured on 1024 x 1024 cells against one piece: 0.53 -> 0.46 ms at k = 1, 1.35 -> 1.27 ms at k = 2, 2.70 -> 2.44 ms at
    // k = 3, 11.1 -> 9.8 ms on 2048 x 2048 at k = 3 (tools/slab_timing.py; 96 Ki ... 256 Ki cells per piece within 2 %)
    // (not in the condensed mode, which writes 720 B per cell instead of 3.9 KB and is not short of HBM bandwidth: there the
    // extra launches and tails cost 2-8 %)
    if (!o.cond && max_cells > PA_PIECE_CELLS) max_cells = PA_PIECE_CELLS;
    if (max_cells < 4096) max_cells = 4096;
    if (piece > max_cells) {                                          // equal pieces, whole multiples of 4096 cells
        const size_t npieces = (n + max_cells - 1) / max_cells;
        piece = (((n + npieces - 1) / npieces) + 4095) & ~(size_t)4095;
    }
    const size_t need = ((piece + 7) / 8) * 8 * (size_t)e->pre_doubles;      // whole tiles of 8 records
    PA_HIP(ctx, ctx->records.pre.grow(need, ctx->stream));
    pa_sizes sz;
    (void)pa_sizes_for(di, quad_kind, &sz);
    const size_t mm = (size_t)sz.msize * (size_t)sz.msize, opn = (size_t)sz.oper_rows * (size_t)sz.msize;
    for (size_t off = 0; off < n; off += piece) {
        const size_t m = n - off < piece ? n - off : piece;
        int g = grid;
        if (m != n) {
            const pa::KernelEntry *e2 = nullptr;
            const int st2 = select_kernel(ctx, di, quad_kind, stab_kind, m, &e2, &g, o.cond);
            if (st2 != PA_OK) return st2;
        }
        pa::LocalOpsArgs a;
        a.tab = ctx->tab.get(); a.points = ctx->mesh.points; a.ptids = ctx->mesh.ptids;
        a.first = first + off; a.n = m;
        a.pre_ring = nullptr;
        pa::PreArgs pa_;
        pa_.tab = ctx->tab.get(); pa_.points = ctx->mesh.points; pa_.ptids = ctx->mesh.ptids;
        pa_.first = first + off; pa_.n = m; pa_.pre = ctx->records.pre.get();
        PA_HIP(ctx, e->launch_pre(pa_, ctx->stream));
        a.pre = ctx->records.pre.get();
        a.oper = d_oper ? d_oper + off * opn : nullptr;
        a.data = d_data ? d_data + off * mm : nullptr;
        a.stab = d_stab ? d_stab + off * mm : nullptr;
        a.lc = d_lc ? d_lc + off * mm : nullptr;
        a.info = d_info ? d_info + off : nullptr;
        const size_t ncond = (size_t)(4 * sz.fbs) * (size_t)(4 * sz.fbs + 1) / 2 + (size_t)(4 * sz.fbs);
        a.rhs = o.rhs ? o.rhs + off * (size_t)sz.cbs : nullptr;
        a.cond = o.cond_out ? o.cond_out + off * ncond : nullptr;
        a.uF = o.uF ? o.uF + off * (size_t)(4 * sz.fbs) : nullptr;
        a.uT = o.uT ? o.uT + off * (size_t)sz.cbs : nullptr;
        a.ablate = ablate;
        a.dbg = nullptr;
        a.scatter = o.scatter;
#ifdef PA_STAGE_CLOCK
        // diagnostic build: per-stage shader clocks of the cooperative kernel, averaged over blocks, to stderr
        static long long *d_dbg = nullptr;
        const size_t ndbg = (size_t)g * PA_NSTAGE;
        if (!d_dbg) (void)hipMalloc((void **)&d_dbg, (size_t)(1 << 20) * sizeof(long long));
        (void)hipMemsetAsync(d_dbg, 0, ndbg * sizeof(long long), ctx->stream);
        a.dbg = d_dbg;
#endif
        PA_HIP(ctx, (o.assemble ? e->launch_asm : o.cond ? e->launch_cond : split ? e->launch_split : e->launch)(a, g, ctx->stream));
#ifdef PA_STAGE_CLOCK
        {
            std::vector<long long> h(ndbg);
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipMemcpy(h.data(), d_dbg, ndbg * sizeof(long long), hipMemcpyDeviceToHost);
            double sum[PA_NSTAGE] = {0};
            for (int b = 0; b < g; ++b) for (int i = 0; i < PA_NSTAGE; ++i) sum[i] += (double)h[(size_t)b * PA_NSTAGE + i];
            const double iters = (double)m / (64 / e->lanes_per_cell);
            std::fprintf(stderr, "PA_STAGE_CLOCK %s grid %d: clocks per wave pass:", e->name, g);
            for (int i = 0; i < PA_NSTAGE; ++i) std::fprintf(stderr, " s%d=%.0f", i, sum[i] / iters);
            std::fprintf(stderr, "\n");
        }
#endif
    }
    return PA_OK;
}

int pa_local_ops_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t first, size_t n,
                       double *d_oper, double *d_data, double *d_stab, double *d_lc, int32_t *d_info)
{
    LocalOpsOut o;
    o.oper = d_oper; o.data = d_data; o.stab = d_stab; o.lc = d_lc; o.info = d_info;
    return run_local_ops(ctx, di, quad_kind, stab_kind, first, n, o);
}

int pa_condensed_ops_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t first, size_t n,
                           const double *d_rhs, double *d_cond, int32_t *d_info)
{
    if (!d_cond) return PA_ERR_INVALID_ARG;
    if (stab_kind == PA_STAB_NONE) return PA_ERR_INVALID_ARG;      // A_TT = data_TT is singular (constants)
    LocalOpsOut o;
    o.cond = true; o.rhs = d_rhs; o.cond_out = d_cond; o.info = d_info;
    return run_local_ops(ctx, di, quad_kind, stab_kind, first, n, o);
}

int pa_condensed_recover_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t first, size_t n,
                               const double *d_rhs, const double *d_uF, double *d_uT, int32_t *d_info)
{
    if (!d_uF || !d_uT) return PA_ERR_INVALID_ARG;
    if (stab_kind == PA_STAB_NONE) return PA_ERR_INVALID_ARG;
    LocalOpsOut o;
    o.cond = true; o.rhs = d_rhs; o.uF = d_uF; o.uT = d_uT; o.info = d_info;
    return run_local_ops(ctx, di, quad_kind, stab_kind, first, n, o);
}

static int launch_info(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t n, bool cond, pa_launch_info *out)
{
    if (!ctx || !out) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const pa::KernelEntry *e = nullptr;
    int grid = 0;
    const int st = select_kernel(ctx, di, quad_kind, stab_kind, n, &e, &grid, cond);
    if (st != PA_OK) return st;
    out->lanes_per_cell = e->lanes_per_cell;
    out->cells_per_block = 64 / e->lanes_per_cell;
    out->block_threads = 64;
    out->lds_bytes_per_block = cond ? e->lds_bytes_cond : e->lds_bytes;
    out->grid_blocks = grid;
    out->kernel_name = cond ? e->name_cond : e->name;
    return PA_OK;
}

int pa_local_ops_launch_info(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t n, pa_launch_info *out)
{
    return launch_info(ctx, di, quad_kind, stab_kind, n, false, out);
}

int pa_condensed_launch_info(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t n, pa_launch_info *out)
{
    return launch_info(ctx, di, quad_kind, stab_kind, n, true, out);
}

// ---- right-hand sides, quadrature points ---------------------------------------------------
template <int QUAD>
static int launch_rhs(pa_context *ctx, int degree, int qdeg, int nqp, int fn, const double *d_fvals, size_t first,
                      size_t n, double *d_rhs, const int8_t *d_cell_loc, int where)
{
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
#define PA_RHS_CASE(D)                                                                                     \
    case D:                                                                                                \
        hipLaunchKernelGGL((pa::cell_rhs_kernel<D, QUAD>), dim3(grid), dim3(block), 0, ctx->stream, ctx->tab.get(), \
                           ctx->mesh.points, ctx->mesh.ptids, first, n, qdeg, nqp, fn, d_fvals, d_rhs, d_cell_loc, where); \
        break;
    switch (degree) {
        PA_RHS_CASE(0) PA_RHS_CASE(1) PA_RHS_CASE(2) PA_RHS_CASE(3) PA_RHS_CASE(4)
    default: return PA_ERR_INVALID_DEGREE;
    }
#undef PA_RHS_CASE
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

template <int QUAD>
static int launch_project(pa_context *ctx, int degree, int qdeg, int nqp, int fn, const double *d_fvals, size_t first,
                          size_t n, double *d_out, int stride, int32_t *d_info)
{
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
#define PA_PROJ_CASE(D)                                                                                    \
    case D:                                                                                                \
        hipLaunchKernelGGL((pa::cell_project_kernel<D, QUAD>), dim3(grid), dim3(block), 0, ctx->stream, ctx->tab.get(), \
                           ctx->mesh.points, ctx->mesh.ptids, first, n, qdeg, nqp, fn, d_fvals, d_out, stride, d_info); \
        break;
    switch (degree) {
        PA_PROJ_CASE(0) PA_PROJ_CASE(1) PA_PROJ_CASE(2) PA_PROJ_CASE(3) PA_PROJ_CASE(4)
    default: return PA_ERR_INVALID_DEGREE;
    }
#undef PA_PROJ_CASE
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int rhs_quadrature(pa_context *ctx, int qdeg, int quad_kind, int *nqp)
{
    if (quad_kind == PA_QUAD_TENSOR) {
        if (pa::gauss_nodes(qdeg) > 8) return PA_ERR_QUADRATURE;      // tables: closed forms to 5 nodes, golub_welsch's rules to 8
    } else if (quad_kind == PA_QUAD_FAN) {
        if (qdeg > 8) return PA_ERR_QUADRATURE;
    } else return PA_ERR_INVALID_ARG;
    *nqp = pa::cell_qp_count(&ctx->host_tab, quad_kind, qdeg);
    return PA_OK;
}

int cell_rhs(pa_context *ctx, int quad_kind, int degree, int qdeg, int nqp, int fn, const double *d_fvals, size_t first, size_t n,
             double *d_rhs, const int8_t *d_cell_loc, int where)
{
    return quad_kind == PA_QUAD_TENSOR ? launch_rhs<pa::QUAD_TENSOR>(ctx, degree, qdeg, nqp, fn, d_fvals, first, n, d_rhs, d_cell_loc, where)
                                       : launch_rhs<pa::QUAD_FAN>(ctx, degree, qdeg, nqp, fn, d_fvals, first, n, d_rhs, d_cell_loc, where);
}

int pa_dirichlet_data_batch(pa_context *ctx, int face_deg, int fn, const double *d_fvals, double *d_g)
{
    if (!ctx || !d_g || face_deg < 0 || face_deg > 3) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (fn < PA_FN_SAMPLED || fn > PA_FN_ONE || (fn == PA_FN_SAMPLED && !d_fvals)) return PA_ERR_INVALID_ARG;
    const uint32_t nf = (uint32_t)ctx->faces.nfaces_local;
    if (nf == 0) return PA_OK;
    const dim3 grid((nf + 255) / 256), block(256);
#define PA_DD_CASE(FD)                                                                                              \
    case FD:                                                                                                        \
        hipLaunchKernelGGL((pa::dirichlet_data_kernel<FD>), grid, block, 0, ctx->stream, ctx->tab.get(), ctx->mesh.points, \
                           ctx->faces.face_pts.get(), ctx->faces.face_dir.get(), nf, fn, d_fvals, d_g);                                 \
        break;
    switch (face_deg) { PA_DD_CASE(0) PA_DD_CASE(1) PA_DD_CASE(2) PA_DD_CASE(3) }
#undef PA_DD_CASE
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_face_quadrature_points(pa_context *ctx, int face_deg, double *d_xyw)
{
    if (!ctx || !d_xyw || face_deg < 0 || face_deg > 7) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    const uint32_t nf = (uint32_t)ctx->faces.nfaces_local;
    if (nf == 0) return PA_OK;
    hipLaunchKernelGGL(pa::face_qpoints_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, ctx->tab.get(),
                       ctx->mesh.points, ctx->faces.face_pts.get(), nf, face_deg + 1, d_xyw);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_cell_rhs_batch(pa_context *ctx, int degree, int dinc, int quad_kind, int fn, const double *d_fvals,
                      size_t first, size_t n, double *d_rhs)
{
    if (!ctx || !d_rhs || degree < 0 || dinc < 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->mesh.points) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    if (fn < PA_FN_SAMPLED || fn > PA_FN_ONE || (fn == PA_FN_SAMPLED && !d_fvals)) return PA_ERR_INVALID_ARG;
    const int qdeg = 2 * (degree + dinc);                          // utils.hpp:165
    int nqp = 0;
    const int st = rhs_quadrature(ctx, qdeg, quad_kind, &nqp);
    if (st != PA_OK) return st;
    if (n == 0) return PA_OK;
    return cell_rhs(ctx, quad_kind, degree, qdeg, nqp, fn, d_fvals, first, n, d_rhs, nullptr, 0);
}

int pa_project_function_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int dinc, int fn,
                              const double *d_cell_fvals, const double *d_face_fvals, size_t first, size_t n,
                              double *d_out, int32_t *d_info)
{
    if (!ctx || !d_out || dinc < 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->mesh.points) return PA_ERR_NO_MESH;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    if (fn < PA_FN_SAMPLED || fn > PA_FN_ONE || (fn == PA_FN_SAMPLED && (!d_cell_fvals || !d_face_fvals))) return PA_ERR_INVALID_ARG;
    const int qdeg = 2 * (di.cell_deg + dinc);                      // utils.hpp:123,165
    int nqp = 0;
    int st = rhs_quadrature(ctx, qdeg, quad_kind, &nqp);
    if (st != PA_OK) return st;
    const int nfq = di.face_deg + dinc + 1;                         // integrate(msh, fc, 2*(facdeg+di))
    if (nfq > 8) return PA_ERR_QUADRATURE;
    if (n == 0) return PA_OK;
    const int cbs = pa::P2(di.cell_deg), msize = cbs + 4 * (di.face_deg + 1);
    st = quad_kind == PA_QUAD_TENSOR
             ? launch_project<pa::QUAD_TENSOR>(ctx, di.cell_deg, qdeg, nqp, fn, d_cell_fvals, first, n, d_out, msize, d_info)
             : launch_project<pa::QUAD_FAN>(ctx, di.cell_deg, qdeg, nqp, fn, d_cell_fvals, first, n, d_out, msize, d_info);
    if (st != PA_OK) return st;
    const int grid = (int)((4 * n + 255) / 256);
#define PA_FPROJ_CASE(D)                                                                                   \
    case D:                                                                                                \
        hipLaunchKernelGGL((pa::face_project_kernel<D>), dim3(grid), dim3(256), 0, ctx->stream, ctx->tab.get(), ctx->mesh.points, \
                           ctx->faces.face_pts.get(), ctx->faces.cell_faces.get(), first, n, nfq, fn, d_face_fvals, d_out, msize, cbs); \
        break;
    switch (di.face_deg) { PA_FPROJ_CASE(0) PA_FPROJ_CASE(1) PA_FPROJ_CASE(2) PA_FPROJ_CASE(3) }
#undef PA_FPROJ_CASE
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_cell_quadrature_points(pa_context *ctx, int degree, int quad_kind, size_t first, size_t n, double *d_xyw,
                              int32_t *nqp_out)
{
    if (!ctx || degree < 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    int nqp = 0;
    const int st = rhs_quadrature(ctx, degree, quad_kind, &nqp);
    if (st != PA_OK) return st;
    if (nqp_out) *nqp_out = nqp;
    if (!d_xyw) return PA_OK;                                       // size query
    if (!ctx->mesh.points) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    if (n == 0 || nqp == 0) return PA_OK;
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
    if (quad_kind == PA_QUAD_TENSOR)
        hipLaunchKernelGGL((pa::cell_qpoints_kernel<pa::QUAD_TENSOR>), dim3(grid), dim3(block), 0, ctx->stream, ctx->tab.get(),
                           ctx->mesh.points, ctx->mesh.ptids, first, n, degree, nqp, d_xyw);
    else
        hipLaunchKernelGGL((pa::cell_qpoints_kernel<pa::QUAD_FAN>), dim3(grid), dim3(block), 0, ctx->stream, ctx->tab.get(),
                           ctx->mesh.points, ctx->mesh.ptids, first, n, degree, nqp, d_xyw);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

// ---- static condensation -------------------------------------------------------------------
int condense(pa_context *ctx, pa_degree_info di, size_t n, const double *d_lc, const double *d_rhs, double *d_S, double *d_g, double *d_rec,
             int32_t *d_info, int packed)
{
    if (!ctx || !d_lc) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    pa_sizes sz;
    const int st = pa_sizes_for(di, PA_QUAD_TENSOR, &sz);
    if (st != PA_OK && st != PA_ERR_QUADRATURE) return st;
    if (n == 0) return PA_OK;
#define PA_SC_CASE(CD, FD)                                                                                    \
    if (di.cell_deg == CD && di.face_deg == FD) {                                                             \
        constexpr int G_ = (pa::P2(CD) <= 16 && 4 * (FD + 1) + 1 <= 16) ? 16 : 32;                            \
        const size_t blocks = (n + 64 / G_ - 1) / (64 / G_), resident = (size_t)ctx->num_cus * 16;             \
        const int grid = (int)(blocks < resident ? blocks : resident);                                        \
        hipLaunchKernelGGL((pa::static_condensation_kernel<pa::P2(CD), 4 * (FD + 1), G_>), dim3(grid), dim3(64), 0, \
                           ctx->stream, n, d_lc, d_rhs, d_S, d_g, d_rec, d_info, packed);                     \
        PA_HIP(ctx, hipGetLastError());                                                                       \
        return PA_OK;                                                                                         \
    }
    PA_SC_CASE(1, 0) PA_SC_CASE(0, 0) PA_SC_CASE(2, 1) PA_SC_CASE(1, 1) PA_SC_CASE(0, 1) PA_SC_CASE(3, 2)
    PA_SC_CASE(2, 2) PA_SC_CASE(1, 2) PA_SC_CASE(4, 3) PA_SC_CASE(3, 3) PA_SC_CASE(2, 3)
#undef PA_SC_CASE
    return PA_ERR_INVALID_DEGREE;
}

int pa_static_condensation_batch(pa_context *ctx, pa_degree_info di, size_t n, const double *d_lc, const double *d_rhs,
                                 double *d_S, double *d_g, double *d_rec, int32_t *d_info)
{
    return condense(ctx, di, n, d_lc, d_rhs, d_S, d_g, d_rec, d_info, 0);
}

int pa_static_condensation_packed_batch(pa_context *ctx, pa_degree_info di, size_t n, const double *d_lc,
                                        const double *d_rhs, double *d_Sp, double *d_g, int32_t *d_info)
{
    return condense(ctx, di, n, d_lc, d_rhs, d_Sp, d_g, nullptr, d_info, 1);
}
