// capi_interface.hip -- the C ABI of the two-sided interface problem: the cut cells' operators of both sides, the
// interface_assembler's system as triplets and in CSR, condensed to the face unknowns with its patch and coarse tables, and by
// row slabs.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "coarse_precond.hpp"
#include "context.hpp"
#include "cut_interface_device.hpp"

// ---- two-sided interface problem -------------------------------------------------------------
static int interface_checks(pa_context *ctx, int face_deg)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (face_deg < 0) return PA_ERR_INVALID_DEGREE;
    if (face_deg > 2) return PA_ERR_QUADRATURE;            // 2*recdeg = 8 selects the empty rules[8]
    return PA_OK;
}

int pa_cut_interface_ops_batch(pa_context *ctx, int face_deg, const pa_level_set *ls, const pa_interface_params *parms,
                               int rhs_fn, double *d_oper, double *d_data, double *d_lc, double *d_rhs, int32_t *d_info)
{
    int st = interface_checks(ctx, face_deg);
    if (st != PA_OK) return st;
    if (!ls || !parms || rhs_fn <= PA_FN_SAMPLED || rhs_fn > PA_FN_ONE) return PA_ERR_INVALID_ARG;
    const size_t ncut = ctx->cut.host->cut_cells.size();
    if (ncut == 0) return PA_OK;
    for (int side = 0; side < 2; ++side) {
        st = ensure_cut_lists(ctx, face_deg, side);
        if (st != PA_OK) return st;
    }
    const int cbs = pa::P2(face_deg + 1), nfd = 4 * (face_deg + 1), ms = cbs + nfd, m2 = 2 * ms;
    double *data = d_data, *stab_n = nullptr, *stab_p = nullptr;      // [data | stab_n | stab_p] when lc is requested
    if (d_lc) {
        // (the scratch lives in the context: a hipMalloc / hipFree pair and a stream synchronisation per call cost more than the
        // kernels of a 512 x 512 mesh's cut cells; everything that touches it is ordered on the context's stream)
        const size_t need = (d_data ? 0 : ncut * (size_t)m2 * m2) + 2 * ncut * (size_t)ms * ms;
        PA_HIP(ctx, ctx->cut.if_scratch.grow(need, ctx->stream));
        double *p = ctx->cut.if_scratch.get();
        if (!d_data) { data = p; p += ncut * (size_t)m2 * m2; }
        stab_n = p; stab_p = p + ncut * (size_t)ms * ms;
        // make_hho_cut_stabilization of both sides through the fictitious-domain kernel (stabilization only: its stages A-E are skipped)
        st = pa_cut_local_ops_batch(ctx, face_deg, ls, PA_LOC_NEGATIVE, PA_FN_ONE, PA_FN_ONE, nullptr, nullptr, stab_n, nullptr, nullptr, nullptr);
        if (st == PA_OK)
            st = pa_cut_local_ops_batch(ctx, face_deg, ls, PA_LOC_POSITIVE, PA_FN_ONE, PA_FN_ONE, nullptr, nullptr, stab_p, nullptr, nullptr, nullptr);
        if (st != PA_OK) return st;
    }
    pa::CutInterfaceArgs a;
    a.points = ctx->mesh.points; a.ptids = ctx->mesh.ptids; a.cut_cells = ctx->cut.cut_cells.get(); a.ncut = (uint32_t)ncut;
    for (int side = 0; side < 2; ++side) {
        a.cell_off[side] = ctx->cut.lists[side].co.get(); a.cell_xyw[side] = ctx->cut.lists[side].cx.get();
        a.fl_xyw[side] = ctx->cut.lists[side].fl.get(); a.fl_cnt[side] = ctx->cut.lists[side].flc.get();
    }
    a.il_off = ctx->cut.lists[0].io.get(); a.il_xyw = ctx->cut.lists[0].ix.get();     // integrate_interface(.., IN_NEGATIVE_SIDE) (:437)
    a.ls = pa::LevelSet{ls->kind, ls->radius, ls->alpha, ls->beta, ls->cut_y};
    a.rhs_fn = rhs_fn; a.kappa[0] = parms->kappa_1; a.kappa[1] = parms->kappa_2; a.eta = parms->eta;
    a.oper = d_oper; a.data = data; a.rhs = d_rhs; a.info = d_info;
    // (46 KB of LDS per block at k = 2: three blocks per compute unit are resident)
    const int grid = (int)(ncut < (size_t)ctx->num_cus * 3 ? ncut : (size_t)ctx->num_cus * 3);
    switch (face_deg) {
    case 0: hipLaunchKernelGGL((pa::cut_interface_kernel<0>), dim3(grid), dim3(64), 0, ctx->stream, a); break;
    case 1: hipLaunchKernelGGL((pa::cut_interface_kernel<1>), dim3(grid), dim3(64), 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL((pa::cut_interface_kernel<2>), dim3(grid), dim3(64), 0, ctx->stream, a); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && d_lc) {
        hipLaunchKernelGGL(pa::cut_interface_lc_kernel, dim3(grid), dim3(256), 0, ctx->stream, (uint32_t)ncut, cbs, nfd,
                           parms->kappa_1, parms->kappa_2, data, stab_n, stab_p, d_lc);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { ctx->last_error = std::string("pa_cut_interface_ops_batch: ") + hipGetErrorString(e); return PA_ERR_HIP; }
    return PA_OK;
}

int pa_cut_interface_uncut_batch(pa_context *ctx, int face_deg, const pa_interface_params *parms, int rhs_fn, double *d_lc,
                                 double *d_rhs, int32_t *d_info)
{
    int st = interface_checks(ctx, face_deg);
    if (st != PA_OK) return st;
    if (!parms || (d_rhs && (rhs_fn <= PA_FN_SAMPLED || rhs_fn > PA_FN_ONE))) return PA_ERR_INVALID_ARG;
    const pa_degree_info di = {face_deg + 1, face_deg, face_deg + 1};
    const size_t n = ctx->mesh.ncells;
    const int ms = pa::P2(face_deg + 1) + 4 * (face_deg + 1), mm = ms * ms;
    if (d_lc) {
        if (parms->kappa_1 == 1.0 && parms->kappa_2 == 1.0) {
            st = pa_local_ops_batch(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, 0, n, nullptr, nullptr, nullptr, d_lc, d_info);
            if (st != PA_OK) return st;
        } else {
            pa::DeviceBuf<double> buf;                    // (freed after the stream has drained, on every path)
            PA_HIP(ctx, buf.alloc(2 * n * (size_t)mm));
            double *scratch = buf.get();
            st = pa_local_ops_batch(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, 0, n, nullptr, scratch, scratch + n * (size_t)mm, nullptr, d_info);
            hipError_t e = hipSuccess;
            if (st == PA_OK) {
                const size_t total = n * (size_t)mm;
                hipLaunchKernelGGL(pa::cut_interface_uncut_lc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, n, mm,
                                   ctx->cut.cell_loc.get(), parms->kappa_1, parms->kappa_2, scratch, scratch + n * (size_t)mm, d_lc);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            }
            if (st != PA_OK) return st;
            PA_HIP(ctx, e);
        }
    }
    if (d_rhs) {
        st = pa_cell_rhs_batch(ctx, face_deg + 1, 0, PA_QUAD_FAN, rhs_fn, nullptr, 0, n, d_rhs);
        if (st != PA_OK) return st;
    }
    return PA_OK;
}

// ---- interface_assembler's system: triplets, CSR (interface_csr.hip) and condensed to the faces (interface_condensed.hip) ----
// the interface numbering is built by pa_cut_preprocess on whole-mesh contexts only
static int if_numbering(pa_context *ctx)
{
    if (ctx->cut.if_cell_table.get()) return PA_OK;
    ctx->last_error = "the interface_assembler's numbering covers the whole mesh: not available on a slab of pa_cut_preprocess_rows";
    return PA_ERR_INVALID_ARG;
}

static pa::IfCsrMesh ifcsr_mesh(const pa_context *ctx)
{
    pa::IfCsrMesh m;
    m.cell_faces = ctx->faces.cell_faces.get(); m.cell_loc = ctx->cut.cell_loc.get(); m.face_loc = ctx->cut.face_loc.get(); m.cut_index = ctx->cut.cut_index.get();
    m.cell_table = ctx->cut.if_cell_table.get(); m.face_table = ctx->cut.if_face_table.get();
    m.ncells = (uint32_t)ctx->mesh.ncells; m.nfaces = (uint32_t)ctx->cut.host->nfaces();
    m.num_all_cells = (uint32_t)ctx->cut.if_num_all_cells; m.num_other_faces = (uint32_t)ctx->cut.if_num_other_faces;
    return m;
}

int pa_interface_assembler_query(pa_context *ctx, int face_deg, pa_interface_info *out)
{
    if (!ctx || !out || face_deg < 0 || face_deg > 3) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (const int st = if_numbering(ctx)) return st;
    out->num_all_cells = ctx->cut.if_num_all_cells;
    out->num_other_faces = ctx->cut.if_num_other_faces;
    out->system_size = (uint64_t)pa::P2(face_deg + 1) * ctx->cut.if_num_all_cells + (uint64_t)(face_deg + 1) * ctx->cut.if_num_other_faces;
    out->ncut = ctx->cut.host->cut_cells.size();
    return PA_OK;
}

// the refusals every entry point of the interface system shares, in this order (cut_arrays: the cut-cell arrays are present or
// not needed)
static int if_refusals(pa_context *ctx, int face_deg, bool cut_arrays)
{
    (void)hipSetDevice(ctx->device);
    if (face_deg < 0 || face_deg > 3) return PA_ERR_INVALID_DEGREE;
    if (!ctx->cut.host || !ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (const int st = if_numbering(ctx)) return st;
    if (ctx->cut.host->cut_cells.size() && !cut_arrays) return PA_ERR_INVALID_ARG;
    pa_interface_info info;
    pa_interface_assembler_query(ctx, face_deg, &info);
    if (info.system_size >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // int32 indices, as Eigen::Triplet's
    return PA_OK;
}

static pa::IfTriplets if_triplets(int32_t *d_rows, int32_t *d_cols, double *d_vals, int32_t *d_rows_cut, int32_t *d_cols_cut,
                                  double *d_vals_cut, int32_t *d_rhs_rows, double *d_rhs_vals, int32_t *d_rhs_rows_cut,
                                  double *d_rhs_vals_cut)
{
    return {d_rows, d_cols, d_vals, d_rows_cut, d_cols_cut, d_vals_cut, d_rhs_rows, d_rhs_vals, d_rhs_rows_cut, d_rhs_vals_cut};
}

int pa_interface_triplets_batch(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_g,
                                const double *d_lc_cut, const double *d_rhs_cut, int32_t *d_rows, int32_t *d_cols,
                                double *d_vals, int32_t *d_rows_cut, int32_t *d_cols_cut, double *d_vals_cut,
                                int32_t *d_rhs_rows, double *d_rhs_vals, int32_t *d_rhs_rows_cut, double *d_rhs_vals_cut)
{
    if (!ctx || !d_lc || !d_rows || !d_cols || !d_vals || !d_rhs_rows || !d_rhs_vals) return PA_ERR_INVALID_ARG;
    const bool cut_arrays = d_lc_cut && d_rows_cut && d_cols_cut && d_vals_cut && d_rhs_rows_cut && d_rhs_vals_cut;
    const int st = if_refusals(ctx, face_deg, cut_arrays);            // no symbolic tables: the triplets need the mesh alone
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcsr_triplets(ctx->stream, ifcsr_mesh(ctx), face_deg, ctx->num_cus * 8, {d_lc, d_rhs, d_g, d_lc_cut, d_rhs_cut},
                                   if_triplets(d_rows, d_cols, d_vals, d_rows_cut, d_cols_cut, d_vals_cut, d_rhs_rows, d_rhs_vals,
                                               d_rhs_rows_cut, d_rhs_vals_cut)));
    return PA_OK;
}

int pa_interface_cell_offsets(pa_context *ctx, int face_deg, int64_t *d_offsets)
{
    if (!ctx || !d_offsets || face_deg < 0 || face_deg > 3) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (const int st = if_numbering(ctx)) return st;
    const pa::CutMeshHost &cm = *ctx->cut.host;
    const size_t nc = cm.ncells();
    const int64_t cbs = pa::P2(face_deg + 1);
    std::vector<int64_t> off(2 * nc);
    int64_t blocks = 0;
    for (size_t c = 0; c < nc; ++c) {                      // :1368-1379
        const bool cut = cm.cell_loc[c] == pa::LOC_CUT;
        off[2 * c] = blocks * cbs;
        off[2 * c + 1] = cut ? (blocks + 1) * cbs : blocks * cbs;
        blocks += cut ? 2 : 1;
    }
    PA_HIP(ctx, hipMemcpyAsync(d_offsets, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PA_OK;
}

// if_refusals, then the side stream joined and the symbolic tables of face_deg built if the context does not hold them
static int ifcsr_prepare(pa_context *ctx, int face_deg, bool cut_arrays)
{
    const int st = if_refusals(ctx, face_deg, cut_arrays);
    if (st != PA_OK) return st;
    PA_HIP(ctx, join_side_stream(ctx));      // cut-cell work still out on the side stream
    if (ctx->cut.ifcsr.t.groups == nullptr || ctx->cut.ifcsr.t.face_deg != face_deg)
        PA_HIP(ctx, pa::ifcsr_build(ctx->stream, ifcsr_mesh(ctx), face_deg, &ctx->cut.ifcsr.t));
    return PA_OK;
}

int pa_interface_csr_query(pa_context *ctx, int face_deg, pa_assembler_csr_info *out)
{
    if (!ctx || !out) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, true);
    if (st != PA_OK) return st;
    out->nrows = ctx->cut.ifcsr.t.nrows;
    out->nnz = ctx->cut.ifcsr.t.nnz;
    return PA_OK;
}

int pa_interface_csr_pattern(pa_context *ctx, int face_deg, int64_t *d_rowptr, int32_t *d_colind)
{
    if (!ctx || !d_rowptr) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, true);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcsr_pattern(ctx->stream, ifcsr_mesh(ctx), ctx->cut.ifcsr.t, d_rowptr, d_colind));
    return PA_OK;
}

int pa_interface_csr_fill(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_g,
                          const double *d_lc_cut, const double *d_rhs_cut, double *d_values, double *d_RHS)
{
    if (!ctx || !d_lc || !d_values) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, d_lc_cut != nullptr);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcsr_fill(ctx->stream, ifcsr_mesh(ctx), ctx->cut.ifcsr.t, {d_lc, d_rhs, d_g, d_lc_cut, d_rhs_cut}, d_values, d_RHS));
    return PA_OK;
}

// ---- condensed to the face unknowns: records and recovery in interface_condensed.hip, the face-only CSR in interface_csr.hip ----
static pa::IfCondArgs ifcond_args(const pa_context *ctx, const double *d_cond, const double *d_cond_cut, const double *d_g)
{
    pa::IfCondArgs a;
    a.cond = d_cond; a.cond_cut = d_cond_cut; a.g = d_g; a.cut_cells = ctx->cut.cut_cells.get();
    a.ncut = (uint32_t)ctx->cut.host->cut_cells.size();
    return a;
}

// the records of the context's cells: the uncut formulas through the plain mesh's static condensation, the cut cells in
// double-double (after `prepare` has let the call through)
static int interface_records(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                             const double *d_rhs_cut, double *d_cond, double *d_cond_cut, int32_t *d_info, int32_t *d_info_cut)
{
    const size_t n = ctx->mesh.ncells, ncut = ctx->cut.host->cut_cells.size();
    const int nf = 4 * (face_deg + 1), ntri = nf * (nf + 1) / 2;
    const pa_degree_info di = {face_deg + 1, face_deg, face_deg + 1};
    // the uncut cells: the plain mesh's static condensation of every row of d_lc (rows of cut cells included, never read back)
    const int sc = condense(ctx, di, n, d_lc, d_rhs, d_cond, d_cond + n * (size_t)ntri, nullptr, d_info, 1);
    if (sc != PA_OK) return sc;
    PA_HIP(ctx, pa::ifcond_info_remap(ctx->stream, n, d_info));
    if (ncut) {
        const size_t blocks = (size_t)ctx->num_cus * 8;
        PA_HIP(ctx, pa::ifcond_cut_records(ctx->stream, face_deg, (int)blocks, (uint32_t)ncut, d_lc_cut, d_rhs_cut, d_cond_cut, d_info_cut));
    }
    return PA_OK;
}

int pa_interface_condensed_query(pa_context *ctx, int face_deg, pa_interface_condensed_info *out)
{
    if (!ctx || !out) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, true);
    if (st != PA_OK) return st;
    const int fbs = face_deg + 1, nf = 4 * fbs, NF = 8 * fbs;
    out->system_size = (uint64_t)fbs * ctx->cut.if_num_other_faces;
    out->nnz = ctx->cut.ifcsr.t.cnnz;
    out->nf = nf;
    out->NF = NF;
    out->cond_doubles = nf * (nf + 1) / 2 + nf;
    out->cond_cut_doubles = NF * (NF + 1) / 2 + NF;
    return PA_OK;
}

int pa_interface_condensed_ops_batch(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                                     const double *d_rhs_cut, double *d_cond, double *d_cond_cut, int32_t *d_info, int32_t *d_info_cut)
{
    if (!ctx || !d_lc || !d_cond) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, d_lc_cut != nullptr && d_cond_cut != nullptr);
    if (st != PA_OK) return st;
    return interface_records(ctx, face_deg, d_lc, d_rhs, d_lc_cut, d_rhs_cut, d_cond, d_cond_cut, d_info, d_info_cut);
}

int pa_interface_condensed_triplets_batch(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                          int32_t *d_rows, int32_t *d_cols, double *d_vals, int32_t *d_rows_cut, int32_t *d_cols_cut,
                                          double *d_vals_cut, int32_t *d_rhs_rows, double *d_rhs_vals, int32_t *d_rhs_rows_cut,
                                          double *d_rhs_vals_cut)
{
    if (!ctx || !d_cond || !d_rows || !d_cols || !d_vals || !d_rhs_rows || !d_rhs_vals) return PA_ERR_INVALID_ARG;
    const bool cut_arrays = d_cond_cut && d_rows_cut && d_cols_cut && d_vals_cut && d_rhs_rows_cut && d_rhs_vals_cut;
    const int st = ifcsr_prepare(ctx, face_deg, cut_arrays);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcond_triplets(ctx->stream, ifcsr_mesh(ctx), face_deg, ctx->num_cus * 8, ifcond_args(ctx, d_cond, d_cond_cut, d_g),
                                    if_triplets(d_rows, d_cols, d_vals, d_rows_cut, d_cols_cut, d_vals_cut, d_rhs_rows, d_rhs_vals,
                                                d_rhs_rows_cut, d_rhs_vals_cut)));
    return PA_OK;
}

int pa_interface_condensed_csr_pattern(pa_context *ctx, int face_deg, int64_t *d_rowptr, int32_t *d_colind)
{
    if (!ctx || !d_rowptr) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, true);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcond_pattern(ctx->stream, ifcsr_mesh(ctx), ctx->cut.ifcsr.t, d_rowptr, d_colind));
    return PA_OK;
}

int pa_interface_condensed_csr_fill(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                    double *d_values, double *d_rhs)
{
    if (!ctx || !d_cond || !d_values) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, d_cond_cut != nullptr);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcond_fill(ctx->stream, ifcsr_mesh(ctx), ctx->cut.ifcsr.t, ifcond_args(ctx, d_cond, d_cond_cut, d_g), d_values, d_rhs));
    return PA_OK;
}

int pa_interface_condensed_recover(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                                   const double *d_rhs_cut, const double *d_g, const double *d_xF, double *d_full)
{
    if (!ctx || !d_lc || !d_xF || !d_full) return PA_ERR_INVALID_ARG;
    const int st = ifcsr_prepare(ctx, face_deg, d_lc_cut != nullptr);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcond_recover(ctx->stream, ifcsr_mesh(ctx), face_deg, ctx->num_cus * 16, ifcond_args(ctx, nullptr, nullptr, d_g), d_lc,
                                   d_rhs, d_lc_cut, d_rhs_cut, d_xF, d_full));
    return PA_OK;
}

// the patch tables of the face-only system: the refusals of pa_interface_csr_* in its order, then the kind and the outputs (with
// `write`), then the side stream joined; counted on the device, written only if the entries fit int32
static int if_patches(pa_context *ctx, int face_deg, int kind, bool write, size_t *npatches, size_t *entries, int64_t *d_patch_ptr,
                      int32_t *d_patch_rows)
{
    const int st = if_refusals(ctx, face_deg, true);
    if (st != PA_OK) return st;
    if (kind != PA_PATCH_FACE && kind != PA_PATCH_CELL) return PA_ERR_INVALID_ARG;
    if (write ? (!d_patch_ptr || (ctx->cut.if_num_other_faces && !d_patch_rows)) : (!npatches || !entries)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, join_side_stream(ctx));      // cut-cell work still out on the side stream
    uint64_t np = 0, ne = 0;
    PA_HIP(ctx, pa::ifcond_patches(ctx->stream, ifcsr_mesh(ctx), face_deg, kind == PA_PATCH_FACE ? pa::IF_PATCH_FACE : pa::IF_PATCH_CELL, &np,
                                   &ne, write ? d_patch_ptr : nullptr, d_patch_rows));
    if (ne >= ((uint64_t)1 << 31)) {                      // int32 slots of pa_patch_precond_*
        ctx->last_error = "pa_interface_condensed_patches: the table has 2^31 entries or more";
        return PA_ERR_INVALID_ARG;
    }
    if (npatches) *npatches = (size_t)np;
    if (entries) *entries = (size_t)ne;
    return PA_OK;
}

int pa_interface_condensed_patches_query(pa_context *ctx, int face_deg, int kind, size_t *npatches, size_t *entries)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return if_patches(ctx, face_deg, kind, false, npatches, entries, nullptr, nullptr);
}

int pa_interface_condensed_patches(pa_context *ctx, int face_deg, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return if_patches(ctx, face_deg, kind, true, nullptr, nullptr, d_patch_ptr, d_patch_rows);
}

// the coarse table of the face-only system: the refusals of pa_interface_csr_* in its order, then H, the parts and the outputs
// (with `write`), then the side stream joined; sized on the device, written only if the columns are within 1..the context's cap (PA_COARSE_MAX_NODES unless set)
static int if_coarse(pa_context *ctx, const char *who, int face_deg, int H, int parts, bool write, size_t *ncoarse, size_t *entries,
                     int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    const int st = if_refusals(ctx, face_deg, true);
    if (st != PA_OK) return st;
    if (H < 1 || (parts != PA_COARSE_ONE && parts != PA_COARSE_BY_SIDE)) return PA_ERR_INVALID_ARG;
    if (write ? (!d_p_ptr || !d_p_cols || !d_p_vals) : (!ncoarse || !entries)) return PA_ERR_INVALID_ARG;
    if (!ctx->faces.structured || !ctx->faces.face_pts.get()) return PA_ERR_NO_MESH;       // (pa_cut_preprocess leaves both)
    PA_HIP(ctx, join_side_stream(ctx));      // cut-cell work still out on the side stream
    const pa::IfCoarseMesh m{ifcsr_mesh(ctx), ctx->faces.sm, ctx->faces.face_pts.get(), parts == PA_COARSE_BY_SIDE ? 1 : 0};
    uint64_t nc = 0, ne = 0;
    const uint64_t cap = ctx->coarse_table_cap;
    PA_HIP(ctx, pa::interface_condensed_coarse(ctx->stream, m, face_deg + 1, H, cap, &nc, &ne, write ? d_p_ptr : nullptr, d_p_cols, d_p_vals));
    if (nc < 1 || nc > cap) return coarse_count_refused(ctx, who, H, nc, cap);
    if (ncoarse) *ncoarse = (size_t)nc;
    if (entries) *entries = (size_t)ne;
    return PA_OK;
}

int pa_interface_condensed_coarse_query(pa_context *ctx, int face_deg, int H, int parts, size_t *ncoarse, size_t *entries)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return if_coarse(ctx, "pa_interface_condensed_coarse_query", face_deg, H, parts, false, ncoarse, entries, nullptr, nullptr, nullptr);
}

int pa_interface_condensed_coarse(pa_context *ctx, int face_deg, int H, int parts, int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return if_coarse(ctx, "pa_interface_condensed_coarse", face_deg, H, parts, true, nullptr, nullptr, d_p_ptr, d_p_cols, d_p_vals);
}

// ---- the face-only system by row slabs (pa_interface_rows_*): a context of pa_cut_preprocess_rows, or of pa_cut_preprocess as
// the one-slab case.  The numbering of the slab comes from the whole-mesh tags every rank holds (interface_rows.hpp). ----
static void ifrows_info_fill(const pa::IfRowsHost &h, int face_deg, uint64_t nnz, pa_interface_rows_info *out)
{
    const uint64_t fbs = (uint64_t)face_deg + 1, nf = 4 * fbs, NF = 8 * fbs;
    const uint64_t rec = nf * (nf + 1) / 2 + nf, rec_cut = NF * (NF + 1) / 2 + NF;
    out->system_size = fbs * h.face_blocks;
    out->row_begin = fbs * (h.fb0 + h.q0);
    out->row_end = fbs * (h.fb0 + h.q1);
    out->nnz_owned = nnz;
    out->col_begin = fbs * h.col_block0;
    out->col_end = fbs * h.col_block1;
    out->cell_block_begin = h.cell_block0;
    out->cell_block_end = h.cell_block1;
    out->nf = (int32_t)nf; out->NF = (int32_t)NF;
    out->cond_doubles = (int32_t)rec; out->cond_cut_doubles = (int32_t)rec_cut;
    out->halo_send_cells = h.ns; out->halo_send_cut = h.nsc;
    out->halo_send_doubles = h.ns * (rec + nf) + h.nsc * rec_cut;
    out->halo_recv_cells = h.nh; out->halo_recv_cut = h.nhc;
    out->halo_recv_doubles = h.nh * (rec + nf) + h.nhc * rec_cut;
}

int pa_interface_rows_partition_info(size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y, const pa_level_set *ls,
                                     int refsteps, size_t row_begin, size_t row_end, int face_deg, pa_interface_rows_info *out)
{
    if (face_deg < 0 || face_deg > 3) return PA_ERR_INVALID_DEGREE;
    if (!out || !ls || refsteps < 0 || refsteps > 10 || (ls->kind != 0 && ls->kind != 1)) return PA_ERR_INVALID_ARG;
    if (Nx == 0 || Ny == 0 || row_begin >= row_end || row_end > Ny || (Nx + 1) * (Ny + 1) >= ((size_t)1 << 32)) return PA_ERR_INVALID_ARG;
    pa::CutMeshHost cm;
    pa::IfRowsHost h;
    try {
        pa::cut_preprocess(cm, (uint32_t)Nx, (uint32_t)Ny, min_x, max_x, min_y, max_y, {ls->kind, ls->radius, ls->alpha, ls->beta, ls->cut_y},
                           refsteps, true);
        pa::if_rows_numbering(cm, (uint32_t)row_begin, (uint32_t)row_end, false, h);
    } catch (const std::exception &) {
        return PA_ERR_INVALID_ARG;
    }
    const uint64_t fbs = (uint64_t)face_deg + 1;
    ifrows_info_fill(h, face_deg, h.nnz_blocks * fbs * fbs, out);
    return PA_OK;
}

static pa::IfCsrMesh ifrows_mesh(const pa_context *ctx)
{
    const auto &r = ctx->cut.ifrows;
    pa::IfCsrMesh m;
    m.cell_faces = r.d.cell_faces.get(); m.cell_loc = r.d.cell_loc.get(); m.face_loc = r.d.face_loc.get(); m.cut_index = r.d.cut_index.get();
    m.cell_table = r.d.cell_table.get(); m.face_table = r.d.face_table.get();
    m.ncells = r.h.ne; m.nfaces = r.h.nfe;
    m.num_all_cells = r.h.num_all_cells; m.num_other_faces = r.h.num_other_faces;
    return m;
}

// the slab alone, by the context's own cell and face ids, blocks counted from the slab's first: what ifcond_recover walks (no face
// blocks to copy)
static pa::IfCsrMesh ifrows_slab_mesh(const pa_context *ctx)
{
    const auto &r = ctx->cut.ifrows;
    pa::IfCsrMesh m;
    m.cell_faces = ctx->faces.cell_faces.get(); m.cell_loc = ctx->cut.cell_loc.get(); m.face_loc = r.d.face_loc.get() + r.h.fshift; m.cut_index = ctx->cut.cut_index.get();
    m.cell_table = r.d.cell_table_slab.get(); m.face_table = r.d.face_table_slab.get();
    m.ncells = (uint32_t)ctx->mesh.ncells; m.nfaces = r.h.nfe - r.h.fshift;
    m.num_all_cells = (uint32_t)(r.h.cell_block1 - r.h.cell_block0); m.num_other_faces = 0;
    return m;
}

// The refusals every pa_interface_rows_* entry point shares, in this order: face degree, no cut mesh, a system of 2^31 unknowns or
// more, the cut-cell arrays missing (cut_arrays: present or not needed) while the slab has cut cells, the halo missing (halo:
// present or not needed) while the slab has a row below.  Then the side stream is joined, and the numbering and the symbolic tables
// of face_deg are built if the context does not hold them.
static int ifrows_prepare(pa_context *ctx, int face_deg, bool cut_arrays, bool halo)
{
    (void)hipSetDevice(ctx->device);
    if (face_deg < 0 || face_deg > 3) return PA_ERR_INVALID_DEGREE;
    if (!ctx->cut.host || !ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    auto &r = ctx->cut.ifrows;
    if (r.h.ne == 0) {                                    // once: the counts stay, the tables go after the upload
        try {
            pa::if_rows_numbering(*ctx->cut.host, ctx->faces.sm.row0, ctx->faces.sm.row1, true, r.h);
        } catch (const std::exception &e) {
            ctx->last_error = std::string("pa_interface_rows: ") + e.what();
            return PA_ERR_INVALID_ARG;
        }
    }
    if ((uint64_t)(face_deg + 1) * r.h.face_blocks >= ((uint64_t)1 << 31)) {       // int32 column ids
        ctx->last_error = "pa_interface_rows: the face-only system has 2^31 unknowns or more";
        return PA_ERR_INVALID_ARG;
    }
    if (r.h.ncut && !cut_arrays) {
        ctx->last_error = "pa_interface_rows: the slab has cut cells: the cut-cell arrays are required";
        return PA_ERR_INVALID_ARG;
    }
    if (r.h.nh && !halo) {
        ctx->last_error = "pa_interface_rows: this slab has a slab below: d_halo_below (pa_interface_rows_halo_pack of that slab) is required";
        return PA_ERR_INVALID_ARG;
    }
    PA_HIP(ctx, join_side_stream(ctx));      // cut-cell work still out on the side stream
    if (!r.ready()) {
        pa::IfRowsArrays d;                               // held by the context only once it is complete
        hipError_t e = hipSuccess;
        auto up = [&](auto &buf, const auto &v) { if (e == hipSuccess) e = buf.upload(v, ctx->stream); };
        up(d.cell_faces, r.h.cell_faces); up(d.cell_loc, r.h.cell_loc); up(d.face_loc, r.h.face_loc); up(d.cut_index, r.h.cut_index);
        up(d.cell_table, r.h.cell_table); up(d.face_table, r.h.face_table);
        up(d.cell_table_slab, r.h.cell_table_slab); up(d.face_table_slab, r.h.face_table_slab);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);       // the host vectors are dropped
        PA_HIP(ctx, e);
        r.d = std::move(d);
        for (auto *v : {&r.h.cut_index, &r.h.cell_table, &r.h.face_table, &r.h.cell_table_slab, &r.h.face_table_slab}) std::vector<int32_t>().swap(*v);
        std::vector<uint32_t>().swap(r.h.cell_faces);
        std::vector<int8_t>().swap(r.h.cell_loc); std::vector<int8_t>().swap(r.h.face_loc);
    }
    if (r.tables.t.groups == nullptr || r.tables.t.face_deg != face_deg) {
        r.tables = pa::IfCsrOwner();                      // the former tables go first: both at once need not fit
        pa::IfCsrOwner t;
        PA_HIP(ctx, pa::ifcsr_build(ctx->stream, ifrows_mesh(ctx), face_deg, &t.t));
        uint64_t v[2] = {0, 0};
        PA_HIP(ctx, hipMemcpy(&v[0], t.t.cvstart + r.h.q0, sizeof(uint64_t), hipMemcpyDeviceToHost));
        PA_HIP(ctx, hipMemcpy(&v[1], t.t.cvstart + r.h.q1, sizeof(uint64_t), hipMemcpyDeviceToHost));
        r.tables = std::move(t);
        r.v0 = v[0]; r.nnz = v[1] - v[0];
    }
    return PA_OK;
}

static pa::IfRowsArgs ifrows_args(const pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                  const double *d_halo_below)
{
    const auto &r = ctx->cut.ifrows;
    pa::IfRowsArgs a;
    a.cond = d_cond; a.cond_cut = d_cond_cut; a.g = d_g; a.halo = d_halo_below;
    a.ncells = r.h.ncells; a.ncut = r.h.ncut; a.nh = r.h.nh; a.nhc = r.h.nhc; a.fshift = r.h.fshift;
    a.q0 = r.h.q0; a.nq = r.h.q1 - r.h.q0;
    a.col0 = (int32_t)((uint64_t)(face_deg + 1) * (r.h.fb0 + r.h.q0));
    a.v0 = r.v0; a.nnz = r.nnz;
    return a;
}

int pa_interface_rows_query(pa_context *ctx, int face_deg, pa_interface_rows_info *out)
{
    if (!ctx || !out) return PA_ERR_INVALID_ARG;
    const int st = ifrows_prepare(ctx, face_deg, true, true);
    if (st != PA_OK) return st;
    ifrows_info_fill(ctx->cut.ifrows.h, face_deg, ctx->cut.ifrows.nnz, out);
    return PA_OK;
}

int pa_interface_rows_ops_batch(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                                const double *d_rhs_cut, double *d_cond, double *d_cond_cut, int32_t *d_info, int32_t *d_info_cut)
{
    if (!ctx || !d_lc || !d_cond) return PA_ERR_INVALID_ARG;
    const int st = ifrows_prepare(ctx, face_deg, d_lc_cut != nullptr && d_cond_cut != nullptr, true);
    if (st != PA_OK) return st;
    return interface_records(ctx, face_deg, d_lc, d_rhs, d_lc_cut, d_rhs_cut, d_cond, d_cond_cut, d_info, d_info_cut);
}

int pa_interface_rows_halo_pack(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                double *d_halo)
{
    if (!ctx || !d_cond || !d_halo) return PA_ERR_INVALID_ARG;
    const int st = ifrows_prepare(ctx, face_deg, d_cond_cut != nullptr, true);
    if (st != PA_OK) return st;
    const pa::IfRowsHost &h = ctx->cut.ifrows.h;
    PA_HIP(ctx, pa::ifrows_halo_pack(ctx->stream, face_deg, ctx->faces.cell_faces.get(), ctx->faces.face_dir.get(), h.ncells, h.ncut, h.ns, h.nsc, d_cond,
                                     d_cond_cut, d_g, d_halo));
    return PA_OK;
}

int pa_interface_rows_csr_pattern(pa_context *ctx, int face_deg, int64_t *d_rowptr, int32_t *d_colind)
{
    if (!ctx || !d_rowptr) return PA_ERR_INVALID_ARG;
    const int st = ifrows_prepare(ctx, face_deg, true, true);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifrows_pattern(ctx->stream, ifrows_mesh(ctx), ctx->cut.ifrows.tables.t, ifrows_args(ctx, face_deg, nullptr, nullptr, nullptr, nullptr),
                                   d_rowptr, d_colind));
    return PA_OK;
}

int pa_interface_rows_csr_fill(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                               const double *d_halo_below, double *d_values, double *d_rhs)
{
    if (!ctx || !d_cond || !d_values) return PA_ERR_INVALID_ARG;
    const int st = ifrows_prepare(ctx, face_deg, d_cond_cut != nullptr, d_halo_below != nullptr);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifrows_fill(ctx->stream, ifrows_mesh(ctx), ctx->cut.ifrows.tables.t,
                                ifrows_args(ctx, face_deg, d_cond, d_cond_cut, d_g, d_halo_below), d_values, d_rhs));
    return PA_OK;
}

int pa_interface_rows_recover(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                              const double *d_rhs_cut, const double *d_g, const double *d_xF, double *d_uT)
{
    if (!ctx || !d_lc || !d_xF || !d_uT) return PA_ERR_INVALID_ARG;
    const int st = ifrows_prepare(ctx, face_deg, d_lc_cut != nullptr, true);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::ifcond_recover(ctx->stream, ifrows_slab_mesh(ctx), face_deg, ctx->num_cus * 16, ifcond_args(ctx, nullptr, nullptr, d_g),
                                   d_lc, d_rhs, d_lc_cut, d_rhs_cut, d_xF, d_uT));
    return PA_OK;
}

// ---- the tables of a slab for pa_conjugated_gradient_rows_patch_coarse: the refusals of pa_interface_rows_* in its order (the
// tables need no operators: neither the cut-cell arrays nor the halo), then the kind / H / parts and the outputs (with `write`);
// counted on the device from the slab's extended tables, written only if they fit ----
static int ifrows_patches(pa_context *ctx, int face_deg, int kind, bool write, size_t *npatches, size_t *entries, int64_t *d_patch_ptr,
                          int32_t *d_patch_rows)
{
    const int st = ifrows_prepare(ctx, face_deg, true, true);
    if (st != PA_OK) return st;
    if (kind != PA_PATCH_FACE && kind != PA_PATCH_CELL) return PA_ERR_INVALID_ARG;
    const pa::IfRowsHost &h = ctx->cut.ifrows.h;
    if (write ? (!d_patch_ptr || (h.q1 > h.q0 && !d_patch_rows)) : (!npatches || !entries)) return PA_ERR_INVALID_ARG;
    uint64_t np = 0, ne = 0;
    PA_HIP(ctx, pa::ifrows_patches(ctx->stream, ifrows_mesh(ctx), h.nh, (int32_t)h.q0, (int32_t)h.q1, (int64_t)h.fb0, face_deg,
                                   kind == PA_PATCH_FACE ? pa::IF_PATCH_FACE : pa::IF_PATCH_CELL, &np, &ne, write ? d_patch_ptr : nullptr,
                                   d_patch_rows));
    if (ne >= ((uint64_t)1 << 31)) {                      // int32 slots of pa_patch_precond_*
        ctx->last_error = "pa_interface_rows_patches: the table has 2^31 entries or more";
        return PA_ERR_INVALID_ARG;
    }
    if (npatches) *npatches = (size_t)np;
    if (entries) *entries = (size_t)ne;
    return PA_OK;
}

int pa_interface_rows_patches_query(pa_context *ctx, int face_deg, int kind, size_t *npatches, size_t *entries)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return ifrows_patches(ctx, face_deg, kind, false, npatches, entries, nullptr, nullptr);
}

int pa_interface_rows_patches(pa_context *ctx, int face_deg, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return ifrows_patches(ctx, face_deg, kind, true, nullptr, nullptr, d_patch_ptr, d_patch_rows);
}

static int ifrows_coarse(pa_context *ctx, const char *who, int face_deg, int H, int parts, bool write, size_t *ncoarse, size_t *entries,
                         int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    const int st = ifrows_prepare(ctx, face_deg, true, true);
    if (st != PA_OK) return st;
    if (H < 1 || (parts != PA_COARSE_ONE && parts != PA_COARSE_BY_SIDE)) return PA_ERR_INVALID_ARG;
    if (write ? (!d_p_ptr || !d_p_cols || !d_p_vals) : (!ncoarse || !entries)) return PA_ERR_INVALID_ARG;
    auto &r = ctx->cut.ifrows;
    const pa::CutMeshHost &cm = *ctx->cut.host;
    if ((uint64_t)(r.h.q1 - r.h.q0) * (face_deg + 1) >= ((uint64_t)1 << 29)) {      // 4 entries a row: below 2^31 (pa_coarse_precond_*'s limit)
        ctx->last_error = std::string(who) + ": the table may have 2^31 entries or more (2^29 owned rows and more)";
        return PA_ERR_INVALID_ARG;
    }
    if (parts == PA_COARSE_BY_SIDE && !r.face_loc_all.get()) {          // the whole mesh's tags: every rank's own preprocessing left them
        pa::DeviceBuf<int8_t> all;
        PA_HIP(ctx, all.upload(cm.face_loc, ctx->stream));
        PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        r.face_loc_all = std::move(all);
    }
    const pa::StructuredMesh sm = ctx->faces.sm;
    pa::IfRowsCoarseMesh m;
    m.im = ifrows_mesh(ctx); m.sm = sm;
    m.face0 = (sm.row0 - (sm.row0 > 0 ? 1u : 0u)) * pa::sm_face_row(sm);
    m.q0 = (int32_t)r.h.q0; m.q1 = (int32_t)r.h.q1;
    m.by_side = parts == PA_COARSE_BY_SIDE ? 1 : 0;
    m.face_loc_all = r.face_loc_all.get(); m.nfaces_all = (uint32_t)cm.nfaces();
    uint64_t nc = 0, ne = 0;
    PA_HIP(ctx, pa::interface_rows_coarse(ctx->stream, m, face_deg + 1, H, &nc, &ne, write ? d_p_ptr : nullptr, d_p_cols, d_p_vals));
    if (nc < 1 || nc > (uint64_t)PA_COARSE_MAX_NODES) return coarse_count_refused(ctx, who, H, nc);
    if (ncoarse) *ncoarse = (size_t)nc;
    if (entries) *entries = (size_t)ne;
    return PA_OK;
}

int pa_interface_rows_coarse_query(pa_context *ctx, int face_deg, int H, int parts, size_t *ncoarse, size_t *entries)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return ifrows_coarse(ctx, "pa_interface_rows_coarse_query", face_deg, H, parts, false, ncoarse, entries, nullptr, nullptr, nullptr);
}

int pa_interface_rows_coarse(pa_context *ctx, int face_deg, int H, int parts, int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    return ifrows_coarse(ctx, "pa_interface_rows_coarse", face_deg, H, parts, true, nullptr, nullptr, d_p_ptr, d_p_cols, d_p_vals);
}
