// capi_cut.hip -- the C ABI of cutHHO on one side of the interface: preprocessing, the cut quadrature lists, the cut cells' local
// operators, the merge into the uncut batches, and the fictitious-domain system in one pass or condensed to its face unknowns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "context.hpp"
#include "cut_device.hpp"
#include "fictdom_condensed.hpp"

// ---- cutHHO -----------------------------------------------------------------------------------
static int cut_preprocess_impl(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                               const pa_level_set *ls, int refsteps, bool displace, size_t row_begin, size_t row_end)
{
    if (!ctx || !ls || refsteps < 0 || refsteps > 10 || (ls->kind != 0 && ls->kind != 1)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    int st = pa_mesh_generate(ctx, Nx, Ny, min_x, max_x, min_y, max_y, row_begin, row_end);
    if (st != PA_OK) return st;
    const bool whole = row_begin == 0 && row_end == Ny;
    pa::CutState cs;                                      // held by the context only once it is complete
    cs.host.reset(new (std::nothrow) pa::CutMeshHost());
    pa::CutMeshHost *cm = cs.host.get();
    if (!cm) return PA_ERR_INVALID_ARG;
    const pa::LevelSet L = {ls->kind, ls->radius, ls->alpha, ls->beta, ls->cut_y};
    try {
        // the host preprocessing always sees the WHOLE mesh (a node is displaced by looking at its neighbours; the tags of a
        // slab's faces and nodes are those of the whole mesh): every rank of a row partition runs the same deterministic pass
        pa::cut_preprocess(*cm, (uint32_t)Nx, (uint32_t)Ny, min_x, max_x, min_y, max_y, L, refsteps, displace);
    } catch (const std::exception &e) {
        ctx->last_error = std::string("cutHHO preprocessing: ") + e.what();
        return PA_ERR_INVALID_ARG;
    }
    const size_t nc_all = cm->ncells(), nc = ctx->mesh.ncells, base = ctx->mesh.cell_base;
    if (!whole) {
        // a slab keeps its own cut cells (global ids on the host, ids relative to the slab on the device) and their polylines
        std::vector<uint32_t> mine;
        std::vector<pa::P2d> ifc;
        for (size_t r = 0; r < cm->cut_cells.size(); ++r) {
            const uint32_t c = cm->cut_cells[r];
            if (c < base || c >= base + nc) continue;
            mine.push_back(c);
            ifc.insert(ifc.end(), cm->iface.begin() + r * cm->nif, cm->iface.begin() + (r + 1) * cm->nif);
        }
        cm->cut_cells.swap(mine);
        cm->iface.swap(ifc);
        cm->cut_index.assign(nc_all, -1);
        for (size_t r = 0; r < cm->cut_cells.size(); ++r) cm->cut_index[cm->cut_cells[r]] = (int32_t)r;
    }
    ctx->cut = pa::CutState();
    const size_t ncut = cm->cut_cells.size();
    std::vector<uint32_t> local_ids(ncut);
    for (size_t r = 0; r < ncut; ++r) local_ids[r] = cm->cut_cells[r] - (uint32_t)base;
    // displaced coordinates of the slab's node rows row_begin .. row_end
    PA_HIP(ctx, hipMemcpyAsync(ctx->mesh.points, cm->pts.data() + 2 * row_begin * (Nx + 1), ctx->mesh.npoints * 2 * sizeof(double),
                               hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, cs.cut_cells.upload(local_ids, ctx->stream));
    PA_HIP(ctx, cs.cell_loc.alloc(nc));
    PA_HIP(ctx, cs.cut_index.alloc(nc));
    PA_HIP(ctx, hipMemcpyAsync(cs.cell_loc.get(), cm->cell_loc.data() + base, nc, hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, hipMemcpyAsync(cs.cut_index.get(), cm->cut_index.data() + base, nc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (!whole) {                // the interface_assembler's tables number the whole mesh: whole-mesh contexts only
        PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->cut = std::move(cs);
        return PA_OK;
    }
    // interface_assembler tables (cuthho_square.cpp:1142-1178): cut cells / cut faces own two blocks, so the
    // first block of an element = its plain (compressed) index + the number of cut elements before it
    const size_t nf = cm->nfaces();
    std::vector<int32_t> cell_table(nc), face_table(nf);
    std::vector<uint32_t> cut_faces;
    for (uint32_t cc : cm->cut_cells) {                     // every cut face belongs to a cut cell
        uint32_t fcs[4];
        cm->cell_face_ids(cc, fcs);
        for (int i = 0; i < 4; ++i)
            if (cm->face_loc[fcs[i]] == pa::LOC_CUT) cut_faces.push_back(fcs[i]);
    }
    std::sort(cut_faces.begin(), cut_faces.end());
    cut_faces.erase(std::unique(cut_faces.begin(), cut_faces.end()), cut_faces.end());
    pa::parallel_ranges(nc, [&](size_t c0, size_t c1) {
        for (size_t c = c0; c < c1; ++c)
            cell_table[c] = (int32_t)(c + (std::lower_bound(cm->cut_cells.begin(), cm->cut_cells.end(), (uint32_t)c) - cm->cut_cells.begin()));
    });
    cs.if_num_all_cells = nc + ncut;
    pa::parallel_ranges(nf, [&](size_t f0, size_t f1) {
        for (uint32_t f = (uint32_t)f0; f < f1; ++f) {
            uint32_t lo, hi; bool dirichlet; int32_t comp;
            pa::sm_face_decode(cm->sm, f, lo, hi, dirichlet, comp);
            face_table[f] = dirichlet ? -1 : comp + (int32_t)(std::lower_bound(cut_faces.begin(), cut_faces.end(), f) - cut_faces.begin());
        }
    });
    cs.if_num_other_faces = pa::sm_num_other_faces(cm->sm) + cut_faces.size();      // cut faces are never on the boundary
    PA_HIP(ctx, cs.face_loc.upload(cm->face_loc, ctx->stream));
    PA_HIP(ctx, cs.if_cell_table.upload(cell_table, ctx->stream));
    PA_HIP(ctx, cs.if_face_table.upload(face_table, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cut = std::move(cs);
    return PA_OK;
}

int pa_cut_preprocess(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                      const pa_level_set *ls, int refsteps)
{
    return cut_preprocess_impl(ctx, Nx, Ny, min_x, max_x, min_y, max_y, ls, refsteps, true, 0, Ny);
}

int pa_cut_preprocess_rows(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                           const pa_level_set *ls, int refsteps, size_t row_begin, size_t row_end)
{
    return cut_preprocess_impl(ctx, Nx, Ny, min_x, max_x, min_y, max_y, ls, refsteps, true, row_begin, row_end);
}

int pa_cut_preprocess_agglomeration(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                                    const pa_level_set *ls, int refsteps)
{
    return cut_preprocess_impl(ctx, Nx, Ny, min_x, max_x, min_y, max_y, ls, refsteps, false, 0, Ny);
}

int pa_cut_agglo_query(pa_context *ctx, int8_t *agglo_set, int32_t *neighbors)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (ctx->mesh.ncells != ctx->cut.host->ncells()) {
        ctx->last_error = "pa_cut_agglo_query: whole-mesh contexts only";
        return PA_ERR_INVALID_ARG;
    }
    if (agglo_set) {
        std::vector<int8_t> a;
        pa::classify_agglomeration(*ctx->cut.host, a);
        std::memcpy(agglo_set, a.data(), a.size());
    }
    if (neighbors) {
        std::vector<int32_t> nb;
        pa::structured_neighbors(ctx->cut.host->sm, nb);
        std::memcpy(neighbors, nb.data(), nb.size() * sizeof(int32_t));
    }
    return PA_OK;
}

int pa_cut_query(pa_context *ctx, size_t *ncut, int8_t *cell_location, int32_t *cut_index)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (ncut) *ncut = ctx->cut.host->cut_cells.size();
    // (the cells of the context: of a slab of pa_cut_preprocess_rows, its own rows)
    if (cell_location) std::memcpy(cell_location, ctx->cut.host->cell_loc.data() + ctx->mesh.cell_base, ctx->mesh.ncells);
    if (cut_index) std::memcpy(cut_index, ctx->cut.host->cut_index.data() + ctx->mesh.cell_base, ctx->mesh.ncells * sizeof(int32_t));
    return PA_OK;
}

// host list building + upload of the cut quadrature of one side: once per (face degree, side)
int ensure_cut_lists(pa_context *ctx, int face_deg, int where)
{
    if (ctx->cut.lists[where].face_deg == face_deg && ctx->cut.lists[where].where == where) return PA_OK;
    pa::CutLists L;
    try {
        pa::build_cut_lists(*ctx->cut.host, ctx->host_tab, face_deg, where, L);
    } catch (const std::invalid_argument &ex) {
        ctx->last_error = ex.what();
        return PA_ERR_QUADRATURE;
    } catch (const std::exception &ex) {
        ctx->last_error = ex.what();
        return PA_ERR_INVALID_ARG;
    }
    ctx->cut.lists[where] = pa::CutListsDev();            // the former lists go first: both at once need not fit
    pa::CutListsDev c;
    hipError_t e = hipSuccess;
    auto up = [&](auto &buf, const auto &v) { if (e == hipSuccess) e = buf.upload(v, ctx->stream); };
    up(c.co, L.cell_off); up(c.io, L.il_off); up(c.ro, L.ir_off);
    up(c.cx, L.cell_xyw); up(c.ix, L.il_xyw); up(c.rx, L.ir_xyw); up(c.fl, L.fl_xyw); up(c.fs, L.fs_xyw);
    up(c.flc, L.fl_cnt); up(c.fsc, L.fs_cnt);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);       // the host vectors go out of scope
    if (e != hipSuccess) { ctx->last_error = std::string("cut lists upload: ") + hipGetErrorString(e); return PA_ERR_HIP; }
    c.face_deg = face_deg; c.where = where;
    ctx->cut.lists[where] = std::move(c);
    return PA_OK;
}

static int cut_local_ops(pa_context *ctx, int face_deg, const pa_level_set *ls, int where, int rhs_fn, int bcs_fn,
                         const double *d_rhs_vals, const double *d_bcs_vals,
                         double *d_oper, double *d_data, double *d_stab, double *d_lc, double *d_rhs, int32_t *d_info)
{
    if (!ctx || !ls || (where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE)) return PA_ERR_INVALID_ARG;
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (face_deg < 0) return PA_ERR_INVALID_DEGREE;
    if (face_deg > 2) return PA_ERR_QUADRATURE;            // 2*recdeg = 8 selects the empty rules[8]
    const size_t ncut = ctx->cut.host->cut_cells.size();
    if (ncut == 0) return PA_OK;
    int st = ensure_cut_lists(ctx, face_deg, where);
    if (st != PA_OK) return st;
    hipError_t e = hipSuccess;
    {
        const auto &c = ctx->cut.lists[where];
        pa::CutArgs a;
        a.tab = ctx->tab.get(); a.points = ctx->mesh.points; a.ptids = ctx->mesh.ptids; a.cut_cells = ctx->cut.cut_cells.get();
        a.ncut = (uint32_t)ncut;
        a.cell_off = c.co.get(); a.il_off = c.io.get(); a.ir_off = c.ro.get();
        a.cell_xyw = c.cx.get(); a.il_xyw = c.ix.get(); a.ir_xyw = c.rx.get(); a.fl_xyw = c.fl.get(); a.fs_xyw = c.fs.get();
        a.fl_cnt = c.flc.get(); a.fs_cnt = c.fsc.get();
        a.ls = pa::LevelSet{ls->kind, ls->radius, ls->alpha, ls->beta, ls->cut_y};
        a.rhs_fn = rhs_fn; a.bcs_fn = bcs_fn; a.rhs_vals = d_rhs_vals; a.bcs_vals = d_bcs_vals;
        a.eta = 5.0;                                                             // cell_eta, cuthho_square.cpp:301-306
        a.oper = d_oper; a.data = d_data; a.stab = d_stab; a.lc = d_lc; a.rhs = d_rhs; a.info = d_info;
        // one wavefront per cut cell and a long serial chain per cell: as many blocks as the chip holds (2 per SIMD),
        // so that a few thousand cut cells take ONE cell's latency, not two or three
        const size_t cap_blocks = (size_t)ctx->num_cus * 8;
        const int grid = (int)(ncut < cap_blocks ? ncut : cap_blocks);
        // With pa_context_set_cut_overlap the kernel goes to the side stream, after everything enqueued on the
        // context's stream so far (the previous merge reads the buffers it writes); pa_cut_merge joins it.
        hipStream_t st_ = ctx->stream;
        if (ctx->cut_overlap && ctx->side) {
            e = hipEventRecord(ctx->ev_main, ctx->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(ctx->side, ctx->ev_main, 0);
            st_ = ctx->side;
        }
        if (e == hipSuccess) {
            switch (face_deg) {
            case 0: hipLaunchKernelGGL((pa::cut_local_ops_kernel<0>), dim3(grid), dim3(64), 0, st_, a); break;
            case 1: hipLaunchKernelGGL((pa::cut_local_ops_kernel<1>), dim3(grid), dim3(64), 0, st_, a); break;
            default: hipLaunchKernelGGL((pa::cut_local_ops_kernel<2>), dim3(grid), dim3(64), 0, st_, a); break;
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess && st_ != ctx->stream) {
            e = hipEventRecord(ctx->ev_side, ctx->side);
            ctx->side_pending = true;
        }
    }
    if (e != hipSuccess) { ctx->last_error = std::string("pa_cut_local_ops_batch: ") + hipGetErrorString(e); return PA_ERR_HIP; }
    return PA_OK;
}

int pa_cut_local_ops_batch(pa_context *ctx, int face_deg, const pa_level_set *ls, int where, int rhs_fn, int bcs_fn,
                           double *d_oper, double *d_data, double *d_stab, double *d_lc, double *d_rhs, int32_t *d_info)
{
    if (rhs_fn <= PA_FN_SAMPLED || rhs_fn > PA_FN_ONE || bcs_fn <= PA_FN_SAMPLED || bcs_fn > PA_FN_ONE) return PA_ERR_INVALID_ARG;
    return cut_local_ops(ctx, face_deg, ls, where, rhs_fn, bcs_fn, nullptr, nullptr, d_oper, d_data, d_stab, d_lc, d_rhs, d_info);
}

int pa_cut_rhs_sampled_batch(pa_context *ctx, int face_deg, const pa_level_set *ls, int where, const double *d_rhs_vals,
                             const double *d_bcs_vals, double *d_rhs)
{
    if (!d_rhs_vals || !d_bcs_vals || !d_rhs) return PA_ERR_INVALID_ARG;
    return cut_local_ops(ctx, face_deg, ls, where, PA_FN_SAMPLED, PA_FN_SAMPLED, d_rhs_vals, d_bcs_vals, nullptr, nullptr, nullptr,
                         nullptr, d_rhs, nullptr);
}

int pa_cut_quadrature_points(pa_context *ctx, int face_deg, int where, int which, uint32_t *h_offsets, double *h_xyw,
                             size_t *count)
{
    if (!ctx || (where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE) || which < 0 || which > 2) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    if (face_deg < 0) return PA_ERR_INVALID_DEGREE;
    if (face_deg > 2) return PA_ERR_QUADRATURE;
    pa::CutLists L;
    try {
        pa::build_cut_lists(*ctx->cut.host, ctx->host_tab, face_deg, where, L);
    } catch (const std::invalid_argument &ex) {
        ctx->last_error = ex.what();
        return PA_ERR_QUADRATURE;
    } catch (const std::exception &ex) {
        ctx->last_error = ex.what();
        return PA_ERR_INVALID_ARG;
    }
    const std::vector<uint32_t> &off = which == 0 ? L.cell_off : which == 1 ? L.il_off : L.ir_off;
    const std::vector<double> &xyw = which == 0 ? L.cell_xyw : which == 1 ? L.il_xyw : L.ir_xyw;
    if (count) *count = xyw.size() / 3;
    if (h_offsets) std::memcpy(h_offsets, off.data(), off.size() * sizeof(uint32_t));
    if (h_xyw) std::memcpy(h_xyw, xyw.data(), xyw.size() * sizeof(double));
    return PA_OK;
}

int pa_cut_query_tags(pa_context *ctx, int8_t *node_location, int8_t *face_location, double *points)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    const pa::CutMeshHost &cm = *ctx->cut.host;
    if (node_location) std::memcpy(node_location, cm.node_loc.data(), cm.npoints());
    if (face_location) std::memcpy(face_location, cm.face_loc.data(), cm.nfaces());
    if (points) std::memcpy(points, cm.pts.data(), cm.pts.size() * sizeof(double));
    return PA_OK;
}

int pa_cut_uncut_rhs_batch(pa_context *ctx, int degree, int where, int fn, double *d_rhs)
{
    if (!ctx || !d_rhs || degree < 0 || (where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host || !ctx->mesh.points || !ctx->cut.cell_loc.get()) return PA_ERR_NO_MESH;
    if (fn <= PA_FN_SAMPLED || fn > PA_FN_ONE) return PA_ERR_INVALID_ARG;
    const int qdeg = 2 * degree;                                   // utils.hpp:165 with di = 0 (cuthho_square.cpp:631)
    int nqp = 0;
    const int st = rhs_quadrature(ctx, qdeg, PA_QUAD_FAN, &nqp);
    if (st != PA_OK) return st;
    const size_t n = ctx->mesh.ncells;
    if (n == 0) return PA_OK;
    return cell_rhs(ctx, PA_QUAD_FAN, degree, qdeg, nqp, fn, nullptr, 0, n, d_rhs, ctx->cut.cell_loc.get(), where);
}

int pa_cut_merge(pa_context *ctx, int face_deg, int where, const double *d_cut_lc, const double *d_cut_rhs, double *d_lc,
                 double *d_rhs)
{
    if (!ctx || face_deg < 0 || face_deg > 2 || (where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    const int cbs = pa::P2(face_deg + 1), ms = cbs + 4 * (face_deg + 1);
    const uint32_t nc = (uint32_t)ctx->mesh.ncells;
    const uint32_t ncut = (uint32_t)ctx->cut.host->cut_cells.size();
    PA_HIP(ctx, join_side_stream(ctx));      // the cut cells' kernel ran on the side stream
    if (d_rhs != nullptr && nc) {
        const size_t total = (size_t)nc * (size_t)cbs;
        hipLaunchKernelGGL(pa::cut_zero_rhs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, total, (uint32_t)cbs,
                           ctx->cut.cell_loc.get(), where, d_rhs);
    }
    if (ncut)
        hipLaunchKernelGGL(pa::cut_merge_cells_kernel, dim3(ncut), dim3(64), 0, ctx->stream, ncut, ctx->cut.cut_cells.get(), ms * ms, cbs, d_cut_lc,
                           d_cut_rhs, d_lc, d_rhs);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_cut_merge_condensed(pa_context *ctx, int face_deg, const double *d_cut_Sp, const double *d_cut_g, double *d_cond)
{
    if (!ctx || !d_cond || face_deg < 0 || face_deg > 2) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host) return PA_ERR_NO_MESH;
    const uint32_t ncut = (uint32_t)ctx->cut.host->cut_cells.size();
    if (ncut == 0) return PA_OK;
    if (!d_cut_Sp || !d_cut_g) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, join_side_stream(ctx));      // the cut cells' kernel ran on the side stream
    const int nf = 4 * (face_deg + 1), ntri = nf * (nf + 1) / 2;
    hipLaunchKernelGGL(pa::cut_merge_condensed_kernel, dim3(ncut), dim3(64), 0, ctx->stream, ncut, ctx->cut.cut_cells.get(), ntri, nf, d_cut_Sp, d_cut_g,
                       d_cond);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

// The fictitious-domain system in one pass: the assembling pass over all cells with the cut cells masked out of its scatter, then
// the cut cells' operators through the same scatter (asm_cut_scatter, assembler_csr.hip).
int pa_fictdom_csr_assemble(pa_context *ctx, int face_deg, int where, const double *d_rhs, const double *d_g, const double *d_cut_lc,
                            const double *d_cut_rhs, double *d_values, double *d_RHS, double *d_lc, int32_t *d_info)
{
    // ---- the refusals, before anything is built or written
    if (!ctx || !d_values || (where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host || !ctx->mesh.points || !ctx->cut.cell_loc.get()) return PA_ERR_NO_MESH;
    if (face_deg < 0) return PA_ERR_INVALID_DEGREE;
    if (face_deg > 2) return PA_ERR_QUADRATURE;            // as the cut entries: 2*recdeg = 8 selects the empty rules[8]
    if (ctx->faces.structured && (ctx->faces.sm.row0 != 0 || ctx->faces.sm.row1 != ctx->faces.sm.Ny)) {      // asm_prepare's refusal, ahead of its tables
        ctx->last_error = "pa_fictdom_csr_assemble: whole-mesh contexts only (pa_cut_preprocess, not pa_cut_preprocess_rows)";
        return PA_ERR_INVALID_ARG;
    }
    const uint32_t ncut = (uint32_t)ctx->cut.host->cut_cells.size();
    if (ncut > 0 && !d_cut_lc) return PA_ERR_INVALID_ARG;
    const pa_degree_info di = {face_deg + 1, face_deg, face_deg + 1};                  // cuthho_square.cpp:871
    const pa::KernelEntry *e = nullptr;
    int grid = 0;
    int st = select_kernel(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, ctx->mesh.ncells, &e, &grid, true);
    if (st != PA_OK) return st;
    if (!e->launch_asm) return PA_ERR_INVALID_DEGREE;
    st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    PA_HIP(ctx, join_side_stream(ctx));      // d_cut_lc may come from the cut kernel on the side stream
    const pa::FaceSystemView v = face_system_view(ctx);
    const int cbs = pa::P2(di.cell_deg), fbs = di.face_deg + 1;
    PA_HIP(ctx, pa::asm_zero_accumulated(ctx->stream, v, cbs, fbs, d_values, d_RHS));
    LocalOpsOut o;
    o.cond = true; o.assemble = true; o.rhs = d_rhs; o.lc = d_lc; o.info = d_info;
    o.scatter.tab = ctx->asmb.scatter.get(); o.scatter.g = d_g; o.scatter.values = d_values; o.scatter.RHS = d_RHS;
    o.scatter.cell_nnz = pa::asm_sizes(v, cbs, fbs).cell_nnz; o.scatter.ncells = ctx->mesh.ncells;
    o.scatter.cell_loc = ctx->cut.cell_loc.get(); o.scatter.where = where;
    st = run_local_ops(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, 0, ctx->mesh.ncells, o);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::asm_cut_scatter(ctx->stream, face_deg, o.scatter, ncut, ctx->cut.cut_cells.get(), d_cut_lc, d_cut_rhs, d_lc));
    return PA_OK;
}

// ---- the same system condensed to its face unknowns: the cut cells' dense work in fictdom_condensed.hip -------------------------
// The refusals of pa_fictdom_csr_assemble in its order (a slab is let through: the work is cell-local), then the side stream
// joined.  `out`: the call's output buffer.
static int fdcond_prepare(pa_context *ctx, int face_deg, int where, const void *out, const double *d_cut_lc, const pa::KernelEntry **e)
{
    if (!ctx || !out || (where != PA_LOC_NEGATIVE && where != PA_LOC_POSITIVE)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->cut.host || !ctx->mesh.points || !ctx->cut.cell_loc.get()) return PA_ERR_NO_MESH;
    if (face_deg < 0) return PA_ERR_INVALID_DEGREE;
    if (face_deg > 2) return PA_ERR_QUADRATURE;            // as the cut entries: 2*recdeg = 8 selects the empty rules[8]
    if (!ctx->cut.host->cut_cells.empty() && !d_cut_lc) return PA_ERR_INVALID_ARG;
    const pa_degree_info di = {face_deg + 1, face_deg, face_deg + 1};                  // cuthho_square.cpp:871
    int grid = 0;
    const int st = select_kernel(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, ctx->mesh.ncells, e, &grid, true);
    if (st != PA_OK) return st;
    PA_HIP(ctx, join_side_stream(ctx));      // d_cut_lc may come from the cut kernel on the side stream
    return PA_OK;
}

int pa_fictdom_condensed_ops_batch(pa_context *ctx, int face_deg, int where, const double *d_rhs, const double *d_cut_lc,
                                   const double *d_cut_rhs, double *d_cond, int32_t *d_info, int32_t *d_info_cut)
{
    const pa::KernelEntry *e = nullptr;
    int st = fdcond_prepare(ctx, face_deg, where, d_cond, d_cut_lc, &e);
    if (st != PA_OK) return st;
    const size_t nc = ctx->mesh.ncells;
    const uint32_t ncut = (uint32_t)ctx->cut.host->cut_cells.size();
    const pa_degree_info di = {face_deg + 1, face_deg, face_deg + 1};
    const int cbs = pa::P2(di.cell_deg);
    // the uncut formulas over every cell (the cut cells' rows are overwritten below), with the masked right-hand side
    PA_HIP(ctx, ctx->cut.fd_scratch.grow(nc * (size_t)cbs, ctx->stream));
    double *rhs = ctx->cut.fd_scratch.get();
    PA_HIP(ctx, pa::fdcond_masked_rhs(ctx->stream, nc, cbs, ctx->cut.cell_loc.get(), where, d_rhs, rhs));
    LocalOpsOut o;
    o.cond = true; o.rhs = rhs; o.cond_out = d_cond; o.info = d_info;
    st = run_local_ops(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, 0, nc, o);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::fdcond_cut_records(ctx->stream, face_deg, ctx->num_cus * 8, ncut, ctx->cut.cut_cells.get(), d_cut_lc, d_cut_rhs, d_cond,
                                       d_info_cut));
    return PA_OK;
}

int pa_fictdom_condensed_recover(pa_context *ctx, int face_deg, int where, const double *d_rhs, const double *d_cut_lc,
                                 const double *d_cut_rhs, const double *d_g, const double *d_xF, double *d_full)
{
    const pa::KernelEntry *e = nullptr;
    int st = fdcond_prepare(ctx, face_deg, where, d_full, d_cut_lc, &e);
    if (st != PA_OK) return st;
    if (!d_xF) return PA_ERR_INVALID_ARG;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    const size_t nc = ctx->mesh.ncells;
    const uint32_t ncut = (uint32_t)ctx->cut.host->cut_cells.size();
    const pa_degree_info di = {face_deg + 1, face_deg, face_deg + 1};
    const int cbs = pa::P2(di.cell_deg), nf = 4 * (face_deg + 1);
    PA_HIP(ctx, ctx->cut.fd_scratch.grow(nc * (size_t)(cbs + nf), ctx->stream));
    double *rhs = ctx->cut.fd_scratch.get(), *uF = rhs + nc * (size_t)cbs;
    double *uT = d_full + ctx->mesh.cell_base * (size_t)cbs;              // the context's cells, cells first
    PA_HIP(ctx, pa::fdcond_masked_rhs(ctx->stream, nc, cbs, ctx->cut.cell_loc.get(), where, d_rhs, rhs));
    st = pa_condensed_take_faces(ctx, di, 0, nc, d_xF, d_g, uF);           // Dirichlet faces: d_g, for cut and uncut cells alike
    if (st != PA_OK) return st;
    LocalOpsOut o;
    o.cond = true; o.rhs = rhs; o.uF = uF; o.uT = uT;
    st = run_local_ops(ctx, di, PA_QUAD_FAN, PA_STAB_NAIVE, 0, nc, o);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::fdcond_cut_recover(ctx->stream, face_deg, ctx->num_cus * 8, ncut, ctx->cut.cut_cells.get(), d_cut_lc, d_cut_rhs, uF, uT));
    PA_HIP(ctx, pa::fdcond_copy(ctx->stream, (size_t)(face_deg + 1) * ctx->faces.num_other_faces, d_xF,
                                d_full + ctx->mesh.ncells_global * (size_t)cbs));
    return PA_OK;
}
