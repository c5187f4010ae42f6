// capi_assembly.hip -- the C ABI of the global systems of an uncut mesh: the assembler's triplets and local data, the energy form,
// the condensed (face-only) system, the assembler's own system directly in CSR, and triplets to CSR.  The solvers of those systems
// and the tables of their preconditioners: capi_solver.hip.
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "csr.hpp"
#include "hho_assembly.hpp"

int pa_triplets_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n, const double *d_lc,
                      const double *d_rhs, const double *d_g, int32_t *d_rows, int32_t *d_cols, double *d_vals,
                      int32_t *d_rhs_rows, double *d_rhs_vals)
{
    if (!ctx || !d_lc || !d_rows || !d_cols || !d_vals || !d_rhs_rows || !d_rhs_vals) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    pa_assembler_info info;
    pa_assembler_query(ctx, di, &info);
    if (info.system_size >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // Eigen::Triplet stores int indices
    if (n == 0) return PA_OK;
    pa::TripletArgs a;
    a.cell_faces = ctx->faces.cell_faces.get(); a.face_dir = ctx->faces.face_dir.get(); a.face_compress = ctx->faces.face_compress.get();
    a.g = d_g; a.lc = d_lc; a.rhs = d_rhs; a.first = first; a.n = n;
    a.cell_base = ctx->mesh.cell_base; a.ncells_global = ctx->mesh.ncells_global;
    a.cbs = pa::P2(di.cell_deg); a.fbs = di.face_deg + 1;
    a.rows = d_rows; a.cols = d_cols; a.vals = d_vals; a.rhs_rows = d_rhs_rows; a.rhs_vals = d_rhs_vals;
    const int msize = a.cbs + 4 * a.fbs;
    const size_t shmem = msize * sizeof(double) + msize * sizeof(int32_t);
    const size_t resident = (size_t)ctx->num_cus * 8;
    const int grid = (int)(n < resident ? n : resident);
    hipLaunchKernelGGL(pa::triplets_kernel, dim3(grid), dim3(256), shmem, ctx->stream, a);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

static int take_local(pa_context *ctx, pa_degree_info di, size_t first, size_t n, const double *d_solution,
                      const double *d_g, int expanded, double *d_out)
{
    if (!ctx || !d_solution || !d_out) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    if (n == 0) return PA_OK;
    pa::TakeArgs a;
    a.cell_faces = ctx->faces.cell_faces.get(); a.face_compress = ctx->faces.face_compress.get(); a.g = d_g; a.solution = d_solution;
    a.first = first; a.n = n; a.cell_base = ctx->mesh.cell_base; a.ncells_global = ctx->mesh.ncells_global;
    a.face_base = ctx->faces.face_base; a.cbs = pa::P2(di.cell_deg); a.fbs = di.face_deg + 1; a.expanded = expanded;
    a.out = d_out;
    const size_t total = n * (size_t)(a.cbs + 4 * a.fbs);
    hipLaunchKernelGGL(pa::take_local_data_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, a);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

int pa_take_local_data_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n, const double *d_solution,
                             const double *d_g, double *d_out)
{
    return take_local(ctx, di, first, n, d_solution, d_g, 0, d_out);
}

int pa_obstacle_take_local_data_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                                      const double *d_expanded, double *d_out)
{
    return take_local(ctx, di, first, n, d_expanded, nullptr, 1, d_out);
}

int pa_energy_form_batch(pa_context *ctx, pa_degree_info di, size_t n, const double *d_lc, const double *d_u,
                         const double *d_v, double *d_out)
{
    if (!ctx || !d_lc || !d_u || !d_out) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (n == 0) return PA_OK;
    const int msize = pa::P2(di.cell_deg) + 4 * (di.face_deg + 1);
    const size_t resident = (size_t)ctx->num_cus * 32;
    hipLaunchKernelGGL(pa::energy_form_kernel, dim3((unsigned)(n < resident ? n : resident)), dim3(64), 0, ctx->stream, n, msize,
                       d_lc, d_u, d_v, d_out);
    PA_HIP(ctx, hipGetLastError());
    return PA_OK;
}

// ---- condensed (face-only) system -----------------------------------------------------------------
static pa::CondMesh cond_mesh(const pa_context *ctx)
{
    pa::CondMesh m;
    m.cell_faces = ctx->faces.cell_faces.get(); m.face_compress = ctx->faces.face_compress.get(); m.adj = ctx->cond.adj.get();
    m.sm = ctx->faces.sm; m.structured = ctx->faces.structured;
    return m;
}

// the context's tables as the assemblers take them; `asmb`: the group under construction inside asm_prepare
static pa::FaceSystemView face_system_view(const pa_context *ctx, const pa::CondTables &cond, const pa::AsmTables &asmb)
{
    pa::FaceSystemView v;
    v.cell_faces = ctx->faces.cell_faces.get(); v.face_compress = ctx->faces.face_compress.get();
    v.faces = cond.cfaces.get(); v.lean = cond.cfaces_lean.get(); v.colprefix = cond.prefix.get();
    v.cprefix = asmb.cprefix.get(); v.fprefix = asmb.fprefix.get();
    v.ncells = (uint32_t)ctx->mesh.ncells; v.nown = cond.nown;
    v.total_cols = cond.total_cols; v.cell_faces_total = asmb.cell_faces_total; v.face_cells_total = asmb.face_cells_total;
    return v;
}

pa::FaceSystemView face_system_view(const pa_context *ctx) { return face_system_view(ctx, ctx->cond, ctx->asmb); }

// first compressed id at or after global face `gid` of the generator mesh (the compress table is monotone)
static int32_t sm_first_compress_from(const pa::StructuredMesh &sm, uint32_t gid)
{
    const uint32_t nfaces = sm.Ny * pa::sm_face_row(sm) + sm.Nx;
    for (uint32_t f = gid; f < nfaces; ++f) {
        uint32_t lo, hi; bool d; int32_t comp;
        pa::sm_face_decode(sm, f, lo, hi, d, comp);
        if (!d) return comp;
    }
    return (int32_t)pa::sm_num_other_faces(sm);
}

// symbolic phase, cached per mesh: adjacency, owned faces, their column faces
int cond_prepare(pa_context *ctx)
{
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (ctx->cond.ready()) return PA_OK;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t owned_range, nown; int32_t p0;
    if (ctx->faces.structured) {
        const pa::StructuredMesh &sm = ctx->faces.sm;
        owned_range = (sm.row1 - sm.row0) * pa::sm_face_row(sm);
        p0 = sm_first_compress_from(sm, sm.row0 * pa::sm_face_row(sm));
        const int32_t p1 = sm_first_compress_from(sm, sm.row1 * pa::sm_face_row(sm));
        nown = (uint32_t)(p1 - p0);
    } else {
        owned_range = (uint32_t)ctx->faces.nfaces_local; p0 = 0; nown = (uint32_t)ctx->faces.num_other_faces;
    }
    pa::CondTables c;                                     // held by the context only once it is complete
    PA_HIP(ctx, c.adj.alloc(ctx->faces.nfaces_local * 2));
    PA_HIP(ctx, c.cfaces.alloc((size_t)nown + 1));
    PA_HIP(ctx, c.cfaces_lean.alloc((size_t)nown + 1));
    PA_HIP(ctx, c.ncols.alloc((size_t)nown + 1));
    PA_HIP(ctx, c.prefix.alloc((size_t)nown + 1));
    PA_HIP(ctx, pa::cond_build_tables(ctx->stream, cond_mesh(ctx), (uint32_t)ctx->faces.nfaces_local, (uint32_t)ctx->mesh.ncells, owned_range, p0,
                                      nown, c));
    uint32_t total = 0;
    PA_HIP(ctx, hipMemcpy(&total, c.prefix.get() + nown, sizeof(uint32_t), hipMemcpyDeviceToHost));
    c.nown = nown; c.owned_range = owned_range; c.p0 = p0; c.total_cols = total;
    ctx->cond = std::move(c);
    return PA_OK;
}

// the part of pa_condensed_info a slab's closed forms determine
static void cond_partition_fill(const pa::StructuredMesh &sm, uint64_t fbs, pa_condensed_info *out)
{
    const int32_t p0 = sm_first_compress_from(sm, sm.row0 * pa::sm_face_row(sm));
    const int32_t p1 = sm_first_compress_from(sm, sm.row1 * pa::sm_face_row(sm));
    out->num_other_faces = pa::sm_num_other_faces(sm);
    out->system_size = fbs * out->num_other_faces;
    out->nf = (int32_t)(4 * fbs);
    out->cond_doubles = (int32_t)(4 * fbs * (4 * fbs + 1) / 2 + 4 * fbs);
    out->row_begin = (uint64_t)p0 * fbs;
    out->row_end = (uint64_t)p1 * fbs;
    out->nnz_owned = 0;
    out->halo_cells = sm.row1 < sm.Ny ? sm.Nx : 0;
    out->halo_doubles = (int32_t)(fbs * (4 * fbs + 1));
    out->has_below = sm.row0 > 0 ? 1 : 0;
}

int pa_condensed_partition_info(size_t Nx, size_t Ny, size_t row_begin, size_t row_end, pa_degree_info di, pa_condensed_info *out)
{
    if (!out || !degree_ok(di) || Nx == 0 || Ny == 0 || row_begin >= row_end || row_end > Ny) return PA_ERR_INVALID_ARG;
    if ((Nx + 1) * (Ny + 1) >= ((size_t)1 << 32)) return PA_ERR_INVALID_ARG;
    const pa::StructuredMesh sm = {(uint32_t)Nx, (uint32_t)Ny, (uint32_t)row_begin, (uint32_t)row_end};
    cond_partition_fill(sm, (uint64_t)di.face_deg + 1, out);
    return PA_OK;
}

int pa_condensed_query(pa_context *ctx, pa_degree_info di, pa_condensed_info *out)
{
    if (!ctx || !out || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const int st = cond_prepare(ctx);
    if (st != PA_OK) return st;
    const uint64_t fbs = (uint64_t)di.face_deg + 1;
    out->num_other_faces = ctx->faces.num_other_faces;
    out->system_size = fbs * ctx->faces.num_other_faces;
    out->nf = (int32_t)(4 * fbs);
    out->cond_doubles = (int32_t)(4 * fbs * (4 * fbs + 1) / 2 + 4 * fbs);
    out->row_begin = (uint64_t)ctx->cond.p0 * fbs;
    out->row_end = ((uint64_t)ctx->cond.p0 + ctx->cond.nown) * fbs;
    out->nnz_owned = ctx->cond.total_cols * fbs * fbs;
    out->halo_cells = (ctx->faces.structured && ctx->faces.sm.row1 < ctx->faces.sm.Ny) ? ctx->faces.sm.Nx : 0;
    out->halo_doubles = (int32_t)(fbs * (4 * fbs + 1));
    out->has_below = (ctx->faces.structured && ctx->faces.sm.row0 > 0) ? 1 : 0;
    return PA_OK;
}

int pa_condensed_triplets_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n, const double *d_cond, const double *d_g,
                                int32_t *d_rows, int32_t *d_cols, double *d_vals, int32_t *d_rhs_rows, double *d_rhs_vals)
{
    if (!ctx || !d_cond || !d_rows || !d_cols || !d_vals || !d_rhs_rows || !d_rhs_vals) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    if ((uint64_t)(di.face_deg + 1) * ctx->faces.num_other_faces >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // int triplet indices
    PA_HIP(ctx, hipSetDevice(ctx->device));
    PA_HIP(ctx, pa::cond_triplets(ctx->stream, cond_mesh(ctx), ctx->num_cus, first, n, di.face_deg + 1, d_cond, d_g, d_rows, d_cols,
                                  d_vals, d_rhs_rows, d_rhs_vals));
    return PA_OK;
}

int pa_condensed_csr_pattern(pa_context *ctx, pa_degree_info di, int64_t *d_rowptr, int32_t *d_colind)
{
    if (!ctx || !d_rowptr || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const int st = cond_prepare(ctx);
    if (st != PA_OK) return st;
    if ((uint64_t)(di.face_deg + 1) * ctx->faces.num_other_faces >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // int32 column ids
    PA_HIP(ctx, pa::cond_pattern(ctx->stream, face_system_view(ctx), di.face_deg + 1, d_rowptr, d_colind));
    return PA_OK;
}

int pa_condensed_csr_fill(pa_context *ctx, pa_degree_info di, const double *d_cond, const double *d_g, const double *d_halo_below,
                          double *d_values, double *d_rhs)
{
    if (!ctx || !d_cond || !d_values || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const int st = cond_prepare(ctx);
    if (st != PA_OK) return st;
    if (ctx->faces.structured && ctx->faces.sm.row0 > 0 && !d_halo_below) {
        ctx->last_error = "pa_condensed_csr_fill: this slab has a slab below: d_halo_below (pa_condensed_halo_pack of that slab) is required";
        return PA_ERR_INVALID_ARG;
    }
    PA_HIP(ctx, hipSetDevice(ctx->device));
    PA_HIP(ctx, pa::cond_fill(ctx->stream, face_system_view(ctx), di.face_deg + 1, d_cond, d_g, d_halo_below, d_values, d_rhs));
    return PA_OK;
}

// ---- the assembler's own system (cell + face unknowns) directly in CSR: assembler_csr.hip ---------------------------
int asm_prepare(pa_context *ctx)
{
    const int st = cond_prepare(ctx);
    if (st != PA_OK) return st;
    if (ctx->faces.structured && (ctx->faces.sm.row0 != 0 || ctx->faces.sm.row1 != ctx->faces.sm.Ny)) {
        ctx->last_error = "pa_assembler_csr_*: whole-mesh contexts only (a slab assembles the face-only system: pa_condensed_*)";
        return PA_ERR_INVALID_ARG;
    }
    if (ctx->asmb.ready()) return PA_OK;
    const uint32_t nc = (uint32_t)ctx->mesh.ncells, nown = ctx->cond.nown;
    pa::AsmTables t;                                      // held by the context only once it is complete
    PA_HIP(ctx, t.nfc.alloc((size_t)nc + 1));
    PA_HIP(ctx, t.cprefix.alloc((size_t)nc + 1));
    PA_HIP(ctx, t.nfcell.alloc((size_t)nown + 1));
    PA_HIP(ctx, t.fprefix.alloc((size_t)nown + 1));
    const pa::FaceSystemView v = face_system_view(ctx, ctx->cond, t);
    PA_HIP(ctx, pa::asm_build_tables(ctx->stream, v, t));
    uint32_t a = 0, b = 0;
    PA_HIP(ctx, hipMemcpy(&a, t.cprefix.get() + nc, sizeof(uint32_t), hipMemcpyDeviceToHost));
    PA_HIP(ctx, hipMemcpy(&b, t.fprefix.get() + nown, sizeof(uint32_t), hipMemcpyDeviceToHost));
    // the per-cell scatter table of the fused path
    PA_HIP(ctx, t.scatter.alloc(nc));
    PA_HIP(ctx, pa::asm_build_scatter_table(ctx->stream, v, t.scatter.get()));
    t.cell_faces_total = a; t.face_cells_total = b;
    ctx->asmb = std::move(t);
    return PA_OK;
}

int pa_assembler_csr_query(pa_context *ctx, pa_degree_info di, pa_assembler_csr_info *out)
{
    if (!ctx || !out || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const int st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    const pa::AsmSizes z = pa::asm_sizes(face_system_view(ctx), pa::P2(di.cell_deg), di.face_deg + 1);
    out->nnz = z.nnz; out->nrows = z.nrows;
    return PA_OK;
}

int pa_assembler_csr_pattern(pa_context *ctx, pa_degree_info di, int64_t *d_rowptr, int32_t *d_colind)
{
    if (!ctx || !d_rowptr || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const int st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    const pa::FaceSystemView v = face_system_view(ctx);
    const int cbs = pa::P2(di.cell_deg), fbs = di.face_deg + 1;
    if (pa::asm_sizes(v, cbs, fbs).nrows >= ((uint64_t)1 << 31)) return PA_ERR_INVALID_ARG;      // int32 column ids
    PA_HIP(ctx, pa::asm_pattern(ctx->stream, v, cbs, fbs, d_rowptr, d_colind));
    return PA_OK;
}

int pa_assembler_csr_fill(pa_context *ctx, pa_degree_info di, const double *d_lc, const double *d_rhs, const double *d_g,
                          double *d_values, double *d_RHS)
{
    if (!ctx || !d_lc || !d_values || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const int st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    PA_HIP(ctx, pa::asm_fill(ctx->stream, face_system_view(ctx), pa::P2(di.cell_deg), di.face_deg + 1, d_lc, d_rhs, d_g, d_values, d_RHS));
    return PA_OK;
}

int pa_assembler_csr_assemble(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, const double *d_rhs, const double *d_g,
                              double *d_values, double *d_RHS, double *d_lc, int32_t *d_info)
{
    if (!ctx || !d_values) return PA_ERR_INVALID_ARG;
    if (stab_kind == PA_STAB_NONE) return PA_ERR_INVALID_ARG;      // as pa_condensed_ops_batch: its instances carry a stabilization
    (void)hipSetDevice(ctx->device);
    if (!ctx->mesh.points) return PA_ERR_NO_MESH;
    // the refusals of pa_condensed_ops_batch for the pair, before anything is built or written
    const pa::KernelEntry *e = nullptr;
    int grid = 0;
    int st = select_kernel(ctx, di, quad_kind, stab_kind, ctx->mesh.ncells, &e, &grid, true);
    if (st != PA_OK) return st;
    if (!e->launch_asm) return PA_ERR_INVALID_DEGREE;
    st = asm_prepare(ctx);
    if (st != PA_OK) return st;
    PA_HIP(ctx, join_side_stream(ctx));      // cut-cell work still out on the side stream
    const pa::FaceSystemView v = face_system_view(ctx);
    const int cbs = pa::P2(di.cell_deg), fbs = di.face_deg + 1;
    PA_HIP(ctx, pa::asm_zero_accumulated(ctx->stream, v, cbs, fbs, d_values, d_RHS));
    LocalOpsOut o;
    o.cond = true; o.assemble = true; o.rhs = d_rhs; o.lc = d_lc; o.info = d_info;
    o.scatter.tab = ctx->asmb.scatter.get(); o.scatter.g = d_g; o.scatter.values = d_values; o.scatter.RHS = d_RHS;
    o.scatter.cell_nnz = pa::asm_sizes(v, cbs, fbs).cell_nnz; o.scatter.ncells = ctx->mesh.ncells;
    return run_local_ops(ctx, di, quad_kind, stab_kind, 0, ctx->mesh.ncells, o);
}

int pa_condensed_halo_pack(pa_context *ctx, pa_degree_info di, const double *d_cond, const double *d_g, double *d_halo)
{
    if (!ctx || !d_cond || !d_halo || !degree_ok(di)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (!ctx->faces.structured || ctx->faces.sm.row1 >= ctx->faces.sm.Ny) return PA_OK;          // nothing above this slab
    PA_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t Nx = ctx->faces.sm.Nx;
    PA_HIP(ctx, pa::cond_halo_pack(ctx->stream, cond_mesh(ctx), (uint32_t)ctx->mesh.ncells - Nx, Nx, di.face_deg + 1, d_cond, d_g, d_halo));
    return PA_OK;
}

int pa_condensed_take_faces(pa_context *ctx, pa_degree_info di, size_t first, size_t n, const double *d_solution, const double *d_g,
                            double *d_uF)
{
    if (!ctx || !d_solution || !d_uF) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    if (first > ctx->mesh.ncells || n > ctx->mesh.ncells - first) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    PA_HIP(ctx, pa::cond_take_faces(ctx->stream, cond_mesh(ctx), first, n, di.face_deg + 1, d_solution, d_g, d_uF));
    return PA_OK;
}

int pa_condensed_expand_solution(pa_context *ctx, pa_degree_info di, const double *d_uT, const double *d_xF, double *d_full)
{
    if (!ctx || !d_uT || !d_full) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!degree_ok(di)) return PA_ERR_INVALID_DEGREE;
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    PA_HIP(ctx, pa::cond_expand(ctx->stream, ctx->mesh.ncells, ctx->mesh.cell_base, ctx->mesh.ncells_global, pa::P2(di.cell_deg),
                                (size_t)(di.face_deg + 1) * ctx->faces.num_other_faces, d_uT, d_xF, d_full));
    return PA_OK;
}

int pa_csr_from_triplets(pa_context *ctx, size_t nslots, const int32_t *d_rows, const int32_t *d_cols, const double *d_vals,
                         size_t nrows, int64_t *d_rowptr, int32_t *d_colind, double *d_values, size_t *nnz)
{
    if (!ctx || !d_rowptr || (nslots && (!d_rows || !d_cols || !d_vals || !d_colind || !d_values))) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (nslots >= ((size_t)1 << 31) || nrows >= ((size_t)1 << 31)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, pa::csr_from_triplets(ctx->stream, nslots, d_rows, d_cols, d_vals, nrows, d_rowptr, d_colind, d_values, nnz));
    return PA_OK;
}
