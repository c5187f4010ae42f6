// capi.hip -- the C ABI declared in include/proton_amd.h: the registry of instantiated kernels, sizes, the context and its memory,
// the mesh entry points.  The workloads are in capi_local_ops.hip, capi_assembly.hip, capi_solver.hip, capi_obstacle.hip, capi_cut.hip and
// capi_interface.hip.  Thin: argument validation, kernel selection, launches on the context's stream.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>

#include "context.hpp"
#include "hho_assembly.hpp"
#include "hho_aux.hpp"
#include "quad_tables.hpp"

// ---- registry of instantiated kernels (one getter per translation unit: context.hpp, pa_configs.def) ----
namespace {

typedef const pa::KernelEntry *(*entries_getter)(int *);
struct ConfigRow { int cd, fd, quad, gmin; entries_getter get; };
const ConfigRow k_configs[] = {
#define PA_CONFIG(cd, fd, q, gmin) {cd, fd, q, gmin, &pa_entries_##cd##_##fd##_##q},
#include "pa_configs.def"
#undef PA_CONFIG
};

}  // namespace

const pa::KernelEntry *find_kernel(int cd, int fd, int quad, int stab, int lanes)
{
    for (const ConfigRow &row : k_configs) {
        if (row.cd != cd || row.fd != fd || row.quad != quad) continue;
        int n = 0;
        const pa::KernelEntry *e = row.get(&n);
        for (int i = 0; i < n; ++i)
            if (e[i].stab == stab && e[i].lanes_per_cell == lanes) return &e[i];
    }
    return nullptr;
}

int min_lanes(int cd, int fd, int quad)
{
    for (const ConfigRow &row : k_configs)
        if (row.cd == cd && row.fd == fd && row.quad == quad) return row.gmin;
    return 0;
}

bool whole_mesh(const pa_context *ctx)
{
    return ctx->faces.cell_faces.get() && ctx->mesh.cell_base == 0 && ctx->mesh.ncells == ctx->mesh.ncells_global;
}

// what a new face numbering (pa_mesh_set_faces, any new mesh) drops
static void release_faces(pa_context *ctx)
{
    ctx->asmb = pa::AsmTables();
    ctx->cond = pa::CondTables();
    ctx->faces = pa::FaceState();
}

// what a new mesh drops: the cut state, the faces, the mesh, in this order
static void release_mesh(pa_context *ctx)
{
    ctx->cut = pa::CutState();
    release_faces(ctx);
    ctx->mesh = pa::MeshState();
}

// accessors for comm.hip (internal to the library)
extern "C" __attribute__((visibility("hidden"))) void *pa_context_stream_(pa_context *ctx) { return (void *)ctx->stream; }
extern "C" __attribute__((visibility("hidden"))) int pa_context_device_(pa_context *ctx) { return ctx->device; }

int pa_abi_version(void) { return PA_ABI_VERSION; }

pa_degree_info pa_degree_info_equal(int degree)
{
    pa_degree_info d = {degree, degree, degree + 1};
    return d;
}

pa_degree_info pa_degree_info_make(int cd, int fd, int *fell_back)
{
    // utils.hpp:75-95
    const bool c1 = fd > 0 && (cd == fd - 1 || cd == fd || cd == fd + 1);
    const bool c2 = fd == 0 && (cd == fd || cd == fd + 1);
    pa_degree_info d;
    if (c1 || c2) { d.cell_deg = cd; d.face_deg = fd; d.rec_deg = fd + 1; }
    else { d.cell_deg = fd; d.face_deg = fd; d.rec_deg = fd + 1; }     // "Reverting to equal-order"
    if (fell_back) *fell_back = !(c1 || c2);
    return d;
}

int pa_sizes_for(pa_degree_info di, int quad_kind, pa_sizes *out)
{
    if (!out || di.cell_deg < 0 || di.face_deg < 0 || di.rec_deg != di.face_deg + 1) return PA_ERR_INVALID_ARG;
    if (quad_kind != PA_QUAD_TENSOR && quad_kind != PA_QUAD_FAN) return PA_ERR_INVALID_ARG;
    out->rbs = pa::P2(di.rec_deg);
    out->cbs = pa::P2(di.cell_deg);
    out->fbs = di.face_deg + 1;
    out->msize = out->cbs + 4 * out->fbs;
    out->oper_rows = out->rbs - 1;
    const int qdeg = 2 * di.rec_deg;
    if (quad_kind == PA_QUAD_TENSOR) {
        const int n = pa::gauss_nodes(qdeg);
        if (n > 5) return PA_ERR_QUADRATURE;          // the local-operator kernels are instantiated for recdeg <= 4 (k <= 3: at most 5 nodes)
        out->cell_qps = n * n;
    } else {
        // quadratures.hpp:245-246 throws above 8; degree 8 itself selects the empty rules[8]
        // (quadratures_dunavant.hpp:129): zero points, singular gr_lhs, NaNs in the reference
        if (qdeg > 8 || pa::dunavant_points(qdeg) == 0) return PA_ERR_QUADRATURE;
        out->cell_qps = 4 * pa::dunavant_points(qdeg);
    }
    out->face_qps = pa::gauss_nodes(2 * di.face_deg);
    return PA_OK;
}

int pa_context_create(int device, void *stream, int own_stream, pa_context **out)
{
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    pa_context *ctx = new (std::nothrow) pa_context();
    if (!ctx) return PA_ERR_INVALID_ARG;
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        if (!own_stream) { ctx->stream = (hipStream_t)stream; ctx->owns_stream = false; }
        else { e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking); ctx->owns_stream = true; }
    }
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
        pa::fill_gauss(ctx->host_tab);
        pa::fill_dunavant(ctx->host_tab);
        pa::fill_face_tables(ctx->host_tab);
        e = ctx->tab.alloc(1);
    }
    if (e == hipSuccess) e = hipMemcpy(ctx->tab.get(), &ctx->host_tab, sizeof(pa::QuadTables), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        std::fprintf(stderr, "proton_amd: pa_context_create failed: %s\n", hipGetErrorString(e));
        ctx->tab.reset();
        if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return PA_ERR_HIP;
    }
    *out = ctx;
    return PA_OK;
}

int pa_context_destroy(pa_context *ctx)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    release_mesh(ctx);
    ctx->tab.reset();
    ctx->records.pre.reset();
    if (ctx->ev_main) (void)hipEventDestroy(ctx->ev_main);
    if (ctx->ev_side) (void)hipEventDestroy(ctx->ev_side);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return PA_OK;
}

hipError_t join_side_stream(pa_context *ctx)
{
    if (!ctx->side_pending) return hipSuccess;
    const hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0);
    if (e == hipSuccess) ctx->side_pending = false;
    return e;
}

int pa_context_synchronize(pa_context *ctx)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->side) { PA_HIP(ctx, hipStreamSynchronize(ctx->side)); ctx->side_pending = false; }
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PA_OK;
}

int pa_context_trim(pa_context *ctx)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->records.pre.reset();
    return PA_OK;
}

int pa_context_set_coarse_table_cap(pa_context *ctx, size_t max_columns)
{
    if (!ctx || max_columns > ((size_t)1 << 24)) return PA_ERR_INVALID_ARG;
    ctx->coarse_table_cap = max_columns ? max_columns : (size_t)PA_COARSE_MAX_NODES;
    return PA_OK;
}

int pa_context_set_record_cap(pa_context *ctx, size_t bytes)
{
    if (!ctx || bytes < ((size_t)1 << 20)) return PA_ERR_INVALID_ARG;
    ctx->records.cap_bytes = bytes;
    return PA_OK;
}

int pa_context_set_cut_overlap(pa_context *ctx, int on)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (on && !ctx->side) {
        PA_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        PA_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_main, hipEventDisableTiming));
        PA_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_side, hipEventDisableTiming));
    }
    if (!on) PA_HIP(ctx, join_side_stream(ctx));      // join what is still out on the side stream
    ctx->cut_overlap = on != 0;
    return PA_OK;
}

const char *pa_last_error(pa_context *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int pa_malloc(pa_context *ctx, size_t bytes, void **d_out)
{
    if (!ctx || !d_out) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    PA_HIP(ctx, hipMalloc(d_out, bytes ? bytes : 1));
    return PA_OK;
}

int pa_free(pa_context *ctx, void *d_ptr)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (d_ptr) PA_HIP(ctx, hipFree(d_ptr));
    return PA_OK;
}

int pa_memcpy_h2d(pa_context *ctx, void *d_dst, const void *src, size_t bytes)
{
    if (!ctx || (!d_dst && bytes) || (!src && bytes)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    PA_HIP(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PA_OK;
}

int pa_memcpy_d2h(pa_context *ctx, void *dst, const void *d_src, size_t bytes)
{
    if (!ctx || (!dst && bytes) || (!d_src && bytes)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    PA_HIP(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PA_OK;
}

int pa_memset(pa_context *ctx, void *d_dst, int value, size_t bytes)
{
    if (!ctx || (!d_dst && bytes)) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    PA_HIP(ctx, hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    return PA_OK;
}

// ---- mesh ---------------------------------------------------------------------------------
int pa_mesh_upload(pa_context *ctx, const double *points, size_t npoints, const uint32_t *cell_ptids, size_t ncells)
{
    if (!ctx || !points || !cell_ptids || npoints == 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    for (size_t i = 0; i < 4 * ncells; ++i)
        if (cell_ptids[i] >= npoints) return PA_ERR_INVALID_ARG;      // the kernels gather points[ptid] unchecked
    PA_HIP(ctx, hipSetDevice(ctx->device));
    release_mesh(ctx);
    pa::MeshState m;
    PA_HIP(ctx, m.own_points.alloc(npoints * 2));
    PA_HIP(ctx, m.own_ptids.alloc(ncells * 4));
    PA_HIP(ctx, hipMemcpyAsync(m.own_points.get(), points, npoints * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, hipMemcpyAsync(m.own_ptids.get(), cell_ptids, ncells * 4 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    m.points = m.own_points.get(); m.ptids = m.own_ptids.get(); m.owns = true;
    m.npoints = npoints; m.ncells = m.ncells_global = ncells;
    ctx->mesh = std::move(m);
    return PA_OK;
}

int pa_mesh_attach_device(pa_context *ctx, const double *d_points, size_t npoints, const uint32_t *d_cell_ptids, size_t ncells)
{
    if (!ctx || !d_points || !d_cell_ptids || npoints == 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    release_mesh(ctx);
    ctx->mesh.points = const_cast<double *>(d_points);
    ctx->mesh.ptids = const_cast<uint32_t *>(d_cell_ptids);
    ctx->mesh.npoints = npoints; ctx->mesh.ncells = ctx->mesh.ncells_global = ncells;
    return PA_OK;
}

int pa_mesh_generate(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                     size_t row_begin, size_t row_end)
{
    if (!ctx || Nx == 0 || Ny == 0 || row_begin >= row_end || row_end > Ny) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const size_t rows = row_end - row_begin;
    const size_t np = (Nx + 1) * (rows + 1), nc = Nx * rows;
    if (np >= ((size_t)1 << 32)) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    release_mesh(ctx);
    pa::MeshState m;
    PA_HIP(ctx, m.own_points.alloc(np * 2));
    PA_HIP(ctx, m.own_ptids.alloc(nc * 4));
    const double hx = (max_x - min_x) / (double)Nx, hy = (max_y - min_y) / (double)Ny;    // basic_mesh.hpp:190-196
    const int block = 256;
    const int grid = (int)((np + block - 1) / block < 65535 ? (np + block - 1) / block : 65535);
    hipLaunchKernelGGL(pa::mesh_generate_kernel, dim3(grid), dim3(block), 0, ctx->stream, m.own_points.get(), m.own_ptids.get(),
                       Nx, row_begin, row_end, min_x, hx, min_y, hy);
    PA_HIP(ctx, hipGetLastError());
    m.points = m.own_points.get(); m.ptids = m.own_ptids.get(); m.owns = true;
    m.npoints = np; m.ncells = nc; m.ncells_global = Nx * Ny; m.cell_base = row_begin * Nx;
    // face connectivity in closed form (basic_mesh.hpp:266-297)
    pa::StructuredMesh sm = {(uint32_t)Nx, (uint32_t)Ny, (uint32_t)row_begin, (uint32_t)row_end};
    const uint32_t nfl = pa::sm_faces_local(sm);
    pa::FaceState f;
    PA_HIP(ctx, f.cell_faces.alloc(nc * 4));
    PA_HIP(ctx, f.face_pts.alloc((size_t)nfl * 2));
    PA_HIP(ctx, f.face_dir.alloc(nfl));
    PA_HIP(ctx, f.face_compress.alloc(nfl));
    const uint32_t nthreads = nfl > nc ? nfl : (uint32_t)nc;
    hipLaunchKernelGGL(pa::structured_faces_kernel, dim3((nthreads + 255) / 256), dim3(256), 0, ctx->stream, sm, nfl,
                       f.face_pts.get(), f.face_dir.get(), f.face_compress.get(), (uint32_t)nc, f.cell_faces.get());
    PA_HIP(ctx, hipGetLastError());
    f.nfaces_local = nfl; f.face_base = pa::sm_face_base(sm); f.num_other_faces = pa::sm_num_other_faces(sm);
    f.sm = sm; f.structured = true;
    ctx->mesh = std::move(m);
    ctx->faces = std::move(f);
    return PA_OK;
}

int pa_mesh_set_points(pa_context *ctx, const double *d_points, size_t npoints)
{
    if (!ctx || !d_points) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->mesh.points || !ctx->mesh.owns) return PA_ERR_NO_MESH;
    if (npoints != ctx->mesh.npoints) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipMemcpyAsync(ctx->mesh.points, d_points, npoints * 2 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return PA_OK;
}

int pa_mesh_set_faces(pa_context *ctx, const uint32_t *cell_faces, const uint32_t *face_pts,
                      const uint8_t *face_is_dirichlet, size_t nfaces)
{
    if (!ctx || !cell_faces || !face_pts || !face_is_dirichlet || nfaces == 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->mesh.points) return PA_ERR_NO_MESH;
    for (size_t i = 0; i < 4 * ctx->mesh.ncells; ++i)
        if (cell_faces[i] >= nfaces) return PA_ERR_INVALID_ARG;
    for (size_t i = 0; i < 2 * nfaces; ++i)
        if (face_pts[i] >= ctx->mesh.npoints) return PA_ERR_INVALID_ARG;
    PA_HIP(ctx, hipSetDevice(ctx->device));
    release_faces(ctx);
    // compress table, hho.hpp:313-323
    int32_t *comp = (int32_t *)std::malloc(nfaces * sizeof(int32_t));
    if (!comp) return PA_ERR_INVALID_ARG;
    size_t co = 0;
    for (size_t i = 0; i < nfaces; ++i) comp[i] = face_is_dirichlet[i] ? -1 : (int32_t)co++;
    pa::FaceState f;
    hipError_t e = f.cell_faces.alloc(ctx->mesh.ncells * 4);
    if (e == hipSuccess) e = f.face_pts.alloc(nfaces * 2);
    if (e == hipSuccess) e = f.face_dir.alloc(nfaces);
    if (e == hipSuccess) e = f.face_compress.alloc(nfaces);
    if (e == hipSuccess) e = hipMemcpy(f.cell_faces.get(), cell_faces, ctx->mesh.ncells * 4 * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(f.face_pts.get(), face_pts, nfaces * 2 * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(f.face_dir.get(), face_is_dirichlet, nfaces, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(f.face_compress.get(), comp, nfaces * sizeof(int32_t), hipMemcpyHostToDevice);
    std::free(comp);
    if (e != hipSuccess) { ctx->last_error = std::string("pa_mesh_set_faces: ") + hipGetErrorString(e); return PA_ERR_HIP; }
    f.nfaces_local = nfaces; f.num_other_faces = co;
    ctx->faces = std::move(f);
    return PA_OK;
}

int pa_assembler_query(pa_context *ctx, pa_degree_info di, pa_assembler_info *out)
{
    if (!ctx || !out || di.cell_deg < 0 || di.face_deg < 0) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (!ctx->faces.cell_faces.get()) return PA_ERR_NO_MESH;
    out->ncells_global = ctx->mesh.ncells_global; out->cell_base = ctx->mesh.cell_base;
    out->nfaces_local = ctx->faces.nfaces_local; out->face_base = ctx->faces.face_base;
    out->num_other_faces = ctx->faces.num_other_faces;
    out->system_size = (uint64_t)pa::P2(di.cell_deg) * ctx->mesh.ncells_global + (uint64_t)(di.face_deg + 1) * ctx->faces.num_other_faces;
    return PA_OK;
}

int pa_copy_to_host(pa_context *ctx, void *host_dst, const void *d_src, size_t bytes)
{
    if (!ctx || (bytes && (!host_dst || !d_src))) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (bytes) PA_HIP(ctx, hipMemcpyAsync(host_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PA_OK;
}

int pa_copy_to_device(pa_context *ctx, void *d_dst, const void *host_src, size_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !host_src))) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (bytes) PA_HIP(ctx, hipMemcpyAsync(d_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PA_OK;
}

int pa_mesh_counts(pa_context *ctx, size_t *npoints, size_t *ncells)
{
    if (!ctx) return PA_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (npoints) *npoints = ctx->mesh.npoints;
    if (ncells) *ncells = ctx->mesh.ncells;
    return PA_OK;
}
