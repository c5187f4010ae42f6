// context.hpp -- struct pa_context and what the capi_*.hip units share.  The context's device memory is held by DeviceBufs,
// grouped by lifetime: a group is dropped by assigning a fresh one, and a "prepare" builds its group in a local variable and
// moves it into the context after the last step that can fail ("Who owns device memory").
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "../../include/proton_amd.h"
#include "assembler_csr.hpp"
#include "condensed.hpp"
#include "cut_host.hpp"
#include "device_buf.hpp"
#include "hho_launch.hpp"
#include "interface_csr.hpp"
#include "interface_rows.hpp"
#include "structured_mesh.hpp"

#define PA_INTERNAL __attribute__((visibility("hidden")))       // shared between the capi units, not exported

#define PA_HIP(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                \
            return PA_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

namespace pa {

// points and cells.  An attached mesh (pa_mesh_attach_device) is the caller's: points / ptids then point at it and the owners
// stay empty.
struct MeshState {
    DeviceBuf<double> own_points;
    DeviceBuf<uint32_t> own_ptids;
    double *points = nullptr;
    uint32_t *ptids = nullptr;
    size_t npoints = 0, ncells = 0, ncells_global = 0, cell_base = 0;
    bool owns = false;
};

// face connectivity for the assembler; sm: the slab of a generator mesh (pa_mesh_generate / pa_cut_preprocess) in closed form
struct FaceState {
    DeviceBuf<uint32_t> cell_faces, face_pts;
    DeviceBuf<uint8_t> face_dir;
    DeviceBuf<int32_t> face_compress;
    size_t nfaces_local = 0, face_base = 0, num_other_faces = 0;
    StructuredMesh sm = {0, 0, 0, 0};
    bool structured = false;
};

// IfCsrTables (interface_csr.hpp) held by a group: released with it.  ifcsr_build frees what *t holds first and leaves it empty
// on failure.
struct IfCsrOwner {
    IfCsrTables t;
    IfCsrOwner() = default;
    IfCsrOwner(IfCsrOwner &&o) noexcept : t(o.t) { o.t = IfCsrTables(); }
    IfCsrOwner &operator=(IfCsrOwner &&o) noexcept
    {
        if (this != &o) { ifcsr_release(&t); t = o.t; o.t = IfCsrTables(); }
        return *this;
    }
    ~IfCsrOwner() { ifcsr_release(&t); }
};

// device copies of the cut quadrature lists of one side, built once per (face degree, side)
struct CutListsDev {
    int face_deg = -1, where = -1;
    DeviceBuf<uint32_t> co, io, ro;
    DeviceBuf<double> cx, ix, rx, fl, fs;
    DeviceBuf<int32_t> flc, fsc;
};

// the numbering of the context's slab with the cell row below it (interface_rows.hpp) on the device and the symbolic tables over
// it (pa_interface_rows_*); fields of their own: if_cell_table stays a whole-mesh context's.  Built on first use.
struct IfRowsArrays {
    DeviceBuf<uint32_t> cell_faces;
    DeviceBuf<int8_t> cell_loc, face_loc;
    DeviceBuf<int32_t> cut_index, cell_table, face_table, cell_table_slab, face_table_slab;
};
struct IfRowsDev {
    IfRowsHost h;                             // the counts (its tables are dropped after the upload)
    IfRowsArrays d;                           // the device copies of h's tables
    bool ready() const { return d.cell_faces.get() != nullptr; }
    IfCsrOwner tables;
    uint64_t v0 = 0, nnz = 0;                 // first entry of the owned rows in the tables' cvstart; entries of the owned rows
    DeviceBuf<int8_t> face_loc_all;           // the WHOLE mesh's face tags (pa_interface_rows_coarse by side), on first use
};

// cutHHO state: host tags and their device copies, and everything built over them
struct CutState {
    std::unique_ptr<CutMeshHost> host;
    CutListsDev lists[2];                     // one slot per side (PA_LOC_NEGATIVE / PA_LOC_POSITIVE)
    DeviceBuf<uint32_t> cut_cells;
    DeviceBuf<int8_t> cell_loc, face_loc;
    DeviceBuf<int32_t> cut_index;
    // interface_assembler tables (cuthho_square.cpp:1137-1185)
    DeviceBuf<int32_t> if_cell_table, if_face_table;
    size_t if_num_all_cells = 0, if_num_other_faces = 0;
    // direct CSR of the interface_assembler's system (interface_csr.hip): row groups and column units of one face degree, built on
    // first use
    IfCsrOwner ifcsr;
    IfRowsDev ifrows;
    // scratch of pa_cut_interface_ops_batch ([data | stab- | stab+] of the cut cells), kept between calls
    DeviceBuf<double> if_scratch;
    // scratch of pa_fictdom_condensed_* (the masked right-hand sides, the cells' face values), kept between calls
    DeviceBuf<double> fd_scratch;
};

// records of the per-cell pre-pass (hho_pre.hpp), grown on demand, reused by every local-operator call
struct RecordBuffer {
    DeviceBuf<double> pre;
    size_t cap_bytes = (size_t)4 << 30;       // pa_context_set_record_cap
};

}  // namespace pa

struct pa_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    int num_cus = 256;
    pa::QuadTables host_tab;
    pa::DeviceBuf<pa::QuadTables> tab;
    // by lifetime.  A new mesh drops cut, then asmb / cond / faces, then mesh; pa_mesh_set_faces drops asmb / cond / faces;
    // pa_cut_preprocess* drops cut; pa_context_trim drops the records.
    pa::MeshState mesh;
    pa::FaceState faces;
    pa::CondTables cond;
    pa::AsmTables asmb;
    pa::CutState cut;
    pa::RecordBuffer records;
    // pa_context_set_coarse_table_cap: the columns up to which pa_condensed_coarse / pa_interface_condensed_coarse write a table
    size_t coarse_table_cap = PA_COARSE_MAX_NODES;
    // pa_context_set_cut_overlap: the cut-cell kernel runs on a side stream next to the uncut cells' kernels
    hipStream_t side = nullptr;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    bool cut_overlap = false, side_pending = false;
    std::string last_error;
};

// ---- shared between the units (each defined in the unit named) --------------------------------------------------------------
// hho_inst.hip: the kernels of one configuration of pa_configs.def
#define PA_CONFIG(cd, fd, q, gmin) extern "C" PA_INTERNAL const pa::KernelEntry *pa_entries_##cd##_##fd##_##q(int *count);
#include "pa_configs.def"
#undef PA_CONFIG

// the degree pairs every entry point with a pa_degree_info accepts (each answers a pair outside with its own status code)
static inline bool degree_ok(pa_degree_info di) { return di.cell_deg >= 0 && di.cell_deg <= 4 && di.face_deg >= 0 && di.face_deg <= 3; }

// capi.hip
// work still out on the side stream (the cut cells' kernel under pa_context_set_cut_overlap) is ordered before what the
// context's stream gets next
PA_INTERNAL hipError_t join_side_stream(pa_context *ctx);
PA_INTERNAL const pa::KernelEntry *find_kernel(int cd, int fd, int quad, int stab, int lanes);
PA_INTERNAL int min_lanes(int cd, int fd, int quad);
PA_INTERNAL bool whole_mesh(const pa_context *ctx);

// capi_local_ops.hip
// outputs of one pass over cells [first, first + n): the local-operator modes write oper / data / stab / lc, the
// condensed mode (cond) reads rhs (and uF) and writes the packed condensed records (or uT)
struct LocalOpsOut {
    double *oper = nullptr, *data = nullptr, *stab = nullptr, *lc = nullptr;
    int32_t *info = nullptr;
    bool cond = false;
    const double *rhs = nullptr, *uF = nullptr;
    double *cond_out = nullptr, *uT = nullptr;
    // the assembling mode (on the condensed mode's instances): rhs in, the CSR arrays of scatter out, lc only if not null
    bool assemble = false;
    pa::AsmScatterArgs scatter = {nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0};
};
PA_INTERNAL int select_kernel(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t n, const pa::KernelEntry **entry,
                              int *grid, bool cond = false);
PA_INTERNAL int run_local_ops(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind, size_t first, size_t n, const LocalOpsOut &o);
PA_INTERNAL int rhs_quadrature(pa_context *ctx, int qdeg, int quad_kind, int *nqp);
// the cell right-hand sides of cells [first, first + n); d_cell_loc given: zero on the cells not on side `where`
PA_INTERNAL int cell_rhs(pa_context *ctx, int quad_kind, int degree, int qdeg, int nqp, int fn, const double *d_fvals, size_t first, size_t n,
                         double *d_rhs, const int8_t *d_cell_loc, int where);
PA_INTERNAL int condense(pa_context *ctx, pa_degree_info di, size_t n, const double *d_lc, const double *d_rhs, double *d_S, double *d_g,
                         double *d_rec, int32_t *d_info, int packed);

// capi_assembly.hip
PA_INTERNAL int cond_prepare(pa_context *ctx);
PA_INTERNAL int asm_prepare(pa_context *ctx);
// the tables of face_system.hpp as the context holds them: the condensed part after cond_prepare, all of it after asm_prepare
PA_INTERNAL pa::FaceSystemView face_system_view(const pa_context *ctx);

// capi_solver.hip
// a coarse table without an interior node or with more than max_columns columns (PA_COARSE_MAX_NODES, or the context's cap for the
// whole-mesh builders): PA_ERR_INVALID_ARG, H and the count in pa_last_error()
PA_INTERNAL int coarse_count_refused(pa_context *ctx, const char *who, int H, uint64_t ncoarse, uint64_t max_columns = PA_COARSE_MAX_NODES);

// capi_cut.hip
PA_INTERNAL int ensure_cut_lists(pa_context *ctx, int face_deg, int where);
