// interface_csr.hip -- interface_assembler's global system (apps/cuthho/cuthho_square.cpp:1091-1443) built directly in CSR.
//
// interface_assembler numbers the unknowns in blocks: a cell block of cbs unknowns per uncut cell and two (negative, positive side)
// per cut cell, cell_table[c] being the first (:1142-1150); behind them a face block of fbs unknowns per non-Dirichlet face and two
// per cut face, face_table[F] the first (:1152-1163).  assemble (:1203-1269) pushes msize^2 triplets for an uncut cell, assemble_cut
// (:1271-1354) (2 msize)^2 for a cut cell whose unknowns are [cell-, cell+, faces-, faces+]: faces+ of a cut face is its second
// block, faces+ of an uncut face its only block (:1319).  So an uncut face of a cut cell appears TWICE among the cell's unknowns and
// a face-face entry collects up to four addends from one cut cell, up to eight from its two cells.  finalize (:1437-1441) is
// setFromTriplets: duplicates summed in push order (cells ascending, row-major within a cell), columns sorted.
//
// Here the same matrix comes out of the tables of pa_cut_preprocess without triplets and without a sort.  A row GROUP is one block
// of unknowns; every row of a group has the same columns, a sorted run of whole blocks (UNITS).  The symbolic phase (once per cut
// mesh and face degree) lists, per group, the (at most two) cells that push rows into it with their local row bases, and per unit
// the local column bases in each of those cells (at most two: the faces- / faces+ copies of an uncut face in a cut cell).  The
// numeric phase is a gather: one wavefront per group, lane e = entry e of the group's rows (consecutive lanes write consecutive
// entries), summing its addends cell by cell, local row outer, local column inner -- the push order -- from the first addend, as
// csr_reduce_kernel (csr.hip) does.  Structure and values are bit-identical to pa_csr_from_triplets of pa_interface_triplets_batch's
// slots in cell order (tests/test_gpu_interface_csr.py); the right-hand side is the triplet path's per-row sums added in cell order.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cstdint>

#include "interface_csr.hpp"

namespace pa {

namespace {

constexpr int8_t IFC_LOC_CUT = 2;          // LOC_CUT of cut_host.hpp
constexpr int IFC_MAX_CELL_UNITS = 10;     // a cut cell: 2 cell blocks + 4 faces x 2 blocks
constexpr int IFC_MAX_UNITS = 2 * IFC_MAX_CELL_UNITS;

inline unsigned blocks_for(size_t n) { return (unsigned)(n ? (n + 255) / 256 : 1); }

struct IfcDims {
    int cbs, fbs;
    uint32_t ngroups;
};

// ---- symbolic phase --------------------------------------------------------------------------------------------------
// the two cells of every face (lower id, higher id; equal for a boundary face), and the element of every block
__global__ __launch_bounds__(256) void ifc_init_kernel(IfCsrMesh m, int32_t *fcell, int32_t *slot_cell, int32_t *slot_face)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m.nfaces) { fcell[2 * (size_t)t] = 0x7fffffff; fcell[2 * (size_t)t + 1] = -1; }
    if (t < m.num_all_cells) slot_cell[t] = -1;
    if (t < m.num_other_faces) slot_face[t] = -1;
}

__global__ __launch_bounds__(256) void ifc_adjacency_kernel(IfCsrMesh m, int32_t *fcell, int32_t *slot_cell, int32_t *slot_face)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m.ncells) {
        for (int q = 0; q < 4; ++q) {
            const uint32_t f = m.cell_faces[4 * (size_t)t + q];
            atomicMin(fcell + 2 * (size_t)f, (int32_t)t);
            atomicMax(fcell + 2 * (size_t)f + 1, (int32_t)t);
        }
        const int32_t s = m.cell_table[t];
        const int nb = m.cell_loc[t] == IFC_LOC_CUT ? 2 : 1;
        for (int b = 0; b < nb; ++b)
            if (s >= 0 && (uint32_t)(s + b) < m.num_all_cells) slot_cell[s + b] = (int32_t)t;
    }
    if (t < m.nfaces) {
        const int32_t s = m.face_table[t];
        const int nb = m.face_loc[t] == IFC_LOC_CUT ? 2 : 1;
        for (int b = 0; b < nb; ++b)
            if (s >= 0 && (uint32_t)(s + b) < m.num_other_faces) slot_face[s + b] = (int32_t)t;
    }
}

struct IfcTmp {
    int32_t key;            // block: cell block id, or num_all_cells + face block id
    uint32_t code;          // local column bases in the cell
};

// the blocks a cell's unknowns fall in, ascending: the triplet kernel's index map (cut_interface_device.hpp, :1223-1234, :1291-1321)
// with its Dirichlet slots dropped
__device__ int ifc_cell_units(const IfCsrMesh &m, int cbs, int fbs, int32_t X, IfcTmp *out)
{
    const bool cut = m.cell_loc[X] == IFC_LOC_CUT;
    const int32_t ct = m.cell_table[X];
    int n = 0;
    out[n++] = {ct, ifc_code1(0)};
    if (cut) out[n++] = {ct + 1, ifc_code1(cbs)};
    int32_t ft[4];
    uint32_t fid[4];
    int lf[4], nf = 0;
    for (int q = 0; q < 4; ++q) {
        const uint32_t f = m.cell_faces[4 * (size_t)X + q];
        const int32_t b = m.face_table[f];
        if (b < 0) continue;                                     // Dirichlet face: its slots are dropped
        int p = nf;
        while (p > 0 && ft[p - 1] > b) { ft[p] = ft[p - 1]; fid[p] = fid[p - 1]; lf[p] = lf[p - 1]; --p; }
        ft[p] = b; fid[p] = f; lf[p] = q;
        ++nf;
    }
    const int ncd = cut ? 2 * cbs : cbs;
    for (int s = 0; s < nf; ++s) {
        const int32_t key = (int32_t)m.num_all_cells + ft[s];
        const int j0 = ncd + lf[s] * fbs;
        if (!cut) out[n++] = {key, ifc_code1(j0)};
        else if (m.face_loc[fid[s]] == IFC_LOC_CUT) { out[n++] = {key, ifc_code1(j0)}; out[n++] = {key + 1, ifc_code1(j0 + 4 * fbs)}; }
        else out[n++] = {key, ifc_code2(j0, j0 + 4 * fbs)};      // faces- and faces+ of an uncut face: one block
    }
    return n;
}

// group g: its cells and their local row bases, its units (sorted, positions filled in) and the row length
__device__ int ifc_group(const IfCsrMesh &m, IfcDims d, const int32_t *fcell, const int32_t *slot_cell, const int32_t *slot_face,
                         uint32_t g, IfUnit *u, int32_t cell[2], uint32_t &rcode, uint32_t &R)
{
    uint32_t rc[2] = {0u, 0u};
    int nc = 0;
    cell[0] = cell[1] = -1;
    if (g < m.num_all_cells) {
        const int32_t X = slot_cell[g];
        if (X >= 0) { cell[0] = X; rc[0] = ifc_code1((int)(g - (uint32_t)m.cell_table[X]) * d.cbs); nc = 1; }
    } else {
        const uint32_t q = g - m.num_all_cells;
        const int32_t F = slot_face[q];
        if (F >= 0) {
            const int dup = (int)(q - (uint32_t)m.face_table[F]);
            const bool fcut = m.face_loc[F] == IFC_LOC_CUT;
            const int32_t lo = fcell[2 * (size_t)F], hi = fcell[2 * (size_t)F + 1];
            for (int s = 0; s < 2; ++s) {
                const int32_t X = s == 0 ? lo : (hi != lo ? hi : -1);
                if (X < 0 || (uint32_t)X >= m.ncells) continue;
                int lf = 0;
                for (int qq = 0; qq < 4; ++qq)
                    if (m.cell_faces[4 * (size_t)X + qq] == (uint32_t)F) lf = qq;
                uint32_t code;
                if (m.cell_loc[X] != IFC_LOC_CUT) {
                    if (dup != 0) continue;                      // an uncut cell only sees the first block of a cut face
                    code = ifc_code1(d.cbs + lf * d.fbs);
                } else {
                    const int j0 = 2 * d.cbs + lf * d.fbs;
                    code = fcut ? ifc_code1(dup ? j0 + 4 * d.fbs : j0) : ifc_code2(j0, j0 + 4 * d.fbs);
                }
                cell[nc] = X; rc[nc] = code; ++nc;
            }
        }
    }
    IfcTmp a[IFC_MAX_CELL_UNITS], b[IFC_MAX_CELL_UNITS];
    const int na = nc > 0 ? ifc_cell_units(m, d.cbs, d.fbs, cell[0], a) : 0;
    const int nb = nc > 1 ? ifc_cell_units(m, d.cbs, d.fbs, cell[1], b) : 0;
    int ia = 0, ib = 0, n = 0;
    uint32_t pos = 0;
    while (ia < na || ib < nb) {
        int32_t key;
        uint32_t ca = 0u, cb = 0u;
        if (ib >= nb || (ia < na && a[ia].key < b[ib].key)) { key = a[ia].key; ca = a[ia++].code; }
        else if (ia >= na || b[ib].key < a[ia].key) { key = b[ib].key; cb = b[ib++].code; }
        else { key = a[ia].key; ca = a[ia++].code; cb = b[ib++].code; }       // the face both cells share
        const bool is_cell = (uint32_t)key < m.num_all_cells;
        const uint32_t w = is_cell ? (uint32_t)d.cbs : (uint32_t)d.fbs;
        u[n].gcol = is_cell ? key * d.cbs : (int32_t)m.num_all_cells * d.cbs + (key - (int32_t)m.num_all_cells) * d.fbs;
        u[n].pos = (uint16_t)pos; u[n].width = (uint16_t)w;
        u[n].ccode = ca | (cb << 16);
        pos += w;
        ++n;
    }
    rcode = rc[0] | (rc[1] << 16);
    R = pos;
    return n;
}

__global__ __launch_bounds__(256) void ifc_count_kernel(IfCsrMesh m, IfcDims d, const int32_t *fcell, const int32_t *slot_cell,
                                                        const int32_t *slot_face, uint32_t *ucount, uint64_t *gnnz)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > d.ngroups) return;
    if (g == d.ngroups) { ucount[g] = 0; gnnz[g] = 0; return; }
    IfUnit u[IFC_MAX_UNITS];
    int32_t cell[2];
    uint32_t rcode, R;
    const int n = ifc_group(m, d, fcell, slot_cell, slot_face, g, u, cell, rcode, R);
    ucount[g] = (uint32_t)n;
    gnnz[g] = (uint64_t)R * (uint64_t)(g < m.num_all_cells ? d.cbs : d.fbs);
}

__global__ __launch_bounds__(256) void ifc_write_kernel(IfCsrMesh m, IfcDims d, const int32_t *fcell, const int32_t *slot_cell,
                                                        const int32_t *slot_face, const uint32_t *ustart, const uint64_t *vstart,
                                                        IfGroup *groups, IfUnit *units)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.ngroups) return;
    IfUnit u[IFC_MAX_UNITS];
    IfGroup G;
    uint32_t rcode, R;
    const int n = ifc_group(m, d, fcell, slot_cell, slot_face, g, u, G.cell, rcode, R);
    G.vstart = vstart[g]; G.ustart = ustart[g]; G.nunits = (uint16_t)n; G.R = (uint16_t)R; G.rcode = rcode; G.pad_ = 0;
    groups[g] = G;
    for (int s = 0; s < n; ++s) units[G.ustart + s] = u[s];
}

// ---- pattern: one thread per row -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ifc_pattern_kernel(IfCsrMesh m, IfcDims d, uint64_t nrows, uint64_t nnz, const IfGroup *groups,
                                                          const IfUnit *units, int64_t *rowptr, int32_t *colind)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrows) return;
    if (r == nrows) { rowptr[r] = (int64_t)nnz; return; }
    const uint64_t cell_rows = (uint64_t)m.num_all_cells * d.cbs;
    const uint32_t g = r < cell_rows ? (uint32_t)(r / d.cbs) : m.num_all_cells + (uint32_t)((r - cell_rows) / d.fbs);
    const uint32_t i = r < cell_rows ? (uint32_t)(r % d.cbs) : (uint32_t)((r - cell_rows) % d.fbs);
    const IfGroup G = groups[g];
    const uint64_t start = G.vstart + (uint64_t)i * G.R;
    rowptr[r] = (int64_t)start;
    if (colind == nullptr) return;
    for (int s = 0; s < G.nunits; ++s) {
        const IfUnit U = units[G.ustart + s];
        for (int k = 0; k < U.width; ++k) colind[start + U.pos + k] = U.gcol + k;
    }
}

// ---- numeric phase ---------------------------------------------------------------------------------------------------
struct IfcFillArgs {
    const double *lc, *rhs, *g, *lc_cut, *rhs_cut;
    double *values, *RHS;
};

// the triplet path's sum of local row li of uncut cell X (:1255-1265): rhs minus the Dirichlet columns times the boundary data
__device__ double ifc_uncut_row_sum(const IfCsrMesh &m, IfcDims d, const IfcFillArgs &a, int32_t X, int li)
{
    const int ms = d.cbs + 4 * d.fbs;
    const double *A = a.lc + (size_t)X * ms * ms;
    double s = (li < d.cbs && a.rhs != nullptr) ? a.rhs[(size_t)X * d.cbs + li] : 0.0;
    for (int lf = 0; lf < 4; ++lf) {
        const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
        if (m.face_table[f] >= 0) continue;
        for (int k = 0; k < d.fbs; ++k) {
            const double dd = a.g != nullptr ? a.g[(size_t)f * d.fbs + k] : 0.0;
            s -= A[li + (size_t)(d.cbs + lf * d.fbs + k) * ms] * dd;
        }
    }
    return s;
}

// one wavefront per group, four groups per block
__global__ __launch_bounds__(256) void ifc_fill_kernel(IfCsrMesh m, IfcDims d, const IfGroup *__restrict__ groups,
                                                       const IfUnit *__restrict__ units, IfcFillArgs a)
{
    const uint32_t lane = threadIdx.x % 64u;
    const uint32_t grp = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + threadIdx.x / 64u);
    if (grp >= d.ngroups) return;
    const IfGroup G = groups[grp];
    const int ms = d.cbs + 4 * d.fbs, m2 = 2 * ms;
    const uint32_t nrows = grp < m.num_all_cells ? (uint32_t)d.cbs : (uint32_t)d.fbs;
    const double *L[2] = {a.lc, a.lc};
    int ld[2] = {ms, ms};
    uint32_t rc[2] = {0u, 0u};
    bool cut[2] = {false, false};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int32_t X = G.cell[s];
        if (X < 0) continue;
        cut[s] = m.cell_loc[X] == IFC_LOC_CUT;
        L[s] = cut[s] ? a.lc_cut + (size_t)m.cut_index[X] * m2 * m2 : a.lc + (size_t)X * ms * ms;
        ld[s] = cut[s] ? m2 : ms;
        rc[s] = (G.rcode >> (16 * s)) & 0xffffu;
    }
    const uint32_t R = G.R, total = nrows * R;
    const IfUnit *U = units + G.ustart;
    for (uint32_t e = lane; e < total; e += 64u) {
        const uint32_t i = e / R, pos = e - i * R;
        uint32_t upos = 0, ucode = U[0].ccode;
        for (int u = 1; u < G.nunits; ++u)
            if (pos >= U[u].pos) { upos = U[u].pos; ucode = U[u].ccode; }
        const uint32_t k = pos - upos;
        // all (at most 8) addends loaded first, then summed in push order: cell, local row, local column
        double v[2][2][2];
        bool on[2][2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t cc = (ucode >> (16 * s)) & 0xffffu;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    on[s][r][c] = r < ifc_count(rc[s]) && c < ifc_count(cc);
                    const uint32_t row = (uint32_t)(r == 0 ? ifc_first(rc[s]) : ifc_second(rc[s])) + i;
                    const uint32_t col = (uint32_t)(c == 0 ? ifc_first(cc) : ifc_second(cc)) + k;
                    v[s][r][c] = on[s][r][c] ? L[s][row + (size_t)col * ld[s]] : 0.0;
                }
        }
        double acc = 0.0;
        bool first = true;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    if (on[s][r][c]) { acc = first ? v[s][r][c] : acc + v[s][r][c]; first = false; }
        a.values[G.vstart + e] = acc;
    }
    if (a.RHS != nullptr && lane < nrows) {
        double acc = 0.0;
        bool first = true;
        for (int s = 0; s < 2; ++s) {
            const int32_t X = G.cell[s];
            for (int r = 0; r < ifc_count(rc[s]); ++r) {
                const int li = (r == 0 ? ifc_first(rc[s]) : ifc_second(rc[s])) + (int)lane;
                double w;
                if (cut[s]) {                                    // :1349: no Dirichlet columns on a cut cell (:1304-1305)
                    const size_t cc = (size_t)m.cut_index[X];
                    w = (li < 2 * d.cbs && a.rhs_cut != nullptr) ? a.rhs_cut[cc * 2 * d.cbs + li] : 0.0;
                } else {
                    w = ifc_uncut_row_sum(m, d, a, X, li);
                }
                acc = first ? w : acc + w;
                first = false;
            }
        }
        const uint64_t row = grp < m.num_all_cells ? (uint64_t)grp * d.cbs
                                                   : (uint64_t)m.num_all_cells * d.cbs + (uint64_t)(grp - m.num_all_cells) * d.fbs;
        a.RHS[row + lane] = acc;
    }
}

}  // namespace

void ifcsr_release(IfCsrTables *t)
{
    if (t->groups) (void)hipFree(t->groups);
    if (t->units) (void)hipFree(t->units);
    if (t->cvstart) (void)hipFree(t->cvstart);
    *t = IfCsrTables();
}

hipError_t ifcsr_build(hipStream_t stream, const IfCsrMesh &m, int face_deg, IfCsrTables *t)
{
    ifcsr_release(t);
    const IfcDims d = {(face_deg + 3) * (face_deg + 2) / 2, face_deg + 1, m.num_all_cells + m.num_other_faces};
    const size_t ng = d.ngroups;
    int32_t *fcell = nullptr, *slot_cell = nullptr, *slot_face = nullptr;
    uint32_t *ucount = nullptr, *ustart = nullptr;
    uint64_t *gnnz = nullptr, *vstart = nullptr;
    void *tmp = nullptr;
    IfCsrTables out;
    hipError_t e = hipSuccess;
    auto cleanup = [&]() {
        (void)hipFree(fcell); (void)hipFree(slot_cell); (void)hipFree(slot_face); (void)hipFree(ucount); (void)hipFree(ustart);
        (void)hipFree(gnnz); (void)hipFree(vstart); (void)hipFree(tmp);
    };
#define IFC_TRY(call) do { e = (call); if (e != hipSuccess) { (void)hipStreamSynchronize(stream); cleanup(); ifcsr_release(&out); return e; } } while (0)
    IFC_TRY(hipMalloc((void **)&fcell, 2 * ((size_t)m.nfaces + 1) * sizeof(int32_t)));
    IFC_TRY(hipMalloc((void **)&slot_cell, ((size_t)m.num_all_cells + 1) * sizeof(int32_t)));
    IFC_TRY(hipMalloc((void **)&slot_face, ((size_t)m.num_other_faces + 1) * sizeof(int32_t)));
    IFC_TRY(hipMalloc((void **)&ucount, (ng + 1) * sizeof(uint32_t)));
    IFC_TRY(hipMalloc((void **)&ustart, (ng + 1) * sizeof(uint32_t)));
    IFC_TRY(hipMalloc((void **)&gnnz, (ng + 1) * sizeof(uint64_t)));
    IFC_TRY(hipMalloc((void **)&vstart, (ng + 1) * sizeof(uint64_t)));
    IFC_TRY(hipMalloc((void **)&out.groups, (ng ? ng : 1) * sizeof(IfGroup)));
    size_t top = m.nfaces;
    if (m.num_all_cells > top) top = m.num_all_cells;
    if (m.num_other_faces > top) top = m.num_other_faces;
    if (m.ncells > top) top = m.ncells;
    hipLaunchKernelGGL(ifc_init_kernel, dim3(blocks_for(top)), dim3(256), 0, stream, m, fcell, slot_cell, slot_face);
    hipLaunchKernelGGL(ifc_adjacency_kernel, dim3(blocks_for(top)), dim3(256), 0, stream, m, fcell, slot_cell, slot_face);
    hipLaunchKernelGGL(ifc_count_kernel, dim3(blocks_for(ng + 1)), dim3(256), 0, stream, m, d, fcell, slot_cell, slot_face, ucount, gnnz);
    IFC_TRY(hipGetLastError());
    size_t b1 = 0, b2 = 0;
    IFC_TRY(rocprim::exclusive_scan(nullptr, b1, ucount, ustart, 0u, ng + 1, rocprim::plus<uint32_t>(), stream));
    IFC_TRY(rocprim::exclusive_scan(nullptr, b2, gnnz, vstart, (uint64_t)0, ng + 1, rocprim::plus<uint64_t>(), stream));
    const size_t tb = b1 > b2 ? b1 : b2;
    IFC_TRY(hipMalloc(&tmp, tb ? tb : 1));
    IFC_TRY(rocprim::exclusive_scan(tmp, b1, ucount, ustart, 0u, ng + 1, rocprim::plus<uint32_t>(), stream));
    IFC_TRY(rocprim::exclusive_scan(tmp, b2, gnnz, vstart, (uint64_t)0, ng + 1, rocprim::plus<uint64_t>(), stream));
    uint32_t nunits = 0;
    uint64_t nnz = 0;
    IFC_TRY(hipMemcpyAsync(&nunits, ustart + ng, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    IFC_TRY(hipMemcpyAsync(&nnz, vstart + ng, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    IFC_TRY(hipStreamSynchronize(stream));
    IFC_TRY(hipMalloc((void **)&out.units, (nunits ? nunits : 1) * sizeof(IfUnit)));
    hipLaunchKernelGGL(ifc_write_kernel, dim3(blocks_for(ng)), dim3(256), 0, stream, m, d, fcell, slot_cell, slot_face, ustart, vstart,
                       out.groups, out.units);
    IFC_TRY(hipGetLastError());
    IFC_TRY(hipStreamSynchronize(stream));
#undef IFC_TRY
    cleanup();
    out.face_deg = face_deg;
    out.nrows = (uint64_t)m.num_all_cells * d.cbs + (uint64_t)m.num_other_faces * d.fbs;
    out.nnz = nnz;
    out.ngroups = d.ngroups;
    out.nunits = nunits;
    *t = out;
    return hipSuccess;
}

hipError_t ifcsr_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind)
{
    const IfcDims d = {(t.face_deg + 3) * (t.face_deg + 2) / 2, t.face_deg + 1, t.ngroups};
    hipLaunchKernelGGL(ifc_pattern_kernel, dim3(blocks_for(t.nrows + 1)), dim3(256), 0, stream, m, d, t.nrows, t.nnz, t.groups, t.units,
                       rowptr, colind);
    return hipGetLastError();
}

hipError_t ifcsr_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const double *lc, const double *rhs, const double *g,
                      const double *lc_cut, const double *rhs_cut, double *values, double *RHS)
{
    if (t.ngroups == 0) return hipSuccess;
    const IfcDims d = {(t.face_deg + 3) * (t.face_deg + 2) / 2, t.face_deg + 1, t.ngroups};
    const IfcFillArgs a = {lc, rhs, g, lc_cut, rhs_cut, values, RHS};
    hipLaunchKernelGGL(ifc_fill_kernel, dim3((t.ngroups + 3) / 4), dim3(256), 0, stream, m, d, t.groups, t.units, a);
    return hipGetLastError();
}

}  // namespace pa
