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
// csr_reduce_kernel (csr.hip) does.  The right-hand side is the triplet path's per-row sums added in cell order.
//
// One gather, three sources.  The face-only system after static condensation (interface_condensed.hip forms its records) is the same
// numbering without its cell blocks: a face group's row is its cell units followed by its face units (IfGroup::fu0, fpos), and the
// condensed row keeps the face units.  if_pattern_kernel and if_fill_kernel are written once over a Source, which answers what
// differs: the groups and units that take part, where an addend is read (IfFullSource: the column-major local matrices;
// IfCondSource: the packed records), one cell's right-hand-side contribution, and where the row lands.  The push order is
// implemented in if_fill_kernel and nowhere else.  The third source (IfRowsSource) is the face-only system of one slab of cell
// rows: the tables are built over the slab's extended cell range as over a small mesh, the owned face groups take part, a halo
// cell's addends come from the halo the slab below sent, rows start at the slab's first row and columns are global
// (tests/test_gpu_interface_rows.py: the slabs stacked are the whole-mesh face-only system).  Structure and values of the first
// two are bit-identical to pa_csr_from_triplets of their triplet kernel's slots taken in cell order
// (tests/test_gpu_interface_csr.py, tests/test_gpu_interface_condensed.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_tmp.hpp"
#include "interface_csr.hpp"

namespace pa {

namespace {

constexpr int IFC_MAX_CELL_UNITS = 10;     // a cut cell: 2 cell blocks + 4 faces x 2 blocks
constexpr int IFC_MAX_UNITS = 2 * IFC_MAX_CELL_UNITS;

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
        const int nb = m.cell_loc[t] == IF_LOC_CUT ? 2 : 1;
        for (int b = 0; b < nb; ++b)
            if (s >= 0 && (uint32_t)(s + b) < m.num_all_cells) slot_cell[s + b] = (int32_t)t;
    }
    if (t < m.nfaces) {
        const int32_t s = m.face_table[t];
        const int nb = m.face_loc[t] == IF_LOC_CUT ? 2 : 1;
        for (int b = 0; b < nb; ++b)
            if (s >= 0 && (uint32_t)(s + b) < m.num_other_faces) slot_face[s + b] = (int32_t)t;
    }
}

struct IfcTmp {
    int32_t key;            // block: cell block id, or num_all_cells + face block id
    uint32_t code;          // local column bases in the cell
};

// the blocks a cell's unknowns fall in, ascending: the index map (if_global_index) block by block, its Dirichlet slots dropped
__device__ int ifc_cell_units(const IfCsrMesh &m, int cbs, int fbs, int32_t X, IfcTmp *out)
{
    const bool cut = m.cell_loc[X] == IF_LOC_CUT;
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
        else if (m.face_loc[fid[s]] == IF_LOC_CUT) { out[n++] = {key, ifc_code1(j0)}; out[n++] = {key + 1, ifc_code1(j0 + 4 * fbs)}; }
        else out[n++] = {key, ifc_code2(j0, j0 + 4 * fbs)};      // faces- and faces+ of an uncut face: one block
    }
    return n;
}

// group g: its cells and their local row bases, its units (sorted, positions filled in), the row length and the face part;
// everything of G but vstart and ustart
__device__ void ifc_group(const IfCsrMesh &m, IfDims d, const int32_t *fcell, const int32_t *slot_cell, const int32_t *slot_face,
                          uint32_t g, IfGroup &G, IfUnit *u)
{
    uint32_t rc[2] = {0u, 0u};
    int nc = 0;
    int32_t *cell = G.cell;
    cell[0] = cell[1] = -1;
    if (g < m.num_all_cells) {
        const int32_t X = slot_cell[g];
        if (X >= 0) { cell[0] = X; rc[0] = ifc_code1((int)(g - (uint32_t)m.cell_table[X]) * d.cbs); nc = 1; }
    } else {
        const uint32_t q = g - m.num_all_cells;
        const int32_t F = slot_face[q];
        if (F >= 0) {
            const int dup = (int)(q - (uint32_t)m.face_table[F]);
            const bool fcut = m.face_loc[F] == IF_LOC_CUT;
            const int32_t lo = fcell[2 * (size_t)F], hi = fcell[2 * (size_t)F + 1];
            for (int s = 0; s < 2; ++s) {
                const int32_t X = s == 0 ? lo : (hi != lo ? hi : -1);
                if (X < 0 || (uint32_t)X >= m.ncells) continue;
                int lf = 0;
                for (int qq = 0; qq < 4; ++qq)
                    if (m.cell_faces[4 * (size_t)X + qq] == (uint32_t)F) lf = qq;
                uint32_t code;
                if (m.cell_loc[X] != IF_LOC_CUT) {
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
    int ia = 0, ib = 0, n = 0, fu0 = -1;
    uint32_t pos = 0, fpos = 0;
    while (ia < na || ib < nb) {
        int32_t key;
        uint32_t ca = 0u, cb = 0u;
        if (ib >= nb || (ia < na && a[ia].key < b[ib].key)) { key = a[ia].key; ca = a[ia++].code; }
        else if (ia >= na || b[ib].key < a[ia].key) { key = b[ib].key; cb = b[ib++].code; }
        else { key = a[ia].key; ca = a[ia++].code; cb = b[ib++].code; }       // the face both cells share
        const bool is_cell = (uint32_t)key < m.num_all_cells;
        const uint32_t w = is_cell ? (uint32_t)d.cbs : (uint32_t)d.fbs;
        if (!is_cell && fu0 < 0) { fu0 = n; fpos = pos; }                     // cell blocks sort first: the face part starts here
        u[n].gcol = is_cell ? key * d.cbs : (int32_t)m.num_all_cells * d.cbs + (key - (int32_t)m.num_all_cells) * d.fbs;
        u[n].pos = (uint16_t)pos; u[n].width = (uint16_t)w;
        u[n].ccode = ca | (cb << 16);
        pos += w;
        ++n;
    }
    G.rcode = rc[0] | (rc[1] << 16);
    G.nunits = (uint16_t)n; G.R = (uint16_t)pos;
    G.fu0 = (uint16_t)(fu0 < 0 ? n : fu0); G.fpos = (uint16_t)(fu0 < 0 ? pos : fpos);
}

// units and entries per group, entries of the face-only system per face group; each list closed by a zero for the scans
__global__ __launch_bounds__(256) void ifc_count_kernel(IfCsrMesh m, IfDims d, const int32_t *fcell, const int32_t *slot_cell,
                                                        const int32_t *slot_face, uint32_t *ucount, uint64_t *gnnz, uint64_t *cgnnz)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, ng = m.num_all_cells + m.num_other_faces;
    if (g > ng) return;
    IfUnit u[IFC_MAX_UNITS];
    IfGroup G = {};
    if (g < ng) ifc_group(m, d, fcell, slot_cell, slot_face, g, G, u);
    ucount[g] = G.nunits;
    gnnz[g] = (uint64_t)G.R * (uint64_t)(g < m.num_all_cells ? d.cbs : d.fbs);
    if (g >= m.num_all_cells) cgnnz[g - m.num_all_cells] = (uint64_t)(G.R - G.fpos) * (uint64_t)d.fbs;
}

__global__ __launch_bounds__(256) void ifc_write_kernel(IfCsrMesh m, IfDims d, const int32_t *fcell, const int32_t *slot_cell,
                                                        const int32_t *slot_face, const uint32_t *ustart, const uint64_t *vstart,
                                                        IfGroup *groups, IfUnit *units)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= m.num_all_cells + m.num_other_faces) return;
    IfUnit u[IFC_MAX_UNITS];
    IfGroup G;
    ifc_group(m, d, fcell, slot_cell, slot_face, g, G, u);
    G.vstart = vstart[g]; G.ustart = ustart[g];
    groups[g] = G;
    for (int s = 0; s < G.nunits; ++s) units[G.ustart + s] = u[s];
}

// ---- the three sources -----------------------------------------------------------------------------------------------
// A Source says which groups take part (first_group, ngroups), which part of a group's row (first_unit, first_pos: the units
// from first_unit on, positions counted from first_pos), how many leading unknowns of the numbering are left out (skipped: rows
// and columns shift by it), where the rows of group number w of the source start in values (vstart), what a cell's slot holds
// (cell), addend (row, col) of a cell by its local indices in the full local matrix (load), the cell's contribution to the
// right-hand side of local row li (rhs), what is added to a column to make it global (col0), and where values and right-hand
// side go.

// the full system: every group, the whole row; addends from the column-major local matrices
struct IfFullSource {
    IfLocalArgs a;
    double *values, *RHS;
    struct Cell {
        const double *L;        // the cell's local matrix
        int ld;                 // its leading dimension: msize, 2 msize for a cut cell
        bool cut;
    };
    __device__ static uint32_t first_group(const IfCsrMesh &) { return 0u; }
    __device__ static uint32_t ngroups(const IfCsrMesh &m) { return m.num_all_cells + m.num_other_faces; }
    __device__ static uint32_t first_unit(const IfGroup &) { return 0u; }
    __device__ static uint32_t first_pos(const IfGroup &) { return 0u; }
    __device__ static uint64_t skipped(const IfCsrMesh &, IfDims) { return 0u; }
    __device__ static int32_t col0() { return 0; }
    __device__ uint64_t vstart(const IfGroup &G, uint32_t) const { return G.vstart; }
    __device__ Cell cell(const IfCsrMesh &m, IfDims d, int32_t X) const
    {
        const int ms = d.cbs + 4 * d.fbs, m2 = 2 * ms;
        if (X < 0) return {a.lc, ms, false};
        const bool cut = m.cell_loc[X] == IF_LOC_CUT;
        return {cut ? a.lc_cut + (size_t)m.cut_index[X] * m2 * m2 : a.lc + (size_t)X * ms * ms, cut ? m2 : ms, cut};
    }
    __device__ static double load(const Cell &c, uint32_t row, uint32_t col) { return c.L[row + (size_t)col * c.ld]; }
    // the triplet path's sum of local row li: a cut cell's right-hand side (:1349: no Dirichlet columns on a cut cell, :1304-1305);
    // an uncut cell's (:1255-1265) minus the Dirichlet columns times the boundary data
    __device__ double rhs(const IfCsrMesh &m, IfDims d, int32_t X, const Cell &c, int li) const
    {
        if (c.cut) return (li < 2 * d.cbs && a.rhs_cut != nullptr) ? a.rhs_cut[(size_t)m.cut_index[X] * 2 * d.cbs + li] : 0.0;
        double s = (li < d.cbs && a.rhs != nullptr) ? a.rhs[(size_t)X * d.cbs + li] : 0.0;
        for (int lf = 0; lf < 4; ++lf) {
            const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
            if (m.face_table[f] >= 0) continue;
            for (int k = 0; k < d.fbs; ++k) {
                const double dd = a.g != nullptr ? a.g[(size_t)f * d.fbs + k] : 0.0;
                s -= c.L[li + (size_t)(d.cbs + lf * d.fbs + k) * c.ld] * dd;
            }
        }
        return s;
    }
};

// the face-only system: the face groups, the face units of their rows; addends from the packed records
struct IfCondSource {
    IfCondArgs a;
    const uint64_t *cvstart;
    double *values, *RHS;
    struct Cell {
        const double *S, *g;    // the cell's packed S and its g
        int off;                // local index of its first face unknown in the local matrix (cbs, or 2 cbs for a cut cell)
        bool cut;
    };
    __device__ static uint32_t first_group(const IfCsrMesh &m) { return m.num_all_cells; }
    __device__ static uint32_t ngroups(const IfCsrMesh &m) { return m.num_other_faces; }
    __device__ static uint32_t first_unit(const IfGroup &G) { return G.fu0; }
    __device__ static uint32_t first_pos(const IfGroup &G) { return G.fpos; }
    __device__ static uint64_t skipped(const IfCsrMesh &m, IfDims d) { return (uint64_t)m.num_all_cells * d.cbs; }
    __device__ static int32_t col0() { return 0; }
    __device__ uint64_t vstart(const IfGroup &, uint32_t w) const { return cvstart[w]; }
    __device__ Cell cell(const IfCsrMesh &m, IfDims d, int32_t X) const
    {
        if (X < 0) return {a.cond, a.cond, 0, false};
        if (m.cell_loc[X] == IF_LOC_CUT) {
            const int NF = 8 * d.fbs, ntri = NF * (NF + 1) / 2;
            const size_t cc = (size_t)m.cut_index[X];
            return {a.cond_cut + cc * ntri, a.cond_cut + (size_t)a.ncut * ntri + cc * NF, 2 * d.cbs, true};
        }
        const int nf = 4 * d.fbs, ntri = nf * (nf + 1) / 2;
        return {a.cond + (size_t)X * ntri, a.cond + (size_t)m.ncells * ntri + (size_t)X * nf, d.cbs, false};
    }
    // entry (i, j) of a packed upper triangle
    __device__ static double packed(const double *S, int i, int j)
    {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        return S[hi * (hi + 1) / 2 + lo];
    }
    __device__ static double load(const Cell &c, uint32_t row, uint32_t col) { return packed(c.S, (int)row - c.off, (int)col - c.off); }
    // g of the record row, less the Dirichlet columns times the boundary data for an uncut cell (accumulated in local column
    // order, as cond_rhs_contrib of condensed.hip); a cut cell's Dirichlet slots are dropped, as pa_interface_triplets_batch drops them
    __device__ double rhs(const IfCsrMesh &m, IfDims d, int32_t X, const Cell &c, int li) const
    {
        const int row = li - c.off;
        double s = c.g[row];
        if (c.cut) return s;
        for (int lf = 0; lf < 4; ++lf) {
            const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
            if (m.face_table[f] >= 0) continue;
            for (int kp = 0; kp < d.fbs; ++kp) {
                const double dd_ = a.g != nullptr ? a.g[(size_t)f * d.fbs + kp] : 0.0;
                s -= packed(c.S, row, lf * d.fbs + kp) * dd_;
            }
        }
        return s;
    }
};

// the face-only system of one slab: the owned face groups of the extended range, the face units of their rows; a cell's addends
// from the slab's records or, for a halo cell, from the received halo, whose last part is the boundary data of its faces
struct IfRowsSource {
    IfRowsArgs a;
    const uint64_t *cvstart;
    double *values, *RHS;
    struct Cell {
        const double *S, *g;    // the cell's packed S and its g
        const double *bd;       // a halo cell: the boundary data of its 4 faces (nf doubles); null: the context's, by face id
        int off;
        bool cut;
    };
    __device__ uint32_t first_group(const IfCsrMesh &m) const { return m.num_all_cells + a.q0; }
    __device__ uint32_t ngroups(const IfCsrMesh &) const { return a.nq; }
    __device__ static uint32_t first_unit(const IfGroup &G) { return G.fu0; }
    __device__ static uint32_t first_pos(const IfGroup &G) { return G.fpos; }
    __device__ uint64_t skipped(const IfCsrMesh &m, IfDims d) const { return (uint64_t)m.num_all_cells * d.cbs + (uint64_t)a.q0 * d.fbs; }
    __device__ int32_t col0() const { return a.col0; }
    __device__ uint64_t vstart(const IfGroup &, uint32_t w) const { return cvstart[a.q0 + w] - a.v0; }
    __device__ Cell cell(const IfCsrMesh &m, IfDims d, int32_t X) const
    {
        if (X < 0) return {a.cond, a.cond, nullptr, 0, false};
        const bool halo = (uint32_t)X < a.nh;
        const int nf = 4 * d.fbs, ntri = nf * (nf + 1) / 2, NF = 8 * d.fbs, NTRI = NF * (NF + 1) / 2;
        const double *hcut = a.halo + (size_t)a.nh * (ntri + nf), *hbd = hcut + (size_t)a.nhc * (NTRI + NF);
        const double *bd = halo ? hbd + (size_t)X * nf : nullptr;
        if (m.cell_loc[X] == IF_LOC_CUT) {
            const size_t cc = (size_t)m.cut_index[X], n = halo ? a.nhc : a.ncut;
            const double *rec = halo ? hcut : a.cond_cut;
            return {rec + cc * NTRI, rec + n * NTRI + cc * NF, bd, 2 * d.cbs, true};
        }
        const size_t x = halo ? (size_t)X : (size_t)X - a.nh, n = halo ? a.nh : a.ncells;
        const double *rec = halo ? a.halo : a.cond;
        return {rec + x * ntri, rec + n * ntri + x * nf, bd, d.cbs, false};
    }
    __device__ static double load(const Cell &c, uint32_t row, uint32_t col)
    {
        return IfCondSource::packed(c.S, (int)row - c.off, (int)col - c.off);
    }
    // IfCondSource::rhs with the boundary data of a halo cell's faces taken from the halo
    __device__ double rhs(const IfCsrMesh &m, IfDims d, int32_t X, const Cell &c, int li) const
    {
        const int row = li - c.off;
        double s = c.g[row];
        if (c.cut) return s;
        for (int lf = 0; lf < 4; ++lf) {
            const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
            if (m.face_table[f] >= 0) continue;
            for (int kp = 0; kp < d.fbs; ++kp) {
                const double dd_ = c.bd != nullptr ? c.bd[lf * d.fbs + kp] : (a.g != nullptr ? a.g[(size_t)(f - a.fshift) * d.fbs + kp] : 0.0);
                s -= IfCondSource::packed(c.S, row, lf * d.fbs + kp) * dd_;
            }
        }
        return s;
    }
};

// ---- pattern: one thread per row -------------------------------------------------------------------------------------
template <class Source>
__global__ __launch_bounds__(256) void if_pattern_kernel(IfCsrMesh m, IfDims d, uint64_t nrows, uint64_t nnz, const IfGroup *groups,
                                                         const IfUnit *units, Source src, int64_t *rowptr, int32_t *colind)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nrows) return;
    if (t == nrows) { rowptr[t] = (int64_t)nnz; return; }
    const uint32_t g0 = src.first_group(m), gf = g0 > m.num_all_cells ? g0 : m.num_all_cells;      // the source's first face group
    const uint64_t cell_rows = (uint64_t)(gf - g0) * d.cbs;                     // the source's rows that are rows of cell groups
    const uint32_t g = t < cell_rows ? g0 + (uint32_t)(t / d.cbs) : gf + (uint32_t)((t - cell_rows) / d.fbs);
    const uint32_t i = t < cell_rows ? (uint32_t)(t % d.cbs) : (uint32_t)((t - cell_rows) % d.fbs);
    const IfGroup G = groups[g];
    const uint32_t poff = Source::first_pos(G);
    const uint64_t start = src.vstart(G, g - g0) + (uint64_t)i * (G.R - poff);
    rowptr[t] = (int64_t)start;
    if (colind == nullptr) return;
    const int32_t skip = (int32_t)src.skipped(m, d) - src.col0();
    for (int s = (int)Source::first_unit(G); s < G.nunits; ++s) {
        const IfUnit U = units[G.ustart + s];
        for (int k = 0; k < U.width; ++k) colind[start + (U.pos - poff) + k] = U.gcol - skip + k;
    }
}

// ---- numeric phase: one wavefront per group, four groups per block ----------------------------------------------------
template <class Source>
__global__ __launch_bounds__(256) void if_fill_kernel(IfCsrMesh m, IfDims d, const IfGroup *__restrict__ groups,
                                                      const IfUnit *__restrict__ units, Source src)
{
    const uint32_t lane = threadIdx.x % 64u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + threadIdx.x / 64u);
    if (w >= src.ngroups(m)) return;
    const uint32_t grp = src.first_group(m) + w;
    const IfGroup G = groups[grp];
    const uint32_t nrows = grp < m.num_all_cells ? (uint32_t)d.cbs : (uint32_t)d.fbs;
    typename Source::Cell C[2];
    uint32_t rc[2] = {0u, 0u};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        C[s] = src.cell(m, d, G.cell[s]);
        if (G.cell[s] >= 0) rc[s] = (G.rcode >> (16 * s)) & 0xffffu;
    }
    const int u0 = (int)Source::first_unit(G);
    const uint32_t poff = Source::first_pos(G), R = G.R - poff, total = nrows * R;
    const IfUnit *U = units + G.ustart;
    const uint64_t vs = src.vstart(G, w);
    for (uint32_t e = lane; e < total; e += 64u) {
        const uint32_t i = e / R, pos = e - i * R + poff;
        uint32_t upos = U[u0].pos, ucode = U[u0].ccode;
        for (int u = u0 + 1; u < G.nunits; ++u)
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
                    v[s][r][c] = on[s][r][c] ? Source::load(C[s], row, col) : 0.0;
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
        src.values[vs + e] = acc;
    }
    if (src.RHS != nullptr && lane < nrows) {
        double acc = 0.0;
        bool first = true;
        for (int s = 0; s < 2; ++s)
            for (int r = 0; r < ifc_count(rc[s]); ++r) {
                const int li = (r == 0 ? ifc_first(rc[s]) : ifc_second(rc[s])) + (int)lane;
                const double wv = src.rhs(m, d, G.cell[s], C[s], li);
                acc = first ? wv : acc + wv;
                first = false;
            }
        const uint64_t row = grp < m.num_all_cells ? (uint64_t)grp * d.cbs
                                                   : (uint64_t)m.num_all_cells * d.cbs + (uint64_t)(grp - m.num_all_cells) * d.fbs;
        src.RHS[row - src.skipped(m, d) + lane] = acc;
    }
}

// ---- triplets: the reference's push order ----------------------------------------------------------------------------
// the full system (assemble :1203-1269, assemble_cut :1271-1354): one block per cell at a time
__global__ __launch_bounds__(256) void if_triplets_kernel(IfCsrMesh m, IfDims d, IfLocalArgs a, IfTriplets o)
{
    extern __shared__ double sh[];       // dirichlet data (2 msize), then int32 idx (2 msize)
    const int msize = d.cbs + 4 * d.fbs, m2 = 2 * msize;
    double *dd = sh;
    int32_t *idx = reinterpret_cast<int32_t *>(sh + m2);
    for (size_t c = blockIdx.x; c < m.ncells; c += gridDim.x) {
        const bool cut = m.cell_loc[c] == IF_LOC_CUT;
        const int n = cut ? m2 : msize;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            size_t bdof;
            idx[i] = if_global_index(m, d, c, cut, i, &bdof);
            dd[i] = (idx[i] < 0 && a.g != nullptr) ? a.g[bdof] : 0.0;
        }
        __syncthreads();
        if (!cut) {
            const double *A = a.lc + c * (size_t)(msize * msize);
            for (int e = threadIdx.x; e < msize * msize; e += blockDim.x) {
                const int i = e / msize, j = e % msize;
                const bool keep = idx[i] >= 0 && idx[j] >= 0;
                const size_t s = c * (size_t)(msize * msize) + e;
                o.rows[s] = keep ? idx[i] : -1;
                o.cols[s] = keep ? idx[j] : -1;
                o.vals[s] = A[i + j * msize];
            }
            for (int i = threadIdx.x; i < msize; i += blockDim.x) {
                double s = (i < d.cbs && a.rhs != nullptr) ? a.rhs[c * d.cbs + i] : 0.0;              // :1265
                if (idx[i] >= 0)
                    for (int j = d.cbs; j < msize; ++j)
                        if (idx[j] < 0) s -= A[i + j * msize] * dd[j];                                // :1261
                o.rhs_rows[c * msize + i] = idx[i];
                o.rhs_vals[c * msize + i] = idx[i] >= 0 ? s : 0.0;
            }
        } else {
            const size_t cc = (size_t)m.cut_index[c];
            const double *A = a.lc_cut + cc * (size_t)(m2 * m2);
            for (int e = threadIdx.x; e < msize * msize; e += blockDim.x) {                           // nothing pushed in the uncut slots
                const size_t s = c * (size_t)(msize * msize) + e;
                o.rows[s] = -1; o.cols[s] = -1; o.vals[s] = 0.0;
            }
            for (int i = threadIdx.x; i < msize; i += blockDim.x) { o.rhs_rows[c * msize + i] = -1; o.rhs_vals[c * msize + i] = 0.0; }
            for (int e = threadIdx.x; e < m2 * m2; e += blockDim.x) {                                 // :1337-1347
                const int i = e / m2, j = e % m2;
                const size_t s = cc * (size_t)(m2 * m2) + e;
                const bool keep = idx[i] >= 0 && idx[j] >= 0;      // always true: the reference rejects Dirichlet faces on cut cells (:1304-1305)
                o.rows_cut[s] = keep ? idx[i] : -1; o.cols_cut[s] = keep ? idx[j] : -1;
                o.vals_cut[s] = A[i + j * m2];
            }
            for (int i = threadIdx.x; i < m2; i += blockDim.x) {                                      // :1349
                o.rhs_rows_cut[cc * m2 + i] = idx[i];
                o.rhs_vals_cut[cc * m2 + i] = (i < 2 * d.cbs && a.rhs_cut != nullptr) ? a.rhs_cut[cc * 2 * d.cbs + i] : 0.0;
            }
        }
        __syncthreads();
    }
}

// the face-only system, one slot per thread
__global__ __launch_bounds__(256) void ifd_triplets_kernel(IfCsrMesh m, IfDims d, IfCondSource src, IfTriplets o)
{
    const int nf = 4 * d.fbs, NF = 8 * d.fbs;
    for (size_t X = blockIdx.x; X < m.ncells; X += gridDim.x) {
        const IfCondSource::Cell c = src.cell(m, d, (int32_t)X);
        const bool cut = c.cut;
        const int n = cut ? NF : nf;
        int32_t *rows = cut ? o.rows_cut + (size_t)m.cut_index[X] * NF * NF : o.rows + X * nf * nf;
        int32_t *cols = cut ? o.cols_cut + (size_t)m.cut_index[X] * NF * NF : o.cols + X * nf * nf;
        double *vals = cut ? o.vals_cut + (size_t)m.cut_index[X] * NF * NF : o.vals + X * nf * nf;
        if (cut) {                                       // the uncut slots of a cut cell are empty
            for (int e = threadIdx.x; e < nf * nf; e += blockDim.x) {
                o.rows[X * nf * nf + e] = -1; o.cols[X * nf * nf + e] = -1; o.vals[X * nf * nf + e] = 0.0;
            }
            for (int e = threadIdx.x; e < nf; e += blockDim.x) { o.rhs_rows[X * nf + e] = -1; o.rhs_vals[X * nf + e] = 0.0; }
        }
        for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
            const int i = e / n, j = e % n;
            const int32_t ri = if_face_index(m, d, X, cut, i), cj = if_face_index(m, d, X, cut, j);
            const bool keep = ri >= 0 && cj >= 0;
            rows[e] = keep ? ri : -1;
            cols[e] = keep ? cj : -1;
            vals[e] = IfCondSource::packed(c.S, i, j);
        }
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int32_t ri = if_face_index(m, d, X, cut, i);
            int32_t *rr = cut ? o.rhs_rows_cut + (size_t)m.cut_index[X] * NF : o.rhs_rows + X * nf;
            double *rv = cut ? o.rhs_vals_cut + (size_t)m.cut_index[X] * NF : o.rhs_vals + X * nf;
            rr[i] = ri;
            rv[i] = ri >= 0 ? src.rhs(m, d, (int32_t)X, c, c.off + i) : 0.0;
        }
    }
}

// the tables of ifcsr_build into *t; on failure what *t holds by then is the caller's to release
hipError_t ifc_build(hipStream_t stream, const IfCsrMesh &m, int face_deg, IfCsrTables *t)
{
    const IfDims d = if_dims(face_deg);
    const size_t ng = (size_t)m.num_all_cells + m.num_other_faces, nq = m.num_other_faces;
    DeviceTmp tmp(stream);
    int32_t *fcell, *slot_cell, *slot_face;
    uint32_t *ucount, *ustart, nunits = 0;
    uint64_t *gnnz, *vstart, *cgnnz;
    if (!tmp.alloc(&fcell, 2 * ((size_t)m.nfaces + 1)) || !tmp.alloc(&slot_cell, (size_t)m.num_all_cells + 1) ||
        !tmp.alloc(&slot_face, nq + 1) || !tmp.alloc(&ucount, ng + 1) || !tmp.alloc(&ustart, ng + 1) || !tmp.alloc(&gnnz, ng + 1) ||
        !tmp.alloc(&vstart, ng + 1) || !tmp.alloc(&cgnnz, nq + 1) ||
        !tmp.ok(hipMalloc((void **)&t->groups, (ng ? ng : 1) * sizeof(IfGroup))) ||
        !tmp.ok(hipMalloc((void **)&t->cvstart, (nq + 1) * sizeof(uint64_t))))
        return tmp.error();
    size_t top = m.nfaces;
    if (m.num_all_cells > top) top = m.num_all_cells;
    if (m.num_other_faces > top) top = m.num_other_faces;
    if (m.ncells > top) top = m.ncells;
    hipLaunchKernelGGL(ifc_init_kernel, dim3(blocks_for(top)), dim3(256), 0, stream, m, fcell, slot_cell, slot_face);
    hipLaunchKernelGGL(ifc_adjacency_kernel, dim3(blocks_for(top)), dim3(256), 0, stream, m, fcell, slot_cell, slot_face);
    hipLaunchKernelGGL(ifc_count_kernel, dim3(blocks_for(ng + 1)), dim3(256), 0, stream, m, d, fcell, slot_cell, slot_face, ucount, gnnz,
                       cgnnz);
    if (!tmp.ok(hipGetLastError())) return tmp.error();
    if (exclusive_scan_with_total(stream, ucount, ustart, ng + 1, tmp, &nunits) != hipSuccess ||
        exclusive_scan_with_total(stream, gnnz, vstart, ng + 1, tmp, &t->nnz) != hipSuccess ||
        exclusive_scan_with_total(stream, cgnnz, t->cvstart, nq + 1, tmp, &t->cnnz) != hipSuccess ||
        !tmp.ok(hipMalloc((void **)&t->units, (nunits ? nunits : 1) * sizeof(IfUnit))))
        return tmp.error();
    hipLaunchKernelGGL(ifc_write_kernel, dim3(blocks_for(ng)), dim3(256), 0, stream, m, d, fcell, slot_cell, slot_face, ustart, vstart,
                       t->groups, t->units);
    if (!tmp.ok(hipGetLastError()) || !tmp.ok(hipStreamSynchronize(stream))) return tmp.error();
    t->face_deg = face_deg;
    t->nrows = (uint64_t)m.num_all_cells * d.cbs + (uint64_t)m.num_other_faces * d.fbs;
    t->ngroups = (uint32_t)ng;
    t->nunits = nunits;
    return hipSuccess;
}

template <class Source>
hipError_t if_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, uint64_t nrows, uint64_t nnz, const Source &src,
                      int64_t *rowptr, int32_t *colind)
{
    hipLaunchKernelGGL(if_pattern_kernel<Source>, dim3(blocks_for(nrows + 1)), dim3(256), 0, stream, m, if_dims(t.face_deg), nrows, nnz,
                       t.groups, t.units, src, rowptr, colind);
    return hipGetLastError();
}

template <class Source>
hipError_t if_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, uint32_t ngroups, const Source &src)
{
    if (ngroups == 0) return hipSuccess;
    hipLaunchKernelGGL(if_fill_kernel<Source>, dim3((ngroups + 3) / 4), dim3(256), 0, stream, m, if_dims(t.face_deg), t.groups, t.units,
                       src);
    return hipGetLastError();
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
    const hipError_t e = ifc_build(stream, m, face_deg, t);       // its temporaries are gone, the stream has drained on failure
    if (e != hipSuccess) ifcsr_release(t);
    return e;
}

hipError_t ifcsr_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind)
{
    return if_pattern(stream, m, t, t.nrows, t.nnz, IfFullSource{{}, nullptr, nullptr}, rowptr, colind);
}

hipError_t ifcsr_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfLocalArgs &a, double *values, double *RHS)
{
    return if_fill(stream, m, t, t.ngroups, IfFullSource{a, values, RHS});
}

hipError_t ifcsr_triplets(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfLocalArgs &a, const IfTriplets &o)
{
    if (m.ncells == 0) return hipSuccess;
    const IfDims d = if_dims(face_deg);
    const int m2 = 2 * (d.cbs + 4 * d.fbs);
    const dim3 grid(m.ncells < (uint32_t)max_blocks ? m.ncells : (uint32_t)max_blocks);
    hipLaunchKernelGGL(if_triplets_kernel, grid, dim3(256), m2 * sizeof(double) + m2 * sizeof(int32_t), stream, m, d, a, o);
    return hipGetLastError();
}

hipError_t ifcond_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind)
{
    const uint64_t nrows = (uint64_t)m.num_other_faces * (t.face_deg + 1);
    return if_pattern(stream, m, t, nrows, t.cnnz, IfCondSource{{}, t.cvstart, nullptr, nullptr}, rowptr, colind);
}

hipError_t ifcond_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfCondArgs &a, double *values, double *RHS)
{
    return if_fill(stream, m, t, m.num_other_faces, IfCondSource{a, t.cvstart, values, RHS});
}

hipError_t ifcond_triplets(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const IfTriplets &o)
{
    if (m.ncells == 0) return hipSuccess;
    const dim3 grid(m.ncells < (uint32_t)max_blocks ? m.ncells : (uint32_t)max_blocks);
    hipLaunchKernelGGL(ifd_triplets_kernel, grid, dim3(256), 0, stream, m, if_dims(face_deg), IfCondSource{a, nullptr, nullptr, nullptr}, o);
    return hipGetLastError();
}

// ---- one slab of cell rows -------------------------------------------------------------------------------------------
namespace {

// the Dirichlet data of the faces of cells [first, first + n), nf per cell in local face order; zero where a face is not Dirichlet
__global__ __launch_bounds__(256) void ifrows_halo_bd_kernel(const uint32_t *cell_faces, const uint8_t *face_dir, uint32_t first, uint32_t n,
                                                             int fbs, const double *g, double *out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, nf = 4u * (uint32_t)fbs;
    if (t >= n * nf) return;
    const uint32_t X = first + t / nf, lf = (t % nf) / (uint32_t)fbs, k = t % (uint32_t)fbs;
    const uint32_t f = cell_faces[4 * (size_t)X + lf];
    out[t] = (g != nullptr && face_dir[f]) ? g[(size_t)f * fbs + k] : 0.0;
}

}  // namespace

hipError_t ifrows_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfRowsArgs &a, int64_t *rowptr, int32_t *colind)
{
    return if_pattern(stream, m, t, (uint64_t)a.nq * (t.face_deg + 1), a.nnz, IfRowsSource{a, t.cvstart, nullptr, nullptr}, rowptr, colind);
}

hipError_t ifrows_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfRowsArgs &a, double *values, double *RHS)
{
    return if_fill(stream, m, t, a.nq, IfRowsSource{a, t.cvstart, values, RHS});
}

hipError_t ifrows_halo_pack(hipStream_t stream, int face_deg, const uint32_t *cell_faces, const uint8_t *face_dir, uint32_t ncells,
                            uint32_t ncut, uint32_t ns, uint32_t nsc, const double *cond, const double *cond_cut, const double *g,
                            double *halo)
{
    if (ns == 0) return hipSuccess;
    const size_t fbs = face_deg + 1, nf = 4 * fbs, ntri = nf * (nf + 1) / 2, NF = 8 * fbs, NTRI = NF * (NF + 1) / 2;
    // the top row's records are the tails of [S | g] and of the cut cells' [S | g]
    const struct { const double *src; size_t n; } part[4] = {{cond + (size_t)(ncells - ns) * ntri, ns * ntri},
                                                             {cond + (size_t)ncells * ntri + (size_t)(ncells - ns) * nf, ns * nf},
                                                             {cond_cut + (size_t)(ncut - nsc) * NTRI, nsc * NTRI},
                                                             {cond_cut + (size_t)ncut * NTRI + (size_t)(ncut - nsc) * NF, nsc * NF}};
    double *out = halo;
    for (const auto &p : part) {
        if (p.n) {
            const hipError_t e = hipMemcpyAsync(out, p.src, p.n * sizeof(double), hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) return e;
        }
        out += p.n;
    }
    hipLaunchKernelGGL(ifrows_halo_bd_kernel, dim3(blocks_for(ns * nf)), dim3(256), 0, stream, cell_faces, face_dir, ncells - ns, ns,
                       (int)fbs, g, out);
    return hipGetLastError();
}

}  // namespace pa
