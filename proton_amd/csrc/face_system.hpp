// face_system.hpp -- the per-mesh face tables the direct-CSR assemblers are built on (condensed.hip, assembler_csr.hip,
// obstacle_csr.hip), stated once: the symbolic record of a face and its bit layout, the non-Dirichlet faces of a cell in
// ascending compressed order, the closed forms that place a block of rows in the CSR arrays, the Dirichlet columns' share of a
// right-hand-side row, and the view of the tables the host functions take.  The layout of `packed` and of a code lives HERE and
// nowhere else: every reader goes through the accessors below (tests/cpp/face_descriptor_check.cpp packs and unpacks every field).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

// ---- the code of one column face of a face F: where it sits in F's cells A and B (6 bits) -----------------------------------
//   bits 0-1: its local face index in cell A, bit 2: present in A; bits 3-4 / 5: the same for B
// (the "present" bits are masks, not predicates: a bool-returning accessor cost asm_fill_faces_kernel 6 to 12 registers)
constexpr uint32_t FCODE_HAS_A = 4u, FCODE_HAS_B = 32u;
__host__ __device__ __forceinline__ constexpr uint32_t fcode_in_A(int lf) { return (uint32_t)lf | FCODE_HAS_A; }
__host__ __device__ __forceinline__ constexpr uint32_t fcode_in_B(int lf) { return ((uint32_t)lf << 3) | FCODE_HAS_B; }
__host__ __device__ __forceinline__ constexpr uint32_t fcode_lf_A(uint32_t code) { return code & 3u; }
__host__ __device__ __forceinline__ constexpr uint32_t fcode_lf_B(uint32_t code) { return (code >> 3) & 3u; }
// `rows` (4 bits): the face's own local index in cell A (bits 0-1) and in cell B (bits 2-3)
__host__ __device__ __forceinline__ constexpr uint32_t frows_make(int rowA, int rowB) { return (uint32_t)rowA | ((uint32_t)rowB << 2); }
__host__ __device__ __forceinline__ constexpr uint32_t frows_A(uint32_t rows) { return rows & 3u; }
__host__ __device__ __forceinline__ constexpr uint32_t frows_B(uint32_t rows) { return (rows >> 2) & 3u; }

// symbolic record of an owned non-Dirichlet face (position = its compressed id - the first owned one)
struct CondFace {
    int32_t cA, cB;          // its cells (local index), -1 none; cA <= -2: cell -2 - cA of the slab below (remote)
    int32_t colcomp[7];      // compressed ids of its column faces, ascending; -1 padded
    uint8_t code[7];         // per column face its code (fcode_*)
    uint8_t rows;            // frows_*
    uint8_t ncol;
    uint32_t face;           // local face index
};

// the part of it the numeric phase reads, one 16-byte load.  packed: bits 6s .. 6s+5: code[s], s < 7; bits 42-45: rows;
// bits 46-48: ncol; bit 49: some face of its local cells is Dirichlet (their data enter the right-hand side); bits 50-63: zero
struct alignas(16) CondFaceLean {
    int32_t cA, cB;
    uint64_t packed;
};

__host__ __device__ __forceinline__ uint64_t lean_pack(const uint8_t (&code)[7], uint32_t rows, uint32_t ncol, bool dirichlet)
{
    uint64_t p = ((uint64_t)(rows & 15u) << 42) | ((uint64_t)(ncol & 7u) << 46) | ((uint64_t)(dirichlet ? 1 : 0) << 49);
    for (int s = 0; s < 7; ++s) p |= (uint64_t)(code[s] & 63) << (6 * s);
    return p;
}
__host__ __device__ __forceinline__ uint32_t lean_code(uint64_t packed, uint32_t s) { return (uint32_t)(packed >> (6 * s)) & 63u; }
__host__ __device__ __forceinline__ uint32_t lean_rows(uint64_t packed) { return (uint32_t)(packed >> 42) & 15u; }
__host__ __device__ __forceinline__ uint32_t lean_ncol(uint64_t packed) { return (uint32_t)(packed >> 46) & 7u; }
__host__ __device__ __forceinline__ bool lean_dirichlet(uint64_t packed) { return (packed >> 49) & 1u; }

// ---- the non-Dirichlet faces of a cell in ascending compressed order: comp[s], local index lf[s], s < n ----------------------
struct CellFaces { int32_t comp[4]; int lf[4]; int n; };
// REGS: the new entry goes in by a select per slot, so that r never needs an indexed store and stays in registers (the one-row
// kernels of obstacle_csr.hip: no private segment); the indexed store keeps r in 40 bytes of scratch while it is sorted, which is
// what the register budgets of the wavefront-per-U-cells fills of assembler_csr.hip were measured with
template <bool REGS = false>
__device__ __forceinline__ CellFaces cell_faces_sorted(const uint32_t *cell_faces, const int32_t *face_compress, uint32_t c)
{
    const uint4 f = *reinterpret_cast<const uint4 *>(cell_faces + 4 * (size_t)c);
    const int32_t cc[4] = {face_compress[f.x], face_compress[f.y], face_compress[f.z], face_compress[f.w]};
    CellFaces r;
    r.n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { r.comp[q] = 0x7fffffff; r.lf[q] = 0; }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (cc[q] >= 0) {
            // insertion into the sorted prefix (at most 4 entries)
            int p = r.n;
#pragma unroll
            for (int s = 2; s >= 0; --s)
                if (s < r.n && r.comp[s] > cc[q]) { r.comp[s + 1] = r.comp[s]; r.lf[s + 1] = r.lf[s]; p = s; }
            if constexpr (REGS) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (s == p) { r.comp[s] = cc[q]; r.lf[s] = q; }
            } else { r.comp[p] = cc[q]; r.lf[p] = q; }
            ++r.n;
        }
    return r;
}

// ---- where a block of rows starts in the CSR arrays of the system with cell AND face unknowns -------------------------------
// cell c's cbs rows hold cbs + fbs (its non-Dirichlet faces) entries each; cpre: non-Dirichlet faces of the cells before c
__host__ __device__ __forceinline__ uint64_t cell_block_start(int cbs, int fbs, uint32_t c, uint32_t cpre)
{
    return (uint64_t)cbs * ((uint64_t)c * cbs + (uint64_t)cpre * fbs);
}
// face q's fbs rows, behind the cell_nnz entries of all cell rows, hold cbs (its cells) + fbs (its column faces) entries each;
// fcpre / colpre: cells / column faces of the faces before q
__host__ __device__ __forceinline__ uint64_t face_block_start(uint64_t cell_nnz, int cbs, int fbs, uint32_t fcpre, uint32_t colpre)
{
    return cell_nnz + (uint64_t)fbs * ((uint64_t)fcpre * cbs + (uint64_t)colpre * fbs);
}

// ---- the Dirichlet columns of local row `row` of cell c (lc: ncells x MS x MS, column-major) times the boundary data, taken
// off `s` in local column order (hho.hpp:401): a cell row starts from its rhs_c(i), a face row from 0
template <int CBS, int FBS>
__device__ __forceinline__ double dirichlet_rhs_contrib(const uint32_t *cell_faces, const int32_t *face_compress, const double *lc,
                                                        const double *g, uint32_t c, uint32_t row, double s)
{
    constexpr int MS = CBS + 4 * FBS;
    const double *A = lc + (size_t)c * (MS * MS);
    const uint4 f = *reinterpret_cast<const uint4 *>(cell_faces + 4 * (size_t)c);
    const uint32_t fl[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int lf = 0; lf < 4; ++lf)
        if (face_compress[fl[lf]] < 0)
            for (int kp = 0; kp < FBS; ++kp) {
                const double dd = g != nullptr ? g[(size_t)fl[lf] * FBS + kp] : 0.0;
                s -= A[(size_t)(CBS + lf * FBS + kp) * MS + row] * dd;
            }
    return s;
}

// ---- one view of the tables: what the host functions of the three assemblers take --------------------------------------------
// Plain device pointers and counts, built from the context by face_system_view() (capi_assembly.hip).  After cond_prepare the
// condensed system's part is set; cprefix / fprefix and their totals only after asm_prepare (whole-mesh contexts).
struct FaceSystemView {
    // mesh
    const uint32_t *cell_faces;        // ncells x 4
    const int32_t *face_compress;      // per local face its compressed id, -1 Dirichlet
    // tables
    const CondFace *faces;             // nown records
    const CondFaceLean *lean;
    const uint32_t *colprefix;         // nown + 1: column faces of the faces before q
    const uint32_t *cprefix;           // ncells + 1: non-Dirichlet faces of the cells before c
    const uint32_t *fprefix;           // nown + 1: cells of the faces before q
    // counts
    uint32_t ncells, nown;
    uint64_t total_cols, cell_faces_total, face_cells_total;      // colprefix[nown], cprefix[ncells], fprefix[nown]
};

// sizes of the assembler's own system for one degree pair (whole-mesh contexts: every non-Dirichlet face is owned)
struct AsmSizes { uint64_t cell_nnz, nnz, nrows; };      // entries of all cell rows; of all rows; rows
inline AsmSizes asm_sizes(const FaceSystemView &v, int cbs, int fbs)
{
    const uint64_t cell_nnz = cell_block_start(cbs, fbs, v.ncells, (uint32_t)v.cell_faces_total);
    return {cell_nnz, face_block_start(cell_nnz, cbs, fbs, (uint32_t)v.face_cells_total, (uint32_t)v.total_cols),
            (uint64_t)cbs * v.ncells + (uint64_t)fbs * v.nown};
}

}  // namespace pa
