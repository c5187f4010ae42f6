// assembler_csr.hip -- the reference's OWN global system (cell + face unknowns) built directly in CSR.
//
// assembler<Mesh> (src/methods/hho_bits/hho.hpp:252-463) numbers the cell unknowns of cell c at c * cbs + i and the
// unknowns of a non-Dirichlet face F behind them at cbs * ncells + compress_table[F] * fbs + k (:362-379), pushes
// msize^2 triplets per cell in row-major local order (:391-403) and hands them to setFromTriplets (:451-455), which
// sums duplicates and sorts the columns of a row.  That is the span the reference's drivers print as "Matrix assembly"
// (apps/cuthho/cuthho_square.cpp:881-905, apps/convergence_test/convergence_test.cpp:201-217).
//
// Here the same matrix comes out of the mesh's face adjacency without triplets and without a sort (the design of
// condensed.hip, extended by the cell block):
//   * a CELL row (c, i) holds the cbs unknowns of its own cell, then the unknowns of the cell's non-Dirichlet faces in
//     ascending order of their compressed ids: one contribution each, lc_c(i, j);
//   * a FACE row (F, k) holds the cell unknowns of F's (at most two) cells, lower cell id first, then the unknowns of the (at
//     most 7) non-Dirichlet faces of those cells in ascending compressed order: one contribution for the cell columns and
//     for the faces of one cell only, two -- lower cell id first, the order in which setFromTriplets meets the duplicates --
//     for F itself.
// Row pointers are closed forms of two prefix counts (non-Dirichlet faces per cell; cells and column faces per face); the
// symbolic phase runs once per mesh, the numeric phase is a pure gather from lc: one thread per CSR entry, consecutive
// lanes writing consecutive entries.  Structure and values are bit-identical to pa_csr_from_triplets(pa_triplets_batch(..))
// (tests/test_gpu_assembler.py); the right-hand side is the triplet path's per-row sums (:401, :405) added in cell order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assembler_csr.hpp"
#include "device_tmp.hpp"

namespace pa {

// ---- symbolic: per cell the number of its non-Dirichlet faces, per non-Dirichlet face the number of its cells ------------
__global__ __launch_bounds__(256) void asm_counts_kernel(uint32_t ncells, uint32_t nown, const uint32_t *cell_faces,
                                                         const int32_t *face_compress, const CondFaceLean *lean, uint32_t *nfc,
                                                         uint32_t *nfcell)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ncells) {
        const uint4 f = *reinterpret_cast<const uint4 *>(cell_faces + 4 * (size_t)t);
        nfc[t] = (face_compress[f.x] >= 0) + (face_compress[f.y] >= 0) + (face_compress[f.z] >= 0) + (face_compress[f.w] >= 0);
    }
    if (t < nown) nfcell[t] = (lean[t].cA >= 0) + (lean[t].cB >= 0);
    if (t == ncells) nfc[ncells] = 0;
    if (t == nown) nfcell[nown] = 0;
}

hipError_t asm_build_tables(hipStream_t stream, const FaceSystemView &v, const AsmTables &t)
{
    const uint32_t top = v.ncells > v.nown ? v.ncells : v.nown;
    hipLaunchKernelGGL(asm_counts_kernel, dim3(blocks_for((size_t)top + 1)), dim3(256), 0, stream, v.ncells, v.nown, v.cell_faces,
                       v.face_compress, v.lean, t.nfc.get(), t.nfcell.get());
    DeviceTmp tmp(stream);
    if (!tmp.ok(hipGetLastError()) ||
        exclusive_scan_with_total<uint32_t>(stream, t.nfc.get(), t.cprefix.get(), (size_t)v.ncells + 1, tmp, nullptr) != hipSuccess ||
        exclusive_scan_with_total<uint32_t>(stream, t.nfcell.get(), t.fprefix.get(), (size_t)v.nown + 1, tmp, nullptr) != hipSuccess)
        return tmp.error();
    tmp.ok(hipStreamSynchronize(stream));
    return tmp.error();
}

// the sizes every kernel of one degree pair takes; the closed forms of the row starts are face_system.hpp's
struct AsmDims {
    int cbs, fbs, ms;
    uint32_t ncells, nown;
    uint64_t cell_nnz;        // entries of all cell rows
};
static AsmDims asm_dims(const FaceSystemView &v, int cbs, int fbs)
{
    return {cbs, fbs, cbs + 4 * fbs, v.ncells, v.nown, asm_sizes(v, cbs, fbs).cell_nnz};
}

// ---- pattern: row pointers and column indices ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void asm_pattern_cells_kernel(AsmDims d, const uint32_t *cell_faces, const int32_t *face_compress,
                                                                const uint32_t *cprefix, int64_t *rowptr, int32_t *colind)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = t / (uint32_t)d.cbs;
    const int i = (int)(t % (uint32_t)d.cbs);
    if (c >= d.ncells) return;
    const CellFaces cf = cell_faces_sorted(cell_faces, face_compress, c);
    const int R = d.cbs + cf.n * d.fbs;
    const uint64_t start = cell_block_start(d.cbs, d.fbs, c, cprefix[c]) + (uint64_t)i * R;
    rowptr[(size_t)c * d.cbs + i] = (int64_t)start;
    if (colind == nullptr) return;
    for (int j = 0; j < d.cbs; ++j) colind[start + j] = (int32_t)((uint64_t)c * d.cbs + j);
    for (int s = 0; s < cf.n; ++s)
        for (int kp = 0; kp < d.fbs; ++kp)
            colind[start + d.cbs + s * d.fbs + kp] = (int32_t)((uint64_t)d.cbs * d.ncells + (uint64_t)cf.comp[s] * d.fbs + kp);
}

__global__ __launch_bounds__(256) void asm_pattern_faces_kernel(AsmDims d, const CondFace *faces, const uint32_t *colprefix,
                                                                const uint32_t *fprefix, int64_t *rowptr, int32_t *colind)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = t / (uint32_t)d.fbs;
    const int k = (int)(t % (uint32_t)d.fbs);
    int64_t *rp = rowptr + (size_t)d.cbs * d.ncells;
    if (q > d.nown || (q == d.nown && k > 0)) return;
    if (q == d.nown) { rp[(size_t)d.nown * d.fbs] = (int64_t)face_block_start(d.cell_nnz, d.cbs, d.fbs, fprefix[d.nown], colprefix[d.nown]); return; }
    const CondFace &r = faces[q];
    const int ncell = (r.cA >= 0) + (r.cB >= 0);
    const int R = ncell * d.cbs + r.ncol * d.fbs;
    const uint64_t start = face_block_start(d.cell_nnz, d.cbs, d.fbs, fprefix[q], colprefix[q]) + (uint64_t)k * R;
    rp[(size_t)q * d.fbs + k] = (int64_t)start;
    if (colind == nullptr) return;
    int o = 0;
    if (r.cA >= 0) { for (int j = 0; j < d.cbs; ++j) colind[start + o + j] = (int32_t)((uint64_t)r.cA * d.cbs + j); o += d.cbs; }
    if (r.cB >= 0) { for (int j = 0; j < d.cbs; ++j) colind[start + o + j] = (int32_t)((uint64_t)r.cB * d.cbs + j); o += d.cbs; }
    for (int s = 0; s < r.ncol; ++s)
        for (int kp = 0; kp < d.fbs; ++kp)
            colind[start + o + s * d.fbs + kp] = (int32_t)((uint64_t)d.cbs * d.ncells + (uint64_t)r.colcomp[s] * d.fbs + kp);
}

hipError_t asm_pattern(hipStream_t stream, const FaceSystemView &v, int cbs, int fbs, int64_t *rowptr, int32_t *colind)
{
    const AsmDims d = asm_dims(v, cbs, fbs);
    hipLaunchKernelGGL(asm_pattern_cells_kernel, dim3(blocks_for((size_t)v.ncells * cbs)), dim3(256), 0, stream, d, v.cell_faces,
                       v.face_compress, v.cprefix, rowptr, colind);
    hipLaunchKernelGGL(asm_pattern_faces_kernel, dim3(blocks_for(((size_t)v.nown + 1) * fbs)), dim3(256), 0, stream, d, v.faces, v.colprefix,
                       v.fprefix, rowptr, colind);
    return hipGetLastError();
}

// ---- numeric phase ---------------------------------------------------------------------------------------------------
// Cell rows: one wavefront per U cells at a time; lane e of a pass holds entry e of the cell's block of rows (row i = e / R,
// position e % R): consecutive lanes write consecutive entries.  The reads run along a row of the column-major lc (stride
// msize); the lines they touch are shared by the rows of the cell and stay in the vector L1 / L2.
template <int CBS, int FBS, int U>
__global__ __launch_bounds__(256) void asm_fill_cells_kernel(AsmDims d, uint32_t c_begin, uint32_t c_end, const uint32_t *__restrict__ cell_faces,
                                                             const int32_t *__restrict__ face_compress,
                                                             const uint32_t *__restrict__ cprefix, const double *__restrict__ lc,
                                                             const double *__restrict__ rhs, const double *__restrict__ g,
                                                             double *__restrict__ values, double *__restrict__ RHS)
{
    constexpr int MS = CBS + 4 * FBS, RMAX = CBS + 4 * FBS, EMAX = CBS * RMAX;
    constexpr int PASSES = (EMAX + 63) / 64;
    const uint32_t lane = threadIdx.x % 64u, wave = blockIdx.x * (256u / 64u) + threadIdx.x / 64u;
    CellFaces cf[U];
    uint32_t cpre[U];
    bool on[U];
    uint32_t cell[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t c = c_begin + wave * U + u;
        on[u] = c < c_end;
        cell[u] = on[u] ? c : 0u;
        cf[u] = cell_faces_sorted(cell_faces, face_compress, cell[u]);
        cpre[u] = cprefix[cell[u]];
    }
    const double *src[U][PASSES];
    size_t dst[U][PASSES];
    bool ok[U][PASSES];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t R = (uint32_t)(CBS + cf[u].n * FBS);
        const uint64_t start = cell_block_start(d.cbs, d.fbs, cell[u], cpre[u]);
        const double *A = lc + (size_t)cell[u] * (MS * MS);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const uint32_t e = lane + 64u * p;
            ok[u][p] = on[u] && e < (uint32_t)CBS * R;
            const uint32_t ee = ok[u][p] ? e : 0u;
            const uint32_t i = ee / R, jj = ee - i * R;
            uint32_t j = jj;
            if (jj >= (uint32_t)CBS) {
                const uint32_t s = (jj - CBS) / (uint32_t)FBS, kp = (jj - CBS) % (uint32_t)FBS;
                const int lf = s == 0 ? cf[u].lf[0] : s == 1 ? cf[u].lf[1] : s == 2 ? cf[u].lf[2] : cf[u].lf[3];
                j = (uint32_t)(CBS + lf * FBS) + kp;
            }
            src[u][p] = A + (size_t)j * MS + i;
            dst[u][p] = (size_t)start + e;
        }
    }
    double v[U][PASSES];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < PASSES; ++p) v[u][p] = *src[u][p];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < PASSES; ++p)
            if (ok[u][p]) values[dst[u][p]] = v[u][p];
    // right-hand side of the cell rows: rhs_c(i) minus the Dirichlet columns times the boundary data, in local column order
    // (hho.hpp:401, 405; the sums pa_triplets_batch returns per local row)
    if (RHS != nullptr) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (on[u] && lane < (uint32_t)CBS) {
                double s = rhs != nullptr ? rhs[(size_t)cell[u] * CBS + lane] : 0.0;
                if (cf[u].n < 4) s = dirichlet_rhs_contrib<CBS, FBS>(cell_faces, face_compress, lc, g, cell[u], lane, s);
                RHS[(size_t)cell[u] * CBS + lane] = s;
            }
        }
    }
}

// Face rows: one wavefront per U faces at a time, lane e of a pass = entry e of the face's block of fbs rows.
template <int CBS, int FBS, int U>
__global__ __launch_bounds__(256) void asm_fill_faces_kernel(AsmDims d, uint32_t q_begin, uint32_t q_end, const uint32_t *__restrict__ cell_faces,
                                                             const int32_t *__restrict__ face_compress,
                                                             const CondFaceLean *__restrict__ lean, const uint32_t *__restrict__ colprefix,
                                                             const uint32_t *__restrict__ fprefix, const double *__restrict__ lc,
                                                             const double *__restrict__ g, double *__restrict__ values,
                                                             double *__restrict__ RHS)
{
    constexpr int MS = CBS + 4 * FBS, RMAX = 2 * CBS + 7 * FBS, EMAX = FBS * RMAX;
    constexpr int PASSES = (EMAX + 63) / 64;
    const uint32_t lane = threadIdx.x % 64u, wave = blockIdx.x * (256u / 64u) + threadIdx.x / 64u;
    CondFaceLean r[U];
    uint32_t cpre[U], fpre[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t q = q_begin + wave * U + u;
        on[u] = q < q_end;
        const uint32_t qq = on[u] ? q : 0u;
        r[u] = lean[qq];
        cpre[u] = colprefix[qq];
        fpre[u] = fprefix[qq];
    }
    const double *pa_[U][PASSES], *pb_[U][PASSES];
    size_t dst[U][PASSES];
    bool ok[U][PASSES], two[U][PASSES];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t ncol = lean_ncol(r[u].packed), rows = lean_rows(r[u].packed);
        const bool hasA_ = r[u].cA >= 0, hasB_ = r[u].cB >= 0;
        const uint32_t ncell = (uint32_t)hasA_ + (uint32_t)hasB_;
        const uint32_t R = ncell * CBS + ncol * FBS;
        const uint64_t start = face_block_start(d.cell_nnz, d.cbs, d.fbs, fpre[u], cpre[u]);
        const double *LA = lc + (size_t)(hasA_ ? r[u].cA : 0) * (MS * MS), *LB = lc + (size_t)(hasB_ ? r[u].cB : 0) * (MS * MS);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const uint32_t e = lane + 64u * p;
            ok[u][p] = on[u] && e < (uint32_t)FBS * R;
            const uint32_t ee = ok[u][p] ? e : 0u;
            const uint32_t k = ee / R, jj = ee - k * R;
            const uint32_t rowA = CBS + frows_A(rows) * FBS + k, rowB = CBS + frows_B(rows) * FBS + k;
            const double *pA = LA, *pB = LB;
            bool useA = false, useB = false;
            if (jj < ncell * CBS) {
                const bool second = jj >= (uint32_t)CBS;               // the second cell block (only with two cells)
                const uint32_t j = second ? jj - CBS : jj;
                const bool fromA = hasA_ && !second;
                useA = fromA; useB = !fromA;
                pA = LA + (size_t)j * MS + rowA;
                pB = LB + (size_t)j * MS + rowB;
            } else {
                const uint32_t s = (jj - ncell * CBS) / (uint32_t)FBS, kp = (jj - ncell * CBS) % (uint32_t)FBS;
                const uint32_t code = lean_code(r[u].packed, s);
                useA = (code & FCODE_HAS_A) != 0; useB = (code & FCODE_HAS_B) != 0;
                pA = LA + (size_t)(CBS + fcode_lf_A(code) * FBS + kp) * MS + rowA;
                pB = LB + (size_t)(CBS + fcode_lf_B(code) * FBS + kp) * MS + rowB;
            }
            useA = useA && ok[u][p]; useB = useB && ok[u][p];
            pa_[u][p] = useA ? pA : (useB ? pB : lc);
            pb_[u][p] = useB ? pB : lc;
            two[u][p] = useA && useB;
            dst[u][p] = (size_t)start + e;
        }
    }
    double va[U][PASSES], vb[U][PASSES];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < PASSES; ++p) { va[u][p] = *pa_[u][p]; vb[u][p] = *pb_[u][p]; }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < PASSES; ++p)
            if (ok[u][p]) values[dst[u][p]] = two[u][p] ? va[u][p] + vb[u][p] : va[u][p];
    if (RHS != nullptr) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (on[u] && lane < (uint32_t)FBS) {
                const uint32_t rows = lean_rows(r[u].packed);
                const bool dcols = lean_dirichlet(r[u].packed);
                const int rowA = CBS + (int)frows_A(rows) * FBS + (int)lane, rowB = CBS + (int)frows_B(rows) * FBS + (int)lane;
                double b = 0.0;
                bool have = false;
                if (r[u].cA >= 0) { b = dcols ? dirichlet_rhs_contrib<CBS, FBS>(cell_faces, face_compress, lc, g, (uint32_t)r[u].cA, rowA, 0.0) : 0.0; have = true; }
                if (r[u].cB >= 0) {
                    const double w = dcols ? dirichlet_rhs_contrib<CBS, FBS>(cell_faces, face_compress, lc, g, (uint32_t)r[u].cB, rowB, 0.0) : 0.0;
                    b = have ? b + w : w;
                }
                RHS[(size_t)d.cbs * d.ncells + (size_t)(q_begin + wave * U + u) * FBS + lane] = b;
            }
        }
    }
}

// cells / faces a wavefront has in flight at a time (their descriptors, then their gathers)
#ifndef PA_ASM_UNROLL
#define PA_ASM_UNROLL 2
#endif
template <int CBS, int FBS>
static hipError_t asm_fill_t(hipStream_t stream, const FaceSystemView &v, const AsmDims &d, const double *lc, const double *rhs,
                             const double *g, double *values, double *RHS)
{
    constexpr int U = PA_ASM_UNROLL;
    hipLaunchKernelGGL((asm_fill_cells_kernel<CBS, FBS, U>), dim3(((size_t)d.ncells + 4 * U - 1) / (4 * U)), dim3(256), 0, stream, d, 0u, d.ncells,
                       v.cell_faces, v.face_compress, v.cprefix, lc, rhs, g, values, RHS);
    if (d.nown > 0)
        hipLaunchKernelGGL((asm_fill_faces_kernel<CBS, FBS, U>), dim3(((size_t)d.nown + 4 * U - 1) / (4 * U)), dim3(256), 0, stream, d, 0u, d.nown,
                           v.cell_faces, v.face_compress, v.lean, v.colprefix, v.fprefix, lc, g, values, RHS);
    return hipGetLastError();
}

hipError_t asm_fill(hipStream_t stream, const FaceSystemView &v, int cbs, int fbs, const double *lc, const double *rhs, const double *g,
                    double *values, double *RHS)
{
    if (v.ncells == 0) return hipSuccess;
    const AsmDims d = asm_dims(v, cbs, fbs);
#define PA_ASM_CASE(C, F) if (cbs == C && fbs == F) return asm_fill_t<C, F>(stream, v, d, lc, rhs, g, values, RHS)
    PA_ASM_CASE(1, 1); PA_ASM_CASE(3, 1); PA_ASM_CASE(1, 2); PA_ASM_CASE(3, 2); PA_ASM_CASE(6, 2); PA_ASM_CASE(3, 3); PA_ASM_CASE(6, 3);
    PA_ASM_CASE(10, 3); PA_ASM_CASE(6, 4); PA_ASM_CASE(10, 4); PA_ASM_CASE(15, 4);
#undef PA_ASM_CASE
    return hipErrorInvalidValue;
}

// ---- the fused path: pa_assembler_csr_assemble ---------------------------------------------------------------------------
// hho_local_ops_kernel<Cfg, MODE_ASM> writes the values from its LDS image (hho_asm_scatter.hpp).  It works cell by cell, so it
// needs the inverse of the face-indexed tables above: per cell, where the rows of its faces start and where its columns sit in
// them.  One thread per cell, once per mesh.
__global__ __launch_bounds__(256) void asm_scatter_table_kernel(uint32_t ncells, const uint32_t *cell_faces, const int32_t *face_compress,
                                                                const uint32_t *cprefix, const CondFace *faces, const uint32_t *colprefix,
                                                                const uint32_t *fprefix, AsmCellRec *out)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const CellFaces cf = cell_faces_sorted(cell_faces, face_compress, c);
    const uint4 f4 = *reinterpret_cast<const uint4 *>(cell_faces + 4 * (size_t)c);
    const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w};
    AsmCellRec rec;
    rec.cpre = cprefix[c];
    rec.order = (uint32_t)cf.n << 8;
    for (int s = 0; s < cf.n; ++s) rec.order |= (uint32_t)cf.lf[s] << (2 * s);
    int32_t comp[4];
    for (int lf = 0; lf < 4; ++lf) comp[lf] = face_compress[f[lf]];
    for (int lf = 0; lf < 4; ++lf) {
        rec.comp[lf] = comp[lf]; rec.face[lf] = f[lf];
        rec.fpre[lf] = rec.colpre[lf] = 0; rec.pack[lf] = 0xfffu;
        if (comp[lf] < 0) continue;
        const CondFace &r = faces[comp[lf]];
        const uint32_t ncell = (uint32_t)(r.cA >= 0) + (uint32_t)(r.cB >= 0);
        const bool second = r.cA >= 0 && r.cA != (int32_t)c;       // the lower cell id comes first
        uint32_t pk = (ncell << 12) | ((uint32_t)second << 14) | ((uint32_t)r.ncol << 16);
        for (int m = 0; m < 4; ++m) {
            uint32_t pos = 7u;
            if (comp[m] >= 0)
                for (int s = 0; s < (int)r.ncol; ++s)
                    if (r.colcomp[s] == comp[m]) pos = (uint32_t)s;
            pk |= pos << (3 * m);
        }
        rec.pack[lf] = pk; rec.fpre[lf] = fprefix[comp[lf]]; rec.colpre[lf] = colprefix[comp[lf]];
    }
    rec.pad_[0] = rec.pad_[1] = 0;
    out[c] = rec;
}

hipError_t asm_build_scatter_table(hipStream_t stream, const FaceSystemView &v, AsmCellRec *out)
{
    if (v.ncells == 0) return hipSuccess;
    hipLaunchKernelGGL(asm_scatter_table_kernel, dim3(blocks_for(v.ncells)), dim3(256), 0, stream, v.ncells, v.cell_faces, v.face_compress,
                       v.cprefix, v.faces, v.colprefix, v.fprefix, out);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

// The entries with more than one contributor -- a face's own fbs x fbs block and its right-hand side -- are accumulated by
// the scatter and start from zero; everything else in `values` is overwritten by exactly one store and is left alone.
// One thread per accumulated entry: (face q, row k, column kp), kp == fbs: the right-hand side of row k.
__global__ __launch_bounds__(256) void asm_zero_accumulated_kernel(AsmDims d, const CondFace *faces, const uint32_t *colprefix,
                                                                   const uint32_t *fprefix, double *values, double *RHS)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = (uint32_t)(d.fbs * (d.fbs + 1));
    const uint64_t q = t / per;
    if (q >= d.nown) return;
    const uint32_t k = (uint32_t)(t % per) / (uint32_t)(d.fbs + 1), kp = (uint32_t)(t % per) % (uint32_t)(d.fbs + 1);
    if (kp == (uint32_t)d.fbs) {
        if (RHS != nullptr) RHS[(uint64_t)d.cbs * d.ncells + q * d.fbs + k] = 0.0;
        return;
    }
    const CondFace &r = faces[q];
    const uint32_t ncell = (uint32_t)(r.cA >= 0) + (uint32_t)(r.cB >= 0);
    const uint32_t R = ncell * d.cbs + (uint32_t)r.ncol * d.fbs;
    for (int s = 0; s < (int)r.ncol; ++s)
        if (r.colcomp[s] == (int32_t)q)
            values[face_block_start(d.cell_nnz, d.cbs, d.fbs, fprefix[q], colprefix[q]) + (uint64_t)k * R + ncell * d.cbs + (uint32_t)s * d.fbs + kp] = 0.0;
}

hipError_t asm_zero_accumulated(hipStream_t stream, const FaceSystemView &v, int cbs, int fbs, double *values, double *RHS)
{
    if (v.nown == 0) return hipSuccess;
    hipLaunchKernelGGL(asm_zero_accumulated_kernel, dim3(blocks_for((size_t)v.nown * fbs * (fbs + 1))), dim3(256), 0, stream,
                       asm_dims(v, cbs, fbs), v.faces, v.colprefix, v.fprefix, values, RHS);
    return hipGetLastError();
}

// ---- the fictitious-domain problem: pa_fictdom_csr_assemble ---------------------------------------------------------------
// The operator pass leaves the cut cells out (AsmScatterArgs::cell_loc); their operators come from the cut kernel in HBM
// (pa_cut_local_ops_batch: ncut x msize^2, column-major) and go through the SAME scatter.  One group of G lanes per cut cell,
// 64 / G cells per wavefront-sized block; G and LDI are those of the assembling instance of the pair.  A group fills its own
// image, the block meets at the barrier (the image is complete before the first read of the scatter), and no image is used
// twice: a block handles one round of cells.
template <int CBS, int FBS>
__global__ __launch_bounds__(64) void asm_cut_scatter_kernel(AsmScatterArgs s, uint32_t ncut, const uint32_t *__restrict__ cut_cells,
                                                             const double *__restrict__ cut_lc, const double *__restrict__ cut_rhs,
                                                             double *lc_out)
{
    constexpr int MS = CBS + 4 * FBS, G = asm_group_lanes(MS), LDI = asm_image_stride(MS), CPW = 64 / G;
    __shared__ double smem[CPW * MS * LDI];
    const int g = (int)threadIdx.x / G, l = (int)threadIdx.x % G;
    const uint64_t cc0 = (uint64_t)blockIdx.x * CPW + (uint32_t)g;
    const bool valid = cc0 < ncut;
    const size_t cc = valid ? (size_t)cc0 : (size_t)ncut - 1;      // (ncut > 0: the grid has no block otherwise)
    const size_t cell = cut_cells[cc];
    const double *src = cut_lc + cc * (size_t)(MS * MS);
    double *img = smem + g * (MS * LDI);
    for (int e = l; e < MS * MS; e += G) {
        const int j = e / MS, i = e - j * MS;
        img[i + j * LDI] = src[e];
    }
    const double fT = (cut_rhs != nullptr && l < CBS) ? cut_rhs[cc * (size_t)CBS + l] : 0.0;
    __syncthreads();
    asm_scatter_cell<G, CBS, FBS, LDI>(s, img, l, cell, valid, fT, lc_out != nullptr ? lc_out + cell * (size_t)(MS * MS) : nullptr);
}

hipError_t asm_cut_scatter(hipStream_t stream, int face_deg, const AsmScatterArgs &s, uint32_t ncut, const uint32_t *cut_cells,
                           const double *cut_lc, const double *cut_rhs, double *lc_out)
{
    if (ncut == 0) return hipSuccess;
#define PA_CUT_CASE(K, C, F)                                                                                                   \
    case K: {                                                                                                                  \
        constexpr uint32_t CPW = 64 / asm_group_lanes(C + 4 * F);                                                              \
        hipLaunchKernelGGL((asm_cut_scatter_kernel<C, F>), dim3((ncut + CPW - 1) / CPW), dim3(64), 0, stream, s, ncut, cut_cells, \
                           cut_lc, cut_rhs, lc_out);                                                                           \
    } break
    switch (face_deg) {
    PA_CUT_CASE(0, 3, 1);
    PA_CUT_CASE(1, 6, 2);
    PA_CUT_CASE(2, 10, 3);
    default: return hipErrorInvalidValue;
    }
#undef PA_CUT_CASE
    return hipGetLastError();
}

}  // namespace pa
