// obstacle_csr.hip -- obstacle_assembler's global system for cell degree 0 built directly in CSR.
//
// obstacle_assembler<Mesh> (src/methods/hho_bits/hho.hpp:471-751) is rebuilt in every iteration of the primal-dual active set
// loop (apps/obstacle/obstacle.cpp:119-193, the cell loop :147-158): assemble (:609-695) pushes the triplets of a cell with its
// columns renumbered by the active set, finalize (:746-750) hands them to setFromTriplets.  For cbs = 1 that system is the plain
// assembler's system of the pair (0, fd) (assembler_csr.hip) with its columns renumbered -- the rows are the same, cell rows at c,
// face rows at ncells + comp fbs + k (:631, :644):
//   * the cell column of an inactive cell c becomes A_ct[c] (:625, :632); that of an active cell disappears, its products with
//     gamma[c] go to the right-hand side (:676-679);
//   * a face column moves from ncells + comp fbs + k to num_I + comp fbs + k (:645);
//   * the row of an active cell gains 1.0 in the multiplier column num_I + fbs num_other + B_ct[c] (:688-693).
// A_ct is monotone in the cell id and the multiplier columns come last, so the pattern is an order-preserving compaction of the
// plain one: a cell row keeps its length (an active one swaps its cell column, the first, for its multiplier column, the last),
// a face row loses one entry per active adjacent cell.  With removed[q] the number of active cells of non-Dirichlet face q and
// rprefix its exclusive prefix sum, the block of face q starts fbs rprefix[q] entries before its place in the plain system and
// nnz = nnz_plain - fbs rprefix[nown].  Only a face's own diagonal block has two addends (one per cell, lower cell id first):
// every entry is written once, by one lane, consecutive lanes writing consecutive entries of a block of rows.
// Row pointers, column indices, values and nnz are bit-identical to pa_csr_from_triplets(pa_obstacle_triplets_batch(..)), the
// right-hand side to the scatter-add of that call's per-row sums in cell order onto zeros (tests/test_gpu_obstacle_csr.py): the
// sums come from the function the triplet kernel calls (obstacle_rhs.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_tmp.hpp"
#include "obstacle_csr.hpp"
#include "obstacle_rhs.hpp"

namespace pa {

// removed[q] = active cells of non-Dirichlet face q (q < nown), removed[nown] = 0: the sentinel of the scan
__global__ __launch_bounds__(256) void obstacle_removed_kernel(uint32_t nown, const CondFaceLean *lean, const uint8_t *in_A,
                                                               uint32_t *removed)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nown) return;
    uint32_t n = 0;
    if (t < nown) {
        const int32_t cA = lean[t].cA, cB = lean[t].cB;
        n = (uint32_t)(cA >= 0 && in_A[cA] != 0) + (uint32_t)(cB >= 0 && in_A[cB] != 0);
    }
    removed[t] = n;
}

// what obstacle_rhs_row needs of cell c: col[j] < 0 for the dropped columns (the cell column of an active cell, the unknowns of
// Dirichlet faces) and the boundary data of the latter (hho.hpp:655-660)
template <int FBS>
__device__ __forceinline__ void obstacle_known(const ObstacleCsrArgs &a, uint32_t c, int32_t (&col)[1 + 4 * FBS],
                                               double (&dd)[1 + 4 * FBS])
{
    const uint4 f = *reinterpret_cast<const uint4 *>(a.v.cell_faces + 4 * (size_t)c);
    const uint32_t fl[4] = {f.x, f.y, f.z, f.w};
    col[0] = a.in_A[c] != 0 ? -1 : 0;
    dd[0] = 0.0;
#pragma unroll
    for (int lf = 0; lf < 4; ++lf) {
        const bool dirichlet = a.v.face_compress[fl[lf]] < 0;
#pragma unroll
        for (int k = 0; k < FBS; ++k) {
            col[1 + lf * FBS + k] = dirichlet ? -1 : 0;
            dd[1 + lf * FBS + k] = (dirichlet && a.g != nullptr) ? a.g[(size_t)fl[lf] * FBS + k] : 0.0;
        }
    }
}

// Cell rows: G lanes per cell, lane e = entry e of the cell's one row (1 + 4 fbs < G entries at most); the group's last lane,
// which holds no entry, forms the right-hand side.
template <int FBS>
__global__ __launch_bounds__(256) void obstacle_csr_cells_kernel(ObstacleCsrArgs a)
{
    constexpr int MS = 1 + 4 * FBS, G = MS < 16 ? 16 : 32;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t / G >= a.v.ncells) return;
    const uint32_t c = (uint32_t)(t / G);
    const int e = (int)(t % G);
    const CellFaces cf = cell_faces_sorted<true>(a.v.cell_faces, a.v.face_compress, c);
    const bool active = a.in_A[c] != 0;
    const int len = 1 + cf.n * FBS;
    const uint64_t start = cell_block_start(1, FBS, c, a.v.cprefix[c]);
    const double *A = a.lc + (size_t)c * (MS * MS);
    if (e == 0) a.rowptr[c] = (int64_t)start;
    if (e < len) {
        int32_t col;
        double v;
        if (!active && e == 0) {                                   // the cell's own column (hho.hpp:625, :632)
            col = a.A_ct[c];
            v = A[0];
        } else if (active && e == len - 1) {                       // the multiplier coupling (:688-693)
            col = (int32_t)(a.num_I + (uint64_t)FBS * a.num_other + (uint64_t)a.B_ct[c]);
            v = 1.0;
        } else {
            const int fe = active ? e : e - 1;
            const int s = fe / FBS, kp = fe % FBS;
            const int32_t cs = s == 0 ? cf.comp[0] : s == 1 ? cf.comp[1] : s == 2 ? cf.comp[2] : cf.comp[3];
            const int lf = s == 0 ? cf.lf[0] : s == 1 ? cf.lf[1] : s == 2 ? cf.lf[2] : cf.lf[3];
            col = (int32_t)(a.num_I + (uint64_t)cs * FBS + kp);    // :645
            v = A[(size_t)(1 + lf * FBS + kp) * MS];
        }
        a.colind[start + e] = col;
        a.values[start + e] = v;
    }
    if (a.RHS != nullptr && e == G - 1) {
        int32_t kcol[MS];
        double dd[MS];
        obstacle_known<FBS>(a, c, kcol, dd);
        const double s = obstacle_rhs_row(A, MS, 1, 0, true, kcol, dd, a.gamma[c], a.rhs != nullptr ? a.rhs + c : nullptr);
        a.RHS[c] = 0.0 + s;
    }
}

// Face rows: G lanes per non-Dirichlet face, lane l = entries l, l + G, .. of the face's block of fbs rows; group nown writes the
// last row pointer.
template <int FBS>
__global__ __launch_bounds__(256) void obstacle_csr_faces_kernel(ObstacleCsrArgs a, const uint32_t *__restrict__ rprefix)
{
    constexpr int MS = 1 + 4 * FBS, G = FBS == 1 ? 16 : FBS == 2 ? 32 : 64;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t / G > a.v.nown) return;
    const uint32_t q = (uint32_t)(t / G);
    const int l = (int)(t % G);
    int64_t *rp = a.rowptr + a.v.ncells;
    const uint64_t start = face_block_start(a.cell_nnz, 1, FBS, a.v.fprefix[q], a.v.colprefix[q]) - (uint64_t)FBS * rprefix[q];
    if (q == a.v.nown) {
        if (l == 0) rp[(size_t)a.v.nown * FBS] = (int64_t)start;
        return;
    }
    const CondFace &r = a.v.faces[q];
    const int32_t cA = r.cA, cB = r.cB;
    const bool hasA = cA >= 0, hasB = cB >= 0;
    const bool keepA = hasA && a.in_A[cA] == 0, keepB = hasB && a.in_A[cB] == 0;
    const int nkeep = (int)keepA + (int)keepB, ncol = r.ncol;
    const int R = nkeep + ncol * FBS;
    const int rowA = 1 + (int)frows_A(r.rows) * FBS, rowB = 1 + (int)frows_B(r.rows) * FBS;
    const double *LA = a.lc + (size_t)(hasA ? cA : 0) * (MS * MS), *LB = a.lc + (size_t)(hasB ? cB : 0) * (MS * MS);
    for (int e = l; e < FBS * R; e += G) {
        const int k = e / R, jj = e - k * R;
        int32_t col;
        double v;
        if (jj < nkeep) {                                          // the inactive cells of the face, lower cell id first
            const bool fromA = keepA && jj == 0;
            col = a.A_ct[fromA ? cA : cB];
            v = fromA ? LA[rowA + k] : LB[rowB + k];
        } else {
            const int s = (jj - nkeep) / FBS, kp = (jj - nkeep) % FBS;
            const uint32_t code = r.code[s];
            const bool useA = (code & FCODE_HAS_A) != 0, useB = (code & FCODE_HAS_B) != 0;
            col = (int32_t)(a.num_I + (uint64_t)r.colcomp[s] * FBS + kp);
            const double va = useA ? LA[(size_t)(1 + fcode_lf_A(code) * FBS + kp) * MS + rowA + k] : 0.0;
            const double vb = useB ? LB[(size_t)(1 + fcode_lf_B(code) * FBS + kp) * MS + rowB + k] : 0.0;
            v = useA && useB ? va + vb : (useA ? va : vb);         // two addends: the face's own block
        }
        a.colind[start + e] = col;
        a.values[start + e] = v;
    }
    if (l < FBS) {
        rp[(size_t)q * FBS + l] = (int64_t)(start + (uint64_t)l * R);
        if (a.RHS != nullptr) {
            int32_t kcol[MS];
            double dd[MS];
            double b = 0.0;                                        // the per-cell sums, added in cell order onto zero
            if (hasA) {
                obstacle_known<FBS>(a, (uint32_t)cA, kcol, dd);
                b += obstacle_rhs_row(LA, MS, 1, rowA + l, true, kcol, dd, a.gamma[cA], nullptr);
            }
            if (hasB) {
                obstacle_known<FBS>(a, (uint32_t)cB, kcol, dd);
                b += obstacle_rhs_row(LB, MS, 1, rowB + l, true, kcol, dd, a.gamma[cB], nullptr);
            }
            a.RHS[(size_t)a.v.ncells + (size_t)q * FBS + l] = b;
        }
    }
}

template <int FBS>
static hipError_t obstacle_csr_fill_t(hipStream_t stream, const ObstacleCsrArgs &a, const uint32_t *rprefix)
{
    constexpr size_t GC = 1 + 4 * FBS < 16 ? 16 : 32, GF = FBS == 1 ? 16 : FBS == 2 ? 32 : 64;
    if (a.v.ncells > 0)
        hipLaunchKernelGGL((obstacle_csr_cells_kernel<FBS>), dim3(blocks_for((size_t)a.v.ncells * GC)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL((obstacle_csr_faces_kernel<FBS>), dim3(blocks_for(((size_t)a.v.nown + 1) * GF)), dim3(256), 0, stream, a, rprefix);
    return hipGetLastError();
}

hipError_t obstacle_csr_assemble(hipStream_t stream, int fbs, const ObstacleCsrArgs &args, uint32_t *removed_total)
{
    if (fbs < 1 || fbs > 4) return hipErrorInvalidValue;
    DeviceTmp tmp(stream);
    uint32_t *removed = nullptr, *rprefix = nullptr;
    if (!tmp.alloc(&removed, (size_t)args.v.nown + 1) || !tmp.alloc(&rprefix, (size_t)args.v.nown + 1)) return tmp.error();
    hipLaunchKernelGGL(obstacle_removed_kernel, dim3(blocks_for((size_t)args.v.nown + 1)), dim3(256), 0, stream, args.v.nown, args.v.lean,
                       args.in_A, removed);
    if (!tmp.ok(hipGetLastError())) return tmp.error();
    if (exclusive_scan_with_total<uint32_t>(stream, removed, rprefix, (size_t)args.v.nown + 1, tmp, nullptr) != hipSuccess) return tmp.error();
    uint32_t total = 0;
    if (!tmp.ok(hipMemcpyAsync(&total, rprefix + args.v.nown, sizeof(uint32_t), hipMemcpyDeviceToHost, stream))) return tmp.error();
    const hipError_t e = fbs == 1 ? obstacle_csr_fill_t<1>(stream, args, rprefix) : fbs == 2 ? obstacle_csr_fill_t<2>(stream, args, rprefix)
                       : fbs == 3 ? obstacle_csr_fill_t<3>(stream, args, rprefix) : obstacle_csr_fill_t<4>(stream, args, rprefix);
    if (!tmp.ok(e)) return tmp.error();
    if (!tmp.ok(hipStreamSynchronize(stream))) return tmp.error();      // the count is on the host, the temporaries are free to go
    *removed_total = total;
    return hipSuccess;
}

}  // namespace pa
