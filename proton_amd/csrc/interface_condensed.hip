// interface_condensed.hip -- the interface problem's global system (apps/cuthho/cuthho_square.cpp:1091-1443) condensed to its face
// unknowns on the device.
//
// Every cell block of interface_assembler's system couples only inside its cell, so the cell unknowns are eliminated cell by cell:
// S = A_FF - A_FT A_TT^-1 A_TF and g = -A_FT A_TT^-1 f_T of each cell's local matrix.  What is left is the same numbering without
// its cell blocks: unknown k of face block b at (face_table[F] + b) fbs + k.  Uncut cells are condensed in double by the plain
// mesh's static_condensation_kernel (hho_aux.hpp); a cut cell, whose [cell-, cell+] block A_TT has condition numbers to 1e8, in
// double-double by ifd_records_kernel<2 cbs, 8 fbs> (ifd_dense.hpp, the text the fictitious-domain problem uses too).  The cut
// cell's local matrix is symmetric (cut_interface_lc_kernel stores both copies of data and of the stabilization), so A_FT = A_TF^T.
//
// This file holds the addressing around the dense per-cell work of ifd_dense.hpp: where the cut cells' records go, the face values
// the recovery of the cell unknowns takes and where it puts u_T, and the info remap.  The face-only CSR and its triplets are the
// gather of interface_csr.hip reading these records (IfCondSource).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dd_arith.hpp"
#include "device_tmp.hpp"
#include "ifd_dense.hpp"
#include "interface_csr.hpp"

namespace pa {

namespace {

// ---- recovery: u_T = A_TT^-1 (f_T - A_TF u_F), one cell per wavefront ------------------------------------------------------
// CUT = false: the uncut cells (N = cbs, 4 fbs face unknowns, in double); CUT = true: the cut cells (N = 2 cbs, 8 fbs, in
// double-double).  u_F of a Dirichlet face: the boundary data for an uncut cell, zero for a cut cell (its slots were dropped).
template <int FD, bool CUT>
__global__ __launch_bounds__(64) void ifcond_recover_kernel(IfCsrMesh m, const uint32_t *cut_cells, uint32_t ncut, const double *lc,
                                                            const double *rhs, const double *g, const double *xF, double *full)
{
    using Ar = IfdAr<CUT>;
    constexpr int CBS = (FD + 3) * (FD + 2) / 2, FBS = FD + 1, N = CUT ? 2 * CBS : CBS, NFL = CUT ? 8 * FBS : 4 * FBS;
    __shared__ double uF[NFL];
    const int lane = threadIdx.x;
    const size_t n = CUT ? ncut : m.ncells;
    for (size_t t = blockIdx.x; t < n; t += gridDim.x) {
        const int32_t X = CUT ? (int32_t)cut_cells[t] : (int32_t)t;
        if (!CUT && m.cell_loc[X] == IF_LOC_CUT) continue;                                  // wave-uniform
        __syncthreads();
        if (lane < NFL) {
            size_t bdof;
            const int32_t j = if_face_index(m, IfDims{CBS, FBS}, (size_t)X, CUT, lane, &bdof);
            uF[lane] = j >= 0 ? xF[j] : ((!CUT && g != nullptr) ? g[bdof] : 0.0);
        }
        const auto *x = ifd_recover_cell<N, NFL, CUT>(lc, rhs, t, uF, lane);
        if (lane < N) full[(size_t)m.cell_table[X] * CBS + lane] = Ar::round(x[lane]);
    }
}

// a failed pivot j of static_condensation_kernel (info j + 1) reported as pa_condensed_ops_batch reports it: 200 + j + 1
__global__ __launch_bounds__(256) void ifcond_info_kernel(size_t n, int32_t *info)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && info[t] != 0) info[t] = 200 + info[t];
}

}  // namespace

// a face degree outside 0..2 is taken as 3
hipError_t ifcond_cut_records(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const double *lc_cut,
                              const double *rhs_cut, double *cond_cut, int32_t *info)
{
    if (ncut == 0) return hipSuccess;
    const dim3 grid(ncut < (uint32_t)max_blocks ? ncut : (uint32_t)max_blocks);
    ifd_for_degree<3>(face_deg >= 0 && face_deg < 3 ? face_deg : 3, [&](auto fd) {
        constexpr int N = (fd + 3) * (fd + 2), NF = 8 * (fd + 1), NTRI = NF * (NF + 1) / 2;
        // a block of S, then a block of g, each indexed by the cut cell's ordinal
        hipLaunchKernelGGL((ifd_records_kernel<N, NF>), grid, dim3(64), 0, stream, ncut, (const uint32_t *)nullptr, lc_cut, rhs_cut, cond_cut,
                           (size_t)NTRI, cond_cut + (size_t)ncut * NTRI, (size_t)NF, info);
    });
    return hipGetLastError();
}

hipError_t ifcond_info_remap(hipStream_t stream, size_t n, int32_t *info)
{
    if (n == 0 || info == nullptr) return hipSuccess;
    hipLaunchKernelGGL(ifcond_info_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, n, info);
    return hipGetLastError();
}

hipError_t ifcond_recover(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const double *lc,
                          const double *rhs, const double *lc_cut, const double *rhs_cut, const double *xF, double *full)
{
    const IfDims d = if_dims(face_deg);
    const size_t nF = (size_t)m.num_other_faces * d.fbs;
    if (nF) {
        hipLaunchKernelGGL(ifd_copy_kernel, dim3(blocks_for(nF)), dim3(256), 0, stream, nF, xF, full + (size_t)m.num_all_cells * d.cbs);
    }
    const dim3 gu(m.ncells < (uint32_t)max_blocks ? (m.ncells ? m.ncells : 1) : (uint32_t)max_blocks);
    const dim3 gc(a.ncut < (uint32_t)max_blocks ? (a.ncut ? a.ncut : 1) : (uint32_t)max_blocks);
    ifd_for_degree<3>(face_deg >= 0 && face_deg < 3 ? face_deg : 3, [&](auto fd) {
        if (m.ncells)
            hipLaunchKernelGGL((ifcond_recover_kernel<fd, false>), gu, dim3(64), 0, stream, m, a.cut_cells, a.ncut, lc, rhs, a.g, xF, full);
        if (a.ncut)
            hipLaunchKernelGGL((ifcond_recover_kernel<fd, true>), gc, dim3(64), 0, stream, m, a.cut_cells, a.ncut, lc_cut, rhs_cut, a.g, xF,
                               full);
    });
    return hipGetLastError();
}

}  // namespace pa
