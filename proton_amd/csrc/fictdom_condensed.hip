// fictdom_condensed.hip -- the fictitious-domain problem's global system (apps/cuthho/cuthho_square.cpp:881-905) condensed to its
// face unknowns on the device: the dense work of the cut cells.
//
// The system is the plain assembler<Mesh>'s over all cells, so numbering, pattern, fill, halo and expansion are condensed.hip's.
// An uncut cell's record comes from the fused condensed pass; a cut cell's local matrix (make_hho_laplacian with the Nitsche terms
// plus make_hho_cut_stabilization, cuthho_square.cpp:893-895) has the plain cell's shape -- cbs cell unknowns, 4 fbs face
// unknowns -- and an A_TT whose condition number reaches 1e8 on sliver cells, so it is eliminated in double-double by
// ifd_records_kernel<cbs, 4 fbs> (ifd_dense.hpp, the text the interface problem uses with 2 cbs and 8 fbs), which writes the packed
// [S | g] record of the cut cell's row.  cut_local_ops_kernel stores both copies of the symmetric entries, so A_FT = A_TF^T exactly.
// fdcond_recover_kernel gives the cut cells' u_T = A_TT^-1 (f_T - A_TF u_F) (take_local_data's cell part, :959-962) through
// ifd_recover_cell of the same header.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dd_arith.hpp"
#include "device_tmp.hpp"
#include "fictdom_condensed.hpp"
#include "ifd_dense.hpp"

namespace pa {

namespace {

// ---- recovery of the cut cells: u_T = A_TT^-1 (f_T - A_TF u_F) in double-double, one cut cell per wavefront ------------------
// u_F of a Dirichlet face is the boundary data (the plain assembler's rule, hho.hpp:408-449): uF holds it already.
template <int FD>
__global__ __launch_bounds__(64) void fdcond_recover_kernel(uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc, const double *cut_rhs,
                                                            const double *uF, double *uT)
{
    constexpr int N = (FD + 3) * (FD + 2) / 2, FBS = FD + 1, NFL = 4 * FBS;
    __shared__ double uf[NFL];
    const int lane = threadIdx.x;
    for (size_t cc = blockIdx.x; cc < ncut; cc += gridDim.x) {
        const size_t X = cut_cells[cc];
        __syncthreads();
        if (lane < NFL) uf[lane] = uF[X * NFL + lane];
        const dd *x = ifd_recover_cell<N, NFL, true>(cut_lc, cut_rhs, cc, uf, lane);
        if (lane < N) uT[X * N + lane] = dd_round(x[lane]);
    }
}

// an uncut cell outside `where` takes a zero right-hand side (cuthho_square.cpp:659-664); a cut cell's comes from cut_rhs
__global__ __launch_bounds__(256) void fdcond_masked_rhs_kernel(size_t total, uint32_t cbs, const int8_t *cell_loc, int where, const double *src,
                                                                double *dst)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int loc = cell_loc[t / cbs];
    dst[t] = (src != nullptr && loc == where) ? src[t] : 0.0;
}

}  // namespace

hipError_t fdcond_cut_records(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc,
                              const double *cut_rhs, double *cond, int32_t *info_cut)
{
    if (ncut == 0) return hipSuccess;
    const dim3 grid(ncut < (uint32_t)max_blocks ? ncut : (uint32_t)max_blocks);
    const bool known = ifd_for_degree<2>(face_deg, [&](auto fd) {
        constexpr int N = (fd + 3) * (fd + 2) / 2, NF = 4 * (fd + 1), NTRI = NF * (NF + 1) / 2;
        // the record of cell cut_cells[cc]: [upper triangle of S, column-packed | g]
        hipLaunchKernelGGL((ifd_records_kernel<N, NF>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, cond, (size_t)(NTRI + NF),
                           cond + NTRI, (size_t)(NTRI + NF), info_cut);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t fdcond_cut_recover(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc,
                              const double *cut_rhs, const double *uF, double *uT)
{
    if (ncut == 0) return hipSuccess;
    const dim3 grid(ncut < (uint32_t)max_blocks ? ncut : (uint32_t)max_blocks);
    const bool known = ifd_for_degree<2>(face_deg, [&](auto fd) {
        hipLaunchKernelGGL((fdcond_recover_kernel<fd>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, uF, uT);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t fdcond_masked_rhs(hipStream_t stream, size_t ncells, int cbs, const int8_t *cell_loc, int where, const double *src, double *dst)
{
    const size_t total = ncells * (size_t)cbs;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(fdcond_masked_rhs_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, total, (uint32_t)cbs, cell_loc, where, src, dst);
    return hipGetLastError();
}

hipError_t fdcond_copy(hipStream_t stream, size_t n, const double *src, double *dst)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ifd_copy_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, n, src, dst);
    return hipGetLastError();
}

}  // namespace pa
