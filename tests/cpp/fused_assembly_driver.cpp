// fused_assembly_driver.cpp -- assembler<Mesh>::assemble_all (local matrices to HBM, triplets, setFromTriplets on the device)
// against assemble_all_fused (pa_assembler_csr_assemble: the CSR values written from the local-operator kernel's on-chip image)
// on two assemblers of the same mesh and degrees: the span convergence_test.cpp:201-217 prints as "Matrix assembly".
// Compiled against proton_amd/host/hho.hpp only: no Eigen, no HIP headers.
//   usage: fused_assembly_driver <cell_degree> <face_degree> <N>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../proton_amd/host/hho.hpp"

using RealType = double;
using mesh_type = quad_mesh<RealType>;

int main(int argc, char **argv)
{
    const size_t cd = argc > 1 ? std::atoi(argv[1]) : 2;
    const size_t fd = argc > 2 ? std::atoi(argv[2]) : 1;
    const size_t N = argc > 3 ? std::atoi(argv[3]) : 8;
    hho_degree_info hdi(cd, fd);
    mesh_init_params<RealType> mip;
    mip.Nx = N; mip.Ny = N;
    mesh_type msh(mip);

    auto two_step = make_assembler(msh, hdi);
    two_step.assemble_all(msh, PA_STAB_FANCY, PA_FN_SIN_SIN_RHS, PA_FN_ONE);
    two_step.finalize();
    auto fused = make_assembler(msh, hdi);
    fused.assemble_all_fused(msh, PA_STAB_FANCY, PA_FN_SIN_SIN_RHS, PA_FN_ONE);
    fused.finalize();

    const auto &A = two_step.LHS, &B = fused.LHS;
    const bool same_pattern = A.rowptr == B.rowptr && A.colind == B.colind && A.values.size() == B.values.size() &&
                              two_step.RHS.size() == fused.RHS.size();
    // largest |difference| of a row over the row's largest |value|; the same for the right-hand side as one row
    RealType worst = 0.0;
    if (same_pattern)
        for (size_t i = 0; i + 1 < A.rowptr.size(); ++i) {
            RealType num = 0.0, den = 0.0;
            for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
                num = std::max(num, std::abs(A.values[k] - B.values[k]));
                den = std::max(den, std::abs(A.values[k]));
            }
            if (num > 0.0) worst = std::max(worst, num / den);
        }
    RealType rnum = 0.0, rden = 0.0;
    if (same_pattern)
        for (size_t i = 0; i < two_step.RHS.size(); ++i) {
            rnum = std::max(rnum, std::abs(two_step.RHS[i] - fused.RHS[i]));
            rden = std::max(rden, std::abs(two_step.RHS[i]));
        }
    std::printf("fused_assembly cd %zu fd %zu N %zu rows %zu nnz %zu same_pattern %d values_err %.3e rhs_err %.3e\n", cd, fd, N,
                two_step.RHS.size(), A.values.size(), (int)same_pattern, worst, rden > 0.0 ? rnum / rden : rnum);
    return same_pattern ? 0 : 1;
}
