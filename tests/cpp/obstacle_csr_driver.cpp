// obstacle_csr_driver.cpp -- obstacle_assembler<Mesh>::assemble_all + finalize (triplets, setFromTriplets on the device, the
// right-hand side scattered on the host) against assemble_all_csr (pa_obstacle_csr_assemble: the system directly in CSR) on two
// assemblers of the same mesh and active set: the cell loop of obstacle.cpp:147-158 with finalize (hho.hpp:609-695, :746-750).
// The active set is the contact disc r < 0.7 of obstacle.cpp at the barycentres, gamma a fixed non-constant vector.
// Compiled against proton_amd/host/hho.hpp only: no Eigen, no HIP headers.
//   usage: obstacle_csr_driver <face_degree> <N>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../proton_amd/host/hho.hpp"

using RealType = double;
using mesh_type = quad_mesh<RealType>;

int main(int argc, char **argv)
{
    const size_t fd = argc > 1 ? std::atoi(argv[1]) : 1;
    const size_t N = argc > 2 ? std::atoi(argv[2]) : 8;
    mesh_init_params<RealType> mip;                                         // obstacle.cpp:234-238,276
    mip.Nx = N; mip.Ny = N;
    mip.min_x = -1; mip.max_x = 1; mip.min_y = -1; mip.max_y = 1;
    mesh_type msh(mip);
    hho_degree_info hdi(0, fd);                                             // obstacle.cpp:51

    const size_t num_cells = msh.cells.size(), num_faces = msh.faces.size();
    pa_sizes sz;
    auto &dev = proton_amd::device::instance();
    dev.check(pa_sizes_for(hdi.c_abi(), PA_QUAD_TENSOR, &sz), "pa_sizes_for");
    proton_amd::batch_cache<mesh_type>::instance().ensure_mesh(msh);
    proton_amd::device_buffer<double> d_lc(num_cells * sz.msize * sz.msize), d_rhs(num_cells * sz.cbs), d_g(num_faces * sz.fbs);
    dev.check(pa_local_ops_batch(dev.ctx(), hdi.c_abi(), PA_QUAD_TENSOR, PA_STAB_FANCY, 0, num_cells, nullptr, nullptr, nullptr, d_lc.get(),
                                 nullptr), "pa_local_ops_batch");
    dev.check(pa_cell_rhs_batch(dev.ctx(), 0, 1, PA_QUAD_TENSOR, PA_FN_OBSTACLE_RHS, nullptr, 0, num_cells, d_rhs.get()), "pa_cell_rhs_batch");
    dev.check(pa_dirichlet_data_batch(dev.ctx(), (int)fd, PA_FN_OBSTACLE_SOL, nullptr, d_g.get()), "pa_dirichlet_data_batch");

    std::vector<bool> in_A(num_cells);
    std::vector<RealType> gamma(num_cells);
    size_t num_A = 0;
    for (size_t c = 0; c < num_cells; ++c) {
        const RealType x = -1.0 + (RealType(c % N) + 0.5) * 2.0 / RealType(N), y = -1.0 + (RealType(c / N) + 0.5) * 2.0 / RealType(N);
        in_A[c] = std::sqrt(x * x + y * y) < 0.7;
        num_A += in_A[c] ? 1 : 0;
        gamma[c] = 0.25 * std::sin(3.0 * x + 1.0) + y * y;
    }

    auto two_step = make_obstacle_assembler(msh, in_A, hdi);
    two_step.assemble_all(msh, d_lc.get(), d_rhs.get(), d_g.get(), gamma);
    two_step.finalize();
    auto direct = make_obstacle_assembler(msh, in_A, hdi);
    direct.assemble_all_csr(msh, d_lc.get(), d_rhs.get(), d_g.get(), gamma);
    direct.finalize();                                                      // a no-op for this assembly

    const auto &A = two_step.LHS, &B = direct.LHS;
    const bool same_pattern = A.rows() == B.rows() && A.rowptr == B.rowptr && A.colind == B.colind;
    bool same_values = A.values.size() == B.values.size();
    for (size_t k = 0; same_values && k < A.values.size(); ++k) same_values = A.values[k] == B.values[k];
    bool same_rhs = two_step.RHS.size() == direct.RHS.size();
    for (size_t i = 0; same_rhs && i < two_step.RHS.size(); ++i) same_rhs = two_step.RHS[i] == direct.RHS[i];
    std::printf("obstacle_csr fd %zu N %zu rows %zu nnz %zu active %zu same_pattern %d same_values %d same_rhs %d\n", fd, N,
                two_step.RHS.size(), A.values.size(), num_A, (int)same_pattern, (int)same_values, (int)same_rhs);
    return same_pattern && same_values && same_rhs ? 0 : 1;
}
