// obstacle_solve_driver.cpp -- the reference's apps/obstacle (obstacle.cpp:47-227) with its primal-dual active set loop
// (:117-197) as one library call: solve_obstacle (proton_amd/host/hho.hpp) -> pa_obstacle_solve.  The local operators, the cell
// right-hand sides and the boundary data are computed once on the device, as in obstacle_driver's batched branch; active set,
// assembly, solve, expand_solution and the stopping test of every iteration stay there.  The energy error against
// project_function(sol_fun, di = 1) is obstacle_driver's, and so is the line printed.
// Compiled against proton_amd/host/hho.hpp only: no Eigen, no HIP headers.
//   usage: obstacle_solve_driver <degree> <N> [max outer iterations, default 50 = obstacle.cpp:119]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../proton_amd/host/hho.hpp"

using RealType = double;
using mesh_type = quad_mesh<RealType>;

int main(int argc, char **argv)
{
    const size_t degree = argc > 1 ? std::atoi(argv[1]) : 1;
    const size_t N = argc > 2 ? std::atoi(argv[2]) : 8;
    const size_t max_outer = argc > 3 ? std::atoi(argv[3]) : 50;               // obstacle.cpp:119: while (iter < 50)

    mesh_init_params<RealType> mip;                                         // obstacle.cpp:234-238,276
    mip.Nx = N; mip.Ny = N;
    mip.min_x = -1; mip.max_x = 1; mip.min_y = -1; mip.max_y = 1;
    mesh_type msh(mip);

    hho_degree_info hdi(0, degree);                                         // obstacle.cpp:51
    const RealType r0 = 0.7;
    auto sol_fun = [=](const mesh_type::point_type &pt) -> RealType {       // obstacle.cpp:76-81
        const RealType r = std::sqrt(pt.x() * pt.x() + pt.y() * pt.y());
        const RealType t = std::max(r * r - r0 * r0, 0.0);
        return t * t;
    };

    const size_t num_cells = msh.cells.size(), num_faces = msh.faces.size();
    std::vector<RealType> alpha, beta, gamma(num_cells, 0.0);               // obstacle.cpp:98-99, :113
    const size_t quadrature_degree_increase = 1;                            // obstacle.cpp:103

    pa_sizes sz;
    auto &dev = proton_amd::device::instance();
    dev.check(pa_sizes_for(hdi.c_abi(), PA_QUAD_TENSOR, &sz), "pa_sizes_for");
    proton_amd::batch_cache<mesh_type>::instance().ensure_mesh(msh);
    proton_amd::device_buffer<double> d_lc(num_cells * sz.msize * sz.msize), d_rhs(num_cells * sz.cbs), d_g(num_faces * sz.fbs);
    dev.check(pa_local_ops_batch(dev.ctx(), hdi.c_abi(), PA_QUAD_TENSOR, PA_STAB_FANCY, 0, num_cells, nullptr, nullptr, nullptr,
                                 d_lc.get(), nullptr), "pa_local_ops_batch");
    dev.check(pa_cell_rhs_batch(dev.ctx(), 0, (int)quadrature_degree_increase, PA_QUAD_TENSOR, PA_FN_OBSTACLE_RHS, nullptr, 0,
                                num_cells, d_rhs.get()), "pa_cell_rhs_batch");
    dev.check(pa_dirichlet_data_batch(dev.ctx(), (int)degree, PA_FN_OBSTACLE_SOL, nullptr, d_g.get()), "pa_dirichlet_data_batch");

    pa_obstacle_solve_params params = obstacle_solve_defaults();            // c = 1 (:101), 1e-7 (:193)
    params.max_outer = max_outer;
    const pa_obstacle_solve_info info = solve_obstacle(msh, hdi, d_lc.get(), d_rhs.get(), d_g.get(), gamma, params, alpha, beta);   // :117-197
    if (info.cg_exit_reason != 0) {
        std::fprintf(stderr, "obstacle system: CG did not converge (exit reason %d)\n", (int)info.cg_exit_reason);
        return 1;
    }

    RealType error = 0.0;                                                   // obstacle.cpp:202-213
    const std::vector<RealType> proj_all = project_function_all(msh, hdi, sol_fun, quadrature_degree_increase);
    for (auto &cl : msh.cells) {
        auto local = take_local_data(msh, cl, hdi, alpha);
        proton_amd::dense_matrix<RealType> proj(local.rows(), 1);
        std::memcpy(proj.data(), proj_all.data() + offset(msh, cl) * local.rows(), local.rows() * sizeof(RealType));
        auto gr = make_hho_laplacian(msh, cl, hdi);
        auto lc = gr.second + make_hho_fancy_stabilization(msh, cl, gr.first, hdi);
        auto diff = local - proj;
        error += diff.dot(lc * diff);
    }
    std::printf("N %zu degree %zu iterations %zu error %.10e converged %d\n", N, degree, (size_t)info.outer_iterations, std::sqrt(error),
                (int)info.converged);
    return 0;
}
