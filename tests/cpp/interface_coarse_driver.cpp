// interface_coarse_driver.cpp -- run_cuthho_interface (apps/cuthho/cuthho_square.cpp:1625-1846) through the drop-in header with
// interface_assembler::solve_condensed and its trailing arguments `coarse`, `coarse_parts`: the face-only system of
// interface_patch_driver.cpp solved by the conjugate gradient with the cell patches and a Galerkin coarse level
// (pa_interface_condensed_coarse, the hats whole or split by side of the interface, + pa_conjugated_gradient_patch_coarse) where that
// driver has the patches alone (the reference's solve is :1737-1743), and the energy-norm error of :1762-1833 through
// take_local_data.  Compiled against proton_amd/host/cuthho.hpp only: no Eigen, no HIP headers.
//   usage: interface_coarse_driver -k <degree> -M <Nx> -N <Ny> -r <refsteps> [-H <coarse step, 0 = patches alone>] [-s side|one]
//                                  [-t <threshold>] [-x <file: the solution vector>]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

#include "../../proton_amd/host/cuthho.hpp"

using RealType = double;
using mesh_type = cuthho_poly_mesh<RealType>;

static RealType grad_error(const mesh_type &msh, const mesh_type::cell_type &cl, const RealType *dofs, size_t cd, element_location where)
{
    // sum_qp w |grad u_exact - grad u_T|^2 over the `where` part of the cell (cuthho_square.cpp:1036-1046)
    RealType acc = 0.0;
    const auto bar = barycenter(msh, cl);
    const auto h = diameter(msh, cl);
    for (auto &qp : integrate(msh, cl, 2 * cd, where)) {
        const double bx = (qp.first.x() - bar.x()) / (0.5 * h), by = (qp.first.y() - bar.y()) / (0.5 * h);
        double gx = 0.0, gy = 0.0;
        size_t pos = 0;
        for (size_t kk = 0; kk <= cd; kk++)                                       // bases.hpp:142-184
            for (size_t ii = 0; ii <= kk; ii++, pos++) {
                if (pos == 0) continue;
                const double px = (double)(kk - ii), py = (double)ii, u = dofs[pos];
                if (kk - ii > 0) gx += u * px * (2.0 / h) * std::pow(bx, px - 1) * std::pow(by, py);
                if (ii > 0) gy += u * py * (2.0 / h) * std::pow(bx, px) * std::pow(by, py - 1);
            }
        const double sx = M_PI * std::cos(M_PI * qp.first.x()) * std::sin(M_PI * qp.first.y());
        const double sy = M_PI * std::sin(M_PI * qp.first.x()) * std::cos(M_PI * qp.first.y());
        acc += qp.second * ((sx - gx) * (sx - gx) + (sy - gy) * (sy - gy));
    }
    return acc;
}

int main(int argc, char **argv)
{
    size_t degree = 0, int_refsteps = 4;                                          // cuthho_square.cpp:1944-1945
    mesh_init_params<RealType> mip;
    mip.Nx = 5; mip.Ny = 5;                                                       // :1954-1955
    int ch, coarse = 4, parts = PA_COARSE_BY_SIDE;
    double threshold = 1e-9;                                                      // :1737-1743
    const char *name = "side", *dump = nullptr;
    while ((ch = getopt(argc, argv, "k:M:N:r:H:s:t:x:")) != -1) {                  // :1964-2011 (-i is what this driver does)
        switch (ch) {
        case 'k': degree = std::atoi(optarg); break;
        case 'M': mip.Nx = std::atoi(optarg); break;
        case 'N': mip.Ny = std::atoi(optarg); break;
        case 'r': int_refsteps = std::atoi(optarg); break;
        case 't': threshold = std::atof(optarg); break;
        case 'H': coarse = std::atoi(optarg); break;
        case 'x': dump = optarg; break;
        case 's':
            if (std::strcmp(optarg, "one") == 0) { parts = PA_COARSE_ONE; name = "one"; }
            else if (std::strcmp(optarg, "side") == 0) { parts = PA_COARSE_BY_SIDE; name = "side"; }
            else { std::printf("wrong arguments\n"); return 1; }
            break;
        default: std::printf("wrong arguments\n"); return 1;
        }
    }
    mesh_type msh(mip);
    auto level_set_function = circle_level_set<RealType>(0.35, 0.5, 0.5);        // :2029-2030

    detect_node_position(msh, level_set_function);                                // :2036-2052
    detect_cut_faces(msh, level_set_function);
    move_nodes(msh, level_set_function);
    detect_cut_faces(msh, level_set_function);
    detect_cut_cells(msh, level_set_function);
    refine_interface(msh, level_set_function, int_refsteps);

    auto sol_fun = [](const mesh_type::point_type &pt) -> RealType { return std::sin(M_PI * pt.x()) * std::sin(M_PI * pt.y()); };
    auto bcs_fun = [&](const mesh_type::point_type &pt) -> RealType { return sol_fun(pt); };

    hho_degree_info hdi(degree + 1, degree);                                      // :1662
    const size_t cd = hdi.cell_degree(), cbs = (cd + 2) * (cd + 1) / 2;
    size_t ncut = 0;
    for (auto &cl : msh.cells) ncut += is_cut(msh, cl) ? 1 : 0;

    params<RealType> parms;
    auto assembler = make_interface_assembler(msh, hdi);
    const size_t full_size = assembler.RHS.size(), face_size = full_size - cbs * (msh.cells.size() + ncut);
    cg_params<RealType> cgp;
    cgp.convergence_threshold = threshold;
    cgp.max_iter = full_size;
    cgp.apply_preconditioner = true;
    size_t iters = 0;
    cg_exit_reason why = cg_exit_reason::MAX_ITER_REACHED;
    const std::vector<RealType> sol = assembler.solve_condensed(msh, parms, PA_FN_SIN_SIN_RHS, PA_FN_SIN_SIN_SOL, cgp, &iters, &why, PA_PATCH_CELL,
                                                                 coarse, parts);
    if (why != cg_exit_reason::CONVERGED) { std::printf("conjugated_gradient did not converge (%d)\n", (int)why); return 2; }
    RealType H1_error = 0.0;                                                      // :1762-1833
    for (auto &cl : msh.cells) {
        if (is_cut(msh, cl)) {
            for (auto where : {element_location::IN_NEGATIVE_SIDE, element_location::IN_POSITIVE_SIDE}) {
                auto locdata = assembler.take_local_data(msh, cl, sol, bcs_fun, where);
                H1_error += grad_error(msh, cl, locdata.data(), cd, where);
            }
        } else {
            auto locdata = assembler.take_local_data(msh, cl, sol, bcs_fun, element_location::IN_POSITIVE_SIDE);
            H1_error += grad_error(msh, cl, locdata.data(), cd, location(msh, cl));
        }
    }
    if (dump) {
        std::FILE *f = std::fopen(dump, "wb");
        if (!f || std::fwrite(sol.data(), sizeof(RealType), sol.size(), f) != sol.size()) { std::printf("cannot write %s\n", dump); return 3; }
        std::fclose(f);
    }
    std::printf("interface_coarse N %zu k %zu r %zu H %d parts %s cut_cells %zu system %zu face_system %zu cg_iters %zu CONVERGED energy_error %.10e\n",
                (size_t)mip.Nx, degree, int_refsteps, coarse, name, ncut, full_size, face_size, iters, std::sqrt(H1_error));
    return 0;
}
