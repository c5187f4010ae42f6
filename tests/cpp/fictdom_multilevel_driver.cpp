// fictdom_multilevel_driver.cpp -- run_cuthho_fictdom (apps/cuthho/cuthho_square.cpp:806-1080) through the drop-in header with
// assembler::solve_condensed_fictdom and its three trailing arguments: the face-only system of fictdom_coarse_driver.cpp solved by
// the conjugate gradient with the cell patches, smoothed hat levels (pa_smoothed_level_*: the diagonal of the Galerkin matrix in
// place of its factor) and a Galerkin coarse level, every hat split by side of the interface (pa_condensed_coarse +
// pa_conjugated_gradient_multilevel), where that driver has the patches and the one exact level (the reference uses SparseLU for -f,
// :915-919), and the energy-norm error of :1030-1049.  Compiled against proton_amd/host/cuthho.hpp only: no Eigen, no HIP headers.
//   usage: fictdom_multilevel_driver -k <degree> -M <Nx> -N <Ny> -r <refsteps> [-H <coarse step, 0 = no exact level>]
//          [-L <H_0,H_1,..: the smoothed levels, default 2,4; 0 = none>] [-x <file>]
//   -x: the solution vector (doubles, binary) is written to <file>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <unistd.h>
#include <vector>

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
    int ch, patches = PA_PATCH_CELL, coarse = 8;
    std::vector<int> levels = {2, 4};
    const char *dump = nullptr;
    while ((ch = getopt(argc, argv, "k:M:N:r:H:L:x:")) != -1) {                      // :1964-2011 (-f is what this driver does)
        switch (ch) {
        case 'k': degree = std::atoi(optarg); break;
        case 'M': mip.Nx = std::atoi(optarg); break;
        case 'N': mip.Ny = std::atoi(optarg); break;
        case 'r': int_refsteps = std::atoi(optarg); break;
        case 'H': coarse = std::atoi(optarg); break;
        case 'L':
            levels.clear();
            for (const char *s = optarg; *s;) {
                char *end = nullptr;
                const long h = std::strtol(s, &end, 10);
                if (end == s) { std::printf("wrong arguments\n"); return 1; }
                if (h > 0) levels.push_back((int)h);
                s = *end == ',' ? end + 1 : end;
            }
            break;
        case 'x': dump = optarg; break;
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

    hho_degree_info hdi(degree + 1, degree);                                      // :871
    const size_t cd = hdi.cell_degree(), cbs = (cd + 2) * (cd + 1) / 2, fbs = degree + 1;
    size_t ncut = 0;
    for (auto &cl : msh.cells) ncut += is_cut(msh, cl) ? 1 : 0;

    const element_location where = element_location::IN_NEGATIVE_SIDE;
    auto assembler = make_assembler(msh, hdi);
    const size_t full_size = assembler.RHS.size(), face_size = full_size - cbs * msh.cells.size();
    cg_params<RealType> cgp;
    cgp.convergence_threshold = 1e-13;                                            // as cuthho_driver -f
    cgp.max_iter = 4 * face_size;
    cgp.apply_preconditioner = true;
    size_t iters = 0;
    cg_exit_reason why = cg_exit_reason::MAX_ITER_REACHED;
    std::vector<RealType> sol;
    try {
        sol = assembler.solve_condensed_fictdom(msh, level_set_function, where, PA_FN_SIN_SIN_RHS, PA_FN_SIN_SIN_SOL, cgp, &iters, &why, patches,
                                                coarse, levels);
    } catch (const std::invalid_argument &e) {                                   // levels that are not nested: refused before any device call
        std::printf("refused: %s\n", e.what());
        return 4;
    }
    if (why != cg_exit_reason::CONVERGED) { std::printf("conjugated_gradient did not converge (%d)\n", (int)why); return 2; }
    RealType H1_error = 0.0;                                                      // :1030-1049
    for (auto &cl : msh.cells) {
        if (location(msh, cl) == element_location::IN_POSITIVE_SIDE) continue;
        H1_error += grad_error(msh, cl, sol.data() + offset(msh, cl) * cbs, cd, where);
    }
    if (dump) {
        std::FILE *f = std::fopen(dump, "wb");
        if (!f || std::fwrite(sol.data(), sizeof(RealType), sol.size(), f) != sol.size()) { std::printf("cannot write %s\n", dump); return 3; }
        std::fclose(f);
    }
    std::printf("fictdom_multilevel N %zu k %zu r %zu H %d levels %zu cut_cells %zu system %zu face_system %zu (fbs %zu) cg_iters %zu CONVERGED "
                "energy_error %.10e\n",
                (size_t)mip.Nx, degree, int_refsteps, coarse, levels.size(), ncut, full_size, face_size, fbs, iters, std::sqrt(H1_error));
    return 0;
}
