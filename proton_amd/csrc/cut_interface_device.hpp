// cut_interface_device.hpp -- the two-sided interface problem of `cuthho_square -i`:
//   make_hho_laplacian_interface                        apps/cuthho/cuthho_square.cpp:390-502
//   make_rhs(msh, cl, degree, where, f)                 src/methods/cuthho_bits/cuthho_utils.hpp:65-84
//   the stabilization blocks of run_cuthho_interface    apps/cuthho/cuthho_square.cpp:1694-1705
//   interface_assembler::assemble / assemble_cut        apps/cuthho/cuthho_square.cpp:1203-1354
// One wavefront per cut cell.  Unknown order of a cut cell: [cell-, cell+, faces-, faces+].
//
// gr_lhs (2 rbs x 2 rbs) is symmetric positive SEMI-definite: its kernel is "the same constant on
// both sides" and every column of gr_rhs is orthogonal to it.  The reference hands it to Eigen's
// pivoted LDLT (:498); here the constant of the negative side is pinned to zero and the remaining
// (2 rbs - 1) system, which is positive definite, is factored by Cholesky.  `data = gr_rhs^T oper`
// (:499) does not depend on the kernel component; `oper` is returned with a zero first row.
#pragma once

#include "cut_device.hpp"

namespace pa {

struct CutInterfaceArgs {
    const double *points;
    const uint32_t *ptids;
    const uint32_t *cut_cells;
    uint32_t ncut;
    const uint32_t *cell_off[2];         // cut-cell quadrature of the negative / positive side
    const double *cell_xyw[2];
    const uint32_t *il_off;              // interface points, integrate_interface(.., IN_NEGATIVE_SIDE)  (:437)
    const double *il_xyw;
    const double *fl_xyw[2];             // face points of each side at degree 2*recdeg
    const int32_t *fl_cnt[2];
    LevelSet ls;
    int rhs_fn;
    double kappa[2], eta;                // params<T>, cuthho_square.cpp:293-299
    double *oper, *data, *rhs;           // ncut x (2rbs x 2msize), ncut x (2msize)^2, ncut x 2cbs
    int32_t *info;
};

// The two-sided reconstruction system in double-double, like the one-sided one (cut_device.hpp, section 3.2 of DESIGN.md; the
// stages the two kernels share are in cut_dd_stages.hpp): its pinned (2 rbs - 1) system is badly conditioned on EVERY cut cell
// (1-norm condition numbers: median 1e7 at k = 2).
template <int FD>
__global__ __launch_bounds__(64, 2) void cut_interface_kernel(CutInterfaceArgs a)
{
    constexpr int RD = FD + 1, RBS = P2(RD), CBS = RBS, FBS = FD + 1, NF = 4 * FBS, MS = CBS + NF;
    constexpr int N2 = 2 * RBS, M2 = 2 * MS, NR = N2 - 1, LD2 = (N2 + 1) & ~1;
    constexpr int NMOM = P2(2 * RD), NFPT = 4 * FACE_SLOTS, CH = 64, NPW = 2 * RD + 1;
    constexpr int PW = 2 * NPW + 1, ROWW = imax(2 * RBS, PW);
    // LDS map (doubles), everything in (hi, lo) pairs; the pinned system is factored from ST
    constexpr int oMOM = 0, oST = (oMOM + 2 * NMOM + 1) & ~1, oGR = oST + 2 * LD2 * N2;
    constexpr int oOP = oGR + 2 * N2 * M2, oTPHI = oOP + 2 * N2 * M2, oEND = oTPHI + CH * ROWW;
    // tables on the point table [oTPHI, oEND): stage B: the interface moments; stage C: phi and w dn of the NFPT face points, then
    // their face-basis values
    constexpr int oCPH = oTPHI, oCDN = oTPHI + 2 * NFPT * RBS, oCFB = oCDN + 2 * NFPT * RBS;
    static_assert(oCFB + 2 * NFPT * FBS <= oEND, "the double-double tables fit the point table");
    static_assert(M2 <= 64 && NMOM <= 64 && NR <= 64, "one lane per column / moment / row");
    __shared__ __attribute__((aligned(16))) double S[oEND];
    const int l = threadIdx.x;

    for (uint32_t cc = blockIdx.x; cc < a.ncut; cc += gridDim.x) {
        uint32_t ids[4];
        double px[4], py[4];
        const CutCellFrame fr = cut_cell_frame(a.points, a.ptids, a.cut_cells[cc], ids, px, py);      // hT: measure(msh, cl), the WHOLE cell (:434)
        const double barx = fr.barx, bary = fr.bary, ihalf = fr.ihalf, ih = fr.ih;
        const double eta_h = a.eta / fr.hT;

        int bad = 0;
        for (int e = l; e < 2 * LD2 * N2; e += 64) S[oST + e] = 0.0;
        wave_sync();
        const dd ih2 = two_prod(ih, ih);
        // ---- A: per side, moments over the side's cut quadrature -> kappa_s * stiffness block (:419-432); the side's volume
        // right-hand side rides along in double (cuthho_utils.hpp:75-81)
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const uint32_t c0 = a.cell_off[side][cc], c1 = a.cell_off[side][cc + 1];
            const double *xyw = a.cell_xyw[side];
            {
                dd macc[NMOM];
                double racc[CBS];
#pragma unroll
                for (int m = 0; m < NMOM; ++m) macc[m] = dd_from(0.0);
#pragma unroll
                for (int m = 0; m < CBS; ++m) racc[m] = 0.0;
                for (uint32_t q = c0 + l; q < c1; q += 64) {
                    const double x = xyw[3 * q], y = xyw[3 * q + 1], w = xyw[3 * q + 2];
                    const double bx = (x - barx) * ihalf, by = (y - bary) * ihalf;
                    dd pbx[NPW], pby[NPW];                  // w bx^e, by^e
                    pbx[0] = dd_from(w); pby[0] = dd_from(1.0);
#pragma unroll
                    for (int e = 1; e < NPW; ++e) { pbx[e] = dd_mul_d(pbx[e - 1], bx); pby[e] = dd_mul_d(pby[e - 1], by); }
#pragma unroll
                    for (int k = 0; k < NPW; ++k)
#pragma unroll
                        for (int r = 0; r <= k; ++r) macc[k * (k + 1) / 2 + r] = dd_add_fast(macc[k * (k + 1) / 2 + r], dd_mul(pbx[k - r], pby[r]));
                    if (a.rhs != nullptr) {
                        const double fv = builtin_fn(a.rhs_fn, x, y);
#pragma unroll
                        for (int k = 0; k <= RD; ++k)
#pragma unroll
                            for (int r = 0; r <= k; ++r) racc[k * (k + 1) / 2 + r] += fv * (pbx[k - r].hi * pby[r].hi);
                    }
                }
                // (the transposed butterfly of dd_arith.hpp: 29 exchanges for the 28 moments instead of 168)
                {
                    dd tot; bool ok = true;
                    const int m = lanes_transpose_reduce<NMOM, 32>(macc, l, dd_from(0.0), [](dd u, dd v_) { return dd_add_fast(u, v_); },
                                                                   [](dd u, int off) { return dd_shfl_xor(u, off); }, tot, ok);
                    if (ok) dd_store(S + oMOM + 2 * m, tot);
                }
                if (a.rhs != nullptr) {
                    double tot; bool ok = true;
                    const int m = lanes_transpose_reduce<CBS, 32>(racc, l, 0.0, [](double u, double v_) { return u + v_; },
                                                                  [](double u, int off) { return __shfl_xor(u, off); }, tot, ok);
                    if (ok) a.rhs[(size_t)cc * (2 * CBS) + side * CBS + m] = tot;      // :1710-1711 (the lanes that end with one entry hold the same sum)
                }
            }
            wave_sync();
            cut_stiffness_from_moments<RD, LD2>(S + oMOM, dd_mul_d(ih2, a.kappa[side]), S + oST + 2 * (side * RBS + side * RBS * LD2), l);
            wave_sync();
        }
        auto basis_dd = [&](double bx, double by, dd (&phi)[RBS], dd (&gx)[RBS], dd (&gy)[RBS]) {
            dd pbx[RD + 1], pby[RD + 1];
            pbx[0] = dd_from(1.0); pby[0] = dd_from(1.0);
#pragma unroll
            for (int e = 1; e <= RD; ++e) { pbx[e] = dd_mul_d(pbx[e - 1], bx); pby[e] = dd_mul_d(pby[e - 1], by); }
            int m = 0;
#pragma unroll
            for (int kk = 0; kk <= RD; ++kk)
#pragma unroll
                for (int ii = 0; ii <= kk; ++ii, ++m) {
                    const int p_ = kk - ii, r_ = ii;
                    phi[m] = dd_mul(pbx[p_], pby[r_]);
                    gx[m] = p_ == 0 ? dd_from(0.0) : dd_mul(dd_mul(pbx[p_ > 0 ? p_ - 1 : 0], pby[r_]), two_prod((double)p_, ih));
                    gy[m] = r_ == 0 ? dd_from(0.0) : dd_mul(dd_mul(pbx[p_], pby[r_ > 0 ? r_ - 1 : 0]), two_prod((double)r_, ih));
                }
        };
        // ---- B: interface terms (:437-459): A_ij = sum k1 w phi_i (dphi_j.n), C_ij = sum k1 w eta/hT phi_i phi_j;
        //   (-,-) += C - A - A^T ;  (+,-) += A - C ;  (-,+) += A^T - C ;  (+,+) += C
        // Through the moments of the interface measures w, w n_x, w n_y (iface_moments, cut_dd_stages.hpp): with P = p_i + p_j,
        // R = r_i + r_j:  C_ij = k1 eta/hT M(P, R),  A_ij = k1 ih (p_j Mx(P - 1, R) + r_j My(P, R - 1)).
        {
            constexpr int NM1 = P2(2 * RD - 1);
            constexpr int oIM = oTPHI, oIX = oIM + 2 * NMOM, oIY = oIX + 2 * NM1;
            static_assert(2 * (NMOM + 2 * NM1) <= CH * ROWW, "the interface moments fit the point table");
            iface_moments<RD>(a.il_xyw, a.il_off[cc], a.il_off[cc + 1], a.ls, barx, bary, ihalf, l, S + oIM, S + oIX, S + oIY);
            wave_sync();
            const dd k1e = two_prod(a.kappa[0], eta_h), k1i = two_prod(a.kappa[0], ih);
            dd vA[(RBS * RBS + 63) / 64], vAt[(RBS * RBS + 63) / 64], vC[(RBS * RBS + 63) / 64];
#pragma unroll
            for (int u = 0; u < (RBS * RBS + 63) / 64; ++u) {
                const int e = l + 64 * u;
                vA[u] = vAt[u] = vC[u] = dd_from(0.0);
                if (e < RBS * RBS) {
                    const int i = e % RBS, j = e / RBS;
                    int p1, r1, p2, r2;
                    mono_exps(i, p1, r1);
                    mono_exps(j, p2, r2);
                    const int P = p1 + p2, R = r1 + r2;
                    const dd mx = P > 0 ? dd_load(S + oIX + 2 * mono_index(P > 0 ? P - 1 : 0, R)) : dd_from(0.0);
                    const dd my = R > 0 ? dd_load(S + oIY + 2 * mono_index(P, R > 0 ? R - 1 : 0)) : dd_from(0.0);
                    vC[u] = dd_mul(dd_load(S + oIM + 2 * mono_index(P, R)), k1e);
                    vA[u] = dd_mul(dd_add(dd_mul_d(mx, (double)p2), dd_mul_d(my, (double)r2)), k1i);
                    vAt[u] = dd_mul(dd_add(dd_mul_d(mx, (double)p1), dd_mul_d(my, (double)r1)), k1i);
                }
            }
            wave_sync();                                   // (the moment tables are dead: the point table is free again)
#pragma unroll
            for (int u = 0; u < (RBS * RBS + 63) / 64; ++u) {
                const int e = l + 64 * u;
                if (e < RBS * RBS) {
                    const int i = e % RBS, j = e / RBS;
                    const dd A_ = vA[u], At = vAt[u], C_ = vC[u];
                    double *p00 = S + oST + 2 * (i + j * LD2), *p10 = S + oST + 2 * ((RBS + i) + j * LD2);
                    double *p01 = S + oST + 2 * (i + (RBS + j) * LD2), *p11 = S + oST + 2 * ((RBS + i) + (RBS + j) * LD2);
                    dd_store(p00, dd_add(dd_load(p00), dd_sub(dd_sub(C_, A_), At)));
                    dd_store(p10, dd_add(dd_load(p10), dd_sub(A_, C_)));
                    dd_store(p01, dd_add(dd_load(p01), dd_sub(At, C_)));
                    dd_store(p11, dd_add(dd_load(p11), C_));
                }
            }
            wave_sync();
        }
        // ---- C: gr_rhs (:461-495).  Columns: [cell- | cell+ | faces- | faces+]
        for (int e = l; e < N2 * M2; e += 64) {
            const int i = e % N2, j = e / N2;
            const dd v = j < CBS ? dd_load(S + oST + 2 * (i + j * LD2)) : (j < 2 * CBS ? dd_load(S + oST + 2 * (i + (RBS + j - CBS) * LD2)) : dd_from(0.0));
            dd_store(S + oGR + 2 * e, v);
        }
        wave_sync();
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            if (l < NFPT) {
                const int f = l / FACE_SLOTS, qq = l % FACE_SLOTS;
                const bool ok = qq < a.fl_cnt[side][cc * 4 + f];
                const double *src = a.fl_xyw[side] + (((size_t)cc * 4 + f) * FACE_SLOTS + qq) * 3;
                const double x = ok ? src[0] : barx, y = ok ? src[1] : bary;
                const dd kw = ok ? two_prod(a.kappa[side], src[2]) : dd_from(0.0);
                const CutFacePoint fp = cut_face_point(ids, px, py, fr, f, x, y);          // outward normal of the CELL on both sides (:464)
                const double nx = fp.nx, ny = fp.ny, ep = fp.ep, bx = fp.bx, by = fp.by;
                dd phi[RBS], gx[RBS], gy[RBS];
                basis_dd(bx, by, phi, gx, gy);
#pragma unroll
                for (int m = 0; m < RBS; ++m) {
                    dd_store(S + oCPH + 2 * (l * RBS + m), phi[m]);
                    dd_store(S + oCDN + 2 * (l * RBS + m), dd_mul(dd_add(dd_mul_d(gx[m], nx), dd_mul_d(gy[m], ny)), kw));
                }
                dd pe = dd_from(1.0);
#pragma unroll
                for (int k = 0; k < FBS; ++k) { dd_store(S + oCFB + 2 * (l * FBS + k), pe); pe = dd_mul_d(pe, ep); }
            }
            wave_sync();
            for (int e = l; e < RBS * MS; e += 64) {
                const int i = e % RBS, j = e / RBS;
                if (j < CBS) {                                              // :479, :491
                    double *dst = S + oGR + 2 * ((side * RBS + i) + (side * CBS + j) * N2);
                    dd sacc = dd_load(dst);
                    for (int p_ = 0; p_ < NFPT; ++p_) sacc = dd_sub_fast(sacc, dd_mul(dd_load(S + oCDN + 2 * (p_ * RBS + i)), dd_load(S + oCPH + 2 * (p_ * RBS + j))));
                    dd_store(dst, sacc);
                } else {                                                    // :480-481, :492-493
                    const int f = (j - CBS) / FBS, k = (j - CBS) % FBS;
                    dd sacc = dd_from(0.0);
                    for (int qq = 0; qq < FACE_SLOTS; ++qq)
                        sacc = dd_add_fast(sacc, dd_mul(dd_load(S + oCDN + 2 * ((f * FACE_SLOTS + qq) * RBS + i)), dd_load(S + oCFB + 2 * ((f * FACE_SLOTS + qq) * FBS + k))));
                    dd_store(S + oGR + 2 * ((side * RBS + i) + (2 * CBS + side * NF + f * FBS + k) * N2), sacc);
                }
            }
            wave_sync();
        }
        // ---- D: the first unknown pinned (see the header comment): Cholesky of ST[1:, 1:] and both substitutions in REGISTERS, one lane
        // per column of [ST[1:, 1:] | gr_rhs[1:, :]] (NR + M2 lanes: 63 of the 64 at k = 2)
        {
            static_assert(NR + M2 <= 64, "a lane per column of the pinned system and of gr_rhs");
            const bool isA = l < NR, isG = l >= NR && l < NR + M2;
            const int gc = isG ? l - NR : 0;
            dd v[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i)
                v[i] = isA ? dd_load(S + oST + 2 * ((i + 1) + (l + 1) * LD2)) : isG ? dd_load(S + oGR + 2 * ((i + 1) + gc * N2)) : dd_from(1.0);
            bad = cut_llt_solve_in_registers<NR>(v, l, isG);
            if (isG) {
                dd_store(S + oOP + 2 * (gc * N2), dd_from(0.0));          // the pinned unknown
#pragma unroll
                for (int k = 0; k < NR; ++k) dd_store(S + oOP + 2 * ((k + 1) + gc * N2), v[k]);
            }
            wave_sync();
            if (a.oper != nullptr)
                for (int e = l; e < N2 * M2; e += 64) a.oper[(size_t)cc * (N2 * M2) + e] = dd_round(dd_load(S + oOP + 2 * e));
        }
        // ---- E: data = gr_rhs^T oper (:499), symmetric: the entries i <= j, two running sums each, rounded once, both copies stored
        if (a.data != nullptr) {
            const size_t off = (size_t)cc * (M2 * M2);
#pragma unroll 1
            for (int e = l; e < M2 * (M2 + 1) / 2; e += 64) {
                int i, j;
                tri_index(e, i, j);
                dd s0 = dd_from(0.0), s1 = dd_from(0.0);
#pragma unroll 4
                for (int k = 0; k < N2; k += 2) {
                    s0 = dd_add_fast(s0, dd_mul(dd_load(S + oGR + 2 * (k + i * N2)), dd_load(S + oOP + 2 * (k + j * N2))));
                    s1 = dd_add_fast(s1, dd_mul(dd_load(S + oGR + 2 * (k + 1 + i * N2)), dd_load(S + oOP + 2 * (k + 1 + j * N2))));
                }
                const double r = dd_round(dd_add_fast(s0, s1));
                a.data[off + i + (size_t)j * M2] = r;
                a.data[off + j + (size_t)i * M2] = r;
            }
        }
        if (a.info != nullptr && l == 0) a.info[cc] = bad;
        wave_sync();
    }
}

// lc of a cut cell (cuthho_square.cpp:1692-1705): data of make_hho_laplacian_interface plus
// kappa_1 * stab_n scattered over the (cell-, faces-) unknowns and kappa_2 * stab_p over (cell+, faces+)
static __global__ __launch_bounds__(256) void cut_interface_lc_kernel(uint32_t ncut, int cbs, int nfd, double k1, double k2,
                                                               const double *data, const double *stab_n, const double *stab_p,
                                                               double *lc)
{
    const int ms = cbs + nfd, m2 = 2 * ms;
    for (size_t cc = blockIdx.x; cc < ncut; cc += gridDim.x)
        for (int e = threadIdx.x; e < m2 * m2; e += blockDim.x) {
            const int i = e % m2, j = e / m2;
            // side and one-sided index of a two-sided unknown
            const int si = i < 2 * cbs ? i / cbs : (i - 2 * cbs) / nfd, li = i < 2 * cbs ? i % cbs : cbs + (i - 2 * cbs) % nfd;
            const int sj = j < 2 * cbs ? j / cbs : (j - 2 * cbs) / nfd, lj = j < 2 * cbs ? j % cbs : cbs + (j - 2 * cbs) % nfd;
            double v = data[cc * (size_t)(m2 * m2) + e];
            if (si == sj) v += (si == 0 ? k1 * stab_n[cc * (size_t)(ms * ms) + li + lj * ms] : k2 * stab_p[cc * (size_t)(ms * ms) + li + lj * ms]);
            lc[cc * (size_t)(m2 * m2) + e] = v;
        }
}

// lc = kappa(side of the cell) * data + stab for the uncut cells (cuthho_square.cpp:1670-1679)
static __global__ __launch_bounds__(256) void cut_interface_uncut_lc_kernel(size_t ncells, int mm, const int8_t *cell_loc, double k1, double k2,
                                                                     const double *data, const double *stab, double *lc)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncells * mm) return;
    const int8_t loc = cell_loc[t / mm];
    lc[t] = (loc == LOC_NEG ? k1 : k2) * data[t] + stab[t];
}

}  // namespace pa
