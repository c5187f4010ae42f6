// cut_device.hpp -- the cut-cell local operators of the fictitious-domain driver:
//   make_hho_laplacian(msh, cl, level_set, di, where)   apps/cuthho/cuthho_square.cpp:308-388
//   make_hho_cut_stabilization                          apps/cuthho/cuthho_square.cpp:566-621
//   make_rhs(msh, cl, degree, f, where, level_set, bcs) apps/cuthho/cuthho_square.cpp:623-666
// for the cells cut by the interface (about 0.5 % of a 512 x 512 mesh).  One wavefront per cut
// cell; the quadrature lists come from the host preprocessing (cut_host.hpp).  The uncut cells
// of the same mesh go through hho_local_ops_kernel (fan quadrature, naive stabilization).
// Assumes celdeg == recdeg == facdeg + 1, as the reference's cut operators do (:381, :871).
//
// Stages A-E -- everything between the scaled coordinates of the quadrature points and `oper` / `data` -- run in double-double
// arithmetic (dd_arith.hpp; the stages shared with the two-sided kernel of cut_interface_device.hpp are in cut_dd_stages.hpp).
// The Nitsche-penalised rbs x rbs system of a sliver cut is badly conditioned (1-norm condition numbers to 1.9e9 on the
// 512 x 512 mesh): in double, ROUNDING gr_lhs and gr_rhs once and solving exactly already costs 1e-11 in `data` (tests/test_oracle_cut_truth.py), and the reference's own operation order in double sits at 1e-10 -- no
// double evaluation is within 1e-12 of another there.  What may stay double without that amplification is what perturbs the
// bilinear forms CONSISTENTLY (the scaled coordinates bx, by of a point, 2/h, the normals, the face coordinate, eta / h_T: a
// slightly different quadrature point or penalty, the same on both sides of the solve); what may not are the sums, the products of
// the powers, the factorization, the substitutions and the final product.  With those in double-double every cut cell is within
// 1e-12 of the 50-digit / binary128 evaluation of the reference's formulas (measured: data <= 4e-14, oper <= 1.3e-13 on all 1 436
// cut cells of config 3).  Stabilization and right-hand side involve no such solve and stay in double (1e-13 everywhere).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cut_dd_stages.hpp"
#include "cut_host.hpp"
#include "dd_arith.hpp"
#include "hho_aux.hpp"
#include "hho_device.hpp"

namespace pa {

struct CutArgs {
    const QuadTables *tab;
    const double *points;
    const uint32_t *ptids;
    const uint32_t *cut_cells;
    uint32_t ncut;
    const uint32_t *cell_off, *il_off, *ir_off;
    const double *cell_xyw, *il_xyw, *ir_xyw, *fl_xyw, *fs_xyw;
    const int32_t *fl_cnt, *fs_cnt;
    LevelSet ls;
    int rhs_fn, bcs_fn;             // FN_SAMPLED: values per point of the cell list / of the rhs interface list
    const double *rhs_vals, *bcs_vals;
    double eta;                     // cell_eta, cuthho_square.cpp:301-306
    double *oper, *data, *stab, *lc, *rhs;
    int32_t *info;
};

__device__ __forceinline__ double ipow(double x, int n)
{
    double v = 1.0;
    for (int e = 0; e < n; ++e) v *= x;
    return v;
}

template <int FD>
// (a block is one wavefront: wave_sync() orders its LDS traffic without the wait for outstanding loads / stores that
// __syncthreads() adds -- the quadrature lists of the next chunk stay in flight)
__global__ __launch_bounds__(64, 2) void cut_local_ops_kernel(CutArgs a)
{
    constexpr int RD = FD + 1, RBS = P2(RD), CBS = RBS, FBS = FD + 1, NF = 4 * FBS, MS = CBS + NF;
    constexpr int NMOM = P2(2 * RD), LD = (RBS + 1) & ~1, NFPT = 4 * FACE_SLOTS, CH = 64;
    // LDS map (doubles): moments, stiffness (factored in place), gr_rhs and oper hold (hi, lo) pairs.
    constexpr int oMOM = 0, oST = (oMOM + 2 * NMOM + 1) & ~1, oGR = oST + 2 * LD * RBS, oOP = oGR + 2 * RBS * MS;
    constexpr int PW = 2 * (2 * RD + 1) + 1;                   // width of a row of the point table: the tables of B, C, F and H fit CH rows
    constexpr int ROWW = imax(2 * RBS, PW);
    constexpr int oTPHI = oOP + 2 * RBS * MS, oTW = oTPHI + CH * ROWW;
    constexpr int oFB = oTW + CH, oMF = oFB + NFPT * FBS, oTR = oMF + 4 * FBS * FBS, oPT = oTR + NF * CBS, oDATA = oPT + NF * CBS, oEND = oDATA + MS * MS;
    // double-double tables on the point table [oTPHI, oTPHI + CH ROWW): stage B: the interface moments; stage C:
    // phi and w dn of the NFPT face points, then their face-basis values
    constexpr int oCPH = oTPHI, oCDN = oTPHI + 2 * NFPT * RBS, oCFB = oCDN + 2 * NFPT * RBS;
    static_assert(oCFB + 2 * NFPT * FBS <= oTPHI + CH * ROWW, "the double-double tables fit the point table");
    __shared__ __attribute__((aligned(16))) double S[oEND];
    const int l = threadIdx.x;

    for (uint32_t cc = blockIdx.x; cc < a.ncut; cc += gridDim.x) {
        uint32_t ids[4];
        double px[4], py[4];
        const CutCellFrame fr = cut_cell_frame(a.points, a.ptids, a.cut_cells[cc], ids, px, py);
        const double barx = fr.barx, bary = fr.bary, ihalf = fr.ihalf, ih = fr.ih, hT = fr.hT;
        const double eta_h = a.eta / hT;

        // the scaled monomials (bases.hpp:93-184), runtime index m -> exponents
        auto phi_m = [&](double bx, double by, int m) {
            int p, r; mono_exps(m, p, r);
            return ipow(bx, p) * ipow(by, r);
        };

        const uint32_t c0 = a.cell_off[cc], c1 = a.cell_off[cc + 1];
        constexpr int NPW = 2 * RD + 1;
        double rhs_acc = 0.0;
        int bad = 0;
        // Only the stabilization wanted (the interface problem takes make_hho_cut_stabilization of both sides from this kernel,
        // cuthho_square.cpp:1694-1705): stages A-E -- the whole reconstruction -- are skipped.
        const bool only_stab = a.oper == nullptr && a.data == nullptr && a.lc == nullptr && a.rhs == nullptr;
        if (!only_stab) {
        // =========== stages A-E in double-double (see the head of the file) ===========
        static_assert(RBS * (RBS + 1) / 2 <= 64 && MS <= 64 && NFPT <= 64, "one lane per pair / column / point");
        // ---- A: moments  sum_q w_q bx^p by^r  over the cut cell's quadrature (cuthho_square.cpp:336-341): one lane per POINT (the
        // points of the list dealt out round robin), 28 double-double accumulators per lane, then a butterfly over the lanes
        // (the volume part of the right-hand side, :639-644, rides along in double: per point f(x) w phi_m, m < cbs)
        {
            dd macc[NMOM];
            double racc[CBS];
#pragma unroll
            for (int m = 0; m < NMOM; ++m) macc[m] = dd_from(0.0);
#pragma unroll
            for (int m = 0; m < CBS; ++m) racc[m] = 0.0;
            for (uint32_t q = c0 + l; q < c1; q += 64) {
                const double x = a.cell_xyw[3 * q], y = a.cell_xyw[3 * q + 1], w = a.cell_xyw[3 * q + 2];
                const double bx = (x - barx) * ihalf, by = (y - bary) * ihalf;
                dd pbx[NPW], pby[NPW];                  // w bx^e, by^e
                pbx[0] = dd_from(w); pby[0] = dd_from(1.0);
#pragma unroll
                for (int e = 1; e < NPW; ++e) { pbx[e] = dd_mul_d(pbx[e - 1], bx); pby[e] = dd_mul_d(pby[e - 1], by); }
#pragma unroll
                for (int k = 0; k < NPW; ++k)
#pragma unroll
                    for (int r = 0; r <= k; ++r)
                        macc[k * (k + 1) / 2 + r] = dd_add_fast(macc[k * (k + 1) / 2 + r], dd_mul(pbx[k - r], pby[r]));
                if (a.rhs != nullptr) {
                    const double fv = a.rhs_fn == FN_SAMPLED ? a.rhs_vals[q] : builtin_fn(a.rhs_fn, x, y);
#pragma unroll
                    for (int k = 0; k <= RD; ++k)
#pragma unroll
                        for (int r = 0; r <= k; ++r) racc[k * (k + 1) / 2 + r] += fv * (pbx[k - r].hi * pby[r].hi);
                }
            }
            // sums over the lanes: a butterfly that halves the values a lane carries at every level (dd_arith.hpp): 29 exchanges
            // for the 28 moments where the plain butterfly makes 168
            {
                dd tot; bool ok = true;
                const int m = lanes_transpose_reduce<NMOM, 32>(macc, l, dd_from(0.0), [](dd x, dd y) { return dd_add_fast(x, y); },
                                                               [](dd x, int off) { return dd_shfl_xor(x, off); }, tot, ok);
                if (ok) dd_store(S + oMOM + 2 * m, tot);      // (the lanes that end with the same entry hold the same sum)
            }
            if (a.rhs != nullptr) {
                double tot; bool ok = true;
                const int m = lanes_transpose_reduce<CBS, 32>(racc, l, 0.0, [](double x, double y) { return x + y; },
                                                              [](double x, int off) { return __shfl_xor(x, off); }, tot, ok);
                // lane m of the wavefront keeps the volume part of mode m for stage H
                S[oTW + (ok ? m : CH - 1)] = tot;       // (scratch: the point weights' row is dead until stage F)
            }
        }
        wave_sync();
        if (a.rhs != nullptr && l < CBS) rhs_acc = S[oTW + l];
        wave_sync();
        cut_stiffness_from_moments<RD, LD>(S + oMOM, two_prod(ih, ih), S + oST, l);
        wave_sync();
        // the scaled monomials and their gradients at a point, double-double from the double coordinates:
        // one monomial of the same basis with RUN-TIME exponents (a lane's share of a point's monomials): the powers are picked from
        // the registers by selects, never by a dynamic index (which would send the arrays to scratch memory)
        auto pick_dd = [&](const dd (&arr)[RD + 1], int i) {
            dd v = arr[0];
#pragma unroll
            for (int e = 1; e <= RD; ++e) { v.hi = i == e ? arr[e].hi : v.hi; v.lo = i == e ? arr[e].lo : v.lo; }
            return v;
        };
        auto powers_dd = [&](double bx, double by, dd (&pbx)[RD + 1], dd (&pby)[RD + 1]) {
            pbx[0] = dd_from(1.0); pby[0] = dd_from(1.0);
#pragma unroll
            for (int e = 1; e <= RD; ++e) { pbx[e] = dd_mul_d(pbx[e - 1], bx); pby[e] = dd_mul_d(pby[e - 1], by); }
        };
        auto basis_dd_one = [&](const dd (&pbx)[RD + 1], const dd (&pby)[RD + 1], int m, dd &phi, dd &gx, dd &gy) {
            int p_, r_;
            mono_exps(m, p_, r_);
            const dd xp = pick_dd(pbx, p_), yr = pick_dd(pby, r_);
            const dd xp1 = pick_dd(pbx, p_ > 0 ? p_ - 1 : 0), yr1 = pick_dd(pby, r_ > 0 ? r_ - 1 : 0);
            phi = dd_mul(xp, yr);
            gx = dd_mul(dd_mul(xp1, yr), two_prod((double)p_, ih));           // (p = 0: the factor is zero)
            gy = dd_mul(dd_mul(xp, yr1), two_prod((double)r_, ih));
        };
        // ---- B: Nitsche terms on the interface (cuthho_square.cpp:347-360):  sum_q w (eta/h_T phi_i phi_j - phi_i dn_j - dn_i phi_j).
        // With P = p_i + p_j, R = r_i + r_j the entry is
        //     eta/h_T M(P, R) - ih ( P Mx(P - 1, R) + R My(P, R - 1) ),
        // M, Mx, My the moments of the interface measures w, w n_x, w n_y (iface_moments, cut_dd_stages.hpp).
        {
            constexpr int NM1 = P2(2 * RD - 1);
            constexpr int oIM = oTPHI, oIX = oIM + 2 * NMOM, oIY = oIX + 2 * NM1;
            static_assert(2 * (NMOM + 2 * NM1) <= CH * ROWW, "the interface moments fit the point table");
            iface_moments<RD>(a.il_xyw, a.il_off[cc], a.il_off[cc + 1], a.ls, barx, bary, ihalf, l, S + oIM, S + oIX, S + oIY);
            wave_sync();
            if (l < RBS * (RBS + 1) / 2) {                                              // this lane's pair, i <= j
                int pj_ = 0;
                while ((pj_ + 1) * (pj_ + 2) / 2 <= l && pj_ + 1 < RBS) ++pj_;
                const int pi_ = l - pj_ * (pj_ + 1) / 2;
                int p1, r1, p2, r2;
                mono_exps(pi_, p1, r1);
                mono_exps(pj_, p2, r2);
                const int P = p1 + p2, R = r1 + r2;
                dd nacc = dd_mul_d(dd_load(S + oIM + 2 * mono_index(P, R)), eta_h);
                dd g = dd_from(0.0);
                if (P > 0) g = dd_mul_d(dd_load(S + oIX + 2 * mono_index(P - 1, R)), (double)P);
                if (R > 0) g = dd_add(g, dd_mul_d(dd_load(S + oIY + 2 * mono_index(P, R - 1)), (double)R));
                nacc = dd_sub(nacc, dd_mul_d(g, ih));
                const dd v = dd_add(dd_load(S + oST + 2 * (pi_ + pj_ * LD)), nacc);
                dd_store(S + oST + 2 * (pi_ + pj_ * LD), v);
                dd_store(S + oST + 2 * (pj_ + pi_ * LD), v);
            }
            wave_sync();
        }
        // ---- C: gr_rhs (cuthho_square.cpp:362-383); face points of the `where` part, LPC lanes per point
        {
            constexpr int LPC = 64 / NFPT;                     // (3 with the 20 slots)
            static_assert(LPC >= 1, "a lane per face point");
            const int pt_ = l / LPC, sub = l % LPC;
            // (the slots of a face without points exist and hold zeros: the loads do not wait for the count)
            const int c_pt = imin(pt_, NFPT - 1);
            const double *c_src = a.fl_xyw + (((size_t)cc * 4 + c_pt / FACE_SLOTS) * FACE_SLOTS + c_pt % FACE_SLOTS) * 3;
            const double c_x = c_src[0], c_y = c_src[1], c_w = c_src[2];
            const int c_n = a.fl_cnt[cc * 4 + c_pt / FACE_SLOTS];
            if (pt_ < NFPT) {
                const int f = pt_ / FACE_SLOTS, qq = pt_ % FACE_SLOTS;
                const bool ok = qq < c_n;
                const double x = ok ? c_x : barx, y = ok ? c_y : bary, w = ok ? c_w : 0.0;
                const CutFacePoint fp = cut_face_point(ids, px, py, fr, f, x, y);
                const double nx = fp.nx, ny = fp.ny, ep = fp.ep, bx = fp.bx, by = fp.by;
                dd pbx[RD + 1], pby[RD + 1];
                powers_dd(bx, by, pbx, pby);
#pragma unroll
                for (int it = 0; it < (RBS + LPC - 1) / LPC; ++it) {
                    const int m = sub + it * LPC;
                    if (m < RBS) {
                        dd phi, gx, gy;
                        basis_dd_one(pbx, pby, m, phi, gx, gy);
                        dd_store(S + oCPH + 2 * (pt_ * RBS + m), phi);
                        dd_store(S + oCDN + 2 * (pt_ * RBS + m), dd_mul_d(dd_add(dd_mul_d(gx, nx), dd_mul_d(gy, ny)), w));
                    }
                }
                if (sub == LPC - 1) {
                    dd pe = dd_from(1.0);
#pragma unroll
                    for (int k = 0; k < FBS; ++k) { dd_store(S + oCFB + 2 * (pt_ * FBS + k), pe); pe = dd_mul_d(pe, ep); }
                }
            }
            wave_sync();
            for (int e = l; e < RBS * MS; e += 64) {
                const int i = e % RBS, j = e / RBS;
                dd sacc;
                if (j < CBS) {
                    // (four running sums over the face points: one sum is a chain of NFPT dependent additions)
                    dd s4[4] = {dd_from(0.0), dd_from(0.0), dd_from(0.0), dd_from(0.0)};
                    static_assert(NFPT % 4 == 0, "four running sums");
#pragma unroll
                    for (int p_ = 0; p_ < NFPT; ++p_)
                        s4[p_ & 3] = dd_add_fast(s4[p_ & 3], dd_mul(dd_load(S + oCDN + 2 * (p_ * RBS + i)), dd_load(S + oCPH + 2 * (p_ * RBS + j))));
                    sacc = dd_sub_fast(dd_load(S + oST + 2 * (i + j * LD)), dd_add_fast(dd_add_fast(s4[0], s4[1]), dd_add_fast(s4[2], s4[3])));
                } else {
                    const int f = (j - CBS) / FBS, k = (j - CBS) % FBS;
                    sacc = dd_from(0.0);
                    for (int qq = 0; qq < FACE_SLOTS; ++qq)
                        sacc = dd_add_fast(sacc, dd_mul(dd_load(S + oCDN + 2 * ((f * FACE_SLOTS + qq) * RBS + i)), dd_load(S + oCFB + 2 * ((f * FACE_SLOTS + qq) * FBS + k))));
                }
                dd_store(S + oGR + 2 * (i + j * RBS), sacc);
            }
            wave_sync();
        }
        // ---- D: oper = llt(gr_lhs).solve(gr_rhs) (cuthho_square.cpp:385) in registers, one lane per COLUMN of [gr_lhs | gr_rhs]
        // (rbs + msize lanes)
        {
            static_assert(RBS + MS <= 64, "a lane per column of [gr_lhs | gr_rhs]");
            const bool isA = l < RBS, isG = l >= RBS && l < RBS + MS;
            const int gc = isG ? l - RBS : 0;
            dd v[RBS];
#pragma unroll
            for (int i = 0; i < RBS; ++i)
                v[i] = isA ? dd_load(S + oST + 2 * (i + l * LD)) : isG ? dd_load(S + oGR + 2 * (i + gc * RBS)) : dd_from(1.0);
            bad = cut_llt_solve_in_registers<RBS>(v, l, isG);
            if (isG) {
#pragma unroll
                for (int k = 0; k < RBS; ++k) dd_store(S + oOP + 2 * (k + gc * RBS), v[k]);
            }
            wave_sync();
            if (a.oper != nullptr)
                for (int e = l; e < RBS * MS; e += 64) a.oper[(size_t)cc * (RBS * MS) + e] = dd_round(dd_load(S + oOP + 2 * e));
        }
        // ---- E: data = gr_rhs^T oper (cuthho_square.cpp:386) = G^T A^-1 G, symmetric: the entries i <= j, two running sums each,
        // rounded once, mirrored into the LDS image
#pragma unroll 1
        for (int e = l; e < MS * (MS + 1) / 2; e += 64) {
            int i, j;
            tri_index(e, i, j);
            dd s0 = dd_from(0.0), s1 = dd_from(0.0);
#pragma unroll
            for (int k = 0; k < RBS; ++k) {
                const dd t = dd_mul(dd_load(S + oGR + 2 * (k + i * RBS)), dd_load(S + oOP + 2 * (k + j * RBS)));
                if (k & 1) s1 = dd_add_fast(s1, t); else s0 = dd_add_fast(s0, t);
            }
            const double r = dd_round(dd_add_fast(s0, s1));
            S[oDATA + i + j * MS] = r;
            S[oDATA + j + i * MS] = r;
        }
        wave_sync();
        }   // !only_stab
        // ---- F: cut stabilization (cuthho_square.cpp:566-621): faces without points are skipped
        {
            if (l < NFPT) {
                const int f = l / FACE_SLOTS, qq = l % FACE_SLOTS;
                const double *src = a.fs_xyw + (((size_t)cc * 4 + f) * FACE_SLOTS + qq) * 3;
                const double f_x = src[0], f_y = src[1], f_w = src[2];
                const bool ok = qq < a.fs_cnt[cc * 4 + f];
                const double x = ok ? f_x : barx, y = ok ? f_y : bary, w = ok ? f_w : 0.0;
                const int f1 = (f + 1) & 3;
                const double ex = px[f1] - px[f], ey = py[f1] - py[f];
                const double len2 = ex * ex + ey * ey;
                const bool flip = ids[f] > ids[f1];
                const double ax = flip ? px[f1] : px[f], ay = flip ? py[f1] : py[f];
                const double bxx = flip ? px[f] : px[f1], byy = flip ? py[f] : py[f1];
                const double fbx = 0.5 * (ax + bxx), fby = 0.5 * (ay + byy);
                const double ep = 4.0 * ((fbx - ax) * (x - fbx) + (fby - ay) * (y - fby)) / len2;
                const double bx = (x - barx) * ihalf, by = (y - bary) * ihalf;
                for (int m = 0; m < CBS; ++m) S[oTPHI + l * RBS + m] = phi_m(bx, by, m);
                for (int k = 0; k < FBS; ++k) S[oFB + l * FBS + k] = ipow(ep, k);
                S[oTW + l] = w;
            }
            wave_sync();
            for (int e = l; e < 4 * FBS * FBS; e += 64) {              // mass_F  (:608)
                const int f = e / (FBS * FBS), k = e % FBS, k2 = (e / FBS) % FBS;
                double s = 0.0;
                for (int qq = 0; qq < FACE_SLOTS; ++qq) {
                    const int p = f * FACE_SLOTS + qq;
                    s += (S[oTW + p] * S[oFB + p * FBS + k]) * S[oFB + p * FBS + k2];
                }
                S[oMF + f * FBS * FBS + k + k2 * FBS] = s;
            }
            for (int e = l; e < NF * CBS; e += 64) {                   // trace_F (:609)
                const int fk = e % NF, i = e / NF, f = fk / FBS, k = fk % FBS;
                double s = 0.0;
                for (int qq = 0; qq < FACE_SLOTS; ++qq) {
                    const int p = f * FACE_SLOTS + qq;
                    s += (S[oTW + p] * S[oFB + p * FBS + k]) * S[oTPHI + p * RBS + i];
                }
                S[oTR + fk + i * NF] = s;
            }
            wave_sync();
            static_assert(4 * CBS <= 64, "a lane per (face, column)");
            if (l < 4 * CBS) {                                         // mass.llt().solve(trace) (:615): one lane per (face, column)
                const int f = l / CBS, c = l % CBS;                    // (the four faces one after the other on cbs lanes: a chain of
                if (a.fs_cnt[cc * 4 + f] != 0) {                       //  4 x 12 square roots and divisions)
                    double Lf[FBS][FBS], ri[FBS], x[FBS];
#pragma unroll
                    for (int j = 0; j < FBS; ++j) {                    // tiny Cholesky, redundantly per lane; 1 / L_jj kept
                        double d = S[oMF + f * FBS * FBS + j + j * FBS];
#pragma unroll
                        for (int k = 0; k < j; ++k) d -= Lf[j][k] * Lf[j][k];
                        ri[j] = fast_rsqrt<2>(d);
                        Lf[j][j] = d * ri[j];
#pragma unroll
                        for (int i = j + 1; i < FBS; ++i) {
                            double s_ = S[oMF + f * FBS * FBS + i + j * FBS];
#pragma unroll
                            for (int k = 0; k < j; ++k) s_ -= Lf[i][k] * Lf[j][k];
                            Lf[i][j] = s_ * ri[j];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < FBS; ++i) {
                        double s_ = S[oTR + (f * FBS + i) + c * NF];
#pragma unroll
                        for (int k = 0; k < i; ++k) s_ -= Lf[i][k] * x[k];
                        x[i] = s_ * ri[i];
                    }
#pragma unroll
                    for (int i = FBS - 1; i >= 0; --i) {
                        double s_ = x[i];
#pragma unroll
                        for (int k = i + 1; k < FBS; ++k) s_ -= Lf[k][i] * x[k];
                        x[i] = s_ * ri[i];
                    }
#pragma unroll
                    for (int i = 0; i < FBS; ++i) S[oPT + (f * FBS + i) + c * NF] = x[i];
                }
            }
            wave_sync();
            // data += oper_F^T mass_F oper_F / hT, oper_F = [ M^-1 trace | -I_F ]  (:599,:615-617); outputs.
            // Two tables first, on the dead face-point table: OPF[(f,k)][i] = oper_F (zero rows for a face without points) and
            // WF[(f,k)][j] = (mass_F oper_F)[k][j]; then every entry is the 4 FBS-term sum  OPF[:, i] . WF[:, j]  over compile-time
            // rows, its reads in flight together -- the same products in the same order as the nested loops over faces and modes
            // they replace (which skipped the zero factors one data-dependent branch at a time: 28 of the kernel's 114 us).
            double *OPF = S + oTPHI, *WF = S + oTPHI + NF * MS;
            static_assert(2 * NF * MS <= CH * ROWW, "the two tables fit the point table");
            for (int e = l; e < NF * MS; e += 64) {
                const int fk = e % NF, i = e / NF, f = fk / FBS, k = fk % FBS;
                const bool on = a.fs_cnt[cc * 4 + f] != 0;
                OPF[fk + i * NF] = !on ? 0.0 : (i < CBS ? S[oPT + fk + i * NF] : (i == CBS + fk ? -1.0 : 0.0));
            }
            wave_sync();
            for (int e = l; e < NF * MS; e += 64) {
                const int fk = e % NF, jc = e / NF, f = fk / FBS, k = fk % FBS;
                double mo = 0.0;
#pragma unroll
                for (int k2 = 0; k2 < FBS; ++k2) mo += S[oMF + f * FBS * FBS + k + k2 * FBS] * OPF[(f * FBS + k2) + jc * NF];
                WF[fk + jc * NF] = mo;
            }
            wave_sync();
            const size_t off = (size_t)cc * (MS * MS);
            // (the stabilization is symmetric like data: the entries i <= jc, two running sums each, both copies stored)
#pragma unroll 1
            for (int e = l; e < MS * (MS + 1) / 2; e += 64) {
                int i, jc;
                tri_index(e, i, jc);
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int fk = 0; fk < NF; fk += 2) {
                    s0 += OPF[fk + i * NF] * WF[fk + jc * NF];
                    s1 += OPF[fk + 1 + i * NF] * WF[fk + 1 + jc * NF];
                }
                const double st = (s0 + s1) * (1.0 / hT), dt = S[oDATA + i + jc * MS];
                const int e1 = i + jc * MS, e2 = jc + i * MS;
                if (a.lc != nullptr) { a.lc[off + e1] = dt + st; a.lc[off + e2] = dt + st; }
                if (a.data != nullptr) { a.data[off + e1] = dt; a.data[off + e2] = dt; }
                if (a.stab != nullptr) { a.stab[off + e1] = st; a.stab[off + e2] = st; }
            }
            if (a.info != nullptr && l == 0) a.info[cc] = bad;
        }

        // ---- H: right-hand side (cuthho_square.cpp:630-657).  The source / boundary functions are
        // evaluated once per quadrature point (one lane each, chunks of 64), then lane i sums its mode.
        if (a.rhs != nullptr) {
            double s = rhs_acc;                                         // volume part, accumulated in stage A
            const uint32_t r0 = a.ir_off[cc], r1 = a.ir_off[cc + 1];      // integrate_interface(msh, cl, degree, where)  (:647)
            for (uint32_t base = r0; base < r1; base += CH) {
                const uint32_t q = base + l;
                // The point's lane stages the POWERS bx^e, by^e (the products ipow forms, in its order) next to the weighted boundary
                // value and the normal; the mode's lane then reads the four powers its monomial and its gradient need.  (With
                // the monomials and their gradients evaluated per point and mode -- exponent search and power loops inside a serial loop over the points --
                // this stage was 45 of the kernel's 114 us.)
                constexpr int HROW = 2 * (RD + 1) + 3;
                static_assert(HROW <= ROWW, "stage H rows fit the point table of stage A");
                if (q < r1) {
                    const double x = a.ir_xyw[3 * q], y = a.ir_xyw[3 * q + 1], wq = a.ir_xyw[3 * q + 2];
                    double nx, ny;
                    a.ls.normal(x, y, nx, ny);
                    const double bx = (x - barx) * ihalf, by = (y - bary) * ihalf;
                    double vx = 1.0, vy = 1.0;
#pragma unroll
                    for (int e = 0; e <= RD; ++e) {
                        S[oTPHI + HROW * l + e] = vx;
                        S[oTPHI + HROW * l + (RD + 1) + e] = vy;
                        vx *= bx; vy *= by;
                    }
                    S[oTPHI + HROW * l + 2 * (RD + 1)] = wq * (a.bcs_fn == FN_SAMPLED ? a.bcs_vals[q] : builtin_fn(a.bcs_fn, x, y));
                    S[oTPHI + HROW * l + 2 * (RD + 1) + 1] = nx;
                    S[oTPHI + HROW * l + 2 * (RD + 1) + 2] = ny;
                }
                wave_sync();
                const int nq = (int)((r1 - base) < (uint32_t)CH ? (r1 - base) : (uint32_t)CH);
                if (l < CBS) {
                    int hp, hr;
                    mono_exps(l, hp, hr);
                    const int hp1 = hp > 0 ? hp - 1 : 0, hr1 = hr > 0 ? hr - 1 : 0;
                    const double cpx = hp == 0 ? 0.0 : hp * ih, cpy = hr == 0 ? 0.0 : hr * ih;      // (p ih, r ih: the leading factors of the gradient)
#pragma unroll 4
                    for (int t = 0; t < nq; ++t) {
                        const double *row = S + oTPHI + HROW * t;
                        const double xp = row[hp], yr = row[(RD + 1) + hr], xp1 = row[hp1], yr1 = row[(RD + 1) + hr1];
                        const double gx = hp == 0 ? 0.0 : cpx * xp1 * yr, gy = hr == 0 ? 0.0 : cpy * xp * yr1;
                        s += row[2 * (RD + 1)] * ((xp * yr) * eta_h - (gx * row[2 * (RD + 1) + 1] + gy * row[2 * (RD + 1) + 2]));
                    }
                }
                wave_sync();
            }
            if (l < CBS) a.rhs[(size_t)cc * CBS + l] = s;
        }
        wave_sync();
    }
}

// fictitious-domain merge: the cut cells' operators replace the rows of the cell-major arrays and
// the right-hand side of cells outside `where` is zeroed (cuthho_square.cpp:628-629, 659-664).
// Two launches: one block per CUT cell (the list of cut cells, ~0.5 % of the mesh) copies its matrix and right-hand side;
// one thread per right-hand-side entry of the whole mesh zeroes those of the cells outside the domain (coalesced stores).
// (One block per cell of the WHOLE mesh, most of them with nothing or 80 bytes to write, took 51 us of config 3's 620.)
static __global__ __launch_bounds__(64) void cut_merge_cells_kernel(uint32_t ncut, const uint32_t *cut_cells, int msize2, int cbs,
                                                            const double *cut_lc, const double *cut_rhs, double *lc, double *rhs)
{
    const size_t cc = blockIdx.x;
    if (cc >= ncut) return;
    const size_t c = cut_cells[cc];
    if (lc != nullptr && cut_lc != nullptr) {
        // (msize^2 is even for the even msize of the cut configurations; the odd tail entry by itself)
        const double *src = cut_lc + cc * (size_t)msize2;
        double *dst = lc + c * (size_t)msize2;
        for (int e = threadIdx.x; e < msize2; e += 64) dst[e] = src[e];
    }
    if (rhs != nullptr && cut_rhs != nullptr)
        for (int e = threadIdx.x; e < cbs; e += 64) rhs[c * (size_t)cbs + e] = cut_rhs[cc * (size_t)cbs + e];
}

// condensed mode: the cut cells' packed records [upper triangle of S | g] into the cell-major record array
static __global__ __launch_bounds__(64) void cut_merge_condensed_kernel(uint32_t ncut, const uint32_t *cut_cells, int ntri, int nf, const double *cut_Sp,
                                                                const double *cut_g, double *cond)
{
    const size_t cc = blockIdx.x;
    if (cc >= ncut) return;
    double *dst = cond + (size_t)cut_cells[cc] * (size_t)(ntri + nf);
    for (int e = threadIdx.x; e < ntri; e += 64) dst[e] = cut_Sp[cc * (size_t)ntri + e];
    for (int e = threadIdx.x; e < nf; e += 64) dst[ntri + e] = cut_g[cc * (size_t)nf + e];
}

static __global__ __launch_bounds__(256) void cut_zero_rhs_kernel(size_t total, uint32_t cbs, const int8_t *cell_loc, int where, double *rhs)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int loc = cell_loc[t / cbs];
    if (loc != LOC_CUT && loc != where) rhs[t] = 0.0;
}

}  // namespace pa
