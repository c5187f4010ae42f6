// cut_dd_stages.hpp -- the double-double stages that the one-sided cut kernel (cut_device.hpp) and the two-sided interface kernel
// (cut_interface_device.hpp) have in common, stated once: the geometry of a cut cell, the stiffness formed from the cell moments,
// the moments of the interface measures, the frame of a face point, the register Cholesky with both substitutions, and the decode
// of a packed triangle.  A block is one wavefront; the functions take LDS pointers, leading dimensions and the lane, never a
// kernel's argument struct.  What the two kernels do differently (the lane split of stage C, the Nitsche scatter, the one-sided
// stages F and H) stays with them.  So do the cell moments of stage A, the same text in both: behind a function boundary of any
// form tried, the one-sided kernel at k = 2 -- which uses its 256 registers in full -- takes one spill slot more (476 against 472
// bytes of scratch).  The lane is taken by reference where a stage hands it on (iface_moments): by value that kernel's scratch
// grew to 496 bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cut_host.hpp"
#include "dd_arith.hpp"
#include "hho_device.hpp"

namespace pa {

// ---- geometry of the WHOLE cell (cell_basis, normals, measure: bases.hpp:85-91, basic_geom.hpp:349-372, cuthho_square.cpp:344):
// the ids of the vertices and their coordinates into the caller's arrays (plain arrays of four: a face picks its endpoints by a
// run-time index, which a struct member would answer from scratch memory); barycentre, 1 / (h / 2) and 2 / h with h the diameter,
// and the measure hT as the value
struct CutCellFrame {
    double barx, bary, ihalf, ih, hT;
};

__device__ __forceinline__ CutCellFrame cut_cell_frame(const double *points, const uint32_t *ptids, uint32_t cell, uint32_t (&ids)[4],
                                                       double (&px)[4], double (&py)[4])
{
    CutCellFrame g;
    const uint4 idv = *reinterpret_cast<const uint4 *>(ptids + 4 * (size_t)cell);
    ids[0] = idv.x; ids[1] = idv.y; ids[2] = idv.z; ids[3] = idv.w;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const double2 p = *reinterpret_cast<const double2 *>(points + 2 * (size_t)ids[v]);
        px[v] = p.x; py[v] = p.y;
    }
    {
        double rx = 0.0, ry = 0.0, den = 0.0;
#pragma unroll
        for (int i = 2; i < 4; ++i) {
            const double ax = px[i - 1] - px[0], ay = py[i - 1] - py[0], bx = px[i] - px[0], by = py[i] - py[0];
            const double d = (ax * by - ay * bx) / 2.0;
            rx += (ax + bx) * d; ry += (ay + by) * d; den += d;
        }
        g.barx = px[0] + rx / (den * 3); g.bary = py[0] + ry / (den * 3);
    }
    double hd = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i + 1; j < 4; ++j) hd = fmax(hd, sqrt((px[j] - px[i]) * (px[j] - px[i]) + (py[j] - py[i]) * (py[j] - py[i])));
    g.ihalf = 1.0 / (0.5 * hd); g.ih = 2.0 / hd;
    double hT = 0.0;
#pragma unroll
    for (int i = 1; i < 3; ++i)
        hT += fabs((px[i] - px[0]) * (py[i + 1] - py[0]) - (py[i] - py[0]) * (px[i + 1] - px[0])) * 0.5;
    g.hT = hT;
    return g;
}

// ---- stiffness from the moments (bases.hpp:170-176), times `scale`, into the rbs x rbs block at dst with leading dimension LD
template <int RD, int LD>
__device__ __forceinline__ void cut_stiffness_from_moments(const double *mom, dd scale, double *dst, int l)
{
    constexpr int RBS = P2(RD);
    for (int e = l; e < RBS * RBS; e += 64) {
        int ai, bi, aj, bj;
        mono_exps(e % RBS, ai, bi);
        mono_exps(e / RBS, aj, bj);
        dd v = dd_from(0.0);
        if (ai * aj) v = dd_add(v, dd_mul_d(dd_load(mom + 2 * mono_index(ai + aj - 2, bi + bj)), (double)(ai * aj)));
        if (bi * bj) v = dd_add(v, dd_mul_d(dd_load(mom + 2 * mono_index(ai + aj, bi + bj - 2)), (double)(bi * bj)));
        dd_store(dst + 2 * ((e % RBS) + (e / RBS) * LD), dd_mul(v, scale));
    }
}

// ---- the moments of the interface measures w, w n_x, w n_y over the interface points [i0, i1) (the normal of the level set, not
// flipped for the positive side: cuthho_square.cpp:352-355): M up to degree 2 RD, Mx and My up to 2 RD - 1, as (hi, lo) pairs.
// The Nitsche terms are sums of these: the basis functions are monomials bx^p by^r, so with P = p_i + p_j, R = r_i + r_j
//     sum_q w phi_i phi_j = M(P, R),   sum_q w phi_i (dphi_j . n) = ih (p_j Mx(P - 1, R) + r_j My(P, R - 1)):
// 28 + 21 + 21 sums at k = 2 instead of the 55 pairs' two products per point, formed like the cell moments (a lane per point, the
// transposed butterfly), in passes over the points so that one pass's accumulators fit the registers.  (Staging phi, w dn and
// w (eta/h phi - dn) per point and summing the pairs' terms point by point was 41 k of the one-sided kernel's 157 k clocks.)
template <int RD>
__device__ __forceinline__ void iface_moments(const double *il_xyw, uint32_t i0, uint32_t i1, const LevelSet &ls, double barx, double bary,
                                              double ihalf, const int &l, double *M, double *Mx, double *My)
{
    constexpr int DM = 2 * RD;
    // (the lane's point of the first 64 -- normally all there are -- and its normal: loaded and formed once for the passes)
    const bool in0 = i0 + l < i1;
    const double x0 = in0 ? il_xyw[3 * (i0 + l)] : barx, y0 = in0 ? il_xyw[3 * (i0 + l) + 1] : bary;
    const double w0 = in0 ? il_xyw[3 * (i0 + l) + 2] : 0.0;
    double nx0, ny0;
    ls.normal(x0, y0, nx0, ny0);
    // one pass: the moments of total degree K0 .. K1 of measure KIND (0: w, 1: w n_x, 2: w n_y)
    auto pass = [&](auto kind_c, auto k0_c, auto k1_c, double *dst) {
        constexpr int KIND = decltype(kind_c)::value, K0 = decltype(k0_c)::value, K1 = decltype(k1_c)::value;
        constexpr int B0 = K0 * (K0 + 1) / 2, NM = P2(K1) - B0;
        dd acc[NM];
        bool first = true;
        for (uint32_t q0 = i0; q0 < i1; q0 += 64) {
            const uint32_t q = q0 + l;
            const bool in = q < i1;
            double x = x0, y = y0, w = w0, nx = nx0, ny = ny0;
            if (q0 != i0) {
                x = in ? il_xyw[3 * q] : barx; y = in ? il_xyw[3 * q + 1] : bary; w = in ? il_xyw[3 * q + 2] : 0.0;
                if (KIND != 0) ls.normal(x, y, nx, ny);
            }
            const double bx = (x - barx) * ihalf, by = (y - bary) * ihalf;
            dd pbx[K1 + 1], pby[K1 + 1];
            pbx[0] = KIND == 0 ? dd_from(w) : two_prod(w, KIND == 1 ? nx : ny);
            pby[0] = dd_from(1.0);
#pragma unroll
            for (int e = 1; e <= K1; ++e) { pbx[e] = dd_mul_d(pbx[e - 1], bx); pby[e] = dd_mul_d(pby[e - 1], by); }
            if (first) {                                             // (the usual case is one point per lane: no addition at all)
#pragma unroll
                for (int k = K0; k <= K1; ++k)
#pragma unroll
                    for (int r = 0; r <= k; ++r) acc[k * (k + 1) / 2 + r - B0] = dd_mul(pbx[k - r], pby[r]);
                first = false;
            } else {
#pragma unroll
                for (int k = K0; k <= K1; ++k)
#pragma unroll
                    for (int r = 0; r <= k; ++r)
                        acc[k * (k + 1) / 2 + r - B0] = dd_add_fast(acc[k * (k + 1) / 2 + r - B0], dd_mul(pbx[k - r], pby[r]));
            }
        }
        if (first) {
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[m] = dd_from(0.0);
        }
        dd tot; bool ok = true;
        const int m = lanes_transpose_reduce<NM, 32>(acc, l, dd_from(0.0), [](dd u, dd v_) { return dd_add_fast(u, v_); },
                                                     [](dd u, int off) { return dd_shfl_xor(u, off); }, tot, ok);
        if (ok) dd_store(dst + 2 * (B0 + m), tot);
    };
    using I0 = std::integral_constant<int, 0>;
    constexpr int KS = DM >= 4 ? DM - 2 : 0;              // (k = 2: degrees 0..4 and 5..6 apart: 15 + 13 accumulators, not 28)
    pass(I0(), I0(), std::integral_constant<int, KS>(), M);
    if constexpr (KS < DM) pass(I0(), std::integral_constant<int, KS + 1>(), std::integral_constant<int, DM>(), M);
    pass(std::integral_constant<int, 1>(), I0(), std::integral_constant<int, DM - 1>(), Mx);
    pass(std::integral_constant<int, 2>(), I0(), std::integral_constant<int, DM - 1>(), My);
}

// ---- the frame of a point (x, y) on face f of the cell: the outward normal of the CELL (basic_geom.hpp:361-369), the face
// coordinate ep in [-1, 1] measured from the lower-id endpoint (the face basis of the WHOLE face, bases.hpp:253-280) and the scaled
// cell coordinates bx, by
struct CutFacePoint {
    double nx, ny, ep, bx, by;
};

__device__ __forceinline__ CutFacePoint cut_face_point(const uint32_t (&ids)[4], const double (&px)[4], const double (&py)[4], const CutCellFrame &g,
                                                       int f, double x, double y)
{
    CutFacePoint p;
    const int f1 = (f + 1) & 3;
    const double ex = px[f1] - px[f], ey = py[f1] - py[f];          // dynamic index: 4 entries, fine here
    const double len = sqrt(ex * ex + ey * ey);
    p.nx = ey / len; p.ny = -ex / len;
    const bool flip = ids[f] > ids[f1];
    const double ax = flip ? px[f1] : px[f], ay = flip ? py[f1] : py[f];
    const double bxx = flip ? px[f] : px[f1], byy = flip ? py[f] : py[f1];
    const double fbx = 0.5 * (ax + bxx), fby = 0.5 * (ay + byy);
    p.ep = 4.0 * ((fbx - ax) * (x - fbx) + (fby - ay) * (y - fby)) / (len * len);
    p.bx = (x - g.barx) * g.ihalf; p.by = (y - g.bary) * g.ihalf;
    return p;
}

// ---- llt(A).solve(G) in registers, one lane per COLUMN of [A | G]: lane c < N holds column c of the symmetric positive definite
// A (kept whole), the isG lanes a column of G each, the others ones; on return the isG lanes hold their column of A^-1 G.  The
// value is 0 or 1 + the first pivot that was not positive.
// Right-looking: at pivot j every lane forms y = v_j / sqrt(d) -- a column of A its entry L_kj, a column of G its
// forward-substituted entry -- and takes  v_i -= L_ij y  for the rows below, L_ij read from lane j's registers (v_readlane: no LDS
// image of the factor, no barrier per pivot).  A pivot's dependent path is rsqrt -> y -> ONE update of the next pivot column; the
// updates of a step are independent of each other.  The left-looking form on an LDS image it replaces had the j-term sum in front
// of every pivot, and its substitutions kept the lanes of G busy with a chain of N (N - 1) / 2 dependent subtractions each way:
// 51 k of the one-sided kernel's 230 k clocks, and most of the two-sided kernel's time.
template <int N>
__device__ __forceinline__ int cut_llt_solve_in_registers(dd (&v)[N], int l, bool isG)
{
    int bad = 0;
    dd rsv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const dd piv = dd_readlane(v[j], j);
        if (!(piv.hi > 0.0) && !bad) bad = j + 1;
        const dd rs = dd_rsqrt_1(piv);
        rsv[j] = rs;
        const dd y = dd_mul(v[j], rs);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            const dd scaled = dd_mul(v[i], rs);                  // (lane j: L_ij)
            const dd lij = dd_readlane(scaled, j);
            const dd upd = dd_sub_fast(v[i], dd_mul(lij, y));
            v[i].hi = l == j ? scaled.hi : l > j ? upd.hi : v[i].hi;
            v[i].lo = l == j ? scaled.lo : l > j ? upd.lo : v[i].lo;
        }
        v[j].hi = l >= j ? y.hi : v[j].hi;
        v[j].lo = l >= j ? y.lo : v[j].lo;
    }
    // backward substitution, column-oriented as well: x_i = v_i / L_ii, then v_k -= L_ik x_i for the rows above
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        const dd x = dd_mul(v[i], rsv[i]);
        if (isG) v[i] = x;
#pragma unroll
        for (int k = 0; k < i; ++k) {
            const dd lik = dd_readlane(v[i], k);                 // entry i of column k of L (the lanes of A are not touched here)
            const dd upd = dd_sub_fast(v[k], dd_mul(lik, x));
            if (isG) v[k] = upd;
        }
    }
    return bad;
}

// ---- packed entry e of a symmetric matrix's triangle -> (i, j), i <= j, e = j (j + 1) / 2 + i
__device__ __forceinline__ void tri_index(int e, int &i, int &j)
{
    j = (int)((__fsqrt_rn((float)(8 * e + 1)) - 1.0f) * 0.5f);
    j += (j + 1) * (j + 2) / 2 <= e ? 1 : 0;
    j -= j * (j + 1) / 2 > e ? 1 : 0;
    i = e - j * (j + 1) / 2;
}

}  // namespace pa
