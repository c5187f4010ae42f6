// hho_device.hpp -- CDNA4 (gfx950) device code for the per-cell HHO local operators.
//
// WHAT is computed is defined by the reference (paths relative to the reference root):
//   make_hho_laplacian            src/methods/hho_bits/hho.hpp:32-96
//   make_hho_naive_stabilization  hho.hpp:99-148      (h = cell AREA,     hho.hpp:119)
//   make_hho_fancy_stabilization  hho.hpp:155-237     (h = cell DIAMETER, hho.hpp:201)
//   cell_basis / face_basis       src/core/core_bits/bases.hpp:70-195, 241-291
//   integrate (tensor / fan / face), gauss_legendre, triangle_quadrature
//                                 src/core/core_bits/quadratures.hpp:78-158, 238-432
//   barycenter/diameter/measure/normals  src/core/core_bits/basic_geom.hpp:247-372
//
// HOW is not the reference's.  The path is two kernels: the per-cell head -- geometry, cell quadrature, moments,
// stiffness, Cholesky of gr_lhs (and the mass rows / factor of the dense fancy form) -- runs one THREAD per cell
// (hho_pre.hpp) and hands a small record per cell to the kernel of this file, in which G lanes of a 64-wide
// wavefront cooperate on one cell:
//   * the cell basis is a set of scaled monomials, so every cell integral of phi_i phi_j or
//     grad phi_i . grad phi_j is a *moment*  sum_q w_q bx_q^p by_q^r  of the same quadrature
//     rule: the pre-pass accumulates P2(2 recdeg) moments and gathers the stiffness / mass matrices from them -- term
//     by term the same sums the reference forms; the moments the cell columns of gr_rhs need travel with the record;
//   * the face basis evaluated at the face Gauss points is t_q^k exactly, so every face mass
//     matrix is (|F|/2) M^ with one constant factorization shared by all faces of all cells;
//   * lane c of a cell owns COLUMN c of every msize-wide matrix (gr_rhs, Y, oper, T, U): uniform
//     loops, broadcast LDS reads, no per-entry index arithmetic;
//   * data = gr_rhs^T (L L^T)^-1 gr_rhs = Y^T Y with Y = L^-1 gr_rhs (forward substitution only), the packed factor
//     in registers and broadcast through DPP operands (the dense fancy instances read an LDS image of it);
//   * stab = (1/h) sum_F B_F^T M_F B_F = U^T U with U_F = sqrt(|F|/2h) L^^T B_F, where
//     B_F = M_F^-1 T_F - E_F is the reference's proj2 + proj3 (hho.hpp:222-231); T_F = [trace_F | 0]
//     for the naive stabilization and for the fancy one when celdeg == recdeg (then
//     pi_T^k p_T^k v == p_T^k v and hho.hpp:184-190 cancels);
//   * lc = Z^T Z with Z = [Y; U]: one symmetric rank update -- on v_mfma_f64_16x16x4_f64 when only lc is
//     asked for (one LDS read per lane feeds 16 FMAs), accumulators to HBM directly or through an LDS image;
//     each lane forming the entries (c, c+d mod msize), d = 0..msize/2, with vector FMAs when data and stab
//     are wanted apart;
//   * the condensed and the assembling mode keep the image on the chip: the cell unknowns are eliminated in it, or its
//     entries go straight to the CSR arrays of the global system;
//   * the block's one wavefront synchronises on its LDS data with wave_sync() (no wait for outstanding
//     stores), and the next cell's record is in flight while the current cell is processed;
//   * reciprocals and square roots are v_rcp/v_rsq seeds refined by Newton steps (<= 1 ulp).
//
// Design choices that were measured and settled are not switches here: DESIGN.md section 6 lists what was tried, the
// figure, and the commit that last held the code.  A switch lives in this header only while its question is open.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hho_asm_scatter.hpp"

// Per-instance settings of the build (proton_amd/_build.py):
// minimum waves per SIMD the register allocator must leave room for (2nd __launch_bounds__
// argument); 0 = per configuration (Cfg::WAVES)
#ifndef PA_WAVES_PER_EU
#define PA_WAVES_PER_EU 0
#endif
// msize from which the lc-only kernel stores its accumulators straight to HBM instead of through an LDS image
#ifndef PA_DIRECT_MIN
#define PA_DIRECT_MIN 14
#endif
// forward substitution Y = L^-1 gr_rhs from the LDS image of L: doubles of L read per LDS round trip (0: row by row)
#ifndef PA_FWD_CAP
#define PA_FWD_CAP 24
#endif
#ifdef PA_MARKERS
#define PA_MARK(x) asm volatile("; PAMARK " x)
#else
#define PA_MARK(x)
#endif
// diagnostic build (-DPA_STAGE_CLOCK): shader-clock stamps at the stage boundaries, summed per block over its cells
// and written to LocalOpsArgs::dbg[block][stage]; PA_TICK(i) closes stage i
#ifdef PA_STAGE_CLOCK
#define PA_NSTAGE 16
#define PA_TICK(i) do { const long long t_ = clock64(); tk_sum[i] += t_ - tk_last; tk_last = t_; } while (0)
#else
#define PA_TICK(i)
#endif
namespace pa {

enum { QUAD_TENSOR = 0, QUAD_FAN = 1 };
enum { STAB_NONE = 0, STAB_NAIVE = 1, STAB_FANCY = 2 };

// Wavefront priority by stage (s_setprio): a wavefront raises its issue priority as it moves through a pass, so that of the
// wavefronts of a SIMD the one closest to its stores wins the issue slot -- the stores of a pass go out earlier, and the
// wavefronts drift apart in phase instead of queueing for the same pipe in the same stage.
constexpr int PRIO_HEAD = 0;      // S0 - S3: the record's scalars, the face-point tables
constexpr int PRIO_S3B = 1;       // S3b: columns of gr_rhs
constexpr int PRIO_MID = 2;       // S4 - S6: substitutions, U
constexpr int PRIO_OUT = 3;       // S7 - S9: product, output, elimination / scatter of the condensed and assembling modes
// condensed mode: number of pivots (cbs) from which the elimination chain runs right-looking (cond_dpp_chain_rl): shorter
// dependent path per step, worth it only on the 15 pivots of k = 3
constexpr int COND_RL_MIN = 12;
// condensed mode: face unknowns (4 fbs) from which the Schur complement A_FF - W^T W is one tile of the matrix pipe; below
// (k <= 1) the tile would be more than half empty
constexpr int COND_SCHUR_MFMA_MIN = 12;

// Quadrature tables, filled by the host (quad_tables.hpp) and passed by device pointer:
//   gauss_*[n][i]: the n-node rule of gauss_legendre() in the reference's emission order;
//   dun[r][row] = (l0, l1, l2, w) of dunavant rules[r] (0-based, rules[r] == rule_{r+1}).
// Face tables for face degree fd (n = fd + 1 Gauss points, fbs = fd + 1 modes): the face basis at
// the Gauss points is t_q^k, so M_F = (|F|/2) M^ with M^ = sum_q w_q t_q^(i+j) = L^ L^^T.
struct FaceTables {
    double fb[4][4];      // [q][k] t_q^k
    double cw[4][4];      // [q][k] w_q t_q^k
    double lf[4][4];      // [i][k] L^ (lower), diagonal holds 1 / L^[i][i]
    double lft[4][4];     // [j][k] (L^^T)[j][k] = L^[k][j], j <= k
};
struct QuadTables {
    double gauss_x[9][8];      // up to 8 nodes: closed forms to 5 (quadratures.hpp:96-150), golub_welsch's rules beyond (:32-75)
    double gauss_w[9][8];
    double dun[9][16][4];
    int dun_n[9];
    FaceTables face[4];
};

__host__ __device__ constexpr int P2(int d) { return (d + 2) * (d + 1) / 2; }
// points of triangle_quadrature(deg) including the rules[deg] off-by-one (quadratures.hpp:257-268)
__host__ __device__ constexpr int dunavant_points(int deg)
{
    const int d = deg == 0 ? 1 : deg;
    return d == 1 ? 3 : d == 2 ? 4 : d == 3 ? 6 : d == 4 ? 7 : d == 5 ? 12 : d == 6 ? 13 : d == 7 ? 16 : 0;
}
__host__ __device__ constexpr int gauss_nodes(int deg) { return ((deg | 1) + 1) / 2; }
__host__ __device__ constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ constexpr int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }

// COND_ = 1: the instance of the condensed mode (static condensation fused behind the product, no lc in HBM): its
// region Q also holds the (MS + 1)-row image of [lc f_T; f_T^T 0] the partial factorization works on.
template <int CD_, int FD_, int QUAD_, int STAB_, int G_, int COND_ = 0>
struct Cfg {
    static constexpr int CD = CD_, FD = FD_, RD = FD_ + 1, QUAD = QUAD_, STAB = STAB_, G = G_;
    static constexpr bool COND = COND_ != 0;
    static constexpr int RBS = P2(RD), CBS = P2(CD), FBS = FD + 1;
    static constexpr int NF = 4 * FBS, MS = CBS + NF, NR = RBS - 1;
    static constexpr int QDEG = 2 * RD;                       // hho.hpp:55,174
    static constexpr int NG = gauss_nodes(QDEG);
    static constexpr int NT = dunavant_points(QDEG);          // per fan triangle
    static constexpr int NQ = QUAD == QUAD_TENSOR ? NG * NG : 4 * NT;
    static constexpr int NFQ = gauss_nodes(2 * FD);           // hho.hpp:74,132,208
    static constexpr int NFP = 4 * NFQ;
    static constexpr bool FANCY = STAB == STAB_FANCY, NAIVE = STAB == STAB_NAIVE;
    static constexpr bool GENERAL_FANCY = FANCY && CD != RD;  // T_F is dense; otherwise T_F = [trace_F | 0]
    // The per-cell head is taken from the pre-pass (hho_pre.hpp); for the dense fancy form its record also carries the
    // rows of the cell mass matrix and the Cholesky factor of its leading block (hho.hpp:173-190).
    // Cell columns of gr_rhs (hho.hpp:64-85): stiff[i, c] - sum_F int_F (grad phi_i . n) phi_c = -int_T phi_c lap(phi_i)
    // (divergence theorem; both quadratures of the reference are exact for these integrands), i.e. 0, 1 or 2 cell
    // moments of degree <= recdeg - 2 + celdeg with integer coefficients.  The moments travel with the record.
    static constexpr int DG = RD - 2 + CD;                    // highest moment degree that is needed
    static constexpr int NMG = RD >= 2 ? P2(DG) : 0, NMGP = (NMG + 1) & ~1;
    // Every lane of a cell reads the SAME element of L in every step of the substitutions Y = L^-1 gr_rhs and L^-T Y: as LDS
    // reads that is a 16-byte broadcast per two FMAs, a quarter of the kernel's LDS cycles at k = 3 -- and the LDS pipeline is
    // its busiest unit.  Instead the packed factor (and the reciprocal diagonal) sits in registers, element e in lane e mod 16 of
    // each row of 16 lanes (ceil((NL + NR) / 16) doubles per lane, one 8-byte LDS read each), and the FMAs take it through the
    // DPP operand  v_fmac_f64_dpp ... row_newbcast:n  (gfx90a+: lane n of the row of 16, for 64-bit operands).  No image of L.
    // The dense fancy instances keep an LDS image of L (batched reads, lds_forward_rd_batched).
    static constexpr bool DPPFWD = !GENERAL_FANCY;
    static constexpr int NPW = 2 * RD + 1;                    // powers 0..2 recdeg (the head: hho_pre.hpp, hho_small.hpp)
    static constexpr int NMOM = P2(2 * RD);
    static constexpr int CPW = 64 / G;                        // cells per wavefront
    static constexpr int PPL = cdiv(NFP, G);                  // face points per lane (S1)
    static constexpr int ND = MS / 2 + 1;                     // rotations of the symmetric update
    // register budget: the k = 3 kernels need > 168 VGPRs to run without spills (measured: 2 waves/SIMD
    // without spills beat 3 with), the others fit 3 waves/SIMD
    // (the dense fancy form carries the mass factor and the dense T_F as well: one step lower, or it spills by the hundred)
    static constexpr int WAVES = PA_WAVES_PER_EU ? PA_WAVES_PER_EU
                              : GENERAL_FANCY ? ((MS > 24 || RBS > 10) ? 1 : (MS > 16 || RBS > 6) ? 2 : (CBS <= 1 ? 4 : 3))      /* (cell degree 0 -- the obstacle pair (0,1): 120 registers --: 4 against 3 waves: -5 % lc, -17 % condensed; (1,1) spills at 4) */
                                            : ((MS > 24 || RBS > 10) ? 2 : 3);
    static constexpr bool HAS_STAB = STAB != STAB_NONE;
    // lc-only path: accumulators -> HBM directly (no LDS image) where the matrix is big enough for the
    // 128-byte runs to pay (measured: -5 % at msize 14, -2 % at 22, -1 % at 31, but +19 % at msize 9)
    static constexpr bool DIRECT_STORE = CBS + 4 * FBS >= PA_DIRECT_MIN;
    // msize 17..24: the bottom-right tile of Z^T Z holds at most 8 x 8 useful entries and would cost the matrix pipe as
    // much as a full one -> vector FMAs, one lane per unordered pair of its columns
    static constexpr int NCORNER = CBS + 4 * FBS - 16;
    static constexpr bool CORNER_VALU = NCORNER > 0 && NCORNER <= 8 && NCORNER * (NCORNER + 1) / 2 <= G;

    // lc with T_F = [trace_F | 0] and 17..32 columns: the second column tile holds face columns only, of the faces UF1..3,
    // and the U rows of the other faces are zero in it.  With the rows of those faces FIRST behind Y (a permutation of the
    // rows of Z does not change Z^T Z) the products of that tile stop after the Y rows and theirs: KS1 k-steps instead of KS.
    static constexpr bool UPERM = HAS_STAB && !GENERAL_FANCY && CBS <= 16 && CBS + 4 * FBS > 16 && CBS + 4 * FBS <= 32;
    static constexpr int UF1 = UPERM ? (16 - CBS) / FBS : 0;
    static constexpr int KS1 = cdiv(((RBS - 1 + 1) & ~1) + (4 - UF1) * FBS, 4);
    // ---- record of a cell written by the pre-pass (doubles): packed lower triangle of L = chol(gr_lhs), row-major,
    // TRUE diagonal | 1/diagonal | pad | sqrt(|F|/2h) x 4, barycenter, 2/h_T, pivot status, the 4 vertices, face
    // orientation bits (bit f: the first vertex of local face f has the HIGHER point id), pad
    struct Pre {
        static constexpr int NL = (RBS - 1) * RBS / 2;
        static constexpr int oSCAL = (NL + (RBS - 1) + 1) & ~1;
        static constexpr int NSCAL = 18 + NMGP;               // ([17]: pivot status of the mass factor; [18..]: the NMG moments)
        // dense fancy form only: rows i < CBS of the cell mass matrix, [j][i]; packed chol(M1), true diagonal; 1/diagonal
        static constexpr int oMR = oSCAL + NSCAL, NMR = GENERAL_FANCY ? CBS * RBS : 0;
        static constexpr int oMC = oMR + NMR, NMC = GENERAL_FANCY ? CBS * (CBS + 1) / 2 : 0;
        static constexpr int oMCR = oMC + NMC;
        static constexpr int NPRE = (oMCR + (GENERAL_FANCY ? CBS : 0) + 1) & ~1;
        static constexpr int NP2 = NPRE / 2;                  // 16-byte pairs
    };
    static constexpr int PLC = cdiv(Pre::NP2, G);             // pairs of the record per lane

    // ---- LDS map (doubles, per cell).  Every vector that is read as a contiguous run starts at
    // an even offset and has an even stride, so the reads are 16-byte ds_read_b128.
    static constexpr int NRP = (NR + 1) & ~1;                 // padded row count of gr_lhs / Y
    // stride of the (symmetric) stiffness matrix / of the image of L: even (16-byte rows); for the 14 rows of k = 3 also
    // LD / 2 odd, so that lanes reading DIFFERENT rows with 16-byte loads (row c-1 of L added to cell column c) do not
    // share banks (LD = 16 put the 14 rows on two bank sets: 8-way conflicts, a quarter of the kernel's conflict cycles)
    static constexpr int LD = (((RBS + 1) & ~1) % 4 == 0 && RBS > 10) ? ((RBS + 1) & ~1) + 2 : ((RBS + 1) & ~1);
    static constexpr int ZR = NRP + (HAS_STAB ? NF : 0);      // rows of Z = [Y; pad; U]
    static constexpr int ZS = ((ZR + 1) & ~1) % 4 == 2 ? ((ZR + 1) & ~1) : ((ZR + 1) & ~1) + 2;   // even, ZS/2 odd
    // region Q: the face-point tables -- dead once the gr_rhs columns are in registers and the trace columns are formed
    // (after S4b); Z = [Y; U] and later the output image reuse it.
    static constexpr int oPHF = 0;                            // NFP x RBS  phi at face points
    static constexpr int oDN = (oPHF + NFP * RBS + 1) & ~1;   // NFP x NRP  (w_q/2) (grad phi . edge normal)
    static constexpr int endQ = oDN + NFP * NRP;
    static constexpr int oZ = 0;                              // ZS x MS    (written from S5 on)
    static constexpr int oOUT = 0;                            // MS x MS    (written in S8, after the last read of Z)
    // condensed mode: image of the symmetric matrix [lc f_T; f_T^T 0], MS + 1 rows, row-major == column-major; stride
    // LDI even (16-byte rows) with LDI / 2 odd (the row-per-lane reads touch every bank once).  It lies over region Q
    // only, which is sized for it: region P keeps its place behind it and takes the next cell's record as soon as S6 is
    // done, as in the other modes.  The packed result (upper triangle of S, then g) is staged on the rows of the cell block once they are dead, or
    // behind the image where that block is too small (cbs <= 3).
    static constexpr int LDI = ((MS + 1) & ~1) % 4 == 2 ? ((MS + 1) & ~1) : ((MS + 1) & ~1) + 2;
    static constexpr int NSP = NF * (NF + 1) / 2, NCOND = NSP + NF;
    static constexpr int oSTG = CBS * LDI >= NCOND ? 0 : (MS + 1) * LDI;
    static constexpr int condNeed = (MS + 1) * LDI + (CBS * LDI >= NCOND ? 0 : NCOND);
    static constexpr int sizeQ = imax(imax(imax(endQ, ZS * MS), MS * MS), COND ? ((condNeed + 1) & ~1) : 0);
    // region P: the cell's record, live until S6 is done.  With DPPFWD the record as it comes (packed L, reciprocals,
    // scalars, moments), 16-byte pairs in place.  Otherwise the image of L (NR x LD, row-major, true diagonal; the upper
    // triangle is zeroed once per kernel and never written again) and the tail of the record as it comes (reciprocals,
    // scalars), shifted so that the scalars start on a 16-byte boundary.
    static constexpr int oREC = (sizeQ + 1) & ~1;
    static constexpr int NLR = cdiv(Pre::NL + (RBS - 1), 16);   // registers of the packed factor + reciprocals
    static constexpr int oLG = (sizeQ + 1) & ~1;
    static constexpr int oLIN = ((oLG + NR * LD + 1) & ~1) + ((Pre::oSCAL - Pre::NL) & 1);
    static constexpr int oRCP = DPPFWD ? oREC + Pre::NL : oLIN;      // NR: 1 / L[i][i]
    static constexpr int oSU = DPPFWD ? oREC + Pre::oSCAL : oLIN + (Pre::oSCAL - Pre::NL);
    static constexpr int oMG = oSU + 18;                      // NMG moments
    static constexpr int oDUMMY = oSU + Pre::NSCAL;           // 4: sink of masked-out stores
    // dense fancy form: mass rows, image of chol(M1) (row-major, stride LDM), its reciprocals, trace table
    static constexpr int LDM = (CBS + 1) & ~1;
    static constexpr int oMRl = (oDUMMY + 4 + 1) & ~1;
    static constexpr int oMCl = (oMRl + Pre::NMR + 1) & ~1;
    static constexpr int oMCRl = oMCl + CBS * LDM;
    static constexpr int oFT = (oMCRl + CBS + 1) & ~1;        // NF x RBS trace / (|F|/2)
    static constexpr int LDS_PER_CELL = GENERAL_FANCY ? ((oFT + NF * RBS + 1) & ~1) : ((oDUMMY + 4 + 1) & ~1);
    static constexpr int LDS_DOUBLES = CPW * LDS_PER_CELL;
};

struct LocalOpsArgs {
    const QuadTables *tab;     // device copy of the quadrature tables
    const double *points;      // np x 2
    const uint32_t *ptids;     // nc x 4
    size_t first, n;
    const double *pre;         // records of Cfg::Pre::NPRE doubles (hho_pre.hpp) in tiles of 8 cells
    double *pre_ring;          // always null, never read: the slot keeps the kernel-argument layout -- without it 248 of the 530
                               // kernels compile to other code (profiles/operator_switches_isa.txt)
    double *oper, *data, *stab, *lc;
    int32_t *info;
    // condensed mode (MODE_COND): f_T per cell (n x cbs, may be null = 0) in; per cell the packed upper triangle of the
    // Schur complement S = A_FF - A_FT A_TT^-1 A_TF (column-packed: S(i,j), i <= j, at j(j+1)/2 + i) followed by
    // g = -A_FT A_TT^-1 f_T, NCOND = nf(nf+1)/2 + nf doubles, out.  With uF (n x nf) the same pass recovers the cell
    // unknowns instead: uT = A_TT^-1 (f_T - A_TF uF) (n x cbs).
    const double *rhs;
    double *cond;
    const double *uF;
    double *uT;
    // Stage mask, 0 in production.  Profiling (PA_ABLATE): bit i skips stage i and the results are garbage.
    // It is ALSO load-bearing: the stages sit in branches on this runtime value, which the compiler cannot
    // prove taken, so it does not hoist their per-lane, cell-invariant subexpressions out of the cell loop.
    // With the branches compiled out the k = 2 kernel spills 26 more VGPRs and runs 7 % slower (measured).
    uint32_t ablate;
    long long *dbg;            // -DPA_STAGE_CLOCK builds only
    // assembling mode (MODE_ASM): where the image goes in the CSR arrays of the assembler's own system (hho_asm_scatter.hpp);
    // reads rhs as the condensed mode does, and writes lc as well when it is not null
    AsmScatterArgs scatter;
};

// index of the monomial bx^p by^r in the graded ordering (total degree, then r)  bases.hpp:114-128
__device__ __forceinline__ int mono_index(int p, int r) { const int k = p + r; return k * (k + 1) / 2 + r; }
// exponents (p, r) of monomial m
__device__ __forceinline__ void mono_exps(int m, int &p, int &r)
{
    int k = 0;
    while ((k + 1) * (k + 2) / 2 <= m) ++k;
    r = m - k * (k + 1) / 2;
    p = k - r;
}

// 1/sqrt(x), 1/x, sqrt(x) for x > 0: hardware seed (~2^-26) + two Newton steps, <= 1 ulp
template <int ITERS = 2>
__device__ __forceinline__ double fast_rsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const double t = x * y;
        const double e = __builtin_fma(-t, y, 1.0);
        y = __builtin_fma(0.5 * y, e, y);
    }
    return y;
}
__device__ __forceinline__ double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = __builtin_fma(-x, y, 1.0);
        y = __builtin_fma(y, e, y);
    }
    return y;
}
__device__ __forceinline__ double fast_sqrt(double x)
{
    const double y = fast_rsqrt<2>(x);
    const double s = x * y;
    const double r = __builtin_fma(-s, s, x);
    return __builtin_fma(0.5 * y, r, s);
}

// Synchronisation of the ONE wavefront of a block on its LDS data.  LDS instructions of a wavefront execute in
// order, so a later read by any lane sees an earlier write by any other: what is needed is that the compiler
// keeps the order, not s_barrier -- and not what __syncthreads() adds to it, a wait for every outstanding global
// store (vmcnt(0)): with it each cell ended with the wavefront idle until HBM had acknowledged its local matrix.
__device__ __forceinline__ void wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// 16-byte LDS read of two consecutive doubles (p is 16-byte aligned by construction of the LDS map)
__device__ __forceinline__ double2 lds_pair(const double *p) { return *reinterpret_cast<const double2 *>(p); }

// s - sum_{k<N} p[k] x[k] with p a contiguous, 16-byte aligned LDS vector
template <int N>
__device__ __forceinline__ double lds_dotsub(double s, const double *p, const double *x)
{
#pragma unroll
    for (int k = 0; k + 1 < N; k += 2) {
        const double2 v = lds_pair(p + k);
        s = __builtin_fma(-v.x, x[k], s);
        s = __builtin_fma(-v.y, x[k + 1], s);
    }
    if (N & 1) s = __builtin_fma(-p[N - 1], x[N - 1], s);
    return s;
}
// same with a count that is a constant after unrolling
__device__ __forceinline__ double lds_dotsub_n(double s, const double *p, const double *x, int n)
{
#pragma unroll
    for (int k = 0; k + 1 < n; k += 2) {
        const double2 v = lds_pair(p + k);
        s = __builtin_fma(-v.x, x[k], s);
        s = __builtin_fma(-v.y, x[k + 1], s);
    }
    if (n & 1) s = __builtin_fma(-p[n - 1], x[n - 1], s);
    return s;
}
template <int N>
__device__ __forceinline__ double lds_dotadd(double s, const double *p, const double *x)
{
#pragma unroll
    for (int k = 0; k + 1 < N; k += 2) {
        const double2 v = lds_pair(p + k);
        s = __builtin_fma(v.x, x[k], s);
        s = __builtin_fma(v.y, x[k + 1], s);
    }
    if (N & 1) s = __builtin_fma(p[N - 1], x[N - 1], s);
    return s;
}

// value of lane j of every G-lane group, broadcast to the lanes of that group.  j is a constant after
// unrolling: v_readlane_b32 (scalar result, no LDS round trip like ds_bpermute) + a select per group.
template <int G>
__device__ __forceinline__ double group_broadcast(double v, int j)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int rlo = __builtin_amdgcn_readlane(lo, j), rhi = __builtin_amdgcn_readlane(hi, j);
    if (G < 64) {
        const int grp = (int)(threadIdx.x & 63) / G;
#pragma unroll
        for (int g = 1; g < 64 / G; ++g) {
            const int slo = __builtin_amdgcn_readlane(lo, g * G + j), shi = __builtin_amdgcn_readlane(hi, g * G + j);
            rlo = grp == g ? slo : rlo;
            rhi = grp == g ? shi : rhi;
        }
    }
    return __hiloint2double(rhi, rlo);
}

// -------------------------------------------------------------------------------------
// Cholesky of an N x N SPD matrix in LDS, one lane per row.  The matrix is symmetric and is
// overwritten ROW-major: L[i][k] lands at A[i * LD + k] (rows contiguous and 16-byte aligned,
// so every later use of a row is a run of ds_read_b128); the diagonal receives 1/L[j][j].
// Returns 0 or 1+index of the first non-positive pivot (uniform over the G-lane group).
// -------------------------------------------------------------------------------------
template <int N, int LD, int G, int RSQ_ITERS = 1>
__device__ __forceinline__ int lds_cholesky(double *A, int l)
{
    double row[N];
    const bool act = l < N;
    const int i = act ? l : 0;
#pragma unroll
    for (int k = 0; k + 1 < N; k += 2) {
        const double2 v = lds_pair(A + i * LD + k);
        row[k] = v.x; row[k + 1] = v.y;
    }
    if (N & 1) row[N - 1] = A[i * LD + N - 1];
    int bad = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        // A[i][j] - sum_{k<j} L[i][k] L[j][k]; row j's prefix is already in LDS
        const double s = j == 0 ? row[0] : lds_dotsub_n(row[j], A + j * LD, row, j);
        const double d = group_broadcast<G>(s, j);
        if (!(d > 0.0) && !bad) bad = j + 1;
        const double r = fast_rsqrt<RSQ_ITERS>(d);   // seed 2^-26 -> ~3e-16 after one Newton step
        row[j] = s * r;
        if (act && l >= j) A[i * LD + j] = (l == j) ? r : row[j];
        wave_sync();
    }
    return bad;
}

// x <- L^-1 x (forward) and x <- L^-T x (backward); L as left by lds_cholesky (row-major).
template <int N, int LD>
__device__ __forceinline__ void lds_forward(const double *L, double (&x)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = i == 0 ? x[0] : lds_dotsub_n(x[i], L + i * LD, x, i);
        x[i] = s * L[i * LD + i];
    }
}
template <int N, int LD>
__device__ __forceinline__ void lds_backward(const double *L, double (&x)[N])
{
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= L[k * LD + i] * x[k];
        x[i] = s * L[i * LD + i];
    }
}

// the same with the TRUE diagonal in L and the reciprocals in rd (the image the pre-pass delivers)
template <int N, int LD>
__device__ __forceinline__ void lds_forward_rd(const double *L, const double *rd, double (&x)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = i == 0 ? x[0] : lds_dotsub_n(x[i], L + i * LD, x, i);
        x[i] = s * rd[i];
    }
}
// The same in batches of rows: the prefixes (and reciprocals) of a batch's rows are read together, one LDS round trip per
// batch instead of one per row -- with a read next to each use the compiler recycles one register quad and every row waits
// for its own reads.  CAP = doubles of L per batch (registers: 2 CAP).
__host__ __device__ constexpr int fwd_batch_end(int b0, int n, int cap)
{
    int used = 0, r = b0;
    while (r < n && (r == b0 || used + 2 * ((r + 1) / 2) <= cap)) { used += 2 * ((r + 1) / 2); ++r; }
    return r;
}
template <int N, int LD, int CAP, int B0 = 0>
__device__ __forceinline__ void lds_forward_rd_batched(const double *L, const double *rd, double (&x)[N])
{
    typedef double v2d_ __attribute__((ext_vector_type(2)));
    constexpr int B1 = fwd_batch_end(B0, N, CAP), NB = B1 - B0, MP = (B1 + 1) / 2;
    v2d_ lr[NB][MP > 0 ? MP : 1];
    double rv[NB];
#pragma unroll
    for (int r = B0; r < B1; ++r) {
#pragma unroll
        for (int k = 0; k < r; k += 2) lr[r - B0][k / 2] = *reinterpret_cast<const v2d_ *>(L + r * LD + k);   // (k = r - 1: the pair ends on the diagonal)
        rv[r - B0] = rd[r];
    }
    // column by column: the updates of a column are independent of each other (written row by row the FMAs of a row are one
    // dependent chain after the other); every row still sums in ascending k, so the results are those of the row form
#pragma unroll
    for (int k = 0; k < B1; ++k) {
        if (k >= B0) x[k] *= rv[k - B0];
#pragma unroll
        for (int r = (k + 1 > B0 ? k + 1 : B0); r < B1; ++r)
            x[r] = __builtin_fma(-((k & 1) ? lr[r - B0][k / 2].y : lr[r - B0][k / 2].x), x[k], x[r]);
    }
    if constexpr (B1 < N) lds_forward_rd_batched<N, LD, CAP, B1>(L, rd, x);
}
// ---- the same substitutions with the packed factor in registers (Cfg::DPPFWD): element e of [packed L | 1 / diagonal] is
// held by lane e mod 16 of each row of 16 lanes in lr[e / 16]; an FMA takes it through its DPP operand (row_newbcast).
// The DPP source registers are written by LDS loads only: the 2 wait states a VALU write would need before a DPP read of
// the same register never arise (tools/spills.py checks the ISA for it).
template <int E>
__device__ __forceinline__ void dpp_fnma(double &acc, double lv, double x)     // acc -= bcast(lv, E) * x
{
    asm("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(lv), "v"(x), "n"(E));
}
template <int E>
__device__ __forceinline__ double dpp_bcast(double lv)                        // bcast(lv, E)
{
    double r;
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(lv), "n"(E));
    return r;
}
template <int NLR, int E>
__device__ __forceinline__ void dpp_fnma_e(double &acc, const double (&lr)[NLR], double x) { dpp_fnma<E % 16>(acc, lr[E / 16], x); }
template <int NLR, int E>
__device__ __forceinline__ double dpp_bcast_e(const double (&lr)[NLR]) { return dpp_bcast<E % 16>(lr[E / 16]); }

// x = L^-1 x, column by column (the updates of a column are independent FMAs; every row sums in ascending k)
template <int N, int NLR, int K, int R>
__device__ __forceinline__ void dpp_forward_col(const double (&lr)[NLR], double (&x)[N])
{
    if constexpr (R < N) {
        dpp_fnma_e<NLR, R * (R + 1) / 2 + K>(x[R], lr, x[K]);
        dpp_forward_col<N, NLR, K, R + 1>(lr, x);
    }
}
template <int N, int NLR, int K = 0>
__device__ __forceinline__ void dpp_forward(const double (&lr)[NLR], double (&x)[N])
{
    constexpr int NL = N * (N + 1) / 2;
    x[K] *= dpp_bcast_e<NLR, NL + K>(lr);
    dpp_forward_col<N, NLR, K, K + 1>(lr, x);
    if constexpr (K + 1 < N) dpp_forward<N, NLR, K + 1>(lr, x);
}
// x = L^-T x: x[K] = (x[K] - sum_{k > K} L[k][K] x[k]) / L[K][K], K descending; column K of L^T is row K of L
template <int N, int NLR, int K, int I>
__device__ __forceinline__ void dpp_backward_row(const double (&lr)[NLR], double (&x)[N])
{
    if constexpr (I < K) {
        dpp_fnma_e<NLR, K * (K + 1) / 2 + I>(x[I], lr, x[K]);
        dpp_backward_row<N, NLR, K, I + 1>(lr, x);
    }
}
template <int N, int NLR, int K = N - 1>
__device__ __forceinline__ void dpp_backward(const double (&lr)[NLR], double (&x)[N])
{
    constexpr int NL = N * (N + 1) / 2;
    x[K] *= dpp_bcast_e<NLR, NL + K>(lr);
    dpp_backward_row<N, NLR, K, 0>(lr, x);
    if constexpr (K > 0) dpp_backward<N, NLR, K - 1>(lr, x);
}

// ---- condensed mode: the first NPV steps of the row-by-row Cholesky factorization of the image with the rows in registers
// (hho_local_ops_kernel, S9).  Step J: s = M[i][J] - sum_{k<J} L[i][k] L[J][k] with L[J][k] = register rA[k] of lane J of the
// row of 16 lanes (DPP), d = s of lane J, L[i][J] = s / sqrt(d).  rA[J - 1] and s were just written by the vector ALU: the
// s_nop ties give their DPP reads the two wait states they need.
template <int NPV, bool TWO, int J, int K>
__device__ __forceinline__ void cond_dpp_dot(double (&sA)[2], double (&sB)[2], const double (&rA)[NPV], const double (&rB)[TWO ? NPV : 1])
{
    if constexpr (K < J) {                                 // (two partial sums per row: the FMAs of a sum are a dependent chain)
        dpp_fnma<J>(sA[K & 1], rA[K], rA[K]);
        if (TWO) dpp_fnma<J>(sB[K & 1], rA[K], rB[K]);
        cond_dpp_dot<NPV, TWO, J, K + 1>(sA, sB, rA, rB);
    }
}
template <int NPV, bool TWO, int J = 0>
__device__ __forceinline__ void cond_dpp_chain(double (&rA)[NPV], double (&rB)[TWO ? NPV : 1], double &rdiag, int &bad, int q)
{
    double pA[2] = {rA[J], 0.0}, pB[2] = {TWO ? rB[J] : 0.0, 0.0};
    if (J > 0) asm volatile("s_nop 1" : "+v"(rA[J > 0 ? J - 1 : 0]));
    cond_dpp_dot<NPV, TWO, J, 0>(pA, pB, rA, rB);
    double sA = J > 1 ? pA[0] + pA[1] : pA[0];
    const double sB = J > 1 ? pB[0] + pB[1] : pB[0];
    asm volatile("s_nop 1" : "+v"(sA));
    const double d = dpp_bcast<J>(sA);
    if (!(d > 0.0) && !bad) bad = J + 1;
    const double r = fast_rsqrt<1>(d);
    rA[J] = sA * r;
    if (TWO) rB[J] = sB * r;
    if (q == J) rdiag = r;
    if constexpr (J + 1 < NPV) cond_dpp_chain<NPV, TWO, J + 1>(rA, rB, rdiag, bad, q);
}

// The same chain RIGHT-looking: once column J is final (s / sqrt(d)), every later column takes its term at once,
//   M[i][K] -= L[i][J] L[K][J],  K = J+1 .. NPV-1   (L[K][J] = register rA[J] of lane K of the row of 16: DPP),
// independent FMAs, so that a step's dependent path is pivot broadcast -> rsqrt -> scale -> ONE FMA into the next pivot
// column, where the left-looking form has the J-term dot product in front of the rsqrt.  Each entry still receives its
// terms in ascending J (the order of the row-by-row LLT).
template <int NPV, bool TWO, int J, int K>
__device__ __forceinline__ void cond_dpp_update(double (&rA)[NPV], double (&rB)[TWO ? NPV : 1])
{
    if constexpr (K < NPV) {
        dpp_fnma<K>(rA[K], rA[J], rA[J]);
        if (TWO) dpp_fnma<K>(rB[K], rA[J], rB[J]);
        cond_dpp_update<NPV, TWO, J, K + 1>(rA, rB);
    }
}
template <int NPV, bool TWO, int J = 0>
__device__ __forceinline__ void cond_dpp_chain_rl(double (&rA)[NPV], double (&rB)[TWO ? NPV : 1], double &rdiag, int &bad, int q)
{
    double sA = rA[J];
    asm volatile("s_nop 1" : "+v"(sA));                    // (written by the previous step's FMA: wait states of its DPP read)
    const double d = dpp_bcast<J>(sA);
    if (!(d > 0.0) && !bad) bad = J + 1;
    const double r = fast_rsqrt<1>(d);
    rA[J] = sA * r;
    if (TWO) rB[J] = rB[J] * r;
    if (q == J) rdiag = r;
    if constexpr (J + 1 < NPV) {
        asm volatile("s_nop 1" : "+v"(rA[J]));
        cond_dpp_update<NPV, TWO, J, J + 1>(rA, rB);
        cond_dpp_chain_rl<NPV, TWO, J + 1>(rA, rB, rdiag, bad, q);
    }
}

template <int N, int LD>
__device__ __forceinline__ void lds_backward_rd(const double *L, const double *rd, double (&x)[N])
{
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= L[k * LD + i] * x[k];
        x[i] = s * rd[i];
    }
}

// forward / backward substitution with the constant face factor L^ (uniform table reads)
template <int FBS>
__device__ __forceinline__ void face_forward(const FaceTables &ft, double (&x)[FBS])
{
#pragma unroll
    for (int i = 0; i < FBS; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= ft.lf[i][k] * x[k];
        x[i] = s * ft.lf[i][i];
    }
}

// force a wave-uniform double into scalar registers
__device__ __forceinline__ double to_sgpr(double v)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// -------------------------------------------------------------------------------------
// The kernel.  One wavefront per block; G lanes per cell; persistent over cells.
// -------------------------------------------------------------------------------------
// MODE_LC:    only lc = data + stab is produced (one accumulator per entry);
// MODE_SPLIT: data and stab are kept apart so that any of lc / data / stab can be written
//             (two accumulator sets and the columns of Y and U in registers: at most 3 waves/SIMD);
// MODE_COND:  lc never leaves the chip: the product lands in an LDS image and the cell unknowns are eliminated there
//             (partial Cholesky of [lc f_T; f_T^T 0] over the cbs cell pivots); the packed Schur complement and the
//             condensed right-hand side are the only output -- or, given the face unknowns, the recovered cell unknowns.
// MODE_ASM:   the condensed mode's pass up to the completed image; instead of the elimination a scatter epilogue writes the
//             image's entries to their places in the CSR values and right-hand side of the assembler's own system
//             (hho_asm_scatter.hpp), and lc itself only when asked for.
enum { MODE_LC = 0, MODE_SPLIT = 1, MODE_COND = 2, MODE_ASM = 3 };
template <class C, int MODE>
__global__ __launch_bounds__(64, (MODE == MODE_SPLIT && C::WAVES > 3) ? 3 : C::WAVES) void hho_local_ops_kernel(LocalOpsArgs a)
{
    constexpr bool SPLIT = MODE == MODE_SPLIT, ASM = MODE == MODE_ASM, COND = MODE == MODE_COND || ASM;
    static_assert(COND == C::COND, "the condensed mode runs on the Cfg instance that reserves its LDS image");
    static_assert(!COND || (C::CBS + C::NF + 1 <= C::G && C::HAS_STAB), "condensed mode: one lane per row of [lc f_T; f_T^T 0]");
    constexpr int G = C::G, RBS = C::RBS, CBS = C::CBS, FBS = C::FBS, MS = C::MS, NR = C::NR, NF = C::NF;
    constexpr int NFQ = C::NFQ, NFP = C::NFP, RD = C::RD;
    constexpr int ZS = C::ZS, ND = C::ND, NRP = C::NRP, LD = C::LD;
    static_assert(MS <= G, "one lane per local-matrix column");
    static_assert(RBS <= G && NF <= G, "one lane per row in the factorizations");
    static_assert(C::NQ > 0, "empty quadrature rule (the rules[8] hole)");

    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x;
    const int g = lane / G, l0 = lane % G;
    const int l = l0;
    double *S = smem + g * C::LDS_PER_CELL;
    const QuadTables *__restrict__ tab = a.tab;
    typedef typename C::Pre PRE;
    // Blocks b and b + 8 share an XCD (round-robin dispatch; a speed assumption only): give the blocks of an XCD
    // consecutive cells, so that the 8 cells of a record tile, and the lines of lc they share, meet in one L2.
    const size_t lblock = gridDim.x % 8 == 0 ? (size_t)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8 : (size_t)blockIdx.x;
    const size_t stride = (size_t)gridDim.x * C::CPW;
#ifdef PA_STAGE_CLOCK
    long long tk_sum[PA_NSTAGE] = {0}, tk_last = clock64();
#endif
    // constant face tables, kept in scalar registers
    FaceTables ft;
#pragma unroll
    for (int q = 0; q < NFQ; ++q)
#pragma unroll
        for (int k = 0; k < FBS; ++k) ft.cw[q][k] = to_sgpr(tab->face[C::FD].cw[q][k]);
#pragma unroll
    for (int i = 0; i < FBS; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) ft.lf[i][k] = to_sgpr(tab->face[C::FD].lf[i][k]);

    // S1: TWO lanes per face point where the group has them -- one forms its row of scaled monomials, the other its row of
    // weighted normal derivatives -- and ONE common run of LDS stores (a store instruction costs its 6 ... 13 cycles of the
    // store path whatever the number of active lanes: 5 instead of 10 of them per pass at k = 2)
    constexpr bool S1_SPLIT = 2 * NFP <= G && C::PPL == 1;
    // ---- per-lane, cell-invariant bookkeeping -------------------------------------------
    // reference coordinate and half weight of the face points this lane evaluates
    double r0[C::PPL], rw[C::PPL];
#pragma unroll
    for (int r = 0; r < C::PPL; ++r) {
        const int p = l + r * G;
        r0[r] = rw[r] = 0.0;
        if (p < NFP || (S1_SPLIT && p < 2 * NFP)) {
            const int q = (S1_SPLIT && p >= NFP ? p - NFP : p) % NFQ;
            r0[r] = tab->gauss_x[NFQ][q];
            rw[r] = 0.5 * tab->gauss_w[NFQ][q];
        }
    }
    // column role of this lane: cell column (c < CBS) or column kf of face fc
    const bool is_col = l < MS, is_cellcol = l < CBS;
    const int c0 = is_col ? l : 0;
    const int fc = is_cellcol ? 0 : (c0 - CBS) / FBS, kf = is_cellcol ? 0 : (c0 - CBS) % FBS;
    // t_q^kf ; column kf of L^^T.  Per lane and cell-invariant: 2 (NFQ + FBS) registers for the whole kernel
    double fbq[NFQ], ufc[FBS];
#pragma unroll
    for (int q = 0; q < NFQ; ++q) fbq[q] = tab->face[C::FD].fb[q][kf];
#pragma unroll
    for (int j = 0; j < FBS; ++j) ufc[j] = tab->face[C::FD].lft[j][kf];

    // Corner tile of Z^T Z on the vector pipe (msize 17..24): with T_F = [trace_F | 0] its columns are face columns, whose
    // U parts are -sqrt(|F|/2h) L^^T e_k on the rows of their own face: the U term of an entry is su_F^2 (L^^ L^^T)[ki][kj]
    // for two columns of one face and nothing otherwise -- a constant per lane; only the Y rows are read from LDS.
    constexpr bool CORNER_SHORT = C::CORNER_VALU && C::HAS_STAB && !C::GENERAL_FANCY && !SPLIT && CBS <= 16;
    double cornerT = 0.0;
    if (CORNER_SHORT && l < C::NCORNER * (C::NCORNER + 1) / 2) {
        int cj_ = 0;
        while ((cj_ + 1) * (cj_ + 2) / 2 <= l) ++cj_;
        const int ci_ = l - cj_ * (cj_ + 1) / 2;
        const int fi_ = (16 + ci_ - CBS) / FBS, ki_ = (16 + ci_ - CBS) % FBS, fj_ = (16 + cj_ - CBS) / FBS, kj_ = (16 + cj_ - CBS) % FBS;
        if (fi_ == fj_) {
#pragma unroll
            for (int j = 0; j < FBS; ++j) cornerT += tab->face[C::FD].lft[j][ki_] * tab->face[C::FD].lft[j][kj_];
        }
    }

    // Per-lane index constants of the unit form of U (S4b / S6) and of the corner tile, PACKED one word each: kept across
    // the cell loop in one register and unpacked per pass (a field extract each) -- recomputed from the opaque lane index
    // they cost ten to seventeen integer instructions per use and pass, held unpacked a register each for the whole kernel.
    //   unit word:   bits 0-11 offset of the unit's first phi value in the face-point table (doubles from oPHF),
    //                bits 12-23 offset of its first U entry in Z (doubles from S; the sink for lanes without a unit), bits 24-25 face
    //   corner word: bits 0-7 ci, 8-15 cj (ci <= cj: the pair of corner columns of this lane), 16-17 face of column ci
    constexpr bool UNIT_U = C::HAS_STAB && !C::GENERAL_FANCY && !SPLIT;
    constexpr bool UPERM_ON = C::UPERM && UNIT_U;
    constexpr int NU = 4 * CBS, UR = UNIT_U ? cdiv(NU, G) : 1;
    uint32_t unit_pk[UR];
#pragma unroll
    for (int r = 0; r < UR; ++r) {
        const int u = l0 + r * G;
        const bool on = u < NU;
        const int uu = on ? u : 0;
        const int f = uu / CBS, cc = uu - f * CBS;
        const int ur = (UPERM_ON ? ((f + 4 - C::UF1) & 3) : f) * FBS;           // row block of face f (see Cfg::UPERM)
        const int zoff = on ? C::oZ + NRP + ur + cc * ZS : C::oDUMMY;            // (the sink holds 4 doubles)
        static_assert(!UNIT_U || (NFP * RBS < 4096 && C::oDUMMY < 4096 && ZS * MS < 4096), "packed unit offsets: 12 bits each");
        unit_pk[r] = (uint32_t)(f * NFQ * RBS + cc) | ((uint32_t)zoff << 12) | ((uint32_t)f << 24);
    }
    uint32_t corner_pk = 0;
    if (C::CORNER_VALU) {
        int cj_ = 0;
#pragma unroll
        for (int j = 1; j < C::NCORNER; ++j) cj_ += l0 >= j * (j + 1) / 2 ? 1 : 0;
        const int ci_ = l0 - cj_ * (cj_ + 1) / 2;                                // ci_ <= cj_
        const int cf_ = (l0 < C::NCORNER * (C::NCORNER + 1) / 2) ? (16 + ci_ - CBS) / FBS : 0;
        corner_pk = (uint32_t)(ci_ & 0xff) | ((uint32_t)cj_ << 8) | ((uint32_t)(cf_ & 3) << 16);
    }

    // Tile (1,1) of Z^T Z where it runs on the matrix pipe (msize 25..32, no vector-pipe corner) with T_F = [trace_F | 0]: its columns
    // are face columns, whose U parts are -sqrt(|F|/2h) L^^T e_k on the rows of their own face, so the U term of an entry is
    // su_F^2 (L^^ L^^T)[ki][kj] for two columns of one face and nothing otherwise: a constant per accumulator times the face's
    // scale, added after the products -- which then stop after the rows of Y (k = 3: 4 of 8 k-steps, 20 instead of 24 matrix
    // instructions per cell).
    constexpr int NTL_ = (MS + 15) / 16;
    constexpr bool T11_SHORT = UNIT_U && NTL_ == 2 && !C::CORNER_VALU && CBS <= 16;
    constexpr bool ACC_PERM_ = !C::DIRECT_STORE && !COND && MS % 2 == 0;
    double t11c[4] = {0.0, 0.0, 0.0, 0.0};
    int t11f = 0;
    if (T11_SHORT) {
        const int kk_ = lane >> 4, jj_ = lane & 15;
        const int col = 16 + (ACC_PERM_ ? 4 * (jj_ & 3) + (jj_ >> 2) : jj_);
        if (col < MS) {
            t11f = (col - CBS) / FBS;
            const int kc = (col - CBS) % FBS;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 + (ACC_PERM_ ? 4 * kk_ + r : kk_ + 4 * r);
                if (row < MS && (row - CBS) / FBS == t11f) {
                    const int kr = (row - CBS) % FBS;
#pragma unroll
                    for (int j = 0; j < FBS; ++j) t11c[r] += tab->face[C::FD].lft[j][kr] * tab->face[C::FD].lft[j][kc];
                }
            }
        }
    }

    // pairs of the cell's pre-pass record this lane moves to LDS, and where their two doubles go
    int pre_dst[C::PLC][2];
#pragma unroll
    for (int t = 0; t < C::PLC; ++t) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = 2 * (l + t * G) + h;
            int dst = C::oDUMMY + h;
            if (C::DPPFWD) {
                if (e < PRE::NPRE) dst = C::oREC + e;            // the record as it comes
            } else if (e < PRE::NL) {
                int i = 0;
                while ((i + 1) * (i + 2) / 2 <= e) ++i;
                dst = C::oLG + i * LD + (e - i * (i + 1) / 2);
            } else if (e < PRE::oMR) {
                dst = C::oLIN + (e - PRE::NL);
            } else if (e < PRE::oMC) {
                dst = C::oMRl + (e - PRE::oMR);
            } else if (e < PRE::oMCR) {
                int i = 0;
                while ((i + 1) * (i + 2) / 2 <= e - PRE::oMC) ++i;
                dst = C::oMCl + i * C::LDM + (e - PRE::oMC - i * (i + 1) / 2);
            } else if (e < PRE::oMCR + (C::GENERAL_FANCY ? CBS : 0)) {
                dst = C::oMCRl + (e - PRE::oMCR);
            }
            pre_dst[t][h] = dst;
        }
    }

    // The record of a cell is fetched one cell ahead: the loads are issued at the top of a cell's pass, land in
    // registers while S1-S6 run, and go to region P when S6 is done with it -- before the stores of S8 are
    // issued, so that no load ever queues behind them (vector memory operations complete in order).
    double2 rec[C::PLC];
    auto rec_issue = [&](size_t b) {
        // records lie in tiles of 8 cells, [tile][pair][cell % 8] (hho_pre.hpp): the pairs of one record are 128 bytes apart
        // (b is a multiple of the CPW cells of a wavefront, CPW divides 8: the wavefront's cells share a tile, whose address is
        // wave-uniform -- scalar arithmetic; a lane adds its slot.  Past the end the lanes read records of the first tile, or
        // the unwritten slots of the last one -- the buffer holds whole tiles --, and nothing they compute is stored.)
        static_assert(8 % C::CPW == 0, "the cells of a wavefront share a record tile");
        const size_t bu = b < a.n ? b : 0;
        const double *pc = a.pre + (bu >> 3) * (size_t)(PRE::NP2 * 16) + (((uint32_t)bu & 7u) + (uint32_t)g) * 2u;
#pragma unroll
        for (int t = 0; t < C::PLC; ++t) {
            const int e2 = l0 + t * G;
            rec[t] = *reinterpret_cast<const double2 *>(pc + 16 * (e2 < PRE::NP2 ? e2 : 0));
        }
    };
    auto rec_deposit = [&]() {
#pragma unroll
        for (int t = 0; t < C::PLC; ++t) {
            if (C::DPPFWD) {
                typedef double v2d_ __attribute__((ext_vector_type(2)));
                *reinterpret_cast<v2d_ *>(S + pre_dst[t][0]) = v2d_{rec[t].x, rec[t].y};      // (16-byte aligned: oREC, oDUMMY and 2 e are even)
            } else {
                S[pre_dst[t][0]] = rec[t].x;
                S[pre_dst[t][1]] = rec[t].y;
            }
        }
    };
    if (!C::DPPFWD) {
        for (int e = l; e < NR * LD; e += G) S[C::oLG + e] = 0.0;
        wave_sync();
    }
    rec_issue(lblock * C::CPW);
    rec_deposit();
    wave_sync();

    for (size_t base = lblock * C::CPW; base < a.n; base += stride) {
        // Re-derive the lane index opaquely per cell: otherwise LICM hoists the index computations
        // of every stage out of the cell loop and the kernel spills.
        int l = l0;
        asm volatile("" : "+v"(l));
        __builtin_amdgcn_s_setprio(PRIO_HEAD);
        l &= G - 1;      // tell the compiler the range again: its index products fit 24 bits (v_mul_u32_u24 / v_mad_u32_u24 are full rate)
        const bool valid = base + g < a.n;
        const size_t cell = a.first + (valid ? base + g : a.n - 1);
        // offset of the lane's cell in an output / input array of X doubles per cell: the block's part is wave-uniform (scalar
        // arithmetic), the lane adds its group's (lanes past the end: the first cell of the pass, which exists)
        const uint32_t gl = valid ? (uint32_t)g : 0u;
        auto rel = [&](uint32_t X) -> size_t { return base * (size_t)X + (size_t)(gl * X); };

        // ================= S0: the cell's scalars ======================================
        // The per-cell head comes from the pre-pass; its record is in region P already (fetched a pass ahead).
        PA_MARK("S0");
        rec_issue(base + stride);
        const double2 bb = lds_pair(S + C::oSU + 4), ihb = lds_pair(S + C::oSU + 6);
        const double barx = bb.x, bary = bb.y, ih = ihb.x;
        const int bad_pre = (int)ihb.y;

        PA_TICK(0);
        // ================= S1: evaluation points ======================================
        PA_MARK("S1");
        if (S1_SPLIT) {
            // face points only (the cell points belong to the pre-pass): lane p < NFP forms phi at point p, lane NFP + p the
            // weighted normal derivatives there; both rows leave through the same store instructions
            if (!(a.ablate & 1u) && l < 2 * NFP) {
                const bool dnrow = l >= NFP;
                const int pf = dnrow ? l - NFP : l;
                const int f = pf / NFQ;
                const double *sc = S + C::oSU;
                const double2 pa_ = lds_pair(sc + 8 + 2 * f), pb_ = lds_pair(sc + 8 + 2 * ((f + 1) & 3));
                const bool descending = (((int)sc[16]) >> f) & 1;                  // the face's first vertex has the higher point id
                const double wnx = rw[0] * (pb_.y - pa_.y), wny = -rw[0] * (pb_.x - pa_.x);      // (w_q |F|/2) n: the edge length cancels
                const double t = descending ? -r0[0] : r0[0];                      // bases.hpp:260-261
                // the point of quadratures.hpp:420-428, 0.5 (1 - t) a + 0.5 (1 + t) b, taken from the endpoint a: b - a is exact for a
                // cell far from the origin and the point cannot leave an axis-parallel face by an ulp of the offset (one ulp of
                // 1000 is 2e-10 of a cell of side 1e-3 and showed as 8e-11 in the stabilization)
                const double cb = 0.5 * (1 + t);
                const double x = __builtin_fma(cb, pb_.x - pa_.x, pa_.x);
                const double y = __builtin_fma(cb, pb_.y - pa_.y, pa_.y);
                const double bx_ = (x - barx) * ih, by_ = (y - bary) * ih;
                double pwx[RD + 1], pwy[RD + 1];
                pwx[0] = 1.0; pwy[0] = 1.0;
#pragma unroll
                for (int e = 1; e <= RD; ++e) { pwx[e] = pwx[e - 1] * bx_; pwy[e] = pwy[e - 1] * by_; }
                double out[RBS];
                // (an empty volatile asm in each arm: a real branch on the execution mask -- if-converted, the arms' results meet in two
                // selects per double)
                if (!dnrow) {
                    asm volatile("");
                    int m = 0;
#pragma unroll
                    for (int kk = 0; kk <= RD; ++kk)
#pragma unroll
                        for (int ii = 0; ii <= kk; ++ii, ++m) out[m] = pwx[kk - ii] * pwy[ii];      // (px,py) = (k-i, i)  bases.hpp:119-120
                } else {
                    asm volatile("");
                    const double gnx = ih * wnx, gny = ih * wny;
                    int m = 0;
#pragma unroll
                    for (int kk = 0; kk <= RD; ++kk)
#pragma unroll
                        for (int ii = 0; ii <= kk; ++ii, ++m) {
                            const int ex_ = kk - ii, ey_ = ii;
                            if (m > 0) {
                                const double gx = ex_ == 0 ? 0.0 : (ex_ * gnx) * pwx[ex_ > 0 ? ex_ - 1 : 0] * pwy[ey_];
                                const double gy = ey_ == 0 ? 0.0 : (ey_ * gny) * pwx[ex_] * pwy[ey_ > 0 ? ey_ - 1 : 0];
                                out[m - 1] = gx + gy;
                            }
                        }
                    out[RBS - 1] = 0.0;
                }
                double *dst = S + (dnrow ? C::oDN + pf * NRP : C::oPHF + pf * RBS);
#pragma unroll
                for (int m = 0; m < RBS; ++m)
                    if (m < NR || !dnrow) dst[m] = out[m];
            }
        } else if (!(a.ablate & 1u)) {
#pragma unroll
            for (int r = 0; r < C::PPL; ++r) {
                const int p = l + r * G;
                if (p < NFP) {
                    // scaled monomials and weighted normal derivatives  bases.hpp:93-184, hho.hpp:77-83
                    const int f = p / NFQ;
                    const double *sc = S + C::oSU;
                    const double2 pa_ = lds_pair(sc + 8 + 2 * f), pb_ = lds_pair(sc + 8 + 2 * ((f + 1) & 3));
                    const double ax = pa_.x, ay = pa_.y, bx = pb_.x, by = pb_.y;
                    const bool descending = (((int)sc[16]) >> f) & 1;      // the face's first vertex has the higher point id
                    // w n = (w_q |F|/2) (e_y, -e_x)/|F|: the edge length cancels  (basic_geom.hpp:361-369,
                    // quadratures.hpp:426); rw holds w_q / 2
                    const double wnx = rw[r] * (by - ay), wny = -rw[r] * (bx - ax);
                    // the face runs from its LOWER-id endpoint (basic_geom.hpp:202-203, bases.hpp:260-261):
                    // its q-th point sits at -t_q in cell order when the ids are descending
                    const double t = descending ? -r0[r] : r0[r];
                    // quadratures.hpp:420-428 taken from the endpoint a (see the split S1 above)
                    const double cb = 0.5 * (1 + t);
                    const double x = __builtin_fma(cb, bx - ax, ax);
                    const double y = __builtin_fma(cb, by - ay, ay);
                    const double bx_ = (x - barx) * ih, by_ = (y - bary) * ih;
                    double pwx[RD + 1], pwy[RD + 1];
                    pwx[0] = 1.0; pwy[0] = 1.0;
#pragma unroll
                    for (int e = 1; e <= RD; ++e) { pwx[e] = pwx[e - 1] * bx_; pwy[e] = pwy[e - 1] * by_; }
                    const double gnx = ih * wnx, gny = ih * wny;
                    int m = 0;
#pragma unroll
                    for (int kk = 0; kk <= RD; ++kk) {
#pragma unroll
                        for (int ii = 0; ii <= kk; ++ii, ++m) {
                            const int ex_ = kk - ii, ey_ = ii;      // (px,py) = (k-i, i)  bases.hpp:119-120
                            S[C::oPHF + p * RBS + m] = pwx[ex_] * pwy[ey_];
                            if (m > 0) {
                                const double gx = ex_ == 0 ? 0.0 : (ex_ * gnx) * pwx[ex_ > 0 ? ex_ - 1 : 0] * pwy[ey_];
                                const double gy = ey_ == 0 ? 0.0 : (ey_ * gny) * pwx[ex_] * pwy[ey_ > 0 ? ey_ - 1 : 0];
                                S[C::oDN + p * NRP + (m - 1)] = gx + gy;
                            }
                        }
                    }
                }
            }
        }
        wave_sync();

        // (S2, cell moments, and S3, stiffness and mass, belong to the pre-pass: hho_pre.hpp)
        PA_MARK("S2");
        PA_MARK("S3");
        PA_TICK(1);
        // ================= S3b: column c of gr_rhs  hho.hpp:64-85 =====================
        __builtin_amdgcn_s_setprio(PRIO_S3B);
        PA_MARK("S3b");
        const int c = l < MS ? l : 0;
        double col[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) asm volatile("" : "=v"(col[i]));      // (every lane writes every row below; only a profiling build's skipped stage leaves them as they are -- a constant here cost a move per row and pass)
        if (a.ablate & 4u) {
        } else if (l < CBS) {
            // -int_T phi_c lap(phi_i) = -(2/h)^2 (a (a-1) MOM(a-2+a', b+b') + b (b-1) MOM(a+a', b-2+b')) for phi_i = bx^a by^b,
            // phi_c = bx^a' by^b'.  In the graded ordering the moment of phi_c times the monomial m of degree d sits at
            // c + d (a' + b') + m: one LDS read per monomial of degree <= recdeg - 2, the rest is in registers.
            constexpr int NDM = RD >= 2 ? P2(RD - 2) : 1;
            double mc[NDM];
            int kcv = 0;                                 // a' + b' (per cell from the opaque lane index: no register held)
#pragma unroll
            for (int k = 1; k <= C::CD; ++k) kcv += l >= k * (k + 1) / 2 ? 1 : 0;
            const double *mg = S + C::oMG + l;
            mc[0] = 0.0;
#pragma unroll
            for (int d = 0; d + 2 <= RD; ++d)
#pragma unroll
                for (int bm = 0; bm <= d; ++bm) mc[d * (d + 1) / 2 + bm] = mg[d * kcv + d * (d + 1) / 2 + bm];
            const double nih2 = -(ih * ih);
#pragma unroll
            for (int ki = 1; ki <= RD; ++ki)
#pragma unroll
                for (int ri = 0; ri <= ki; ++ri) {
                    const int ai = ki - ri, bi = ri, row = ki * (ki + 1) / 2 + ri - 1;
                    double v = 0.0;
                    if (ai >= 2) v = (double)(ai * (ai - 1)) * mc[(ki - 2) * (ki - 1) / 2 + bi];
                    if (bi >= 2) v = __builtin_fma((double)(bi * (bi - 1)), mc[(ki - 2) * (ki - 1) / 2 + bi - 2], v);
                    col[row] = nih2 * v;
                }
        }
        if (a.ablate & 4u) {
        } else if (l < CBS) {
        } else {
            // the rows of the face's table in batches of QG points (<= 32 doubles), one LDS round trip each, then the products
            typedef double v2d_ __attribute__((ext_vector_type(2)));
            constexpr int QG = imax(1, imin(NFQ, 32 / NRP));
#pragma unroll
            for (int i = 0; i < NR; ++i) col[i] = 0.0;
#pragma unroll
            for (int q0 = 0; q0 < NFQ; q0 += QG) {
                v2d_ dnv[QG][NRP / 2];
#pragma unroll
                for (int q = q0; q < q0 + QG; ++q)
#pragma unroll
                    for (int i = 0; i < NRP; i += 2)
                        if (q < NFQ) dnv[q - q0][i / 2] = *reinterpret_cast<const v2d_ *>(S + C::oDN + (fc * NFQ + q) * NRP + i);
#pragma unroll
                for (int i = 0; i < NR; ++i)
#pragma unroll
                    for (int q = q0; q < q0 + QG; ++q)
                        if (q < NFQ) col[i] = __builtin_fma((i & 1) ? dnv[q - q0][i / 2].y : dnv[q - q0][i / 2].x, fbq[q], col[i]);
            }
        }
        wave_sync();

        // ================= S4/S5: Y = L^-1 gr_rhs, L = chol(gr_lhs) from the record  hho.hpp:63,92
        PA_TICK(2);
        __builtin_amdgcn_s_setprio(PRIO_MID);
        PA_MARK("S4");
        double *LG = S + C::oLG;                 // image of L (without DPPFWD)
        double lreg[C::NLR];                     // DPPFWD: [packed L | 1 / diagonal], element e in lane e mod 16 of a row, register e / 16
        int bad = bad_pre;
        if (!(a.ablate & 16u)) {
            if (C::DPPFWD) {
#pragma unroll
                for (int t = 0; t < C::NLR; ++t) lreg[t] = S[C::oREC + (lane & 15) + 16 * t];      // (reads past NL + NR stay inside the record)
                dpp_forward<NR, C::NLR>(lreg, col);
            } else if (PA_FWD_CAP > 0) lds_forward_rd_batched<NR, LD, PA_FWD_CAP>(LG, S + C::oRCP, col);
            else lds_forward_rd<NR, LD>(LG, S + C::oRCP, col);
        }
        PA_TICK(11);
        // The trace columns are formed only now (not next to the gr_rhs columns in S3b): they stay
        // out of the register budget of the factorization.  They read the face tables of region Q,
        // which Z overwrites: Y goes to LDS after the barrier below.
        // trace columns / (|F|/2):  tr[fk] = sum_q w_q t_q^k phi_c(x_fq)   hho.hpp:209-216 / 133-140.
        // Point q of face f IS the reference's q-th face point (S1 mirrors t for faces whose lower-id
        // endpoint comes second), so its face-basis value is t_q^k for either orientation.
        // lc only, T_F = [trace_F | 0]: the cell part of U is formed by UNITS (face f, cell column cc), one lane each --
        // 4 CBS units of FBS entries (trace, L^^-1, scale) instead of every column lane carrying all NF rows of its
        // column through the same steps with CBS of G lanes useful; the face columns of U are -sqrt(|F|/2h) L^^T E_F,
        // constants times the face's scale.  Nothing of U is held in registers across the stages.
        double uval[UR][FBS];
        double uph[UR][NFQ], usu[UR];
        uint32_t upk[UR];
#pragma unroll
        for (int r = 0; r < UR; ++r) { upk[r] = unit_pk[r]; asm volatile("" : "+v"(upk[r])); }      // (unpacked per pass, not hoisted)
        if (UNIT_U && !(a.ablate & 32u)) {
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const double *ph = S + C::oPHF + (upk[r] & 0xfffu);
#pragma unroll
                for (int q = 0; q < NFQ; ++q) uph[r][q] = ph[q * RBS];
                usu[r] = S[C::oSU + (upk[r] >> 24)];
            }
            // (every read of the units first: one LDS round trip)
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                double x[FBS];
#pragma unroll
                for (int k = 0; k < FBS; ++k) x[k] = 0.0;
#pragma unroll
                for (int q = 0; q < NFQ; ++q)
#pragma unroll
                    for (int k = 0; k < FBS; ++k) x[k] += ft.cw[q][k] * uph[r][q];
                face_forward<FBS>(ft, x);
#pragma unroll
                for (int k = 0; k < FBS; ++k) uval[r][k] = usu[r] * x[k];
            }
        }
        PA_TICK(12);
        double ucol[C::HAS_STAB ? NF : 1];
#pragma unroll
        for (int r = 0; r < (C::HAS_STAB ? NF : 1); ++r) asm volatile("" : "=v"(ucol[r]));
        if (C::HAS_STAB && !UNIT_U && !(a.ablate & 32u)) {
            constexpr int TCOLS = C::GENERAL_FANCY ? RBS : CBS;
            const int m = l < TCOLS ? l : 0;
#pragma unroll
            for (int r = 0; r < NF; ++r) ucol[r] = 0.0;
#pragma unroll
            for (int f = 0; f < 4; ++f)
#pragma unroll
                for (int q = 0; q < NFQ; ++q) {
                    const double ph = S[C::oPHF + (f * NFQ + q) * RBS + m];
#pragma unroll
                    for (int k = 0; k < FBS; ++k) ucol[f * FBS + k] += ft.cw[q][k] * ph;
                }
            if (C::GENERAL_FANCY && l < RBS) {
#pragma unroll
                for (int r = 0; r < NF; ++r) S[C::oFT + r + m * NF] = ucol[r];
            }
        }
        wave_sync();
        if (l < MS) {
#pragma unroll
            for (int k = 0; k < NR; ++k) S[C::oZ + k + c * ZS] = col[k];
            if (NRP != NR) S[C::oZ + NR + c * ZS] = 0.0;
        }
        double ycol[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) ycol[k] = col[k];
        if (C::GENERAL_FANCY || a.oper != nullptr) {
            if (C::DPPFWD) dpp_backward<NR, C::NLR>(lreg, col);
            else lds_backward_rd<NR, LD>(LG, S + C::oRCP, col);      // col = oper[:, c]
            if (a.oper != nullptr && valid && l < MS) {
                double *dst = a.oper + rel(NR * MS) + (size_t)c * NR;
#pragma unroll
                for (int k = 0; k < NR; ++k) dst[k] = col[k];
            }
        }

        PA_TICK(3);
        // ================= S6: column c of U ==========================================
        PA_MARK("S6");
        if (UNIT_U && !(a.ablate & 32u)) {
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                double *zu = S + ((upk[r] >> 12) & 0xfffu);
#pragma unroll
                for (int k = 0; k < FBS; ++k) zu[k] = uval[r][k];
            }
            if (l >= CBS && l < MS) {
                // the NF rows of a face column: zeros (16-byte stores), then the block of its own face on top of them
                // (LDS writes of a lane land in order)
                double *zc = S + C::oZ + NRP + c * ZS;
                static_assert(NF % 2 == 0 && NRP % 2 == 0 && ZS % 2 == 0, "16-byte aligned U columns");
#pragma unroll
                for (int r = 0; r < NF; r += 2) *reinterpret_cast<double2 *>(zc + r) = double2{0.0, 0.0};
                const double msu = -S[C::oSU + fc];
#pragma unroll
                for (int k = 0; k < FBS; ++k) zc[(UPERM_ON ? ((fc + 4 - C::UF1) & 3) : fc) * FBS + k] = msu * ufc[k];
            }
        }
        if (C::HAS_STAB && !UNIT_U && !(a.ablate & 32u)) {
            if (C::GENERAL_FANCY) {
                // proj1[:, c] = e_c - M1^-1 (M2 R[:, c])   hho.hpp:184-190
                double pr[CBS];
#pragma unroll
                for (int i = 0; i < CBS; ++i) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < NR; ++k)
                        s += S[C::oMRl + (1 + k) * CBS + i] * col[k];
                    pr[i] = s;
                }
                const int badm = (int)S[C::oSU + 17];      // chol(M1) comes with the record
                lds_forward_rd<CBS, C::LDM>(S + C::oMCl, S + C::oMCRl, pr);
                lds_backward_rd<CBS, C::LDM>(S + C::oMCl, S + C::oMCRl, pr);
                if (badm && !bad) bad = 100 + badm;
#pragma unroll
                for (int i = 0; i < CBS; ++i) pr[i] = (i == c ? 1.0 : 0.0) - pr[i];
                // T_F[:, c] / (|F|/2) = MR1 R[:, c] + MR2 proj1[:, c]   (hho.hpp:222-230; piKF.solve is linear)
#pragma unroll
                for (int r = 0; r < NF; ++r) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < NR; ++k) s += S[C::oFT + r + (1 + k) * NF] * col[k];
#pragma unroll
                    for (int k = 0; k < CBS; ++k) s += S[C::oFT + r + k * NF] * pr[k];
                    ucol[r] = s;
                }
            } else if (l >= CBS) {
#pragma unroll
                for (int r = 0; r < NF; ++r) ucol[r] = 0.0;     // T_F = [trace_F | 0]
            }
            // U_F = sqrt(|F|/2h) ( L^^-1 T_F/(|F|/2) - L^^T E_F )
            const double4 su4 = *reinterpret_cast<const double4 *>(S + C::oSU);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double su = f == 0 ? su4.x : f == 1 ? su4.y : f == 2 ? su4.z : su4.w;
                double xf[FBS];
#pragma unroll
                for (int k = 0; k < FBS; ++k) xf[k] = ucol[f * FBS + k];
                face_forward<FBS>(ft, xf);
#pragma unroll
                for (int k = 0; k < FBS; ++k) {
                    const double e = (l >= CBS && fc == f) ? ufc[k] : 0.0;      // (L^^T E_F)[k][c]
                    ucol[f * FBS + k] = su * (xf[k] - e);
                }
            }
            if (l < MS) {
#pragma unroll
                for (int r = 0; r < NF; ++r) S[C::oZ + NRP + r + c * ZS] = ucol[r];
            }
        }
        wave_sync();
        PA_TICK(4);
        // region P is free (L, reciprocals, scalars all consumed) once the face scales below are read: next cell's record
        // corner tile on the vector pipe, short form: its U term needs the face scale, which the next record is about to replace
        double cornerU = 0.0;
        int cic = 0, cjc = 0;
        if (C::CORNER_VALU && !SPLIT) {
            uint32_t cpk = corner_pk;
            asm volatile("" : "+v"(cpk));
            cic = (int)(cpk & 0xffu); cjc = (int)((cpk >> 8) & 0xffu);       // cic <= cjc
            if (CORNER_SHORT && l < C::NCORNER * (C::NCORNER + 1) / 2) {
                const double su = S[C::oSU + (cpk >> 16)];
                cornerU = cornerT * su * su;
            }
        }
        double t11s[T11_SHORT ? C::CPW : 1];      // squared scale of the lane's tile-(1,1) column face, for each cell of the wavefront
        if (T11_SHORT) {
#pragma unroll
            for (int gi = 0; gi < C::CPW; ++gi) {
                const double su = smem[gi * C::LDS_PER_CELL + C::oSU + t11f];
                t11s[gi] = su * su;
            }
        }
        rec_deposit();
        // condensed mode: the cell's right-hand side (lanes < CBS) and, for the recovery, its face unknowns (lanes < NF),
        // one value per lane, in flight during the product
        double fT_l = 0.0, uF_l = 0.0;
        if (COND) {
            if (a.rhs != nullptr && l < CBS) fT_l = a.rhs[rel(CBS) + l];
            if (a.uF != nullptr && l < NF) uF_l = a.uF[rel(NF) + l];
        }

        // ================= S7/S8 (lc only): lc = Z^T Z on the matrix pipe ============
        // v_mfma_f64_16x16x4_f64: D(16x16) += A(16x4) B(4x16); lane l supplies A[l&15][l>>4] and
        // B[l>>4][l&15] and receives D[(l>>4) + 4r][l&15], r = 0..3.  For a tile (I, J) of Z^T Z both
        // operands are elements of Z: A[i][k] = Z[k][16I+i], B[k][j] = Z[k][16J+j] -- one LDS read per
        // lane feeds 16 FMAs (the vector form reads one LDS double per FMA).  All 64 lanes work on one
        // cell at a time; the CPW cells of the wavefront are processed in turn.
        PA_TICK(5);
        __builtin_amdgcn_s_setprio(PRIO_OUT);
        if (!SPLIT) {
            PA_MARK("S7m");
            constexpr int NTL = (MS + 15) / 16;              // column tiles
            constexpr int KS = (C::ZR + 3) / 4;              // k-steps
            constexpr int NPAIRS = NTL * (NTL + 1) / 2;
            typedef double v4d __attribute__((ext_vector_type(4)));
            const int kk = lane >> 4, jj = lane & 15;
            constexpr bool DIRECT = C::DIRECT_STORE && !COND;      // condensed mode: always through the LDS image
            constexpr int OS = COND ? C::LDI : MS;                 // stride of the image
            // Through the image with an even stride: the columns of Z are fed to the tiles in the order pi(i) = 4 (i & 3) + (i >> 2),
            // both operands alike, so that the lane's four accumulators D[kk + 4 r][jj] are lc[16 I + 4 kk + r][16 J + pi(jj)], r = 0..3:
            // FOUR CONSECUTIVE rows of one column of the image -- two 16-byte LDS writes instead of four 8-byte ones, and the 16 lanes
            // of a write cycle (kk fixed, pi(jj) = all 16 columns) fall on 16 different bank quads where the 8-byte column writes at
            // stride 22 met two by two.  The mirror copy of an off-diagonal tile stays 8-byte writes.
            constexpr bool ACC_PERM = !DIRECT && !COND && OS % 2 == 0;      // (condensed k = 2: 8 spilled registers with it, and no gain)
            const int pj = ACC_PERM ? 4 * (jj & 3) + (jj >> 2) : jj;
            static_assert(!T11_SHORT || ACC_PERM == ACC_PERM_, "the per-lane constants of tile (1,1) assume this tile's lane -> (row, column) map");
            const bool want_image = COND || a.lc != nullptr;
            // no barrier is needed between the cells: the wavefront reads a cell's Z and then overwrites
            // it with the same cell's output image in program order
            wave_sync();      // Z complete (all columns written)
            // corner tile on the vector pipe: every group for its own cell, before the image may overwrite Z
            double corner = 0.0;
            if (C::CORNER_VALU && l < C::NCORNER * (C::NCORNER + 1) / 2 && !(a.ablate & 64u)) {
                const double *zi = S + C::oZ + (16 + cic) * ZS, *zj = S + C::oZ + (16 + cjc) * ZS;
                constexpr int NROW = CORNER_SHORT ? NRP : C::ZR;             // (row NR of Z is a zero pad)
                typedef double v2d_ __attribute__((ext_vector_type(2)));
                v2d_ pz[NROW / 2], qz[NROW / 2];                             // every read first: one LDS round trip
#pragma unroll
                for (int k = 0; k + 1 < NROW; k += 2) {
                    pz[k / 2] = *reinterpret_cast<const v2d_ *>(zi + k);
                    qz[k / 2] = *reinterpret_cast<const v2d_ *>(zj + k);
                }
                double s0 = cornerU, s1 = 0.0;
#pragma unroll
                for (int k = 0; k + 1 < NROW; k += 2) {
                    s0 = __builtin_fma(pz[k / 2].x, qz[k / 2].x, s0);
                    s1 = __builtin_fma(pz[k / 2].y, qz[k / 2].y, s1);
                }
                if (NROW & 1) s0 = __builtin_fma(zi[NROW - 1], zj[NROW - 1], s0);
                corner = s0 + s1;
            }
#pragma unroll
            for (int gi = 0; gi < C::CPW; ++gi) {
                v4d acc[NPAIRS];
                const double *Zg = smem + gi * C::LDS_PER_CELL + C::oZ;
                double *Og = smem + gi * C::LDS_PER_CELL + C::oOUT;
                // (the accumulators start from the zero operand of each tile's first instruction; on the profiling path that
                // skips the product they are left undefined -- zeroing them ahead of the branch cost 8 moves per cell)
                if (a.ablate & 64u) {
#pragma unroll
                    for (int t = 0; t < NPAIRS; ++t) asm volatile("" : "=v"(acc[t]));
                } else {
#pragma unroll
                    for (int t = 0; t < NPAIRS; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const int k = 4 * ks + kk;
                        double z[NTL];
#pragma unroll
                        for (int t = 0; t < NTL; ++t) {
                            if (UPERM_ON && t == 1 && ks >= C::KS1) { z[t] = 0.0; continue; }
                            const int col = 16 * t + pj;
                            // (decided at compile time wherever the whole tile row / k-step is inside Z)
                            const bool rok = 4 * ks + 3 < C::ZR || k < C::ZR, cok = 16 * t + 15 < MS || col < MS;
                            const double v = Zg[(rok && cok) ? k + col * ZS : 0];
                            // A lane beyond the last COLUMN of Z feeds only the rows / columns >= MS of the tiles (D[i][j] takes row i of
                            // A and column j of B), which are never stored: whatever it read (element 0 of Z) may stay.  A lane beyond the
                            // last ROW of Z would add to entries that are.
                            z[t] = rok ? v : 0.0;
                        }
                        // tile (1,1), short form: rows of Y only (the last of their k-steps may also hold rows of U: masked)
                        constexpr int KSY = cdiv(NRP, 4);
                        double z1y = z[NTL - 1];
                        if (T11_SHORT && ks == KSY - 1 && NRP % 4 != 0) z1y = k < NRP ? z1y : 0.0;
                        int t = 0;
#pragma unroll
                        for (int I = 0; I < NTL; ++I)
#pragma unroll
                            for (int J = I; J < NTL; ++J, ++t) {
                                if (T11_SHORT && I == 1 && J == 1) {
                                    if (ks < KSY) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(z1y, z1y, acc[t], 0, 0, 0);
                                } else if (!(C::CORNER_VALU && I == 1 && J == 1) && !(UPERM_ON && J == 1 && ks >= C::KS1))
                                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[I], z[J], acc[t], 0, 0, 0);
                            }
                    }
                    if (T11_SHORT) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[NPAIRS - 1][r] = __builtin_fma(t11c[r], t11s[gi], acc[NPAIRS - 1][r]);
                    }
                }
                PA_TICK(6 + 2 * (gi & 1));
                PA_MARK("S8m");
                if (DIRECT) {
                    // ---- S8 (lc only): straight from the accumulators to HBM, no LDS image.  lc is symmetric:
                    // the lane's D[row][col] is written at (col, row), where the 16 lanes of a group
                    // (jj = 0..15) cover 16 consecutive rows of one column = one 128-byte run; the second copy
                    // of an off-diagonal tile is 32-byte runs (kk = 0..3).  All 64 lanes work on cell gi.
                    if (a.lc != nullptr && !(a.ablate & 128u)) {
                        const bool valid_g = base + gi < a.n;
                        double *o = a.lc + (valid_g ? base + gi : 0) * (size_t)(MS * MS);
                        int t = 0;
#pragma unroll
                        for (int I = 0; I < NTL; ++I)
#pragma unroll
                            for (int J = I; J < NTL; ++J, ++t) {
                                const int colj = 16 * J + jj;
                                if (C::CORNER_VALU && I == 1 && J == 1) continue;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int row = 16 * I + kk + 4 * r;
                                    if (16 * I + 4 * r < MS && valid_g && (16 * J + 15 < MS || colj < MS) &&
                                        (16 * I + 4 * r + 3 < MS || row < MS)) {
                                        const double v = acc[t][r];
                                        o[colj + row * MS] = v;                 // entry (colj, row)
                                        if (I != J) o[row + colj * MS] = v;     // entry (row, colj)
                                    }
                                }
                            }
                    }
                } else {
                if (want_image && !(a.ablate & 128u)) {
                    int t = 0;
#pragma unroll
                    for (int I = 0; I < NTL; ++I)
#pragma unroll
                        for (int J = I; J < NTL; ++J, ++t) {
                            const int colj = 16 * J + pj;
                            if ((16 * J + 15 < MS || colj < MS) && !(C::CORNER_VALU && I == 1 && J == 1)) {
                                if (ACC_PERM) {
                                    const int row0 = 16 * I + 4 * kk;
                                    typedef double v2d_ __attribute__((ext_vector_type(2)));
                                    if (16 * I + 15 < MS || row0 + 3 < MS) {
                                        *reinterpret_cast<v2d_ *>(Og + row0 + colj * OS) = v2d_{acc[t][0], acc[t][1]};
                                        *reinterpret_cast<v2d_ *>(Og + row0 + 2 + colj * OS) = v2d_{acc[t][2], acc[t][3]};
                                    } else {
#pragma unroll
                                        for (int r = 0; r < 4; ++r)
                                            if (row0 + r < MS) Og[row0 + r + colj * OS] = acc[t][r];
                                    }
                                    if (I != J) {
#pragma unroll
                                        for (int r = 0; r < 4; ++r)
                                            if (16 * I + 15 < MS || row0 + r < MS) Og[colj + (row0 + r) * OS] = acc[t][r];
                                    }
                                } else {
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int row = 16 * I + kk + 4 * r;
                                    if (16 * I + 4 * r < MS && (16 * I + 4 * r + 3 < MS || row < MS)) {
                                        const double v = acc[t][r];
                                        Og[row + colj * OS] = v;
                                        if (I != J) Og[colj + row * OS] = v;
                                    }
                                }
                                }
                            }
                        }
                }
                }
                PA_TICK(7 + 2 * (gi & 1));
            }
            if (C::CORNER_VALU && want_image && !(a.ablate & 128u) && l < C::NCORNER * (C::NCORNER + 1) / 2) {
                if (DIRECT) {
                    if (valid) {
                        double *o = a.lc + rel(MS * MS);
                        o[(16 + cic) + (16 + cjc) * MS] = corner;
                        o[(16 + cjc) + (16 + cic) * MS] = corner;
                    }
                } else {
                    S[C::oOUT + (16 + cic) + (16 + cjc) * OS] = corner;
                    S[C::oOUT + (16 + cjc) + (16 + cic) * OS] = corner;
                }
            }
            if constexpr (ASM) {
                // ================= S9' (assembling mode): the image to its places in the global CSR system ==================
                PA_MARK("S9a");
                wave_sync();      // the image is complete
                static_assert(C::LDI == asm_image_stride(MS), "asm_cut_scatter_kernel lays its image out as this one");
                bool scatter_ok = valid;
                asm_apply_tags(a.scatter, cell, scatter_ok, fT_l);      // (fictitious domain: cut cells are not this pass's)
                asm_scatter_cell<G, CBS, FBS, C::LDI>(a.scatter, S + C::oOUT, l, cell, scatter_ok, fT_l,
                                                      a.lc != nullptr ? a.lc + rel(MS * MS) : nullptr);
                PA_TICK(13);
                wave_sync();      // every read of the image is done
            } else if (COND) {
                // ================= S9 (condensed mode): eliminate the cell unknowns in the LDS image ==================
                // Row i of the symmetric (MS + 1) x (MS + 1) matrix  M = [A_TT A_TF f_T; A_FT A_FF 0; f_T^T 0 0]  belongs to
                // lane i.  The first CBS steps of its Cholesky factorization, row by row (left-looking, Eigen's LLT order on
                // A_TT), leave  L_TT = chol(A_TT)  in the cell rows,  W^T = A_FT L_TT^-T  in the face rows and
                // w0^T = f_T^T L_TT^-T  in the last one -- the forward substitutions ride on the factorization's chain --
                // and the Schur complement of the pivots is what is asked for:
                //   S = A_FF - W^T W,   g = -W^T w0,   uT = L_TT^-T (w0 - W uF).
                PA_MARK("S9");
                constexpr int LDI = C::LDI, NPV = CBS;
                double *A = S + C::oOUT;
                if (l < CBS) A[MS * LDI + l] = fT_l;                            // row MS: f_T
                if (a.uF != nullptr && l < NF) A[MS * LDI + CBS + l] = uF_l;       // (behind it: the face unknowns)
                wave_sync();
                const int i = l <= MS ? l : 0;                                  // (lanes beyond the last row mirror row 0)
                double row[NPV];
#pragma unroll
                for (int k = 0; k + 1 < NPV; k += 2) {
                    const double2 v = lds_pair(A + i * LDI + k);
                    row[k] = v.x; row[k + 1] = v.y;
                }
                if (NPV & 1) row[NPV - 1] = A[i * LDI + NPV - 1];
                int badc = 0;
                constexpr bool COND_DPP = NPV <= 16 && MS + 1 <= 32 && G <= 32;
                if (COND_DPP) {
                    // The chain in registers: lane q of each row of 16 lanes holds image rows q and q + 16 (both rows of 16 lanes
                    // of a 32-lane group hold the same pairs), so every pivot row -- there are at most 16 -- sits in lane j of the
                    // row of 16 and its prefix reaches the other lanes through the DPP operand of the FMAs (row_newbcast:j):
                    // no LDS read of the pivot row, no broadcast of the pivot by v_readlane, no LDS write and wait per step.
                    if (!(a.ablate & 256u)) {
                    constexpr bool TWO = MS + 1 > 16;
                    const int q = lane & 15;
                    const int iA = q <= MS ? q : 0, iB = (TWO && q + 16 <= MS) ? q + 16 : 0;
                    double rA[NPV], rB[TWO ? NPV : 1], rdiag = 0.0;
#pragma unroll
                    for (int k = 0; k + 1 < NPV; k += 2) {
                        const double2 va = lds_pair(A + iA * LDI + k);
                        rA[k] = va.x; rA[k + 1] = va.y;
                        if (TWO) { const double2 vb = lds_pair(A + iB * LDI + k); rB[k] = vb.x; rB[k + 1] = vb.y; }
                    }
                    if (NPV & 1) { rA[NPV - 1] = A[iA * LDI + NPV - 1]; if (TWO) rB[NPV - 1] = A[iB * LDI + NPV - 1]; }
                    if (NPV >= COND_RL_MIN) cond_dpp_chain_rl<NPV, TWO>(rA, rB, rdiag, badc, q);
                    else cond_dpp_chain<NPV, TWO>(rA, rB, rdiag, badc, q);
                    // back to the image (the diagonal holds 1 / L[j][j]); one row of 16 lanes writes
                    if ((G == 16 || l < 16)) {
#pragma unroll
                        for (int k = 0; k < NPV; ++k) {
                            if (q <= MS) A[iA * LDI + k] = (k == q) ? rdiag : rA[k];
                            if (TWO && q + 16 <= MS) A[iB * LDI + k] = rB[k];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NPV; ++k) row[k] = (TWO && l >= 16) ? rB[TWO ? k : 0] : rA[k];
                    wave_sync();
                    }
                } else if (!(a.ablate & 256u)) {
#pragma unroll
                for (int j = 0; j < NPV; ++j) {
                    // M[i][j] - sum_{k<j} L[i][k] L[j][k]; row j's prefix is in LDS already
                    const double s = j == 0 ? row[0] : lds_dotsub_n(row[j], A + j * LDI, row, j);
                    const double d = group_broadcast<G>(s, j);
                    if (!(d > 0.0) && !badc) badc = j + 1;
                    const double r = fast_rsqrt<1>(d);
                    row[j] = s * r;
                    if (l <= MS && l >= j) A[i * LDI + j] = (l == j) ? r : row[j];      // the diagonal holds 1 / L[j][j]
                    wave_sync();
                }
                }
                PA_TICK(13);
                if (badc && !bad) bad = 200 + badc;
                if (a.uF == nullptr) {
                    // Schur complement, row i' = l - CBS of it by lane l: entries (m', i'), m' <= i', are the run
                    // i'(i'+1)/2 .. of the column-packed upper triangle
                    double *stg = S + C::oOUT + C::oSTG;
                    const int ip = l - CBS;
                    const bool frow = l >= CBS && l < MS;
                    constexpr bool SCHUR_MFMA = NF >= COND_SCHUR_MFMA_MIN && NF <= 16;
                    if (a.ablate & 512u) {
                    } else if (SCHUR_MFMA) {
                        // W^T W on the matrix pipe, all 64 lanes on one cell at a time: W[k][j] = L[CBS + j][k] is both
                        // operands of the one 16 x 16 tile (one LDS read per lane and k-step); the lane's P[kk + 4r][jj]
                        // meets A_FF(kk + 4r, jj) of the image's lower triangle and goes to the packed upper one
                        const double gi = lds_dotsub<NPV>(0.0, A + MS * LDI, row);
#pragma unroll
                        for (int gi_ = 0; gi_ < C::CPW; ++gi_) {
                            const double *Ag = smem + gi_ * C::LDS_PER_CELL + C::oOUT;
                            double *sg = smem + gi_ * C::LDS_PER_CELL + C::oOUT + C::oSTG;
                            v4d p = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                            for (int ks = 0; ks < (NPV + 3) / 4; ++ks) {
                                const int k = 4 * ks + kk;
                                const bool ok = (4 * ks + 3 < NPV || k < NPV) && (NF == 16 || jj < NF);
                                const double w = Ag[ok ? (CBS + jj) * LDI + k : 0];
                                const double wz = ok ? w : 0.0;
                                p = __builtin_amdgcn_mfma_f64_16x16x4f64(wz, wz, p, 0, 0, 0);
                            }
                            double aff[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int ir = kk + 4 * r;
                                const bool up = ir <= jj && (NF == 16 || jj < NF);
                                aff[r] = Ag[up ? (CBS + jj) * LDI + CBS + ir : 0];
                            }
                            // (the staging area lies on the cell rows: every read of W above has been issued, and LDS
                            // operations of a wavefront execute in order)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int ir = kk + 4 * r;
                                if (4 * r < NF && ir <= jj && (NF == 16 || jj < NF)) sg[jj * (jj + 1) / 2 + ir] = aff[r] - p[r];
                            }
                        }
                        if (frow) stg[C::NSP + ip] = gi;
                    } else {
#pragma unroll
                    for (int mp = 0; mp < NF; ++mp) {
                        const double s = lds_dotsub<NPV>(A[i * LDI + CBS + mp], A + (CBS + mp) * LDI, row);
                        if (frow && mp <= ip) stg[ip * (ip + 1) / 2 + mp] = s;
                    }
                    const double gi = lds_dotsub<NPV>(0.0, A + MS * LDI, row);
                    if (frow) stg[C::NSP + ip] = gi;
                    }
                    wave_sync();
                    PA_TICK(14);
                    if (valid && a.cond != nullptr) {
                        double *o = a.cond + rel(C::NCOND);
                        static_assert(C::NCOND % 2 == 0, "16-byte stores of the packed record");
#pragma unroll
                        for (int e0 = 0; e0 < C::NCOND / 2; e0 += G) {
                            const int e = e0 + l;
                            if (e < C::NCOND / 2)
                                *reinterpret_cast<double2 *>(o + 2 * e) = *reinterpret_cast<const double2 *>(stg + 2 * e);
                        }
                    }
                } else {
                    // recovery: t = w0 - W uF (lane k < CBS: column k of the face rows), then L_TT^T uT = t column by column
                    double t = 0.0;
                    const int k = l < CBS ? l : 0;
                    t = A[MS * LDI + k];
#pragma unroll
                    for (int ip = 0; ip < NF; ++ip) t = __builtin_fma(-A[(CBS + ip) * LDI + k], A[MS * LDI + CBS + ip], t);
                    const double rdk = A[k * LDI + k];
#pragma unroll
                    for (int m = NPV - 1; m >= 0; --m) {
                        const double um = group_broadcast<G>(t * rdk, m);
                        if (l == m) t = um;
                        else if (l < m) t = __builtin_fma(-A[m * LDI + k], um, t);
                    }
                    if (valid && a.uT != nullptr && l < CBS) a.uT[rel(CBS) + l] = t;
                }
                wave_sync();      // every read of the image is done
            } else if (DIRECT) {
                wave_sync();      // the next cell's tables overwrite Z
            } else {
                if (a.lc != nullptr && !(a.ablate & 128u)) {
                    wave_sync();
                    if (valid) {
                        // (profiling, bit 1024: every pass of a block writes the same two matrices -- the stores without their HBM traffic)
                        // (the block's part of the address is wave-uniform: scalar arithmetic; the lane adds its group's matrix)
                        const size_t cb = (a.ablate & 1024u) ? lblock * C::CPW : base;
                        double *o = a.lc + cb * (size_t)(MS * MS) + (uint32_t)g * (uint32_t)(MS * MS);
                        constexpr int NPAIR = MS * MS / 2, NIT = cdiv(NPAIR, G);
                        // every read of the image first, then the stores: with a read and its store per step the compiler
                        // reuses one register quad and the steps become a chain of LDS round trips
                        typedef double v2d_ __attribute__((ext_vector_type(2)));
                        v2d_ img[NIT];
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const int e = it * G + l;
                            img[it] = *reinterpret_cast<const v2d_ *>(S + C::oOUT + 2 * (((it + 1) * G <= NPAIR || e < NPAIR) ? e : 0));
                        }
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const int e = it * G + l;
                            if ((it + 1) * G <= NPAIR || e < NPAIR) *reinterpret_cast<v2d_ *>(o + 2 * e) = img[it];
                        }
                        if ((MS * MS) & 1) {
                            if (l == 0) o[MS * MS - 1] = S[C::oOUT + MS * MS - 1];
                        }
                    }
                }
                wave_sync();
            }
        } else {
        // ================= S7 (data and stab apart): Z^T Z, entries (c, c + d mod MS) ==
        PA_MARK("S7");
        double acc_d[ND], acc_s[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) { acc_d[d] = 1.0; acc_s[d] = 1.0; }
        if (!(a.ablate & 64u)) {
            int cp = c;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const double *zc = S + C::oZ + cp * ZS;
                double s = lds_dotadd<NR>(0.0, zc, ycol);
                double u = 0.0;
                if (C::HAS_STAB) u = lds_dotadd<NF>(0.0, zc + NRP, ucol);
                asm volatile("" : "+v"(s), "+v"(u));     // pin: keep the FMAs next to their LDS reads
                acc_d[d] = s; acc_s[d] = u;
                cp = (cp + 1 == MS) ? 0 : cp + 1;
            }
        }
        wave_sync();      // every read of L and Z is done: the output image may overwrite Z

        // ================= S8: mirror through LDS, stream to HBM ======================
        PA_MARK("S8");
#pragma unroll
        for (int which = 0; which < 3; ++which) {
            double *dst = which == 0 ? a.lc : which == 1 ? a.data : a.stab;
            if (dst == nullptr || (a.ablate & 128u)) continue;
            if (l < MS) {
                int cp = c;
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const double v = which == 0 ? acc_d[d] + acc_s[d] : which == 1 ? acc_d[d] : acc_s[d];
                    S[C::oOUT + c + cp * MS] = v;
                    S[C::oOUT + cp + c * MS] = v;
                    cp = (cp + 1 == MS) ? 0 : cp + 1;
                }
            }
            wave_sync();
            if (valid) {
                double *o = dst + rel(MS * MS);
                constexpr int NPAIR = MS * MS / 2, NIT = cdiv(NPAIR, G);
                typedef double v2d_ __attribute__((ext_vector_type(2)));
                v2d_ img[NIT];                             // reads first, then the stores (see the lc-only path)
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int e = it * G + l;
                    img[it] = *reinterpret_cast<const v2d_ *>(S + C::oOUT + 2 * (((it + 1) * G <= NPAIR || e < NPAIR) ? e : 0));
                }
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int e = it * G + l;
                    if ((it + 1) * G <= NPAIR || e < NPAIR) *reinterpret_cast<v2d_ *>(o + 2 * e) = img[it];
                }
                if ((MS * MS) & 1) {
                    if (l == 0) o[MS * MS - 1] = S[C::oOUT + MS * MS - 1];
                }
            }
            wave_sync();
        }
        }
        if (valid && a.info != nullptr && l == 0) a.info[rel(1)] = bad;
        PA_TICK(10);
    }
#ifdef PA_STAGE_CLOCK
    if (a.dbg != nullptr && lane == 0)
        for (int i = 0; i < PA_NSTAGE; ++i) a.dbg[(size_t)blockIdx.x * PA_NSTAGE + i] = tk_sum[i];
#endif
}

}  // namespace pa
