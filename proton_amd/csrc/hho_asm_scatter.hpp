// hho_asm_scatter.hpp -- the scatter epilogue of hho_local_ops_kernel<Cfg, MODE_ASM>: the LDS image of a cell's lc goes
// straight to its places in the CSR arrays of the assembler's own system (assembler_csr.hip), no lc in HBM.
//
// assembler<Mesh>::assemble (src/methods/hho_bits/hho.hpp:344-406) turns a cell's local matrix into global entries in the loop
// iteration that formed it; here the cooperative kernel does the same with the image it holds.  The fills of
// assembler_csr.hip are gathers and their tables are indexed by face; the scatter needs the inverse, one record per cell.
// asm_scatter_cell has a second caller, asm_cut_scatter_kernel (assembler_csr.hip), which feeds it the cut cells' operators of the
// fictitious-domain problem from an image it copies out of HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

// Where the entries of one cell go.  The record holds counts, not offsets, so that one table serves every degree pair of a
// mesh: the offsets are the closed forms of face_system.hpp (cell_block_start, face_block_start) in the block sizes the
// kernel instance knows at compile time.
struct alignas(16) AsmCellRec {
    uint32_t cpre;           // non-Dirichlet faces of the cells before this one (cprefix)
    uint32_t order;          // bits 2s, 2s+1: local index of the cell's s-th non-Dirichlet face in ascending compressed order;
                             // bits 8-10: their number
    int32_t comp[4];         // per local face its compressed id, -1 Dirichlet
    uint32_t face[4];        // per local face its face id (the boundary data g are indexed by it)
    uint32_t fpre[4];        // per non-Dirichlet local face F: cells of the faces before F (fprefix) ...
    uint32_t colpre[4];      // ... and their column faces (colprefix)
    uint32_t pack[4];        // per non-Dirichlet local face F: bits 3m .. 3m+2: position of local face m among F's column faces
                             // (7: m is Dirichlet); bits 12-13: F's cells; bit 14: this cell is F's second cell block;
                             // bits 16-18: F's column faces
    uint32_t pad_[2];
};

struct AsmScatterArgs {
    const AsmCellRec *tab;   // per cell of the context
    const double *g;         // boundary data per face (nfaces x fbs), may be null = 0
    double *values, *RHS;    // CSR values; right-hand side (may be null)
    uint64_t cell_nnz;       // entries of all cell rows
    uint64_t ncells;
    // fictitious-domain assembly (pa_fictdom_csr_assemble): the tags of the context's cells, null everywhere else.  A cell tagged
    // ASM_LOC_CUT is left to asm_cut_scatter_kernel (nothing of it is scattered here); an uncut cell whose tag is not `where`
    // takes a zero right-hand side (cuthho_square.cpp:659-664)
    const int8_t *cell_loc;
    int32_t where;
};

constexpr int8_t ASM_LOC_CUT = 2;                // LOC_CUT of cut_host.hpp, PA_LOC_ON_INTERFACE

// The assembling instances' group size and image stride as functions of msize alone (Cfg::G of the instance pa_configs.def
// selects for the pair, Cfg::LDI), for the second caller of asm_scatter_cell that holds no Cfg: asm_cut_scatter_kernel
constexpr int asm_group_lanes(int ms) { return ms + 1 <= 16 ? 16 : ms + 1 <= 32 ? 32 : 64; }
constexpr int asm_image_stride(int ms) { return ((ms + 1) & ~1) % 4 == 2 ? ((ms + 1) & ~1) : ((ms + 1) & ~1) + 2; }

// what the operator pass does with a cell under the tags above: scatter it or not, and with which right-hand side
__device__ __forceinline__ void asm_apply_tags(const AsmScatterArgs &s, size_t cell, bool &valid, double &fT)
{
    if (s.cell_loc == nullptr) return;
    const int loc = s.cell_loc[cell];
    valid = valid && loc != ASM_LOC_CUT;
    if (loc != s.where) fT = 0.0;
}

// One group of G lanes (lane l) per cell.  img: the cell's image, entry (i, j) of lc at img[i + j * LDI] (what the fills read
// at lc[j * MS + i]).  fT: lane l < CBS holds the cell's right-hand side l (0 without one).
//
// Cell rows: one contiguous run of CBS (CBS + n FBS) values, lane e of a step on entry e.  Face rows: per non-Dirichlet local
// face F the FBS x MS block of image rows of F, lanes along the row; a position has one contributor except F's own diagonal
// block and F's right-hand side, which take one addend per adjacent cell: those are added with the hardware FP64 atomic onto
// entries asm_zero_accumulated() cleared -- 0 + a + b and 0 + b + a are the same double, so the result is the gather's
// lc_A + lc_B whatever the timing.  Every step reads its image entries first and stores afterwards.
template <int G, int CBS, int FBS, int LDI>
__device__ __forceinline__ void asm_scatter_cell(const AsmScatterArgs &s, const double *img, int l, size_t cell, bool valid, double fT,
                                                 double *lc_out)
{
    constexpr int MS = CBS + 4 * FBS;
    constexpr int CH = 8;                                   // image entries a lane holds between its reads and its stores
    const AsmCellRec *rp = s.tab + cell;
    if (!valid) return;
    // ---- optional lc, the layout of pa_local_ops_batch (column-major MS x MS): lane e on entry e
    if (lc_out != nullptr) {
        constexpr int NIT = (MS * MS + G - 1) / G;
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += CH) {
            double v[CH];
#pragma unroll
            for (int it = it0; it < it0 + CH && it < NIT; ++it) {
                const int e = it * G + l;
                const int ee = ((it + 1) * G <= MS * MS || e < MS * MS) ? e : 0;
                const int j = ee / MS, i = ee - j * MS;
                v[it - it0] = img[i + j * LDI];
            }
#pragma unroll
            for (int it = it0; it < it0 + CH && it < NIT; ++it) {
                const int e = it * G + l;
                if ((it + 1) * G <= MS * MS || e < MS * MS) lc_out[e] = v[it - it0];
            }
        }
    }
    const uint32_t order = rp->order;
    const int n = (int)((order >> 8) & 7u);
    // ---- cell rows
    {
        const int R = CBS + n * FBS;
        // e / R for e < 2^10, R < 2^6: exact with a 16-bit reciprocal rounded up
        const uint32_t inv = n == 0 ? (65536u + CBS - 1) / CBS : n == 1 ? (65536u + CBS + FBS - 1) / (CBS + FBS)
                           : n == 2 ? (65536u + CBS + 2 * FBS - 1) / (CBS + 2 * FBS)
                           : n == 3 ? (65536u + CBS + 3 * FBS - 1) / (CBS + 3 * FBS) : (65536u + MS - 1) / MS;
        static_assert(CBS * MS < 1024 && MS < 64, "the reciprocal division of the cell rows");
        double *dst = s.values + (uint64_t)CBS * ((uint64_t)cell * CBS + (uint64_t)rp->cpre * FBS);         // cell_block_start
        constexpr int NIT = (CBS * MS + G - 1) / G;
        const int E = CBS * R;
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += CH) {
            double v[CH];
#pragma unroll
            for (int it = it0; it < it0 + CH && it < NIT; ++it) {
                const int e = it * G + l;
                const uint32_t ee = e < E ? (uint32_t)e : 0u;
                const uint32_t i = (ee * inv) >> 16, jj = ee - i * (uint32_t)R;
                uint32_t j = jj;
                if (jj >= (uint32_t)CBS) {
                    const uint32_t sidx = (jj - CBS) / (uint32_t)FBS, kp = (jj - CBS) - sidx * FBS;
                    j = (uint32_t)CBS + ((order >> (2 * sidx)) & 3u) * FBS + kp;
                }
                v[it - it0] = img[i + j * LDI];
            }
#pragma unroll
            for (int it = it0; it < it0 + CH && it < NIT; ++it) {
                const int e = it * G + l;
                if (e < E) dst[e] = v[it - it0];
            }
        }
    }
    // ---- face rows, face by face
    const uint64_t face_rhs0 = (uint64_t)CBS * s.ncells;
#pragma unroll
    for (int lf = 0; lf < 4; ++lf) {
        const int32_t comp = rp->comp[lf];
        if (comp < 0) continue;
        const uint32_t pk = rp->pack[lf];
        const uint32_t ncell = (pk >> 12) & 3u, ncol = (pk >> 16) & 7u;
        const uint32_t R = ncell * CBS + ncol * FBS;
        const uint32_t coff = (pk & (1u << 14)) ? (uint32_t)CBS : 0u;
        double *dst = s.values + s.cell_nnz + (uint64_t)FBS * ((uint64_t)rp->fpre[lf] * CBS + (uint64_t)rp->colpre[lf] * FBS);      // face_block_start
        constexpr int NIT = (FBS * MS + G - 1) / G;
        static_assert(NIT <= CH, "one chunk per face");
        double v[NIT];
        uint32_t off[NIT];      // position in the block of F's rows; bit 31: F's own block (accumulated); ~0: nothing to write
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = it * G + l;
            const bool in = (it + 1) * G <= FBS * MS || e < FBS * MS;
            const int ee = in ? e : 0;
            const int k = ee / MS, j = ee - k * MS;
            v[it] = img[(CBS + lf * FBS + k) + j * LDI];
            uint32_t o;
            if (j < CBS) o = (uint32_t)k * R + coff + (uint32_t)j;
            else {
                const int m = (j - CBS) / FBS, kp = (j - CBS) - m * FBS;
                const uint32_t pos = (pk >> (3 * m)) & 7u;
                o = pos == 7u ? ~0u : ((uint32_t)k * R + ncell * CBS + pos * FBS + (uint32_t)kp) | (m == lf ? 0x80000000u : 0u);
            }
            off[it] = in ? o : ~0u;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (off[it] == ~0u) continue;
            if (off[it] & 0x80000000u) unsafeAtomicAdd(dst + (off[it] & 0x7fffffffu), v[it]);
            else dst[off[it]] = v[it];
        }
    }
    // ---- right-hand side: the terms and the order of dirichlet_rhs_contrib (face_system.hpp; the triplet path's
    // rhs - sum lc g over the Dirichlet columns in local column order, hho.hpp:401, 405)
    if (s.RHS != nullptr && l < MS) {
        const bool crow = l < CBS;
        const int lfo = crow ? 0 : (l - CBS) / FBS;
        const int32_t comp = rp->comp[lfo];
        double acc = crow ? fT : 0.0;
        if (n < 4) {
#pragma unroll
            for (int lf = 0; lf < 4; ++lf)
                if (rp->comp[lf] < 0) {
                    const uint32_t f = rp->face[lf];
                    for (int kp = 0; kp < FBS; ++kp) {
                        const double dd = s.g != nullptr ? s.g[(size_t)f * FBS + kp] : 0.0;
                        acc -= img[l + (CBS + lf * FBS + kp) * LDI] * dd;
                    }
                }
        }
        if (crow) s.RHS[cell * CBS + l] = acc;
        else if (comp >= 0) unsafeAtomicAdd(s.RHS + face_rhs0 + (uint64_t)comp * FBS + (uint32_t)((l - CBS) - lfo * FBS), acc);
    }
}

}  // namespace pa
