// interface_rows.hpp -- the interface_assembler's numbering (cuthho_square.cpp:1142-1178) of ONE SLAB of cell rows, on the host.
//
// Every rank of a row partition runs the deterministic whole-mesh preprocessing, so it holds cell_loc and face_loc of the whole
// mesh; the first block of any cell or face is then a prefix count (cell c: c + cut cells before c; face f: compressed id + cut
// faces before f).  A slab needs the numbering of its own cells and of the cell row below it (the halo row, whose records the
// rank below sends up): the EXTENDED range, cell rows [row0 - 1, row1).  Its faces are one contiguous range of global face ids
// (structured_mesh.hpp: every node row owns its horizontals and verticals), so the extended tables are slices of the whole-mesh
// ones, renumbered from the first cell block / face block of the range.  interface_csr.hip runs its symbolic phase over these
// tables as over a small mesh; the rows source of its gather shifts rows and columns back to the global face-only numbering.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "cut_host.hpp"
#include "structured_mesh.hpp"

namespace pa {

struct IfRowsHost {
    uint32_t Nx = 0, row0 = 0, row1 = 0;
    uint32_t ne = 0, nfe = 0;                    // cells and faces of the extended range
    uint32_t nh = 0, nhc = 0;                    // halo cells received from below (0 or Nx) and the cut cells among them
    uint32_t ns = 0, nsc = 0;                    // top-row cells sent up (0 on the top slab) and the cut cells among them
    uint32_t ncells = 0, ncut = 0;               // the slab's own
    uint32_t fshift = 0;                         // extended id of the context's face 0
    uint32_t num_all_cells = 0, num_other_faces = 0;     // cell / face blocks of the extended range
    uint32_t q0 = 0, q1 = 0;                     // owned face blocks, in the extended numbering
    uint64_t fb0 = 0;                            // global face block of the extended numbering's face block 0
    uint64_t face_blocks = 0;                    // of the whole mesh
    uint64_t cell_block0 = 0, cell_block1 = 0;   // the slab's cell blocks in the full numbering
    uint64_t col_block0 = 0, col_block1 = 0;     // global face blocks the slab's and the halo row's cells touch
    uint64_t nnz_blocks = 0;                     // column blocks summed over the owned row blocks
    // the extended tables (IfCsrMesh of interface_csr.hpp; cut_index of a halo cell: its row among the received cut records)
    std::vector<uint32_t> cell_faces;
    std::vector<int8_t> cell_loc, face_loc;
    std::vector<int32_t> cut_index, cell_table, face_table;
    // the recovery's view of the slab alone: cell blocks from the slab's first, face blocks from its first owned one, by the
    // context's own cell and face ids
    std::vector<int32_t> cell_table_slab, face_table_slab;
};

// tables = false: the counts alone (pa_interface_rows_partition_info)
inline void if_rows_numbering(const CutMeshHost &cm, uint32_t row0, uint32_t row1, bool tables, IfRowsHost &h)
{
    const StructuredMesh sm = cm.sm;
    const uint32_t Nx = sm.Nx, Ny = sm.Ny, frow = sm_face_row(sm);
    const size_t nc = cm.ncells(), nf = cm.nfaces();
    // cut elements before every element of the whole mesh; every cut face belongs to a cut cell (:1152-1163)
    std::vector<uint8_t> fcut(nf, 0);
    std::vector<uint32_t> cbefore(nc + 1, 0), fbefore(nf + 1, 0);
    for (size_t c = 0; c < nc; ++c) {
        const bool cut = cm.cell_loc[c] == LOC_CUT;
        cbefore[c + 1] = cbefore[c] + (cut ? 1u : 0u);
        if (!cut) continue;
        uint32_t f[4];
        cm.cell_face_ids((uint32_t)c, f);
        for (int q = 0; q < 4; ++q)
            if (cm.face_loc[f[q]] == LOC_CUT) fcut[f[q]] = 1;
    }
    for (size_t f = 0; f < nf; ++f) fbefore[f + 1] = fbefore[f] + fcut[f];
    auto block_of = [&](uint32_t f) -> int64_t {            // first global block of face f, -1: Dirichlet
        uint32_t lo, hi; bool dir; int32_t comp;
        sm_face_decode(sm, f, lo, hi, dir, comp);
        return dir ? -1 : (int64_t)comp + fbefore[f];
    };
    auto block_from = [&](size_t gid) -> uint64_t {         // first global block at or after face gid
        for (size_t f = gid; f < nf; ++f) {
            const int64_t b = block_of((uint32_t)f);
            if (b >= 0) return (uint64_t)b;
        }
        return (uint64_t)sm_num_other_faces(sm) + fbefore[nf];
    };
    const uint32_t hb = row0 > 0 ? 1u : 0u, er0 = row0 - hb;
    const size_t ec0 = (size_t)er0 * Nx, sc0 = (size_t)row0 * Nx, sc1 = (size_t)row1 * Nx, ef0 = (size_t)er0 * frow;
    h = IfRowsHost();
    h.Nx = Nx; h.row0 = row0; h.row1 = row1;
    h.ne = (uint32_t)(sc1 - ec0);
    h.nfe = (row1 - er0) * frow + (row1 < Ny ? frow : Nx);
    h.nh = hb * Nx; h.nhc = cbefore[sc0] - cbefore[ec0];
    h.ns = row1 < Ny ? Nx : 0; h.nsc = row1 < Ny ? cbefore[sc1] - cbefore[sc1 - Nx] : 0;
    h.ncells = (uint32_t)(sc1 - sc0); h.ncut = cbefore[sc1] - cbefore[sc0];
    h.fshift = hb * frow;
    h.num_all_cells = h.ne + (cbefore[sc1] - cbefore[ec0]);
    h.face_blocks = (uint64_t)sm_num_other_faces(sm) + fbefore[nf];
    h.fb0 = block_from(ef0);
    h.num_other_faces = (uint32_t)(block_from(ef0 + h.nfe) - h.fb0);
    h.q0 = (uint32_t)(block_from((size_t)row0 * frow) - h.fb0);
    h.q1 = (uint32_t)(block_from((size_t)row1 * frow) - h.fb0);
    const uint64_t cb0 = ec0 + cbefore[ec0];
    h.cell_block0 = sc0 + cbefore[sc0]; h.cell_block1 = sc1 + cbefore[sc1];
    // the blocks of a cell's unknowns (ifc_cell_units of interface_csr.hip): a cut cell sees both blocks of a cut face
    auto cell_blocks = [&](size_t c, uint64_t *out) -> int {
        uint32_t f[4];
        cm.cell_face_ids((uint32_t)c, f);
        const bool cut = cm.cell_loc[c] == LOC_CUT;
        int n = 0;
        for (int q = 0; q < 4; ++q) {
            const int64_t b = block_of(f[q]);
            if (b < 0) continue;
            out[n++] = (uint64_t)b;
            if (cut && fcut[f[q]]) out[n++] = (uint64_t)b + 1;
        }
        return n;
    };
    h.col_block0 = h.face_blocks; h.col_block1 = 0;
    for (size_t c = ec0; c < sc1; ++c) {
        uint64_t b[8];
        const int n = cell_blocks(c, b);
        for (int s = 0; s < n; ++s) { h.col_block0 = std::min(h.col_block0, b[s]); h.col_block1 = std::max(h.col_block1, b[s] + 1); }
    }
    if (h.col_block1 == 0) h.col_block0 = 0;
    // an owned row block's columns: the blocks of the (at most two) cells that push rows into it -- the cells of its face; the
    // second block of a cut face takes rows from cut cells only (ifc_group)
    h.nnz_blocks = 0;
    for (size_t f = (size_t)row0 * frow; f < (size_t)row1 * frow; ++f) {
        if (block_of((uint32_t)f) < 0) continue;
        const uint32_t j = (uint32_t)(f / frow), pos = (uint32_t)(f % frow);
        const bool horizontal = pos % 2 == 0 && pos < 2 * Nx;
        const uint32_t i = horizontal ? pos / 2 : (pos == 2 * Nx ? Nx : pos / 2);
        const size_t cells[2] = {horizontal ? (size_t)(j - 1) * Nx + i : (size_t)j * Nx + i - 1, (size_t)j * Nx + i};   // interior faces
        for (int dup = 0; dup < (fcut[f] ? 2 : 1); ++dup) {
            uint64_t u[16];
            int n = 0;
            for (int s = 0; s < 2; ++s) {
                if (dup == 1 && cm.cell_loc[cells[s]] != LOC_CUT) continue;
                n += cell_blocks(cells[s], u + n);
            }
            std::sort(u, u + n);
            h.nnz_blocks += (uint64_t)(std::unique(u, u + n) - u);
        }
    }
    if (!tables) return;
    h.cell_faces.resize(4 * (size_t)h.ne);
    h.cell_loc.resize(h.ne); h.cut_index.resize(h.ne); h.cell_table.resize(h.ne);
    h.face_loc.resize(h.nfe); h.face_table.resize(h.nfe);
    for (size_t c = ec0; c < sc1; ++c) {
        const size_t e = c - ec0;
        uint32_t f[4];
        cm.cell_face_ids((uint32_t)c, f);
        for (int q = 0; q < 4; ++q) h.cell_faces[4 * e + q] = f[q] - (uint32_t)ef0;
        const bool cut = cm.cell_loc[c] == LOC_CUT;
        h.cell_loc[e] = cm.cell_loc[c];
        h.cut_index[e] = cut ? (int32_t)(cbefore[c] - cbefore[c < sc0 ? ec0 : sc0]) : -1;
        h.cell_table[e] = (int32_t)(c + cbefore[c] - cb0);
    }
    for (size_t t = 0; t < h.nfe; ++t) {
        const int64_t b = block_of((uint32_t)(ef0 + t));
        h.face_loc[t] = cm.face_loc[ef0 + t];
        h.face_table[t] = b < 0 ? -1 : (int32_t)(b - (int64_t)h.fb0);
    }
    h.cell_table_slab.resize(h.ncells);
    for (size_t x = 0; x < h.ncells; ++x) h.cell_table_slab[x] = h.cell_table[h.nh + x] - h.cell_table[h.nh];
    h.face_table_slab.resize(h.nfe - h.fshift);
    for (size_t t = 0; t < h.face_table_slab.size(); ++t) {
        const int32_t b = h.face_table[h.fshift + t];
        h.face_table_slab[t] = b < 0 ? -1 : b - (int32_t)h.q0;
    }
}

}  // namespace pa
