"""The judge of pa_interface_condensed_patches (proton_amd/csrc/interface_condensed.hip): the two patch tables of the interface
problem's face-only system restated in numpy from the oracle's numbering (interface_tables(), cell_faces, cell_loc, face_loc), and
the Schur complement of the oracle's `-i` system on which the tables are worth what tests/test_interface_patch_cpu.py asserts.

Rows are rows of pa_interface_condensed_csr_pattern: unknown k of face block b at b fbs + k, a cut face owning the two blocks
face_table[f] (negative side) and face_table[f] + 1 (positive side), an uncut face the one block face_table[f].
  face: one patch per non-Dirichlet face by ascending face id, all rows of its blocks.
  cell: by ascending cell id; an uncut cell gives one patch, the blocks of its non-Dirichlet faces in the order bottom, right, top,
        left; a cut cell one per side, negative first: of a cut face the side's block, of an uncut face its block only where the
        face lies on that side.  Dirichlet faces (face_table < 0) are skipped, a side without rows gives no patch."""
import functools

import numpy as np

import patch_pcg_twin as P

NEG, POS, CUT = 0, 1, 2                    # element_location as oracle_lib's CUT_NEG, CUT_POS, CUT_ON_INTERFACE


def _table(block_lists, fbs):
    block_lists = [b for b in block_lists if b]
    ptr = np.zeros(len(block_lists) + 1, dtype=np.int64)
    if block_lists:
        np.cumsum([len(b) * fbs for b in block_lists], out=ptr[1:])
    rows = [np.arange(b * fbs, (b + 1) * fbs) for bl in block_lists for b in bl]
    return P.Patches(ptr, np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32))


def face_blocks(face_table, face_loc):
    """per non-Dirichlet face, ascending: its blocks"""
    return [[int(b)] + ([int(b) + 1] if face_loc[f] == CUT else []) for f, b in enumerate(face_table) if b >= 0]


def cell_side_blocks(face_table, cell_faces, cell_loc, face_loc):
    """-> list of (cell, side or None for an uncut cell, blocks), empty ones included"""
    out = []
    for c in range(cell_faces.shape[0]):
        fs = [int(f) for f in cell_faces[c]]
        if cell_loc[c] != CUT:
            out.append((c, None, [int(face_table[f]) for f in fs if face_table[f] >= 0]))
            continue
        for s in (NEG, POS):
            bl = []
            for f in fs:
                if face_table[f] < 0:
                    continue
                if face_loc[f] == CUT:
                    bl.append(int(face_table[f]) + s)
                elif face_loc[f] == s:
                    bl.append(int(face_table[f]))
            out.append((c, s, bl))
    return out


def tables(face_table, cell_faces, cell_loc, face_loc, fbs):
    """-> (face, cell) as patch_pcg_twin.Patches"""
    face = _table(face_blocks(face_table, face_loc), fbs)
    cell = _table([bl for _, _, bl in cell_side_blocks(face_table, cell_faces, cell_loc, face_loc)], fbs)
    return face, cell


def device_face_table(bnd, face_loc):
    """pa_cut_preprocess's face_table restated (capi_cut.hip: the compress-table value of a non-Dirichlet face plus the cut faces
    of lower id) -> (face_table, num_other_faces = non-Dirichlet faces + cut faces, as cuthho_square.cpp:1155-1166 counts them).
    It is interface_tables() wherever no cut face lies on the Dirichlet boundary -- every circle inside the square.  A cut face on
    the boundary (the line level set) is counted though it owns nothing: the block after the faces before it stays unowned, an
    empty row group of pa_interface_condensed_csr_pattern that belongs to no patch."""
    bnd, cutf = np.asarray(bnd) != 0, np.asarray(face_loc) == CUT
    before = lambda m: np.cumsum(m) - m                  # noqa: E731
    ft = np.where(bnd, -1, before(~bnd) + before(cutf)).astype(np.int64)
    return ft, int(np.count_nonzero(~bnd) + np.count_nonzero(cutf))


def mesh_tables(msh, k, device_numbering=False):
    """the tables of an oracle_lib.CutMesh at face degree k, and the number of rows; device_numbering: from device_face_table"""
    ct, ft, num_all_cells, num_other = msh.interface_tables()
    if device_numbering:
        ft, num_other = device_face_table(msh.bnd, msh.face_loc)
    face, cell = tables(ft, msh.cell_faces, msh.cell_loc, msh.face_loc, k + 1)
    return face, cell, (k + 1) * num_other


@functools.lru_cache(maxsize=None)
def oracle_interface_condensed(N, k, kappa=(1.0, 1.0)):
    """The Schur complement on the face unknowns of the system tests/cuthho_driver.py:run_interface assembles for `-i`
    (oracle_interface_provider + CutMesh.interface_assemble; the cell blocks couple only inside their cell -- a cut cell's two
    blocks with each other -- and are eliminated cell by cell), symmetrised, with its two patch tables -> patch_pcg_twin.Condensed"""
    import scipy.sparse as sp

    import cuthho_driver as drv
    import oracle_lib as o
    msh = o.CutMesh(N, refsteps=4)
    di = o.degrees(k + 1, k)
    plain = o.Assembler(o.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, di, bf_id=2)
    ct, ft, num_all_cells, num_other = msh.interface_tables()
    cbs, fbs = di.cbs, di.fbs
    size = cbs * num_all_cells + fbs * num_other
    local = drv.oracle_interface_provider(msh, di, kappa)
    rows, cols, vals = [], [], []
    RHS = np.zeros(size)
    for c in range(msh.nc):
        lc, f = local[c]
        dd = np.zeros(lc.shape[0])
        if msh.cell_loc[c] != o.CUT_ON_INTERFACE:
            for lf in range(4):
                dd[cbs + lf * fbs: cbs + (lf + 1) * fbs] = plain.g[int(msh.cell_faces[c, lf])]
        tr, tc, tv, rr, rv = msh.interface_assemble(di, c, ct, ft, num_all_cells, lc, f, dd)
        rows.append(tr); cols.append(tc); vals.append(tv)
        ok = rr >= 0
        np.add.at(RHS, rr[ok], rv[ok])
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(size, size))
    c0 = cbs * num_all_cells
    KTT, KTF, KFT, KFF = K[:c0, :c0], K[:c0, c0:], K[c0:, :c0], K[c0:, c0:]
    inv = []
    for c in range(msh.nc):
        a = int(ct[c]) * cbs
        w = (2 if msh.cell_loc[c] == o.CUT_ON_INTERFACE else 1) * cbs
        inv.append(np.linalg.inv(KTT[a:a + w, a:a + w].toarray()))
    iTT = sp.block_diag(inv, format="csr")
    S = (KFF - KFT @ iTT @ KTF).tocsr()
    S = ((S + S.T) * 0.5).tocsr()
    S.sort_indices()
    b = RHS[c0:] - KFT @ (iTT @ RHS[:c0])
    face, cell = tables(ft, msh.cell_faces, msh.cell_loc, msh.face_loc, fbs)
    return P.Condensed(S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.copy(), b, face, cell)
