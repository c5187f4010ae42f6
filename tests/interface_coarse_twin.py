"""The judge of pa_interface_condensed_coarse (proton_amd/csrc/coarse_precond.hip): the coarse table of the interface problem's
face-only system, defined as the table pa_condensed_coarse(.., PA_COARSE_BY_SIDE, where = negative) would build if every block were a
face of its own.  That sentence is all this module does: it expands interface_assembler's numbering (interface_patch_twin: a cut face
owns face_table[f] on the negative side and face_table[f] + 1 on the positive side, an uncut face its one block) into one item per
block -- the face's two points, the block id as compressed id, the side -- and hands the items to coarse_twin.table.  The hats, their
products, the two modes and the order of the columns are coarse_twin's; nothing of them is restated here.

A block nobody owns (pa_cut_preprocess counts a cut face on the Dirichlet boundary, which owns nothing: interface_patch_twin.
device_face_table) becomes an item whose two points are the corner vertex 0, where every interior hat vanishes: its rows stay empty
and it touches no column."""
import functools

import numpy as np

import coarse_twin as CT
import interface_patch_twin as I


def block_items(face_table, face_loc, faces, num_other):
    """-> (points [num_other, 2], block ids [num_other], sides [num_other] in {0, 1}), one item per block of the numbering"""
    pts, blk, side = [], [], []
    for f, b in enumerate(face_table):
        if b < 0:
            continue
        if face_loc[f] == I.CUT:
            for s in (I.NEG, I.POS):
                pts.append(faces[f]); blk.append(int(b) + s); side.append(s)
        else:
            pts.append(faces[f]); blk.append(int(b)); side.append(int(face_loc[f]))
    for b in sorted(set(range(num_other)) - set(blk)):                # unowned: no hat reaches vertex 0
        pts.append((0, 0)); blk.append(b); side.append(I.NEG)
    assert sorted(blk) == list(range(num_other))
    return np.asarray(pts, dtype=np.int64).reshape(-1, 2), np.asarray(blk, dtype=np.int64), np.asarray(side, dtype=np.int64)


def table(N, H, fbs, face_table, face_loc, faces, num_other, parts, shift=None, Ny=None):
    """pa_interface_condensed_coarse on the N x Ny mesh (Ny = None: N x N): parts "one" or "side" -> coarse_twin.Table, or None where
    the entry refuses"""
    pts, blk, side = block_items(face_table, face_loc, faces, num_other)
    return CT.table(N, N if Ny is None else Ny, H, fbs, blk, pts, num_other, side if parts == "side" else None, 0, shift)


def mesh_table(msh, faces, k, H, parts, device_numbering=False, shift=None):
    """the table of an oracle_lib.CutMesh at face degree k; faces: the plain assembler's; device_numbering: pa_cut_preprocess's"""
    _, ft, _, num_other = msh.interface_tables()
    if device_numbering:
        ft, num_other = I.device_face_table(msh.bnd, msh.face_loc)
    return table(msh.Nx, H, k + 1, ft, msh.face_loc, faces, num_other, parts, shift, Ny=msh.Ny)


@functools.lru_cache(maxsize=None)
def oracle_interface_coarse(N, k, H, kappa=(1.0, 1.0)):
    """interface_patch_twin.oracle_interface_condensed(N, k, kappa) with its two coarse tables of H -> coarse_twin.Condensed"""
    import oracle_lib as o
    sy = I.oracle_interface_condensed(N, k, kappa)
    msh = o.CutMesh(N, refsteps=4)
    faces, _ = o.mesh_faces(o.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0))
    one, side = (mesh_table(msh, faces, k, H, parts) for parts in ("one", "side"))
    return CT.Condensed(sy.rowptr, sy.colind, sy.values, sy.b, sy.face, sy.cell, one, side, N, k + 1)
