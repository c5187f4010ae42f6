"""The judge of pa_interface_rows_patches / pa_interface_rows_coarse (patch_precond.hip, coarse_precond.hip): the tables of ONE SLAB
of the interface problem's face-only system, by their definitions in terms of the whole-mesh tables of interface_patch_twin.tables
and interface_coarse_twin.table.  Nothing of those tables is restated; this module only says which part of them a slab holds.

A slab of cell rows [r0, r1) owns the rows [row_begin, row_end): the first face block at or after its first face r0 (2 Nx + 1), up to
the first at or after face r1 (2 Nx + 1) -- computed here from the oracle mesh's tags (interface_patch_twin.device_face_table), not
from the product.
  face: the whole-mesh face patches whose rows lie in the range, in order.
  cell: the whole-mesh patches of the slab's OWN cells (one per uncut cell, one per side of a cut cell, negative first, by
        ascending cell id), every row outside the range deleted, a patch that keeps no row dropped.
  coarse: rows [row_begin, row_end) of the whole-mesh table, the pointer rebased; the columns are the whole mesh's.
Two planted defects (what a slab builder gets wrong first): `halo` gives the cells of the row below the slab patches as well,
`keep_top` deletes no row.  local_columns is the negative control of the compaction by side: the numbering a compaction over the
slab's own blocks would give."""
from collections import namedtuple

import numpy as np

import interface_coarse_twin as IC
import interface_patch_twin as I
import patch_pcg_twin as P
import rows_pcg_twin as R

# the catalogue: name -> (Nx, cell-row bounds of the slabs, cut_preprocess's further arguments or a name of cut_meshes.CATALOGUE)
CASES = {
    "circle-12-thin": (12, (0, 1, 5, 6, 12), {}),
    "circle-12": (12, (0, 3, 8, 12), {}),
    "circle-12-two": (12, (0, 7, 12), {}),
    "circle-12-one-slab": (12, (0, 12), {}),
    "line-12": (12, (0, 5, 6, 12), {"line_y": 0.43}),
    "B": (15, (0, 4, 5, 11), "B"),
    "E": (9, (0, 2, 3, 5), "E"),
}


def case(name):
    """-> (Nx, bounds, kwargs of cut_preprocess / oracle_lib.CutMesh after N)"""
    import cut_meshes as CM
    N, bounds, kw = CASES[name]
    return N, bounds, (CM.kwargs(kw) if isinstance(kw, str) else dict(kw))


def oracle_mesh(o, name):
    N, _, kw = case(name)
    return o.CutMesh(N, refsteps=4, **kw)


Numbering = namedtuple("Numbering", "ft num_other")


def numbering(msh):
    """pa_cut_preprocess's face numbering from the oracle's tags"""
    ft, num_other = I.device_face_table(msh.bnd, msh.face_loc)
    return Numbering(np.asarray(ft), int(num_other))


def row_range(msh, rows, fbs):
    """the owned rows of the slab of cell rows [rows[0], rows[1])"""
    nb = numbering(msh)
    frow = 2 * msh.Nx + 1

    def first_block(face):
        b = nb.ft[face:]
        b = b[b >= 0]
        return int(b[0]) if b.size else nb.num_other
    return fbs * first_block(rows[0] * frow), fbs * first_block(rows[1] * frow)


def ranges(msh, bounds, fbs):
    return [row_range(msh, r, fbs) for r in zip(bounds[:-1], bounds[1:])]


def whole_patches(msh, k):
    """-> (face, cell, per cell patch its cell) of the whole mesh in the device's numbering"""
    nb = numbering(msh)
    face, cell = I.tables(nb.ft, msh.cell_faces, msh.cell_loc, msh.face_loc, k + 1)
    owner = np.asarray([c for c, _, bl in I.cell_side_blocks(nb.ft, msh.cell_faces, msh.cell_loc, msh.face_loc) if bl], dtype=np.int64)
    assert owner.size == cell.ptr.size - 1
    return face, cell, owner


def slab_patches(msh, k, bounds, halo=False, keep_top=False):
    """per slab: (face, cell) as patch_pcg_twin.Patches with global rows"""
    face, cell, cell_of = whole_patches(msh, k)
    rg = ranges(msh, bounds, k + 1)
    out = []
    for (r0, r1), (a, b) in zip(zip(bounds[:-1], bounds[1:]), rg):
        first = face.rows[face.ptr[:-1]]
        fl = [face.rows[face.ptr[p]:face.ptr[p + 1]] for p in np.nonzero((first >= a) & (first < b))[0]]
        lo = (r0 - 1 if halo and r0 > 0 else r0) * msh.Nx
        cl = []
        for p in np.nonzero((cell_of >= lo) & (cell_of < r1 * msh.Nx))[0]:
            rows = cell.rows[cell.ptr[p]:cell.ptr[p + 1]]
            if not keep_top:
                rows = rows[(rows >= a) & (rows < b)]
            if rows.size:
                cl.append(rows)
        out.append((R._table(fl), R._table(cl)))
    return out


def whole_coarse(msh, k, H, parts):
    return IC.mesh_table(msh, msh.faces, k, H, parts, device_numbering=True)


def slab_coarse(msh, k, H, parts, bounds):
    """per slab: rows [row_begin, row_end) of the whole-mesh table (None where the whole-mesh entry refuses)"""
    tb = whole_coarse(msh, k, H, parts)
    if tb is None:
        return None
    return [R.slab_coarse(tb, a, b) for a, b in ranges(msh, bounds, k + 1)]


def local_columns(tb):
    """the column ids a compaction over the slab's own blocks alone would give: the columns the slab's rows touch, renumbered in order"""
    used = np.unique(tb.cols)
    return np.searchsorted(used, tb.cols).astype(np.int32), int(used.size)


def same_patches(x, y):
    return np.array_equal(x.ptr, y.ptr) and np.array_equal(x.rows, y.rows)


def same_table(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]


def covers(pt, a, b, exists):
    """every row within [a, b), and every owned row that exists (exists: bool per row of the system) in at least one patch"""
    if pt.rows.size and (pt.rows.min() < a or pt.rows.max() >= b):
        return False
    seen = np.zeros(exists.size, dtype=bool)
    seen[pt.rows] = True
    return bool(np.all(seen[a:b] == exists[a:b]))


def existing_rows(msh, k):
    """rows of the system that some face owns (an unowned block's rows exist in no patch)"""
    nb = numbering(msh)
    fbs = k + 1
    ex = np.zeros(nb.num_other * fbs, dtype=bool)
    for bl in I.face_blocks(nb.ft, msh.face_loc):
        for b in bl:
            ex[b * fbs:(b + 1) * fbs] = True
    return ex


def stacked(tables):
    """the slabs' patch tables one after the other: a valid whole-mesh table"""
    return R.concat(tables)


__all__ = ["CASES", "case", "oracle_mesh", "row_range", "ranges", "whole_patches", "slab_patches", "whole_coarse", "slab_coarse",
           "local_columns", "same_patches", "same_table", "covers", "existing_rows", "stacked", "P"]
