"""What makes tests/interface_rows_pcg_twin.py a judge of pa_interface_rows_patches / pa_interface_rows_coarse, without a GPU: on
the catalogue of the GPU test (tests/test_gpu_interface_rows_pcg.py) the slab tables by their definitions tile the whole-mesh
tables, meet the contract of pa_conjugated_gradient_rows_patch_coarse, hold the hard cases -- a trimmed top row, cut top faces, a
slab without cut cells, a global compaction that a slab alone cannot reproduce --, and the comparisons the GPU test makes catch the
two defects a slab builder gets wrong first.  The ctypes binding lists the new entry points."""
import numpy as np
import pytest

import interface_patch_twin as I
import interface_rows_pcg_twin as T

KS = (0, 1, 2, 3)
HS = (3, 4)
NEW = ["pa_interface_rows_patches_query", "pa_interface_rows_patches", "pa_interface_rows_coarse_query", "pa_interface_rows_coarse"]


@pytest.fixture(scope="module")
def meshes(oracle):
    return {name: T.oracle_mesh(oracle, name) for name in T.CASES}


def test_binding_lists_the_new_symbols():
    from proton_amd import capi
    L = capi.lib()
    for n in NEW:
        assert capi.EXPORTS.count(n) == 1 and getattr(L, n).argtypes is not None
    from proton_amd.batch import BatchAssembler
    for m in ("interface_rows_patches", "interface_rows_coarse"):
        assert callable(getattr(BatchAssembler, m))
    for m in ("interface_rows_patches_query", "interface_rows_patches", "interface_rows_coarse_query", "interface_rows_coarse"):
        assert callable(getattr(capi.Context, m))


@pytest.mark.parametrize("name", list(T.CASES))
def test_row_ranges_are_the_products(meshes, name):
    """the ranges from the oracle's tags are pa_interface_rows_partition_info's (host only), and tile the system"""
    from proton_amd import capi
    msh = meshes[name]
    N, bounds, kw = T.case(name)
    if "line_y" in kw:
        ls = capi.LevelSet(1, 0.0, 0.0, 0.0, kw["line_y"])
    else:
        cx, cy = kw.get("center", (0.5, 0.5))
        ls = capi.LevelSet(0, kw.get("radius", 0.35), cx, cy, 0.0)
    lo, hi = kw.get("lo", (0.0, 0.0)), kw.get("hi", (1.0, 1.0))
    for k in KS:
        rg = T.ranges(msh, bounds, k + 1)
        assert rg[0][0] == 0 and rg[-1][1] == (k + 1) * T.numbering(msh).num_other
        assert all(a[1] == b[0] for a, b in zip(rg[:-1], rg[1:]))
        for rows, (a, b) in zip(zip(bounds[:-1], bounds[1:]), rg):
            i = capi.interface_rows_partition_info(msh.Nx, msh.Ny, ls, 4, rows, k, lo=lo, hi=hi)
            assert (i.row_begin, i.row_end) == (a, b), (name, k, rows)


@pytest.mark.parametrize("name", list(T.CASES))
def test_slab_patches_tile_and_cover(meshes, name):
    """face tables concatenated are the whole table; both kinds lie within the range and cover every owned row that exists; the
    slabs' cell tables stacked are a valid whole-mesh table (every existing row covered)"""
    msh = meshes[name]
    _, bounds, _ = T.case(name)
    for k in KS:
        face, cell, _ = T.whole_patches(msh, k)
        slabs = T.slab_patches(msh, k, bounds)
        rg = T.ranges(msh, bounds, k + 1)
        ex = T.existing_rows(msh, k)
        assert T.same_patches(T.stacked([s[0] for s in slabs]), face)
        for (f, c), (a, b) in zip(slabs, rg):
            assert T.covers(f, a, b, ex) and T.covers(c, a, b, ex)
            assert int(f.ptr[0]) == 0 and int(c.ptr[0]) == 0
            sizes = np.diff(c.ptr)
            assert sizes.size == 0 or (sizes.min() >= 1 and sizes.max() <= 4 * (k + 1))
        assert T.covers(T.stacked([s[1] for s in slabs]), 0, ex.size, ex)
        if len(bounds) == 2:                             # one slab: the whole-mesh tables themselves
            assert T.same_patches(slabs[0][1], cell)


def lost_rows(msh, k, bounds):
    """per own cell patch of every slab that is not the last: (cell, is cut, rows lost, rows of the cell's top face)"""
    nb = T.numbering(msh)
    fbs = k + 1
    _, cell, cell_of = T.whole_patches(msh, k)
    out = []
    for (r0, r1), (a, b) in zip(zip(bounds[:-1], bounds[1:]), T.ranges(msh, bounds, fbs)):
        if r1 == msh.Ny:
            continue
        for p in np.nonzero((cell_of >= r0 * msh.Nx) & (cell_of < r1 * msh.Nx))[0]:
            rows = cell.rows[cell.ptr[p]:cell.ptr[p + 1]]
            lost = rows[(rows < a) | (rows >= b)]
            c = int(cell_of[p])
            top = int(msh.cell_faces[c, 2])
            tb = [int(nb.ft[top])] + ([int(nb.ft[top]) + 1] if msh.face_loc[top] == I.CUT else [])
            top_rows = np.concatenate([np.arange(q * fbs, (q + 1) * fbs) for q in tb])
            out.append((c, msh.cell_loc[c] == I.CUT, msh.face_loc[top] == I.CUT, lost, top_rows, rows.size - lost.size))
    return out


def test_the_catalogue_holds_the_trimmed_cells(meshes):
    """only top-face rows are ever lost, and only in the top row of a slab that is not the last; an uncut cell and a cut cell with a
    cut top face each lose exactly their top-face rows (the cut cell's side patch: that side's block of the face).  No cell side of
    the catalogue is dropped for lack of rows: every side of a top-row cell keeps a bottom or vertical face (counted below)."""
    k = 1
    uncut = cut_top = dropped = 0
    for name, msh in meshes.items():
        _, bounds, _ = T.case(name)
        tops = {r1 - 1 for r1 in bounds[1:-1]}
        for c, is_cut, top_cut, lost, top_rows, kept in lost_rows(msh, k, bounds):
            if lost.size == 0:
                continue
            assert c // msh.Nx in tops, (name, c)
            assert np.all(np.isin(lost, top_rows)), (name, c)
            if not is_cut and np.array_equal(np.sort(lost), top_rows):
                uncut += 1
            if is_cut and top_cut and lost.size == k + 1:
                cut_top += 1
            dropped += kept == 0
    assert uncut > 0 and cut_top > 0
    assert dropped == 0                                  # the catalogue has none: said in the docstring


def test_a_slab_without_cut_cells_keeps_both_parts(meshes):
    """circle-12 (0, 1, ..): slab 0 has no cut cell; its "side" table still carries the whole mesh's ncoarse and column ids"""
    msh = meshes["circle-12-thin"]
    _, bounds, _ = T.case("circle-12-thin")
    assert not np.any(msh.cell_loc[:msh.Nx] == I.CUT)
    for H in HS:
        whole = T.whole_coarse(msh, 1, H, "side")
        slabs = T.slab_coarse(msh, 1, H, "side", bounds)
        assert all(s.ncoarse == whole.ncoarse for s in slabs)
        assert slabs[0].cols.size > 0


@pytest.mark.parametrize("name", list(T.CASES))
def test_coarse_rows_stack_to_the_whole_table(meshes, name):
    msh = meshes[name]
    _, bounds, _ = T.case(name)
    for k in KS:
        for H in HS:
            for parts in ("one", "side"):
                whole = T.whole_coarse(msh, k, H, parts)
                assert whole is not None
                slabs = T.slab_coarse(msh, k, H, parts, bounds)
                ptr = np.concatenate([[0]] + [s.ptr[1:] + off for s, off in zip(slabs, np.cumsum([0] + [s.cols.size for s in slabs[:-1]]))])
                assert np.array_equal(ptr, whole.ptr)
                assert np.array_equal(np.concatenate([s.cols for s in slabs]), whole.cols)
                assert np.array_equal(np.concatenate([s.vals for s in slabs]), whole.vals)
                for s, (a, b) in zip(slabs, T.ranges(msh, bounds, k + 1)):
                    assert s.ptr.size == b - a + 1 and int(s.ptr[0]) == 0


def test_by_side_compacts_and_a_slab_cannot_do_it_alone(meshes):
    """ncoarse by side is below twice the node count (columns are dropped) on at least one mesh, and -- the negative control -- on at
    least one slab the compaction over the slab's own blocks numbers the columns differently from the whole mesh's"""
    compacted = differs = 0
    for name, msh in meshes.items():
        _, bounds, _ = T.case(name)
        for H in HS:
            one, side = T.whole_coarse(msh, 1, H, "one"), T.whole_coarse(msh, 1, H, "side")
            compacted += side.ncoarse < 2 * one.ncoarse
            for s in T.slab_coarse(msh, 1, H, "side", bounds):
                cols, n = T.local_columns(s)
                differs += (n != s.ncoarse) or not np.array_equal(cols, s.cols)
    assert compacted > 0 and differs > 0


@pytest.mark.parametrize("name", ["circle-12-thin", "line-12", "B", "E"])
def test_planted_defects_are_caught(meshes, name):
    """halo-row cells given patches, and the top face kept: the comparison the GPU test makes (same_patches against the twin's
    tables) tells both from the true cell tables.  The kept top face also breaks the solver's contract (a row outside the range);
    the halo row's patches do not -- their foreign rows are deleted, what stays is the slab's bottom faces once more --, so only
    the comparison finds them"""
    msh = meshes[name]
    _, bounds, _ = T.case(name)
    k = 1
    good = T.slab_patches(msh, k, bounds)
    rg = T.ranges(msh, bounds, k + 1)
    ex = T.existing_rows(msh, k)
    for defect in ("halo", "keep_top"):
        bad = T.slab_patches(msh, k, bounds, **{defect: True})
        assert any(not T.same_patches(b[1], g[1]) for b, g in zip(bad, good)), defect
        assert all(T.same_patches(b[0], g[0]) for b, g in zip(bad, good))           # the face tables have neither defect
        inside = [T.covers(b[1], a, e, ex) for b, (a, e) in zip(bad, rg)]
        assert all(inside) if defect == "halo" else not all(inside)
        if defect == "halo":
            assert sum(b[1].ptr.size for b in bad) > sum(g[1].ptr.size for g in good)
