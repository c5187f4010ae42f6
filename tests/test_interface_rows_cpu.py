"""The row partition of the interface problem's face-only system without a GPU: pa_interface_rows_partition_info is host only (the
whole-mesh preprocessing every rank runs, then prefix counts), so the slabs' owned rows, entries, cell blocks and halo sizes are
checked here; the ctypes binding lists the new entry points."""
import pytest

CIRCLE = dict(kind=0, radius=0.35, alpha=0.5, beta=0.5, cut_y=0.0)
LINE = dict(kind=1, radius=0.0, alpha=0.0, beta=0.0, cut_y=0.43)
CASES = [(12, CIRCLE, (0, 1, 5, 6, 12)), (12, CIRCLE, (0, 3, 8, 12)), (20, CIRCLE, (0, 7, 20)), (12, LINE, (0, 5, 6, 12))]
IDS = ["circle-12-thin", "circle-12", "circle-20", "line-12"]
NEW = ["pa_interface_rows_partition_info", "pa_interface_rows_query", "pa_interface_rows_ops_batch", "pa_interface_rows_halo_pack",
       "pa_interface_rows_csr_pattern", "pa_interface_rows_csr_fill", "pa_interface_rows_recover"]


def info(N, ls, rows, fd):
    from proton_amd import capi
    return capi.interface_rows_partition_info(N, N, capi.LevelSet(ls["kind"], ls["radius"], ls["alpha"], ls["beta"], ls["cut_y"]), 4, rows, fd)


@pytest.mark.parametrize("N,ls,bounds", CASES, ids=IDS)
@pytest.mark.parametrize("fd", [0, 1, 2, 3])
def test_slabs_tile_the_system(N, ls, bounds, fd):
    whole = info(N, ls, (0, N), fd)
    fbs, cbs = fd + 1, (fd + 3) * (fd + 2) // 2
    assert (whole.row_begin, whole.row_end) == (0, whole.system_size) and whole.system_size % fbs == 0
    assert (whole.col_begin, whole.col_end) == (0, whole.system_size)
    assert whole.halo_send_doubles == whole.halo_recv_doubles == 0
    assert (whole.nf, whole.NF) == (4 * fbs, 8 * fbs)
    assert whole.cond_doubles == whole.nf * (whole.nf + 1) // 2 + whole.nf and whole.cond_cut_doubles == whole.NF * (whole.NF + 1) // 2 + whole.NF
    assert whole.cell_block_begin == 0 and whole.cell_block_end > N * N            # every mesh here has cut cells
    slabs = [info(N, ls, r, fd) for r in zip(bounds[:-1], bounds[1:])]
    row, blk = 0, 0
    for s in slabs:
        assert s.system_size == whole.system_size
        assert s.row_begin == row and s.row_end >= s.row_begin                      # disjoint, ascending, no gap
        assert s.cell_block_begin == blk and s.cell_block_end > blk
        assert s.col_begin <= s.row_begin and s.col_end >= s.row_end and s.col_end <= whole.system_size
        assert (s.nf, s.NF, s.cond_doubles, s.cond_cut_doubles) == (whole.nf, whole.NF, whole.cond_doubles, whole.cond_cut_doubles)
        row, blk = s.row_end, s.cell_block_end
    assert row == whole.system_size and blk == whole.cell_block_end
    assert sum(s.nnz_owned for s in slabs) == whole.nnz_owned
    assert slabs[0].halo_recv_doubles == 0 and slabs[-1].halo_send_doubles == 0
    for lo, up in zip(slabs[:-1], slabs[1:]):
        assert lo.halo_send_cells == up.halo_recv_cells == N
        assert lo.halo_send_cut == up.halo_recv_cut
        assert lo.halo_send_doubles == up.halo_recv_doubles == N * (whole.cond_doubles + whole.nf) + lo.halo_send_cut * whole.cond_cut_doubles
        assert up.col_begin < up.row_begin                                          # the rows of its bottom faces read the slab below
    assert cbs > 0


def test_partition_info_refusals():
    import ctypes as C
    from proton_amd import capi
    L = capi.lib()
    out = capi.InterfaceRowsInfo()
    ls = capi.LevelSet(0, 0.35, 0.5, 0.5, 0.0)

    def call(N, rows, fd, lsp=C.byref(ls), outp=C.byref(out), refsteps=4):
        return L.pa_interface_rows_partition_info(N, N, 0.0, 1.0, 0.0, 1.0, lsp, refsteps, rows[0], rows[1], fd, outp)
    assert call(12, (0, 12), 1) == 0
    assert call(12, (0, 12), -1) == 2 and call(12, (0, 12), 4) == 2
    assert call(12, (5, 5), 1) == 1 and call(12, (5, 13), 1) == 1 and call(0, (0, 0), 1) == 1
    assert call(12, (0, 12), 1, lsp=None) == 1 and call(12, (0, 12), 1, outp=None) == 1 and call(12, (0, 12), 1, refsteps=11) == 1


def test_binding_lists_the_new_symbols():
    from proton_amd import capi
    L = capi.lib()
    for n in NEW:
        assert capi.EXPORTS.count(n) == 1 and getattr(L, n).argtypes is not None
    from proton_amd.batch import BatchAssembler
    for m in ("interface_rows_info", "interface_rows_ops", "interface_rows_halo_pack", "interface_rows_csr_pattern", "interface_rows_csr_fill",
              "interface_rows_recover"):
        assert callable(getattr(BatchAssembler, m))


@pytest.mark.parametrize("N,bounds", [(12, (0, 1, 5, 6, 12)), (20, (0, 7, 20))])
def test_slab_ranges_against_the_oracle_tables(oracle, N, bounds):
    """the prefix counts against the oracle's restatement of interface_assembler's tables (cuthho_square.cpp:1142-1178): a slab's
    first cell block is cell_table of its first cell, its first row the first face block at or after its first face"""
    import numpy as np
    fd, frow = 1, 2 * N + 1
    ct, ft, num_all_cells, num_other = oracle.CutMesh(N, refsteps=4).interface_tables()
    ct, ft = np.asarray(ct), np.asarray(ft)

    def first_block(face):
        b = ft[face:]
        b = b[b >= 0]
        return int(b[0]) if b.size else num_other
    for r in zip(bounds[:-1], bounds[1:]):
        i = info(N, CIRCLE, r, fd)
        assert i.system_size == (fd + 1) * num_other
        assert i.cell_block_begin == ct[r[0] * N] and i.cell_block_end == (ct[r[1] * N] if r[1] < N else num_all_cells)
        assert i.row_begin == (fd + 1) * first_block(r[0] * frow) and i.row_end == (fd + 1) * first_block(r[1] * frow)
