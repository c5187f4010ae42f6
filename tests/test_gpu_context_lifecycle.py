"""One context, several meshes in a row: what a context holds from an earlier mesh (face tables, the condensed and the assembler's
symbolic tables, the cut state, the record buffer) is dropped and rebuilt, never reused.  Every case compares a reused
BatchAssembler against a fresh one on the last mesh, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def fresh():
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def patterns(a, cd, fd):
    """-> [rowptr, colind] of the condensed system, then of the assembler's own"""
    out = [*a.condensed_csr_pattern(cd, fd), *a.assembler_csr_pattern(cd, fd)]
    a.synchronize()
    return out


def tables(a, cd, fd):
    """patterns() and the values and right-hand side of the fused assembly"""
    import proton_amd as pa
    out = patterns(a, cd, fd)
    fused = a.assembler_csr_assemble(cd, fd, rhs=a.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS))
    a.synchronize()
    return out + [fused["values"], fused["RHS"]]


def same(got, want):
    import torch
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), k


def test_generated_mesh_then_another(asm):
    """the tables of an 8 x 6 mesh at (1, 1) do not survive into a 5 x 7 mesh at (2, 2)"""
    asm.generate_mesh(8, 6)
    tables(asm, 1, 1)
    asm.generate_mesh(5, 7)
    got = tables(asm, 2, 2)
    ref = fresh()
    ref.generate_mesh(5, 7)
    same(got, tables(ref, 2, 2))


def test_slab_after_whole_mesh(asm):
    """a slab after the whole mesh: its condensed tables are the slab's, and the assembler's CSR is still refused"""
    import proton_amd as pa
    asm.generate_mesh(6, 8)
    asm.assembler_csr_pattern(1, 1)
    asm.generate_mesh(6, 8, rows=(2, 5))
    info = asm.condensed_info(1, 1)
    got = list(asm.condensed_csr_pattern(1, 1))
    asm.synchronize()
    ref = fresh()
    ref.generate_mesh(6, 8, rows=(2, 5))
    want_info = ref.condensed_info(1, 1)
    for name, _ in type(info)._fields_:
        assert getattr(info, name) == getattr(want_info, name), name
    want = list(ref.condensed_csr_pattern(1, 1))
    ref.synchronize()
    same(got, want)
    with pytest.raises(pa.capi.ProtonAmdError, match="whole-mesh contexts only"):
        asm.assembler_csr_pattern(1, 1)


def test_set_faces_twice(asm, oracle):
    """pa_mesh_set_faces on the same uploaded 4 x 4 mesh with other Dirichlet flags: the tables follow the second flags"""
    N = 4
    mp, points, ptids = oracle.make_mesh(N, N)
    o = oracle.Assembler(mp, points, ptids, oracle.degrees(1, 1))
    left = (points[o.faces[:, 0].astype(np.int64), 0] == 0.0) & (points[o.faces[:, 1].astype(np.int64), 0] == 0.0)
    assert left.sum() == N and o.is_dir[left].all()
    first = o.is_dir.copy()
    first[left] = 0                                      # the left boundary open
    second = first.copy()
    second[np.flatnonzero(left)[0]] = 1                  # one more boundary face marked
    asm.set_mesh(points, ptids)
    asm.set_faces(o.cell_faces, o.faces, first)
    patterns(asm, 1, 1)
    asm.set_faces(o.cell_faces, o.faces, second)
    got = patterns(asm, 1, 1)
    ref = fresh()
    ref.set_mesh(points, ptids)
    ref.set_faces(o.cell_faces, o.faces, second)
    same(got, patterns(ref, 1, 1))


def test_cut_state_dropped_by_plain_mesh(asm):
    """a cut mesh and its interface tables, then a plain generated mesh"""
    asm.cut_preprocess(10)
    asm.interface_csr_pattern(1)
    asm.generate_mesh(8, 6)
    got = tables(asm, 1, 1)
    ref = fresh()
    ref.generate_mesh(8, 6)
    same(got, tables(ref, 1, 1))


def test_record_buffer_trim_and_grow(asm):
    """the record buffer given back (pa_context_trim) and allocated again, then grown for a larger record"""
    import torch
    asm.generate_mesh(16, 16)
    a = asm.local_ops(3, 2)["lc"]
    asm.synchronize()
    asm.ctx.trim()
    b = asm.local_ops(3, 2)["lc"]
    c = asm.local_ops(4, 3)["lc"]
    asm.synchronize()
    assert torch.equal(a, b)
    ref = fresh()
    ref.generate_mesh(16, 16)
    want = ref.local_ops(4, 3)["lc"]
    ref.synchronize()
    assert torch.equal(c, want)
