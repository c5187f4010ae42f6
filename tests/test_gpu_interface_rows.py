"""The interface problem's face-only system assembled, solved and recovered by row slabs (pa_interface_rows_*): every slab in its
own context, one after the other on the GPU, the real packed halo of the slab below handed to the next one.  The slabs stacked
are the whole-mesh pa_interface_condensed_* path BIT FOR BIT (records, rowptr / colind / values / rhs, recovered cell unknowns);
the rows solve (ranks = threads behind test_gpu_cg_rows.ThreadTransport) reproduces the whole-mesh solve."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from interface_helpers import condensed_sizes as sizes, real_ops
from test_gpu_cg_rows import ThreadTransport

pytestmark = pytest.mark.gpu

THIN = (0, 1, 5, 6, 12)          # slab (0, 1) without a cut cell; (5, 6) one cell row, cut faces on both of its boundaries
MESHES = {"circle-12-thin": (12, THIN, {}), "circle-12": (12, (0, 3, 8, 12), {}), "circle-20": (20, (0, 7, 20), {}),
          "line-12": (12, (0, 5, 6, 12), {"line_y": 0.43}), "circle-12-one-slab": (12, (0, 12), {})}


def new_asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


_whole = {}


def whole_mesh(N, k, kw=(), synthetic_seed=None):
    """the whole-mesh path, once per (mesh, degree): operators, Dirichlet data, records, the face-only CSR; never modified"""
    import torch
    key = (N, k, tuple(sorted(dict(kw).items())), synthetic_seed)
    if key in _whole:
        return _whole[key]
    a = new_asm()
    w = {"asm": a}
    if synthetic_seed is None:
        w["ops"], w["g"] = real_ops(a, N, k, **dict(kw))
        w["rec"] = a.interface_condensed_ops(k, w["ops"])
    else:                                               # as test_gpu_interface_condensed.synthetic_records
        a.cut_preprocess(N, **{"refsteps": 4, **dict(kw)})
        qi = a.ctx.interface_condensed_query(k)
        gen = torch.Generator(device=a.device).manual_seed(synthetic_seed)
        f64 = dict(dtype=torch.float64, device=a.device)
        w["rec"] = {"cond": torch.rand(a.ncells * qi.cond_doubles, generator=gen, **f64) - 0.5,
                    "cond_cut": torch.rand(max(a.ncut * qi.cond_cut_doubles, 1), generator=gen, **f64) - 0.5}
        Ny = dict(kw).get("Ny", N)
        w["g"] = (torch.rand((N * (Ny + 1) + (N + 1) * Ny) * (k + 1), generator=gen, **f64) - 0.5).reshape(-1, k + 1)
    w["rp"], w["ci"] = a.interface_condensed_csr_pattern(k)
    w["va"], w["RH"] = a.interface_condensed_csr_fill(k, w["rec"], w["g"])
    a.synchronize()
    assert a.ncut > 0
    w["cut_index"] = np.asarray(a.cut_index).copy()
    _whole[key] = w
    return w


def slices_of(w, N, k, rows, Ny=None):
    """the whole-mesh records and Dirichlet data of the slab `rows` of the N x Ny mesh (Ny = None: N x N): (records dict, g by the
    slab's own faces)"""
    import torch
    cbs, fbs, nf, NF = sizes(k)
    ntri, NTRI = nf * (nf + 1) // 2, NF * (NF + 1) // 2
    Ny = N if Ny is None else Ny
    n, ncut = N * Ny, int((w["cut_index"] >= 0).sum())
    c0, c1 = rows[0] * N, rows[1] * N
    k0, k1 = int((w["cut_index"][:c0] >= 0).sum()), int((w["cut_index"][:c1] >= 0).sum())
    cond, cc = w["rec"]["cond"], w["rec"]["cond_cut"]
    rec = {"cond": torch.cat([cond[c0 * ntri:c1 * ntri], cond[n * ntri + c0 * nf:n * ntri + c1 * nf]]),
           "cond_cut": torch.cat([cc[k0 * NTRI:k1 * NTRI], cc[ncut * NTRI + k0 * NF:ncut * NTRI + k1 * NF]])}
    frow = 2 * N + 1
    nfl = (rows[1] - rows[0]) * frow + (frow if rows[1] < Ny else N)
    g = w["g"].reshape(-1, fbs)[rows[0] * frow:rows[0] * frow + nfl].contiguous()
    return rec, g, (k0, k1)


def partition_info(a, N, k, rows, refsteps=4):
    """from the mesh parameters the assembler `a` was last preprocessed with (N: its Nx)"""
    from proton_amd import capi
    assert a.Nx == N
    return capi.interface_rows_partition_info(a.Nx, a.Ny, a.level_set, refsteps, rows, k, lo=a.lo, hi=a.hi)


def same_info(x, y):
    return all(getattr(x, f) == getattr(y, f) for f, _ in x._fields_)


def assemble_slabs(N, k, bounds, kw, w, synthetic):
    """every slab in its own BatchAssembler, bottom to top -> list of dict(asm, info, ops, g, rec, rp, ci, va, RH)"""
    out, halo = [], None
    Ny, refsteps = kw.get("Ny", N), kw.get("refsteps", 4)
    for rows in zip(bounds[:-1], bounds[1:]):
        a = new_asm()
        s = {"asm": a, "rows": rows}
        if synthetic:
            a.cut_preprocess(N, rows=rows, **{"refsteps": 4, **kw})
            s["rec"], s["g"], _ = slices_of(w, N, k, rows, Ny)
        else:
            s["ops"], s["g"] = real_ops(a, N, k, rows=rows, **kw)
            s["rec"] = a.interface_rows_ops(k, s["ops"])
        s["info"] = a.interface_rows_info(k)
        assert same_info(s["info"], partition_info(a, N, k, rows, refsteps))
        assert s["info"].halo_recv_doubles == (0 if halo is None else halo.numel())
        s["rp"], s["ci"] = a.interface_rows_csr_pattern(k)
        s["va"], s["RH"] = a.interface_rows_csr_fill(k, s["rec"], s["g"], halo_below=halo)
        halo = a.interface_rows_halo_pack(k, s["rec"], s["g"]).clone() if rows[1] < Ny else None
        a.synchronize()
        out.append(s)
    return out


def check_stacked(slabs, w):
    """the slabs' rows stacked are the whole-mesh system"""
    import torch
    rows = nnz = 0
    for s in slabs:
        i = s["info"]
        n, z = i.row_end - i.row_begin, i.nnz_owned
        assert i.row_begin == rows and s["rp"].numel() == n + 1 and int(s["rp"][0]) == 0 and int(s["rp"][-1]) == z
        assert torch.equal(s["rp"] + nnz, w["rp"][rows:rows + n + 1])
        assert torch.equal(s["ci"], w["ci"][nnz:nnz + z])
        assert torch.equal(s["va"], w["va"][nnz:nnz + z])
        assert torch.equal(s["RH"], w["RH"][rows:rows + n])
        rows, nnz = rows + n, nnz + z
    assert rows == w["RH"].numel() == slabs[0]["info"].system_size and nnz == w["va"].numel()


# ---- the chosen meshes ----------------------------------------------------------------------------------------------------
def test_the_chosen_meshes_hold_the_hard_cases():
    """N = 12, bounds (0, 1, 5, 6, 12): the slabs' cut cells partition the whole mesh's, slab (0, 1) has none, and cut horizontal faces
    lie on both boundaries of the one-row slab (5, 6): a face with two blocks whose two cut cells sit on different ranks"""
    from proton_amd import capi
    N = 12
    a = new_asm()
    ncut = a.cut_preprocess(N, refsteps=4)
    face_loc = np.zeros(2 * N * (N + 1), dtype=np.int8)
    assert capi.lib().pa_cut_query_tags(a.ctx.h, None, face_loc.ctypes.data, None) == 0
    for j in (5, 6):                                    # the horizontal faces of node row j: global ids j (2N + 1) + 2i
        assert np.any(face_loc[j * (2 * N + 1) + 2 * np.arange(N)] == capi.LOC_ON_INTERFACE), j
    counts = []
    for rows in zip(THIN[:-1], THIN[1:]):
        counts.append(a.cut_preprocess(N, refsteps=4, rows=rows))
    assert sum(counts) == ncut and counts[0] == 0 and all(c > 0 for c in counts[1:])
    # the line level set: every cell of row 5 is cut, its end cells on the Dirichlet boundary
    a.cut_preprocess(N, refsteps=4, rows=(5, 6), line_y=0.43)
    assert a.ncut == N and np.all(np.asarray(a.cut_index) >= 0)


# ---- the records ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_slab_records_equal_the_whole_mesh_rows(k):
    import torch
    N = 12
    w = whole_mesh(N, k)
    a = new_asm()
    for rows in zip(THIN[:-1], THIN[1:]):
        ops, _ = real_ops(a, N, k, rows=rows)
        rec = a.interface_rows_ops(k, ops)
        a.synchronize()
        ref, _, (k0, k1) = slices_of(w, N, k, rows)
        assert a.ncut == k1 - k0
        assert torch.equal(rec["cond"], ref["cond"]) and torch.equal(rec["cond_cut"], ref["cond_cut"])
        assert int(rec["info"].abs().sum()) == 0 and int(rec["info_cut"].abs().sum()) == 0


# ---- the system -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("k", [0, 1, 2])
def test_stacked_slabs_are_the_whole_mesh_system(mesh, k):
    """real operators; "one-slab": a whole-mesh context through the new entry points is pa_interface_condensed_csr_*"""
    N, bounds, kw = MESHES[mesh]
    w = whole_mesh(N, k, tuple(kw.items()))
    check_stacked(assemble_slabs(N, k, bounds, kw, w, synthetic=False), w)


@pytest.mark.parametrize("mesh", ["circle-12-thin", "line-12"])
def test_stacked_slabs_face_degree_3_synthetic(mesh):
    """seeded random records and Dirichlet data (the interface operators stop at face degree 2), every slab given its slices"""
    N, bounds, kw = MESHES[mesh]
    w = whole_mesh(N, 3, tuple(kw.items()), synthetic_seed=13)
    check_stacked(assemble_slabs(N, 3, bounds, kw, w, synthetic=True), w)


# ---- the solve ------------------------------------------------------------------------------------------------------------
def solve_by_ranks(slabs, b, tol):
    """pa_conjugated_gradient_rows, rank r = a thread with slab r's context -> [(result, x on the host)]"""
    import torch
    R = len(slabs)
    tt = ThreadTransport(R)
    out, keep = [None] * R, []

    def run(r):
        s, inf = slabs[r], slabs[r]["info"]
        tp, cbs = tt.make(r, s["asm"].ctx)
        keep.append(cbs)
        bs = b[inf.row_begin:inf.row_end].clone()
        x = torch.zeros_like(bs)
        try:
            res = s["asm"].ctx.conjugated_gradient_rows(tp, inf.row_begin, inf.row_end, s["rp"].data_ptr(), s["ci"].data_ptr(), s["va"].data_ptr(),
                                                        bs.data_ptr(), x.data_ptr(), tol=tol, max_iter=10000)
            s["asm"].synchronize()
            out[r] = (res, x.cpu())
        except BaseException as e:      # noqa: BLE001  (a failed rank must not leave the others at a barrier)
            out[r] = e
            tt.bar.abort()

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert all(not t.is_alive() for t in th)
    for o in out:
        assert not isinstance(o, BaseException), o
    return out


@pytest.mark.parametrize("bounds", [THIN, (0, 3, 8, 12)], ids=["thin", "three"])
@pytest.mark.parametrize("k", [1, 2])
def test_ranks_reproduce_the_whole_mesh_solve(k, bounds):
    """Every rank converges, all in the same iteration, within 3 of pa_conjugated_gradient's count (the dot products are grouped by
    rank).  The solution: within 10 e_ref of scipy's sparse direct solve of the whole-mesh system, e_ref the max-norm distance of the
    whole-mesh pa_conjugated_gradient solution (the path this one is modelled on) to it.  A seeded random vector is added to the
    right-hand side: the assembled one is close to an eigenvector of the preconditioned operator (test_gpu_cg_rows.py).
    Measured on an MI355X (tolerance 1e-11): e_ref 1.632e-11 at k = 1 (the ranks: 1.628e-11 and 1.629e-11 for the two sets of
    bounds, 157 iterations as the whole mesh), 1.986e-10 at k = 2 (the ranks: 1.987e-10 and 1.890e-10, 554 iterations against 553);
    MEASURED_E_REF below."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import torch
    N, tol = 12, 1e-11
    w = whole_mesh(N, k)
    a, n = w["asm"], w["RH"].numel()
    gen = torch.Generator().manual_seed(1234 + N + k)
    b = (w["RH"].cpu() + torch.rand(n, generator=gen, dtype=torch.float64) - 0.5).to(a.device)
    xw, reason, iters, _ = a.conjugated_gradient(w["rp"], w["ci"], w["va"], b, tol=tol, max_iter=10000)
    a.synchronize()
    assert reason == 0 and iters > 30
    A = sp.csr_matrix((w["va"].cpu().numpy(), w["ci"].cpu().numpy(), w["rp"].cpu().numpy()), shape=(n, n))
    direct = spla.spsolve(A.tocsc(), b.cpu().numpy())
    e_ref = float(np.abs(xw.cpu().numpy() - direct).max())
    slabs = assemble_slabs(N, k, bounds, {}, w, synthetic=False)
    out = solve_by_ranks(slabs, b, tol)
    assert all(o[0][0] == 0 for o in out)
    assert len({o[0][1] for o in out}) == 1
    assert abs(out[0][0][1] - iters) <= 3
    x = torch.cat([o[1] for o in out]).numpy()
    err = float(np.abs(x - direct).max())
    print("k %d bounds %s: e_ref %.3e, ranks %.3e, iterations %d / %d" % (k, bounds, e_ref, err, out[0][0][1], iters))
    assert x.size == n and e_ref > 0.0
    assert err <= 10.0 * e_ref


# test_ranks_reproduce_the_whole_mesh_solve as measured on an MI355X:
# (k, bounds) -> (e_ref, distance of the ranks' solution to the direct solve, iterations of the ranks / of the whole mesh)
MEASURED_E_REF = {(1, (0, 1, 5, 6, 12)): (1.632e-11, 1.628e-11, 157, 157), (1, (0, 3, 8, 12)): (1.632e-11, 1.629e-11, 157, 157),
                  (2, (0, 1, 5, 6, 12)): (1.986e-10, 1.987e-10, 554, 553), (2, (0, 3, 8, 12)): (1.986e-10, 1.890e-10, 554, 553)}


# ---- the recovery ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["circle-12-thin", "line-12", "circle-12-one-slab"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_recovered_cell_blocks_equal_the_whole_mesh(mesh, k):
    """the whole-mesh face solution sliced to each slab's [row_begin, col_end): the slab's cell blocks are the whole-mesh
    pa_interface_condensed_recover's, bit for bit.  On the line level set the whole-mesh Jacobi-PCG leaves at the reference's
    divergence test (exit reason 1 on the parent's path: the sin sin data with cut cells on the boundary), so a seeded random
    face vector stands in for the solution there: the recovery is the same arithmetic on any face vector."""
    import torch
    N, bounds, kw = MESHES[mesh]
    cbs = sizes(k)[0]
    w = whole_mesh(N, k, tuple(kw.items()))
    a = w["asm"]
    if "full" not in w:
        if kw:
            gen = torch.Generator().manual_seed(77 + k)
            w["xF"] = (torch.rand(w["RH"].numel(), generator=gen, dtype=torch.float64) - 0.5).to(a.device)
        else:
            w["xF"], reason, _, _ = a.conjugated_gradient(w["rp"], w["ci"], w["va"], w["RH"], tol=1e-9, max_iter=20 * w["RH"].numel())
            assert reason == 0
        w["full"] = a.interface_condensed_recover(k, w["ops"], w["xF"], w["g"]).clone()
        a.synchronize()
    s = new_asm()
    blocks = 0
    for rows in zip(bounds[:-1], bounds[1:]):
        ops, g = real_ops(s, N, k, rows=rows, **kw)
        i = s.interface_rows_info(k)
        assert i.cell_block_begin == blocks
        uT = s.interface_rows_recover(k, ops, w["xF"][i.row_begin:i.col_end].clone(), g)
        s.synchronize()
        assert torch.equal(uT, w["full"][i.cell_block_begin * cbs:i.cell_block_end * cbs])
        blocks = i.cell_block_end
    assert blocks * cbs + w["xF"].numel() == w["full"].numel()


# ---- end to end -----------------------------------------------------------------------------------------------------------
def energy_error(o, sol, N, k):
    """the energy-norm error of the full vector (cuthho_square.cpp:1762-1833), as test_condensed_path_reproduces_xlsx evaluates it"""
    msh = o.CutMesh(N, refsteps=4)
    di = o.degrees(k + 1, k)
    ct, ft, num_all_cells, num_other = msh.interface_tables()
    assert sol.size == di.cbs * num_all_cells + di.fbs * num_other
    L = o.lib()
    cbs, rd = di.cbs, di.rec_deg
    H1 = 0.0
    gx, gy, bar = np.zeros(32), np.zeros(32), np.zeros(2)
    for c in range(msh.nc):
        pts = np.ascontiguousarray(msh.points[msh.ptids[c].astype(np.int64)].reshape(8))
        L.hho_cell_barycenter(o._dp(pts), o._dp(bar))
        h = L.hho_cell_diameter(o._dp(pts))
        sides = (o.CUT_NEG, o.CUT_POS) if msh.cell_loc[c] == o.CUT_ON_INTERFACE else (int(msh.cell_loc[c]),)
        for where in sides:
            o0 = L.cut_interface_cell_offset(msh.h, di, c, o._i64p(ct), where)
            dofs = sol[o0:o0 + cbs]
            qx, qy, qw = msh.cell_quadrature(c, 2 * di.cell_deg, where)
            for q in range(len(qw)):
                L.hho_cell_basis_grad(o._dp(bar), h, rd, qx[q], qy[q], o._dp(gx), o._dp(gy))
                g0 = float(np.dot(dofs[1:], gx[1:cbs]))
                g1 = float(np.dot(dofs[1:], gy[1:cbs]))
                s0 = math.pi * math.cos(math.pi * qx[q]) * math.sin(math.pi * qy[q])
                s1 = math.pi * math.sin(math.pi * qx[q]) * math.cos(math.pi * qy[q])
                H1 += qw[q] * ((s0 - g0) ** 2 + (s1 - g1) ** 2)
    return math.sqrt(H1)


def test_slab_path_reproduces_xlsx(oracle):
    """N = 20, k = 1, two slabs: assembled by slabs, solved by ranks (threshold 1e-9, Jacobi), recovered by slabs; the energy error of
    the concatenated full vector against the xlsx Interface table, at test_condensed_path_reproduces_xlsx's tolerance"""
    import torch
    N, k, bounds, ref = 20, 1, (0, 7, 20), 5.22389e-3
    w = whole_mesh(N, k)
    slabs = assemble_slabs(N, k, bounds, {}, w, synthetic=False)
    out = solve_by_ranks(slabs, w["RH"], 1e-9)
    assert all(o[0][0] == 0 for o in out)
    xF = torch.cat([o[1] for o in out])
    assert xF.numel() == slabs[0]["info"].system_size
    cells = []
    for s in slabs:
        i, a = s["info"], s["asm"]
        cells.append(a.interface_rows_recover(k, s["ops"], xF[i.row_begin:i.col_end].to(a.device), s["g"]).cpu())
        a.synchronize()
    sol = torch.cat(cells + [xF]).numpy()
    err = energy_error(oracle, sol, N, k)
    assert abs(err - ref) / ref < 6e-6, err


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_rows_refusals():
    """face degree, no cut mesh, (system size,) the cut-cell arrays, the halo -- in this order; the whole-mesh entry points keep
    refusing the slab afterwards"""
    import torch
    from proton_amd import capi
    L = capi.lib()
    out = capi.InterfaceRowsInfo()
    cout = capi.InterfaceCondensedInfo()
    a = new_asm()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=a.device)
    sink = torch.zeros(1 << 16, dtype=torch.float64, device=a.device)
    p, q = buf.data_ptr(), sink.data_ptr()

    def calls(h, fd, cut=p, halo=p):
        return [L.pa_interface_rows_query(h, fd, C.byref(out)),
                L.pa_interface_rows_ops_batch(h, fd, p, None, cut, None, p, cut, None, None),
                L.pa_interface_rows_halo_pack(h, fd, p, cut, None, p),
                L.pa_interface_rows_csr_pattern(h, fd, q, None),
                L.pa_interface_rows_csr_fill(h, fd, p, cut, None, halo, q, None),
                L.pa_interface_rows_recover(h, fd, p, None, cut, None, None, p, p)]
    assert calls(a.ctx.h, 1) == [5] * 6                          # no mesh
    assert calls(a.ctx.h, 4) == [2] * 6                          # the face degree comes first
    a.generate_mesh(8, 8)
    assert calls(a.ctx.h, 1) == [5] * 6                          # a plain mesh, no cut mesh
    a.cut_preprocess(12, rows=(5, 6))
    assert a.ncut > 0
    for fd in (-1, 4):
        assert calls(a.ctx.h, fd, cut=None, halo=None) == [2] * 6
    # the cut-cell arrays before the halo: query and pattern need neither
    assert calls(a.ctx.h, 1, cut=None, halo=None) == [0, 1, 1, 0, 1, 1]
    assert "cut-cell arrays" in L.pa_last_error(a.ctx.h).decode()
    assert L.pa_interface_rows_csr_fill(a.ctx.h, 1, p, p, None, None, p, None) == 1
    assert "d_halo_below" in L.pa_last_error(a.ctx.h).decode()
    assert L.pa_interface_rows_query(a.ctx.h, 1, None) == 1 and L.pa_interface_rows_csr_pattern(a.ctx.h, 1, None, None) == 1
    assert L.pa_interface_rows_csr_fill(a.ctx.h, 1, None, p, None, p, p, None) == 1
    assert L.pa_interface_rows_csr_fill(a.ctx.h, 1, p, p, None, p, None, None) == 1
    # slab 0 needs no halo, a slab without cut cells no cut-cell arrays
    a.cut_preprocess(12, rows=(0, 1))
    assert a.ncut == 0
    assert L.pa_interface_rows_csr_fill(a.ctx.h, 1, p, None, None, None, q, None) == 0
    a.synchronize()
    # the new entry points have run on this slab: the whole-mesh ones still refuse it
    a.cut_preprocess(12, rows=(3, 8))
    assert L.pa_interface_rows_query(a.ctx.h, 1, C.byref(out)) == 0 and out.row_end > out.row_begin > 0
    assert L.pa_interface_condensed_query(a.ctx.h, 1, C.byref(cout)) == 1
    assert "whole mesh" in L.pa_last_error(a.ctx.h).decode()
    assert L.pa_interface_condensed_csr_pattern(a.ctx.h, 1, p, None) == 1
    assert L.pa_interface_csr_pattern(a.ctx.h, 1, p, None) == 1
    assert L.pa_interface_condensed_recover(a.ctx.h, 1, p, None, p, None, None, p, p) == 1
