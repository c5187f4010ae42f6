"""The Galerkin coarse level and the two-level conjugate gradient (proton_amd/csrc/coarse_precond.hip) on the device:
pa_condensed_coarse bit for bit against the table of tests/coarse_twin.py, pa_coarse_precond_factor / _apply and every iterate of
pa_conjugated_gradient_patch_coarse against the twin (gate max(2^-45, 10 e_ref), all of it measured on the CPU:
tests/test_coarse_pcg_cpu.py), the contract of the entry points, and the Poisson and fictitious-domain solves end to end.  One run:
profiles/coarse_pcg_parity.txt (COARSE_PCG_PROFILE=that file python -m pytest tests/test_gpu_coarse_pcg.py -m gpu -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import cg_twin as T
import coarse_twin as CT
import patch_pcg_twin as PT

pytestmark = pytest.mark.gpu

REPORT = []


def say(line):
    print(line)
    REPORT.append(line)


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def _dev(a, v):
    import torch
    return torch.tensor(np.ascontiguousarray(v)).to(a.device)


def _upload(a, case):
    """-> (rowptr, colind, values, b), (patch_ptr, patch_rows), (p_ptr, p_cols, p_vals, ncoarse) on the device"""
    sy, pt, tb = PT.system(CT.base(case)), PT.patches(CT.base(case)), CT.coarse(case)
    return ((_dev(a, sy.rowptr), _dev(a, sy.colind), _dev(a, sy.values), _dev(a, sy.b)), (_dev(a, pt.ptr), _dev(a, pt.rows)),
            _table(a, tb))


def _table(a, tb):
    return (_dev(a, tb.ptr.astype(np.int64)), _dev(a, tb.cols.astype(np.int32)), _dev(a, tb.vals.astype(np.float64)), tb.ncoarse)


# ---- 1. the table builder ---------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    ptr, cols, vals, nc = got
    assert nc == want.ncoarse, what
    ptr, cols, vals = ptr.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
    assert ptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64
    assert np.array_equal(ptr, want.ptr), what
    assert np.array_equal(cols, want.cols), what
    assert np.array_equal(vals.view(np.int64), want.vals.view(np.int64)), what              # bit for bit


@pytest.mark.parametrize("Nx,Ny,H", [(4, 4, 2), (8, 8, 4), (12, 8, 4), (7, 5, 3), (6, 6, 1)])
def test_condensed_coarse_against_the_twin(asm, oracle, Nx, Ny, H):
    """k = 0..3, one part, bit for bit; the same table after the points have moved"""
    asm.generate_mesh(Nx, Ny)
    mp, points, ptids = oracle.make_mesh(Nx, Ny)
    for k in range(4):
        o = oracle.Assembler(mp, points, ptids, oracle.degrees(k + 1, k))
        want = CT.table(Nx, Ny, H, k + 1, o.compress, o.faces, o.num_other)
        got = asm.condensed_coarse(k + 1, k, H)
        asm.synchronize()
        _same(got, want, (Nx, Ny, H, k))
        assert np.diff(want.ptr).max() <= CT.MAX_ROW
    moved = points.copy()
    ij = np.arange(points.shape[0])
    interior = (ij % (Nx + 1) > 0) & (ij % (Nx + 1) < Nx) & (ij // (Nx + 1) > 0) & (ij // (Nx + 1) < Ny)
    moved[interior] += np.random.default_rng(3).uniform(-0.2 / max(Nx, Ny), 0.2 / max(Nx, Ny), size=points.shape)[interior]
    d = _dev(asm, moved)
    asm.ctx.mesh_set_points(d.data_ptr(), moved.shape[0])
    _same(asm.condensed_coarse(3, 2, H), CT.table(Nx, Ny, H, 3, o.compress, o.faces, o.num_other), "moved points")
    asm.synchronize()


@pytest.mark.parametrize("N,kw", [(16, {}), (20, {}), (12, dict(line_y=0.47))], ids=["circle16", "circle20", "line12"])
def test_condensed_coarse_by_side_against_the_twin(asm, oracle, N, kw):
    """by side of the circle and of the line level set, both values of `where`, H = 2 and 4, k = 0 and 2"""
    asm.cut_preprocess(N, refsteps=4 if not kw else 3, **kw)
    msh = oracle.CutMesh(N, refsteps=4 if not kw else 3, **kw)
    for k in (0, 2):
        o = oracle.Assembler(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, oracle.degrees(k + 1, k))
        for H in (2, 4):
            for where in (0, 1):
                want = CT.table(N, N, H, k + 1, o.compress, o.faces, o.num_other, msh.face_loc, where)
                got = asm.condensed_coarse(k + 1, k, H, "side", where)
                asm.synchronize()
                _same(got, want, (N, k, H, where))
                one = CT.table(N, N, H, k + 1, o.compress, o.faces, o.num_other)
                assert want.ncoarse > one.ncoarse                 # some hat is split


def test_condensed_coarse_refusals(asm):
    """2 x 2 with H = 2 (no interior node), too many columns, a slab, by side without the cut preprocessing, bad arguments: nothing
    is written"""
    import torch
    from proton_amd import capi
    from proton_amd.batch import BatchAssembler
    L = capi.lib()
    di, _ = capi.degree_info(3, 2)
    ptr = torch.full((8192,), -5, dtype=torch.int64, device=asm.device)
    cols = torch.full((8192,), -7, dtype=torch.int32, device=asm.device)
    vals = torch.full((8192,), 2.5, dtype=torch.float64, device=asm.device)
    a, b = C.c_size_t(0), C.c_size_t(0)
    p = lambda t: t.data_ptr()
    asm.generate_mesh(2, 2)
    assert L.pa_condensed_coarse(asm.ctx.h, di, 2, capi.COARSE_ONE, 0, p(ptr), p(cols), p(vals)) == 1
    text = L.pa_last_error(asm.ctx.h).decode()
    assert "H = 2" in text and " 0 coarse" in text, text
    assert L.pa_condensed_coarse_query(asm.ctx.h, di, 2, capi.COARSE_ONE, 0, C.byref(a), C.byref(b)) == 1
    asm.generate_mesh(80, 80)
    assert L.pa_condensed_coarse_query(asm.ctx.h, di, 1, capi.COARSE_ONE, 0, C.byref(a), C.byref(b)) == 1
    assert "6241" in L.pa_last_error(asm.ctx.h).decode()
    asm.generate_mesh(8, 8)
    assert L.pa_condensed_coarse(asm.ctx.h, di, 4, capi.COARSE_BY_SIDE, 0, p(ptr), p(cols), p(vals)) == 5          # PA_ERR_NO_MESH
    assert L.pa_condensed_coarse(asm.ctx.h, di, 0, capi.COARSE_ONE, 0, p(ptr), p(cols), p(vals)) == 1
    assert L.pa_condensed_coarse(asm.ctx.h, di, 4, 2, 0, p(ptr), p(cols), p(vals)) == 1
    assert L.pa_condensed_coarse(asm.ctx.h, di, 4, capi.COARSE_ONE, 0, None, p(cols), p(vals)) == 1
    slab = BatchAssembler(0)
    slab.generate_mesh(8, 8, rows=(2, 6))
    assert L.pa_condensed_coarse(slab.ctx.h, di, 4, capi.COARSE_ONE, 0, p(ptr), p(cols), p(vals)) == 1
    assert b"whole-mesh" in L.pa_last_error(slab.ctx.h)
    assert L.pa_condensed_coarse_query(slab.ctx.h, di, 4, capi.COARSE_ONE, 0, C.byref(a), C.byref(b)) == 1
    slab.synchronize(); asm.synchronize()
    assert bool((ptr == -5).all()) and bool((cols == -7).all()) and bool((vals == 2.5).all())


# ---- 2. factor + apply against the twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CT.case_table(), ids=CT.case_id)
def test_factor_and_apply(asm, case):
    """A_c exactly symmetric and at the gate; z of both test vectors, with and without accumulate, at the gate; two calls and two
    factors give the same bits; r is read only"""
    import torch
    dv, dp, dc = _upload(asm, case)
    pre = asm.coarse_precond_factor(dv[0], dv[1], dv[2], dc, want_matrix=True)
    asm.synchronize()
    assert pre["pivot"] == 0
    assert pre["sizes"].factor_doubles == case.ncoarse * (case.ncoarse + 1) // 2 and pre["sizes"].entries == CT.coarse(case).ptr[-1]
    Ac = pre["matrix"].cpu().numpy()
    assert np.array_equal(Ac, Ac.T)
    gm = CT.gate(CT.matrix_e_ref(case))
    em = CT.matrix_error(case, Ac)
    say("matrix %-12s e_gpu %.3e e_ref %.3e gate %.3e ratio %.3f" % (CT.case_id(case), em, CT.matrix_e_ref(case), gm, em / gm))
    assert em <= gm
    g = CT.gate(CT.apply_e_ref(case))
    for w in (0, 1):
        r = _dev(asm, CT.test_vectors(case)[w])
        keep = r.clone()
        for acc in (False, True):
            z0 = _dev(asm, CT.test_vectors(case)[1 - w]) if acc else torch.full_like(r, float("nan"))
            z = asm.coarse_precond_apply(pre, r, z0.clone(), accumulate=acc)
            z2 = asm.coarse_precond_apply(pre, r, z0.clone(), accumulate=acc)
            asm.synchronize()
            assert torch.equal(z, z2) and torch.equal(r, keep)
            e = CT.scaled_error(case, z.cpu().numpy(), CT.apply_truth(case, w, acc))
            say("apply  %-12s vector %d accumulate %d: e_gpu %.3e e_ref %.3e gate %.3e ratio %.3f" %
                (CT.case_id(case), w, acc, e, CT.apply_e_ref(case), g, e / g))
            assert e <= g
    pre2 = asm.coarse_precond_factor(dv[0], dv[1], dv[2], dc, want_matrix=True)
    asm.synchronize()
    assert torch.equal(pre["factor"], pre2["factor"]) and torch.equal(pre["matrix"], pre2["matrix"]) and torch.equal(pre["pt"], pre2["pt"])


def test_not_spd_is_reported_with_its_pivot(asm):
    """a P with an empty column j: pivot j + 1; -A: pivot 1; the solver says PA_ERR_NOT_SPD before the first iteration, x untouched"""
    import torch
    from proton_amd import capi
    case = CT.Case(257, 33)
    dv, dp, dc = _upload(asm, case)
    tb = CT.coarse(case)
    j = 17
    keep = tb.cols != j
    sizes = np.bincount(np.repeat(np.arange(case.n), np.diff(tb.ptr))[keep], minlength=case.n)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    hole = _table(asm, CT.Table(ptr, tb.cols[keep], tb.vals[keep], tb.ncoarse))
    pre = asm.coarse_precond_factor(dv[0], dv[1], dv[2], hole)
    assert pre["pivot"] == j + 1
    neg = asm.coarse_precond_factor(dv[0], dv[1], -dv[2], dc)
    assert neg["pivot"] == 1
    x = torch.full_like(dv[3], 7.0)
    with pytest.raises(capi.ProtonAmdError) as e:
        asm.conjugated_gradient_patch_coarse(dv[0], dv[1], dv[2], dv[3], dp, hole, x=x)
    asm.synchronize()
    assert e.value.status == 6 and bool((x == 7.0).all())


# ---- 3. the solver, iterate by iterate --------------------------------------------------------------------------------------------
def _pcg(a, dv, dp, dc, x=None, **kw):
    import torch
    if x is None:
        x = torch.full_like(dv[3], float("nan"))
    x, reason, iters, rr = a.conjugated_gradient_patch_coarse(dv[0], dv[1], dv[2], dv[3], dp, dc, x=x, **kw)
    a.synchronize()
    return x.cpu().numpy(), reason, iters, rr


@pytest.mark.parametrize("case", CT.case_table(), ids=CT.case_id)
def test_every_iterate(asm, case):
    """x_m, the reported residual, the exit reason and the count for m = 1..8 against the twin"""
    sy = PT.system(CT.base(case))
    dv, dp, dc = _upload(asm, case)
    tr, er = CT.truth(case), CT.e_ref(case)
    assert CT.judged(case) == list(range(1, len(tr.rr) + 1))
    for m in range(1, len(tr.rr) + 1):
        kw, want = CT.iterate_call(case, m)
        x, reason, iters, rr = _pcg(asm, dv, dp, dc, **kw)
        assert (reason, iters) == want, (m, reason, iters, want)
        g = CT.gate(er[m - 1])
        e = T.scaled_error(x, tr.x[m - 1], sy.diag)
        t = tr.rr[m - 1]
        drr = abs(rr - t) / t if t >= T.EXACT else rr
        say("pcg    %-12s m %d: e_gpu %.3e rr %.3e e_ref %.3e gate %.3e ratio %.3f" % (CT.case_id(case), m, e, drr, er[m - 1], g, max(e, drr) / g))
        assert e <= g and drr <= g


def test_contract_of_the_solver(asm):
    """x is the only output, the inputs are read only, two calls give the same bits whatever x held; the max_iter and the divergence
    exits; n = 0 and b = 0 as pa_conjugated_gradient has them"""
    import torch
    case = CT.Case(257, 33)
    dv, dp, dc = _upload(asm, case)
    keep = [t.clone() for t in dv + dp + dc[:3]]
    kw = dict(tol=0.0, div=T.HUGE, max_iter=5)
    x0, *s0 = _pcg(asm, dv, dp, dc, **kw)
    x1, *s1 = _pcg(asm, dv, dp, dc, **kw)
    x2, *s2 = _pcg(asm, dv, dp, dc, x=torch.full_like(dv[3], 1e300), **kw)
    assert s0 == s1 == s2 and s0[:2] == [2, 6] and np.isfinite(x0).all()                   # 2: max_iter
    assert np.array_equal(x0, x1) and np.array_equal(x0, x2)
    xd, reason, iters, _ = _pcg(asm, dv, dp, dc, tol=0.0, div=0.0, max_iter=1000)
    assert (reason, iters) == CT.iterate_call(case, 1)[1] == (1, 0)                        # 1: the divergence exit
    assert all(torch.equal(a, b) for a, b in zip(keep, dv + dp + dc[:3]))
    x = torch.full((4,), 7.0, dtype=torch.float64, device=asm.device)
    res = asm.ctx.conjugated_gradient_patch_coarse(0, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), x.data_ptr(), 0,
                                                   dp[0].data_ptr(), dp[1].data_ptr(), 33, dc[0].data_ptr(), dc[1].data_ptr(), dc[2].data_ptr())
    asm.synchronize()
    assert tuple(res) == (0, 0, 0.0) and bool((x == 7.0).all())
    xz, *sz = _pcg(asm, (dv[0], dv[1], dv[2], torch.zeros_like(dv[3])), dp, dc, tol=1e-9, div=100.0, max_iter=1000)
    assert sz == [0, 0, 0.0] and (xz == 0.0).all()


def _bad_tables(tb):
    """(name, ptr, cols, vals, ncoarse, word of pa_last_error) for every refusal of the validation"""
    out = []
    big = int(np.nonzero(np.diff(tb.ptr) >= 2)[0][0])
    ptr = tb.ptr.copy(); ptr[1:] += 5 - int(np.diff(tb.ptr)[0])
    out.append(("a 5-entry row", ptr, np.concatenate([np.arange(5), tb.cols[tb.ptr[1]:]]).astype(np.int32),
                np.concatenate([np.ones(5), tb.vals[tb.ptr[1]:]]), tb.ncoarse, "0 to 4"))
    c = tb.cols.copy(); c[tb.ptr[big + 1] - 1] = tb.ncoarse
    out.append(("column = ncoarse", tb.ptr, c, tb.vals, tb.ncoarse, "outside"))
    c = tb.cols.copy(); c[tb.ptr[big]] = -1
    out.append(("column < 0", tb.ptr, c, tb.vals, tb.ncoarse, "outside"))
    c = tb.cols.copy(); c[tb.ptr[big]], c[tb.ptr[big] + 1] = c[tb.ptr[big] + 1], c[tb.ptr[big]]
    out.append(("descending columns", tb.ptr, c, tb.vals, tb.ncoarse, "ascend"))
    c = tb.cols.copy(); c[tb.ptr[big] + 1] = c[tb.ptr[big]]
    out.append(("repeated column", tb.ptr, c, tb.vals, tb.ncoarse, "ascend"))
    v = tb.vals.copy(); v[7] = np.nan
    out.append(("a NaN", tb.ptr, tb.cols, v, tb.ncoarse, "finite"))
    v = tb.vals.copy(); v[9] = np.inf
    out.append(("an infinity", tb.ptr, tb.cols, v, tb.ncoarse, "finite"))
    out.append(("ncoarse 0", tb.ptr, tb.cols, tb.vals, 0, "1 to 4096"))
    out.append(("ncoarse 4097", tb.ptr, tb.cols, tb.vals, 4097, "1 to 4096"))
    out.append(("ptr[0] != 0", tb.ptr + 1, np.concatenate([[0], tb.cols]).astype(np.int32), np.concatenate([[1.0], tb.vals]), tb.ncoarse,
                "start at 0"))
    return out


def test_refusals_touch_no_output(asm):
    """every refusal of the table validation: PA_ERR_INVALID_ARG with text; x, the transpose, the factor, the coarse matrix untouched; a
    bad patch table is named before a bad coarse table"""
    import torch
    from proton_amd import capi
    L = capi.lib()
    case = CT.Case(257, 33)
    tb = CT.coarse(case)
    dv, dp, dc = _upload(asm, case)
    n = case.n
    sz = asm.ctx.coarse_precond_query(n, tb.ncoarse, dc[0].data_ptr())
    x = torch.full_like(dv[3], 7.0)
    ptb = torch.full((int(sz.pt_bytes) + 4096,), 3, dtype=torch.uint8, device=asm.device)
    factor = torch.full((int(sz.factor_doubles) + 4096,), 1.5, dtype=torch.float64, device=asm.device)
    matrix = torch.full((4097 * 8,), 2.5, dtype=torch.float64, device=asm.device)
    scratch = torch.zeros(int(sz.scratch_bytes) + (1 << 20), dtype=torch.uint8, device=asm.device)
    z = torch.full_like(dv[3], 4.0)
    p = lambda t: t.data_ptr()
    for name, ptr, cols, vals, nc, word in _bad_tables(tb):
        d = (_dev(asm, ptr.astype(np.int64)), _dev(asm, cols.astype(np.int32)), _dev(asm, vals.astype(np.float64)))
        st = L.pa_conjugated_gradient_patch_coarse(asm.ctx.h, n, p(dv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(x), dp[0].numel() - 1, p(dp[0]), p(dp[1]),
                                                   nc, p(d[0]), p(d[1]), p(d[2]), 1e-9, 100.0, 10, None, None, None)
        text = L.pa_last_error(asm.ctx.h).decode()
        assert st == 1 and word in text, (name, st, text)
        st = L.pa_coarse_precond_factor(asm.ctx.h, n, p(dv[0]), p(dv[1]), p(dv[2]), nc, p(d[0]), p(d[1]), p(d[2]), p(ptb), p(factor), p(scratch),
                                        p(matrix), None)
        assert st == 1 and word in L.pa_last_error(asm.ctx.h).decode(), (name, st)
        if nc != tb.ncoarse or "ptr" in name or "5-entry" in name:        # what the query itself refuses, the apply refuses too
            assert L.pa_coarse_precond_apply(asm.ctx.h, n, nc, p(d[0]), p(d[1]), p(d[2]), p(ptb), p(factor), p(scratch), 0, p(dv[3]), p(z)) == 1
        asm.synchronize()
        assert bool((x == 7.0).all()) and bool((ptb == 3).all()) and bool((factor == 1.5).all()) and bool((matrix == 2.5).all()), name
        assert bool((z == 4.0).all()), name
    # both tables bad: the patch table's refusal comes first
    bad = _bad_tables(tb)[1]
    d = (_dev(asm, bad[1].astype(np.int64)), _dev(asm, bad[2].astype(np.int32)), _dev(asm, bad[3]))
    rows = dp[1].clone(); rows[5] = n
    st = L.pa_conjugated_gradient_patch_coarse(asm.ctx.h, n, p(dv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(x), dp[0].numel() - 1, p(dp[0]), p(rows),
                                               bad[4], p(d[0]), p(d[1]), p(d[2]), 1e-9, 100.0, 10, None, None, None)
    assert st == 1 and "patch table" in L.pa_last_error(asm.ctx.h).decode()
    # NULL pointers
    assert L.pa_conjugated_gradient_patch_coarse(asm.ctx.h, n, p(dv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(x), dp[0].numel() - 1, p(dp[0]), p(dp[1]),
                                                 tb.ncoarse, None, p(dc[1]), p(dc[2]), 1e-9, 100.0, 10, None, None, None) == 1
    assert L.pa_coarse_precond_factor(asm.ctx.h, n, p(dv[0]), p(dv[1]), p(dv[2]), tb.ncoarse, p(dc[0]), p(dc[1]), p(dc[2]), None, p(factor),
                                      p(scratch), None, None) == 1
    asm.synchronize()
    assert bool((x == 7.0).all()) and bool((factor == 1.5).all())


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def _poisson(asm, N, cd, fd, points=None):
    import proton_amd as pa
    asm.generate_mesh(N, N)
    if points is not None:
        d = _dev(asm, points)
        asm.ctx.mesh_set_points(d.data_ptr(), points.shape[0])
        asm.synchronize()
    rhs = asm.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS, pa.QUAD_TENSOR)
    g = asm.dirichlet_data(fd, pa.capi.FN_SIN_SIN_SOL)
    return asm.condensed_ops(cd, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, rhs=rhs), g


def _spsolve(asm, cd, fd, rec, g):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    rowptr, colind = asm.condensed_csr_pattern(cd, fd)
    values, b = asm.condensed_csr_fill(cd, fd, rec, g)
    asm.synchronize()
    n = b.numel()
    A = sp.csr_matrix((values.cpu().numpy(), colind.cpu().numpy(), rowptr.cpu().numpy()), shape=(n, n))
    return spla.spsolve(A.tocsc(), b.cpu().numpy())


POISSON_COUNTS = {}


@pytest.mark.parametrize("N", [32, 64])
def test_poisson_condensed_solve_with_the_coarse_level(asm, N):
    """condensed_solve(patches = "cell", coarse = 4) at k = 2 to 1e-13: x_F against spsolve of the downloaded CSR within 1e-8 of its
    largest entry; coarse = None gives the bits of the call without the keyword.  The two count conditions are the issue's, in the
    set-up they were measured in -- the same matrix with a random right-hand side (seed 1), x_0 = 0, 1e-13: at 64 count <= cell
    patches / 3, and count at 64 <= 1.15 x count at 32 (measured on the device: 142 -> 58 and 281 -> 59; the CPU twin on the oracle's
    system: 143 -> 59 and 282 -> 60).
    With the smooth right-hand side of sin(pi x) sin(pi y) the patches alone need fewer iterations and the gain is smaller: 65 -> 40 at
    32, 115 -> 41 at 64 (2.8 x); those counts are printed, the count at 64 is held to 1.15 x the count at 32 as well."""
    import torch
    rec, g = _poisson(asm, N, 3, 2)
    ref = _spsolve(asm, 3, 2, rec, g)
    xp, reason, ip, _ = asm.condensed_solve(3, 2, rec, g, tol=1e-13, patches="cell")
    xn, _, inone, _ = asm.condensed_solve(3, 2, rec, g, tol=1e-13, patches="cell", coarse=None)
    xc, reason_c, ic, _ = asm.condensed_solve(3, 2, rec, g, tol=1e-13, patches="cell", coarse=4)
    asm.synchronize()
    assert reason == 0 and reason_c == 0 and torch.equal(xp, xn) and ip == inone
    err = np.abs(xc.cpu().numpy() - ref).max() / np.abs(ref).max()
    say("poisson %d^2 k = 2: cell patches %d, + coarse H = 4 %d iterations; against spsolve %.3e of max|ref|" % (N, ip, ic, err))
    assert err <= 1e-8
    rowptr, colind = asm.condensed_csr_pattern(3, 2)
    values, b = asm.condensed_csr_fill(3, 2, rec, g)
    br = _dev(asm, np.random.default_rng(1).standard_normal(b.numel()))
    cell, tb = asm.condensed_patches(3, 2, "cell"), asm.condensed_coarse(3, 2, 4)
    _, r0, i0, _ = asm.conjugated_gradient_patch(rowptr, colind, values, br, cell, tol=1e-13, max_iter=4 * b.numel())
    _, r1, i1, _ = asm.conjugated_gradient_patch_coarse(rowptr, colind, values, br, cell, tb, tol=1e-13, max_iter=4 * b.numel())
    asm.synchronize()
    say("poisson %d^2 k = 2, random right-hand side: cell patches %d, + coarse H = 4 %d iterations" % (N, i0, i1))
    assert r0 == 0 and r1 == 0
    POISSON_COUNTS[N] = (i1, ic)
    if N == 64:
        assert 3 * i1 <= i0
        assert 32 in POISSON_COUNTS and i1 <= 1.15 * POISSON_COUNTS[32][0] and ic <= 1.15 * POISSON_COUNTS[32][1]
    with pytest.raises(ValueError):
        asm.condensed_solve(3, 2, rec, g, coarse=4)


def test_poisson_on_general_quadrilaterals(asm, oracle):
    """16 x 16 general quadrilaterals (the generated mesh with its interior points moved), k = 3: the two-level solve against spsolve
    of the downloaded CSR within 1e-8 of its largest entry"""
    N, cd, fd = 16, 4, 3
    mp, points, ptids = oracle.make_mesh(N, N)
    ij = np.arange(points.shape[0])
    interior = (ij % (N + 1) > 0) & (ij % (N + 1) < N) & (ij // (N + 1) > 0) & (ij // (N + 1) < N)
    points[interior] += np.random.default_rng(11).uniform(-0.2 / N, 0.2 / N, size=points.shape)[interior]
    rec, g = _poisson(asm, N, cd, fd, points)
    ref = _spsolve(asm, cd, fd, rec, g)
    xp, _, ip, _ = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches="cell")
    xc, reason, ic, _ = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches="cell", coarse=4)
    asm.synchronize()
    err = np.abs(xc.cpu().numpy() - ref).max() / np.abs(ref).max()
    say("poisson 16^2 general quadrilaterals k = 3: cell patches %d, + coarse H = 4 %d iterations; against spsolve %.3e" % (ip, ic, err))
    assert reason == 0 and err <= 1e-8 and ic < ip
    asm.generate_mesh(4, 4)                          # leave a generated mesh behind


@pytest.mark.parametrize("N", [32, 64])
def test_fictdom_condensed_solve_with_the_coarse_level(asm, oracle, N):
    """fictdom_condensed_solve(patches = "cell", coarse = 4) at k = 2 to 1e-13: the recovered vector against spsolve of the full system
    within 1e-8 max|ref| (the tolerance of the patch solves); coarse = None gives the bits of the call without the keyword; at 64:
    by side <= cell patches / 1.5 and by side <= one part; at 32 the energy error against the patch solve's (the xlsx has no row for
    N = 32: tests/test_gpu_patch_pcg.py checks the xlsx value at N = 20, which is checked here too)"""
    import scipy.sparse.linalg as spla
    import torch

    import test_gpu_fictdom_condensed as F
    k = 2
    asm.cut_preprocess(N, refsteps=4)
    op = F.operators(asm, k, F.NEG)
    K, b, _ = F.full_system(asm, k, F.NEG, op)
    ref = spla.spsolve(K.tocsc(), b)
    fp, ip, rp = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell")
    fn, inone, _ = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell", coarse=None)
    fc, ic, rc = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell", coarse=4)
    asm.synchronize()
    assert rp == 0 and rc == 0 and torch.equal(fp, fn) and ip == inone
    err = np.abs(fc.cpu().numpy() - ref).max() / np.abs(ref).max()
    say("fictdom (%d, 2): cell patches %d, + coarse H = 4 by side %d iterations; against spsolve %.3e of max|ref|" % (N, ip, ic, err))
    assert err <= 1e-8
    if N == 64:
        # one part, through the generic entry on the same system
        rec = F.records(asm, k, F.NEG, op)
        rowptr, colind = asm.condensed_csr_pattern(k + 1, k)
        values, bF = asm.condensed_csr_fill(k + 1, k, rec["cond"], op["g"])
        _, r1, i1, _ = asm.conjugated_gradient_patch_coarse(rowptr, colind, values, bF, asm.condensed_patches(k + 1, k, "cell"),
                                                            asm.condensed_coarse(k + 1, k, 4, "one"), tol=F.CG_TOL, max_iter=4 * bF.numel())
        asm.synchronize()
        say("fictdom (64, 2): + coarse H = 4 one part %d iterations" % i1)
        assert r1 == 0 and 1.5 * ic <= ip and ic <= i1


def test_fictdom_energy_error_with_the_coarse_level(asm, oracle):
    """the energy error of the two-level solve at (20, 2) against cuthho.xlsx, and at (32, 2) against the patch solve's"""
    import test_gpu_fictdom_condensed as F
    k = 2
    asm.cut_preprocess(20, refsteps=4)
    full, _, reason = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell", coarse=4)
    asm.synchronize()
    e = F.energy_error(oracle, oracle.CutMesh(20, refsteps=4), k, full.cpu().numpy())
    say("fictdom (20, 2) + coarse: energy error %.10e (xlsx %.6e)" % (e, F.XLSX[(k, 20)]))
    assert reason == 0 and abs(e - F.XLSX[(k, 20)]) / F.XLSX[(k, 20)] < 6e-6
    asm.cut_preprocess(32, refsteps=4)
    msh = oracle.CutMesh(32, refsteps=4)
    fp, _, _ = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell")
    fc, _, _ = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell", coarse=4)
    asm.synchronize()
    ep, ec = (F.energy_error(oracle, msh, k, f.cpu().numpy()) for f in (fp, fc))
    say("fictdom (32, 2): energy error %.10e with the coarse level, %.10e with the patches alone" % (ec, ep))
    assert abs(ec - ep) / ep < 6e-6


def test_zz_report():
    """the lines of the run (with -s); written to the file COARSE_PCG_PROFILE names, if it names one"""
    path = os.environ.get("COARSE_PCG_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_coarse_pcg.py on one MI355X: the device's error against the truth of tests/coarse_twin.py (longdouble),\n"
                    "e_ref = the same computation in IEEE double on the CPU, gate = max(2^-45, 10 e_ref); cases: n rows, c coarse columns.\n")
            f.write("\n".join(REPORT) + "\n")
