"""The smoothed coarse levels and the multilevel conjugate gradient (proton_amd/csrc/multilevel_precond.hip) on the device:
pa_smoothed_level_setup / _apply and every iterate of pa_conjugated_gradient_multilevel against the twin of tests/multilevel_twin.py
(gate max(2^-45, 10 e_ref), all of it measured on the CPU: tests/test_multilevel_cpu.py), bit-identity with the two-level solvers
without a smoothed level, every refusal in its order, the table builders beyond 4096 columns bit for bit against the twin's tables,
and the Poisson, fictitious-domain and interface solves end to end.  One run: profiles/multilevel_pcg_parity.txt
(MULTILEVEL_PCG_PROFILE=that file python -m pytest tests/test_gpu_multilevel_pcg.py -m gpu -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import cg_twin as T
import coarse_twin as CT
import multilevel_twin as ML
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


def _table(a, tb):
    return (_dev(a, tb.ptr.astype(np.int64)), _dev(a, tb.cols.astype(np.int32)), _dev(a, tb.vals.astype(np.float64)), tb.ncoarse)


def _system(a, n):
    """-> (rowptr, colind, values, b), (patch_ptr, patch_rows) of patch_pcg_twin's system of n rows on the device"""
    sy, pt = PT.system(PT.Case(n)), PT.patches(PT.Case(n))
    return (_dev(a, sy.rowptr), _dev(a, sy.colind), _dev(a, sy.values), _dev(a, sy.b)), (_dev(a, pt.ptr), _dev(a, pt.rows))


# ---- 1. set-up + apply against the twin -------------------------------------------------------------------------------------------
LANES = set()


@pytest.mark.parametrize("case", ML.case_table(), ids=ML.case_id)
def test_setup_and_apply(asm, case):
    """1 / d_j and z of both test vectors, with and without accumulate, at the gate; two calls and two set-ups give the same bits; r
    is read only; the lanes per column are the twin's choice"""
    import torch
    sy = ML.system(case)
    dv = (_dev(asm, sy.rowptr), _dev(asm, sy.colind), _dev(asm, sy.values))
    dc = _table(asm, ML.level(case))
    pre = asm.smoothed_level_setup(dv[0], dv[1], dv[2], dc)
    asm.synchronize()
    assert pre["column"] == 0
    assert pre["sizes"].entries == ML.level(case).ptr[-1] and pre["sizes"].dinv_doubles == case.ncoarse
    assert pre["sizes"].lanes_per_column == ML.lanes_per_column(ML.level(case))
    LANES.add(pre["sizes"].lanes_per_column)
    gd = ML.gate(ML.dinv_e_ref(case))
    ed = ML.dinv_error(case, pre["dinv"].cpu().numpy())
    say("dinv   %-18s e_gpu %.3e e_ref %.3e gate %.3e ratio %.3f (%d lanes per column)" %
        (ML.case_id(case), ed, ML.dinv_e_ref(case), gd, ed / gd, pre["sizes"].lanes_per_column))
    assert ed <= gd
    g = ML.gate(ML.apply_e_ref(case))
    for w in (0, 1):
        r = _dev(asm, ML.test_vectors(case)[w])
        keep = r.clone()
        for acc in (False, True):
            z0 = _dev(asm, ML.test_vectors(case)[1 - w]) if acc else torch.full_like(r, float("nan"))
            z = asm.smoothed_level_apply(pre, r, z0.clone(), accumulate=acc)
            z2 = asm.smoothed_level_apply(pre, r, z0.clone(), accumulate=acc)
            asm.synchronize()
            assert torch.equal(z, z2) and torch.equal(r, keep)
            e = ML.scaled_error(case, z.cpu().numpy(), ML.apply_truth(case, w, acc))
            say("apply  %-18s vector %d accumulate %d: e_gpu %.3e e_ref %.3e gate %.3e ratio %.3f" %
                (ML.case_id(case), w, acc, e, ML.apply_e_ref(case), g, e / g))
            assert e <= g
    pre2 = asm.smoothed_level_setup(dv[0], dv[1], dv[2], dc)
    asm.synchronize()
    assert torch.equal(pre["dinv"], pre2["dinv"]) and torch.equal(pre["pt"], pre2["pt"])


def test_both_column_shapes_ran():
    """a quarter wavefront per column (the table of 5000 short columns) and a wavefront per column (the column of 5000 entries)"""
    assert LANES == {16, 64}


def test_a_column_without_a_positive_diagonal_is_reported(asm):
    """a P with an empty column j: *column = j + 1, PA_ERR_NOT_SPD, d_dinv untouched; -A: column 1"""
    import torch
    from proton_amd import capi
    L = capi.lib()
    case = ML.Case(257, 33, "ct")
    sy, tb = ML.system(case), ML.level(case)
    dv = (_dev(asm, sy.rowptr), _dev(asm, sy.colind), _dev(asm, sy.values))
    hole = _table(asm, _without_column(tb, 17))
    assert asm.smoothed_level_setup(dv[0], dv[1], dv[2], hole)["column"] == 18
    assert asm.smoothed_level_setup(dv[0], dv[1], -dv[2], _table(asm, tb))["column"] == 1
    sz = asm.ctx.smoothed_level_query(case.n, tb.ncoarse, hole[0].data_ptr())
    pt = torch.zeros(int(sz.pt_bytes), dtype=torch.uint8, device=asm.device)
    dinv = torch.full((tb.ncoarse + 64,), 1.5, dtype=torch.float64, device=asm.device)
    scratch = torch.zeros(int(sz.scratch_bytes), dtype=torch.uint8, device=asm.device)
    col = C.c_int32(0)
    p = lambda t: t.data_ptr()
    st = L.pa_smoothed_level_setup(asm.ctx.h, case.n, p(dv[0]), p(dv[1]), p(dv[2]), tb.ncoarse, p(hole[0]), p(hole[1]), p(hole[2]), p(pt), p(dinv),
                                   p(scratch), C.byref(col))
    asm.synchronize()
    assert st == 6 and col.value == 18 and "column 17" in L.pa_last_error(asm.ctx.h).decode() and bool((dinv == 1.5).all())


def _without_column(tb, j):
    keep = tb.cols != j
    n = tb.ptr.size - 1
    sizes = np.bincount(np.repeat(np.arange(n), np.diff(tb.ptr))[keep], minlength=n)
    return CT.Table(np.concatenate([[0], np.cumsum(sizes)]), tb.cols[keep], tb.vals[keep], tb.ncoarse)


# ---- 2. the solver, iterate by iterate --------------------------------------------------------------------------------------------
def _solve_tables(a, s):
    levels, exact = ML.solve_levels(s)
    return [_table(a, t) for t in levels], (_table(a, exact) if exact is not None else None)


def _pcg(a, dv, dp, levels, exact, x=None, **kw):
    import torch
    if x is None:
        x = torch.full_like(dv[3], float("nan"))
    x, reason, iters, rr = a.conjugated_gradient_multilevel(dv[0], dv[1], dv[2], dv[3], dp, levels, exact, x=x, **kw)
    a.synchronize()
    return x.cpu().numpy(), reason, iters, rr


@pytest.mark.parametrize("s", ML.solve_table(), ids=ML.solve_id)
def test_every_iterate(asm, s):
    """x_m, the reported residual, the exit reason and the count for m = 1..8 against the twin: 0, 1 and 3 smoothed levels, with and
    without an exact level"""
    sy = PT.system(PT.Case(s.n))
    dv, dp = _system(asm, s.n)
    levels, exact = _solve_tables(asm, s)
    tr, er = ML.truth(s), ML.e_ref(s)
    assert ML.judged(s) == list(range(1, len(tr.rr) + 1))
    for m in range(1, len(tr.rr) + 1):
        kw, want = ML.iterate_call(s, m)
        x, reason, iters, rr = _pcg(asm, dv, dp, levels, exact, **kw)
        assert (reason, iters) == want, (m, reason, iters, want)
        g = ML.gate(er[m - 1])
        e = T.scaled_error(x, tr.x[m - 1], sy.diag)
        t = tr.rr[m - 1]
        drr = abs(rr - t) / t if t >= T.EXACT else rr
        say("pcg    %-24s m %d: e_gpu %.3e rr %.3e e_ref %.3e gate %.3e ratio %.3f" % (ML.solve_id(s), m, e, drr, er[m - 1], g, max(e, drr) / g))
        assert e <= g and drr <= g


def test_without_a_smoothed_level_the_solver_is_its_parents(asm):
    """nlevels = 0: x and the three results are pa_conjugated_gradient_patch_coarse's with an exact table and
    pa_conjugated_gradient_patch's without, bit for bit; with levels two calls give the same bits whatever x held, and the inputs are
    read only"""
    import torch
    s = ML.Solve(257, (65, 33, 31), 2)
    dv, dp = _system(asm, s.n)
    levels, exact = _solve_tables(asm, s)
    for kw in (dict(tol=0.0, div=T.HUGE, max_iter=5), dict(tol=1e-9, div=100.0, max_iter=1000)):
        x0, *s0 = _pcg(asm, dv, dp, [], exact, **kw)
        xc, rc, ic, rrc = asm.conjugated_gradient_patch_coarse(dv[0], dv[1], dv[2], dv[3], dp, exact, **kw)
        asm.synchronize()
        assert np.array_equal(x0, xc.cpu().numpy()) and s0 == [rc, ic, rrc] and np.isfinite(x0).all()
        x0, *s0 = _pcg(asm, dv, dp, [], None, **kw)
        xp, rp, ip, rrp = asm.conjugated_gradient_patch(dv[0], dv[1], dv[2], dv[3], dp, **kw)
        asm.synchronize()
        assert np.array_equal(x0, xp.cpu().numpy()) and s0 == [rp, ip, rrp]
    keep = [t.clone() for t in dv + dp + tuple(t for lv in levels + [exact] for t in lv[:3])]
    kw = dict(tol=0.0, div=T.HUGE, max_iter=5)
    x1, *s1 = _pcg(asm, dv, dp, levels, exact, **kw)
    x2, *s2 = _pcg(asm, dv, dp, levels, exact, x=torch.full_like(dv[3], 1e300), **kw)
    assert s1 == s2 and s1[:2] == [2, 6] and np.array_equal(x1, x2) and np.isfinite(x1).all()
    assert all(torch.equal(a, b) for a, b in zip(keep, dv + dp + tuple(t for lv in levels + [exact] for t in lv[:3])))
    x = torch.full((4,), 7.0, dtype=torch.float64, device=asm.device)
    res = asm.ctx.conjugated_gradient_multilevel(0, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), x.data_ptr(), 0,
                                                 dp[0].data_ptr(), dp[1].data_ptr(), [(33, 0, 0, 0)], None)
    asm.synchronize()
    assert tuple(res) == (0, 0, 0.0) and bool((x == 7.0).all())                             # n = 0 as pa_conjugated_gradient has it


# ---- 3. the refusals, in their order ------------------------------------------------------------------------------------------------
def test_refusals_in_their_order_touch_no_output(asm):
    """the patch table, each level's table in order, the exact table (PA_ERR_INVALID_ARG, the level's index in the text), then
    PA_ERR_NOT_SPD of the patches, a level (a zero column at level 1 of 3: its index and column), the exact level; nlevels = 9; a NULL
    `levels` with nlevels > 0: d_x keeps its pattern through all of them"""
    import torch
    from proton_amd import capi
    L = capi.lib()
    s = ML.Solve(257, (65, 33, 31), 2)
    n = s.n
    dv, dp = _system(asm, n)
    host_levels, host_exact = ML.solve_levels(s)
    levels, exact = _solve_tables(asm, s)
    x = _dev(asm, np.arange(n) * 0.5 - 7.0)
    pattern = x.clone()
    p = lambda t: t.data_ptr()
    tab = lambda t: capi.CoarseTable(t[3], p(t[0]), p(t[1]), p(t[2]))

    def call(lv, ex, rows=dp[1], values=dv[2], nlevels=None, null_levels=False):
        arr = (capi.CoarseTable * 9)(*[tab(t) for t in lv])
        e = tab(ex) if ex is not None else None
        st = L.pa_conjugated_gradient_multilevel(asm.ctx.h, n, p(dv[0]), p(dv[1]), p(values), p(dv[3]), p(x), dp[0].numel() - 1, p(dp[0]), p(rows),
                                                 len(lv) if nlevels is None else nlevels, None if null_levels else arr,
                                                 C.byref(e) if e is not None else None, 1e-9, 100.0, 10, None, None, None)
        asm.synchronize()
        assert torch.equal(x, pattern)
        return st, L.pa_last_error(asm.ctx.h).decode()

    def broken(tb, how):
        c = tb.cols.copy()
        big = int(np.nonzero(np.diff(tb.ptr) >= 2)[0][0])
        if how == "index":
            c[tb.ptr[big + 1] - 1] = tb.ncoarse
        else:
            c[tb.ptr[big]], c[tb.ptr[big] + 1] = c[tb.ptr[big] + 1], c[tb.ptr[big]]
        return _table(asm, CT.Table(tb.ptr, c, tb.vals, tb.ncoarse))

    bad_rows = dp[1].clone(); bad_rows[5] = n
    bad1, bad2, bad_exact = broken(host_levels[1], "index"), broken(host_levels[2], "order"), broken(host_exact, "index")
    hole1 = _table(asm, _without_column(host_levels[1], 9))
    hole_exact = _table(asm, _without_column(host_exact, 1))
    # 1: the patch table before everything
    st, text = call([levels[0], bad1, bad2], bad_exact, rows=bad_rows)
    assert st == 1 and "patch table" in text, text
    # 2: the levels in the caller's order
    st, text = call([levels[0], bad1, bad2], bad_exact)
    assert st == 1 and "outside" in text and "level 1" in text, text
    st, text = call([levels[0], levels[1], bad2], bad_exact)
    assert st == 1 and "ascend" in text and "level 2" in text, text
    st, text = call([levels[0], (levels[1][0], levels[1][1], levels[1][2], (1 << 24) + 1), levels[2]], exact)
    assert st == 1 and "16777216" in text and "level 1" in text, text
    # 3: the exact table after them, before any matrix is judged
    st, text = call([levels[0], hole1, levels[2]], bad_exact, values=-dv[2])
    assert st == 1 and "outside" in text and "smoothed level" not in text, text
    st, text = call([levels[0], hole1, levels[2]], (exact[0], exact[1], exact[2], 4097))
    assert st == 1 and "1 to 4096" in text, text
    # 4: not positive definite: the patches, then a level, then the exact level
    st, text = call([levels[0], hole1, levels[2]], hole_exact, values=-dv[2])
    assert st == 6 and "patch" in text, text
    st, text = call([levels[0], hole1, levels[2]], hole_exact)
    assert st == 6 and "column 9" in text and "level 1" in text, text
    st, text = call(levels, hole_exact)
    assert st == 6 and "pivot 1" in text, text
    # the arguments
    st, _ = call(levels * 3, exact, nlevels=9)
    assert st == 1
    st, _ = call(levels, exact, null_levels=True)
    assert st == 1
    # and the same tables, unbroken, solve
    x, reason, iters, _ = asm.conjugated_gradient_multilevel(dv[0], dv[1], dv[2], dv[3], dp, levels, exact, tol=1e-9, max_iter=1000)
    asm.synchronize()
    assert reason == 0 and iters > 0 and bool(torch.isfinite(x).all())


# ---- 4. the table cap -------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    ptr, cols, vals, nc = got
    assert nc == want.ncoarse, what
    ptr, cols, vals = ptr.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
    assert ptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64
    assert np.array_equal(ptr, want.ptr), what
    assert np.array_equal(cols, want.cols), what
    assert np.array_equal(vals.view(np.int64), want.vals.view(np.int64)), what              # bit for bit


def test_cap_of_the_plain_table(asm, oracle):
    """(140, 140, 2), 69^2 = 4761 columns: refused at the default with today's text; built after set_coarse_table_cap(8192), equal
    to the twin's ptr, cols and vals bit for bit; cap 0 restores the refusal; 2^24 + 1 is refused"""
    from proton_amd import capi
    L = capi.lib()
    N, H, k = 140, 2, 1
    di, _ = capi.degree_info(k + 1, k)
    a, b = C.c_size_t(0), C.c_size_t(0)
    asm.generate_mesh(N, N)
    try:
        assert L.pa_condensed_coarse_query(asm.ctx.h, di, H, capi.COARSE_ONE, 0, C.byref(a), C.byref(b)) == 1
        assert "H = 2 gives 4761 coarse columns; 1 to 4096 are served" in L.pa_last_error(asm.ctx.h).decode()
        asm.ctx.set_coarse_table_cap(8192)
        mp, points, ptids = oracle.make_mesh(N, N)
        o = oracle.Assembler(mp, points, ptids, oracle.degrees(k + 1, k))
        want = ML.table(N, N, H, k + 1, o.compress, o.faces, o.num_other)
        assert want.ncoarse == 4761
        _same(asm.condensed_coarse(k + 1, k, H), want, "140^2 H 2")
        asm.synchronize()
        assert L.pa_condensed_coarse_query(asm.ctx.h, di, 1, capi.COARSE_ONE, 0, C.byref(a), C.byref(b)) == 1
        assert "19321 coarse columns; 1 to 8192 are served" in L.pa_last_error(asm.ctx.h).decode()
        assert L.pa_context_set_coarse_table_cap(asm.ctx.h, (1 << 24) + 1) == 1
        assert asm.ctx.condensed_coarse_query(di, H, capi.COARSE_ONE, 0)[0] == 4761          # (the refused value changed nothing)
        asm.ctx.set_coarse_table_cap(0)
        assert L.pa_condensed_coarse_query(asm.ctx.h, di, H, capi.COARSE_ONE, 0, C.byref(a), C.byref(b)) == 1
        assert "1 to 4096 are served" in L.pa_last_error(asm.ctx.h).decode()
        say("cap    plain (140, 140, 2): 4761 columns refused at 4096, built at 8192 equal to the twin, refused again at 0")
    finally:
        asm.ctx.set_coarse_table_cap(0)
        asm.generate_mesh(4, 4)


def test_cap_of_the_tables_by_side_and_of_the_interface(asm, oracle):
    """the circle on 140^2 cells, H = 2: pa_condensed_coarse by side and pa_interface_condensed_coarse in one part and by side are
    refused at the default, and with the cap at 16384 equal to the twin's tables bit for bit"""
    import interface_coarse_twin as IC
    import interface_patch_twin as I
    from proton_amd import capi
    N, H, k = 140, 2, 0
    asm.cut_preprocess(N, refsteps=4)
    msh = oracle.CutMesh(N, refsteps=4)
    try:
        with pytest.raises(capi.ProtonAmdError):
            asm.condensed_coarse(k + 1, k, H, "side", 0)
        with pytest.raises(capi.ProtonAmdError):
            asm.interface_condensed_coarse(k, H, "one")
        asm.ctx.set_coarse_table_cap(16384)
        o = oracle.Assembler(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, oracle.degrees(k + 1, k))
        want = ML.table(N, N, H, k + 1, o.compress, o.faces, o.num_other, msh.face_loc, 0)
        assert want.ncoarse > 4761
        _same(asm.condensed_coarse(k + 1, k, H, "side", 0), want, "by side")
        say("cap    by side (140, 140, 2): %d columns equal to the twin" % want.ncoarse)
        faces, _ = oracle.mesh_faces(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0))
        ft, num_other = I.device_face_table(msh.bnd, msh.face_loc)
        pts, blk, side = IC.block_items(ft, msh.face_loc, faces, num_other)
        for parts in ("one", "side"):
            want = ML.table(N, N, H, k + 1, blk, pts, num_other, side if parts == "side" else None, 0)
            assert want.ncoarse >= 4761
            _same(asm.interface_condensed_coarse(k, H, parts), want, parts)
            say("cap    interface %-4s (140, 140, 2): %d columns equal to the twin" % (parts, want.ncoarse))
        asm.synchronize()
    finally:
        asm.ctx.set_coarse_table_cap(0)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def _twin_count(asm, rowptr, colind, values, b, patches, levels, exact, tol):
    sysm = PT.Condensed(rowptr.cpu().numpy(), colind.cpu().numpy(), values.cpu().numpy(), b.cpu().numpy(), None, None)
    host = lambda t: CT.Table(t[0].cpu().numpy(), t[1].cpu().numpy(), t[2].cpu().numpy(), t[3])
    pt = PT.Patches(patches[0].cpu().numpy(), patches[1].cpu().numpy())
    return ML.multilevel_iterations(sysm, pt, [host(t) for t in levels], host(exact) if exact is not None else None, tol=tol)


def test_poisson_on_general_quadrilaterals(asm, oracle):
    """64 x 64 general quadrilaterals (the generated mesh with its interior points moved), k = 2, coarse_levels = (2, 4), coarse = 8
    to 1e-13: x_F against spsolve of the downloaded CSR within 1e-8 of its largest entry; the count within 2 of the twin's PCG on the
    downloaded system and no larger than the two-level count with coarse = 8 alone; coarse_levels = None is the call without it"""
    import torch

    import test_gpu_coarse_pcg as G
    N, cd, fd = 64, 3, 2
    mp, points, ptids = oracle.make_mesh(N, N)
    ij = np.arange(points.shape[0])
    interior = (ij % (N + 1) > 0) & (ij % (N + 1) < N) & (ij // (N + 1) > 0) & (ij // (N + 1) < N)
    points[interior] += np.random.default_rng(11).uniform(-0.2 / N, 0.2 / N, size=points.shape)[interior]
    rec, g = G._poisson(asm, N, cd, fd, points)
    ref = G._spsolve(asm, cd, fd, rec, g)
    x2, r2, i2, _ = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches="cell", coarse=8)
    xn, _, inone, _ = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches="cell", coarse=8, coarse_levels=None)
    xm, rm, im, _ = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches="cell", coarse=8, coarse_levels=(2, 4))
    xo, ro, io, _ = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches="cell", coarse_levels=(2, 4, 8))
    asm.synchronize()
    assert r2 == 0 and rm == 0 and ro == 0 and torch.equal(x2, xn) and i2 == inone
    err = np.abs(xm.cpu().numpy() - ref).max() / np.abs(ref).max()
    erro = np.abs(xo.cpu().numpy() - ref).max() / np.abs(ref).max()
    rowptr, colind = asm.condensed_csr_pattern(cd, fd)
    values, b = asm.condensed_csr_fill(cd, fd, rec, g)
    tables = [asm.condensed_coarse(cd, fd, H) for H in (2, 4, 8)]
    twin = _twin_count(asm, rowptr, colind, values, b, asm.condensed_patches(cd, fd, "cell"), tables[:2], tables[2], 1e-13)
    say("poisson 64^2 general quadrilaterals k = 2: exact 8 alone %d, smoothed {2, 4} + exact 8 %d (twin %d), smoothed {2, 4, 8} alone %d "
        "iterations; against spsolve %.3e and %.3e of max|ref|" % (i2, im, twin, io, err, erro))
    assert err <= 1e-8 and erro <= 1e-8
    assert abs(im - twin) <= 2 and im <= i2
    with pytest.raises(ValueError):
        asm.condensed_solve(cd, fd, rec, g, patches="cell", coarse=8, coarse_levels=(2, 3))
    with pytest.raises(ValueError):
        asm.condensed_solve(cd, fd, rec, g, coarse_levels=(2, 4))
    asm.generate_mesh(4, 4)                          # leave a generated mesh behind


def test_fictdom_by_side(asm, oracle):
    """fictdom_condensed_solve (32, 2) by side with coarse_levels = (2, 4), coarse = 8 to 1e-13: the recovered vector against spsolve
    of the full system within 1e-8 max|ref|; the count within 2 of the twin's and no larger than the two-level count"""
    import scipy.sparse.linalg as spla

    import test_gpu_fictdom_condensed as F
    N, k = 32, 2
    asm.cut_preprocess(N, refsteps=4)
    op = F.operators(asm, k, F.NEG)
    K, b, _ = F.full_system(asm, k, F.NEG, op)
    ref = spla.spsolve(K.tocsc(), b)
    f2, i2, r2 = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell", coarse=8)
    fm, im, rm = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches="cell", coarse=8, coarse_levels=(2, 4))
    asm.synchronize()
    err = np.abs(fm.cpu().numpy() - ref).max() / np.abs(ref).max()
    rec = F.records(asm, k, F.NEG, op)
    rowptr, colind = asm.condensed_csr_pattern(k + 1, k)
    values, bF = asm.condensed_csr_fill(k + 1, k, rec["cond"], op["g"])
    tables = [asm.condensed_coarse(k + 1, k, H, "side", F.NEG) for H in (2, 4, 8)]
    twin = _twin_count(asm, rowptr, colind, values, bF, asm.condensed_patches(k + 1, k, "cell"), tables[:2], tables[2], F.CG_TOL)
    say("fictdom (32, 2) by side: exact 8 alone %d, smoothed {2, 4} + exact 8 %d (twin %d) iterations; against spsolve %.3e of max|ref|"
        % (i2, im, twin, err))
    assert r2 == 0 and rm == 0 and err <= 1e-8
    assert abs(im - twin) <= 2 and im <= i2


@pytest.mark.parametrize("parts", ["one", "side"])
def test_interface(asm, parts):
    """interface_condensed_solve (32, 2) with coarse_levels = (2, 4), coarse = 8 to 1e-13, one part and by side: the recovered vector
    within 1e-8 max|ref| of the refined spsolve of the full system (test_gpu_interface_coarse.full_reference says why refined); the
    count within 2 of the twin's and no larger than the two-level count"""
    import test_gpu_interface_coarse as G
    N, k = 32, 2
    ops, g = G.real_ops(asm, N, k)
    _, ref = G.full_reference(asm, k, ops, g)
    f2, i2, r2 = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell", coarse=8, coarse_parts=parts)
    fm, im, rm = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell", coarse=8, coarse_parts=parts, coarse_levels=(2, 4))
    asm.synchronize()
    err = np.abs(fm.cpu().numpy() - ref).max() / np.abs(ref).max()
    rec = asm.interface_condensed_ops(k, ops)
    rowptr, colind = asm.interface_condensed_csr_pattern(k)
    values, b = asm.interface_condensed_csr_fill(k, rec, g)
    tables = [asm.interface_condensed_coarse(k, H, parts) for H in (2, 4, 8)]
    twin = _twin_count(asm, rowptr, colind, values, b, asm.interface_condensed_patches(k, "cell"), tables[:2], tables[2], 1e-13)
    say("interface (32, 2) %-4s: exact 8 alone %d, smoothed {2, 4} + exact 8 %d (twin %d) iterations; against spsolve refined %.3e of "
        "max|ref|" % (parts, i2, im, twin, err))
    assert r2 == 0 and rm == 0 and err <= 1e-8
    assert abs(im - twin) <= 2 and im <= i2


def test_zz_report():
    """the lines of the run (with -s); written to the file MULTILEVEL_PCG_PROFILE names, if it names one"""
    path = os.environ.get("MULTILEVEL_PCG_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_multilevel_pcg.py on one MI355X: the device's error against the truth of tests/multilevel_twin.py\n"
                    "(longdouble), e_ref = the same computation in IEEE double on the CPU in the kernels' order, gate = max(2^-45, 10 e_ref);\n"
                    "cases: n rows, c coarse columns; solves: n rows, l the columns of the smoothed levels, e those of the exact level.\n")
            f.write("\n".join(REPORT) + "\n")
