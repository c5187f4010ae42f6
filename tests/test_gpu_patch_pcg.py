"""The patch preconditioner and its conjugate gradient (proton_amd/csrc/patch_precond.hip) on the device: pa_condensed_patches
against the assembler's numbering, pa_patch_precond_factor / _apply and every iterate of pa_conjugated_gradient_patch against the
twin of tests/patch_pcg_twin.py (gate max(2^-45, 10 e_ref), all of it measured on the CPU: tests/test_patch_pcg_cpu.py), the
contract of the entry points, and the fictitious-domain and Poisson solves end to end.  One run: profiles/patch_pcg_parity.txt
(PATCH_PCG_PROFILE=that file python -m pytest tests/test_gpu_patch_pcg.py -m gpu -s)."""
import os

import numpy as np
import pytest

import cg_twin as T
import patch_pcg_twin as P

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


def _upload(a, sy, pt):
    """-> (rowptr, colind, values, b), (patch_ptr, patch_rows) on the device"""
    return (_dev(a, sy.rowptr), _dev(a, sy.colind), _dev(a, sy.values), _dev(a, sy.b)), (_dev(a, pt.ptr), _dev(a, pt.rows))


# ---- 1. the table builder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny", [(3, 3), (4, 2), (1, 1)])
def test_condensed_patches_against_the_numbering(asm, oracle, Nx, Ny):
    """both kinds for k = 0..3 against numpy on the oracle's numbering (compress table, cell faces bottom / right / top / left):
    every row covered, boundary cells with 2 or 3 faces; on the 1 x 1 mesh no rows and no patches"""
    asm.generate_mesh(Nx, Ny)
    mp, points, ptids = oracle.make_mesh(Nx, Ny)
    for k in range(4):
        o = oracle.Assembler(mp, points, ptids, oracle.degrees(k + 1, k))
        fbs = k + 1
        face, cell = P.numbering_patches(o.compress, o.cell_faces, o.num_other, fbs)
        n = asm.condensed_info(k + 1, k).system_size
        assert n == o.num_other * fbs
        for kind, want in (("face", face), ("cell", cell)):
            ptr, rows = asm.condensed_patches(k + 1, k, kind)
            asm.synchronize()
            ptr, rows = ptr.cpu().numpy(), rows.cpu().numpy()
            assert ptr.dtype == np.int64 and rows.dtype == np.int32
            assert np.array_equal(ptr, want.ptr) and np.array_equal(rows, want.rows), (k, kind)
            if Nx * Ny == 1:
                assert n == 0 and ptr.tolist() == [0] and rows.size == 0
                continue
            assert np.array_equal(np.unique(rows), np.arange(n))
            sizes = np.diff(ptr)
            if kind == "cell":
                assert ptr.size - 1 == Nx * Ny and set(sizes // fbs) == ({2, 3, 4} if min(Nx, Ny) > 2 else {2, 3})
                assert sizes.max() <= P.PMAX
            else:
                assert (sizes == fbs).all()


def test_condensed_patches_refuse_a_slab_and_bad_arguments(asm):
    import torch
    from proton_amd import capi
    from proton_amd.batch import BatchAssembler
    L = capi.lib()
    slab = BatchAssembler(0)
    slab.generate_mesh(4, 4, rows=(1, 3))
    di, _ = capi.degree_info(3, 2)
    ptr = torch.full((64,), -5, dtype=torch.int64, device=asm.device)
    rows = torch.full((1024,), -7, dtype=torch.int32, device=asm.device)
    import ctypes as C
    a, b = C.c_size_t(0), C.c_size_t(0)
    for kind in (capi.PATCH_FACE, capi.PATCH_CELL):
        assert L.pa_condensed_patches(slab.ctx.h, di, kind, ptr.data_ptr(), rows.data_ptr()) == 1
        assert b"whole-mesh" in L.pa_last_error(slab.ctx.h)
        assert L.pa_condensed_patches_query(slab.ctx.h, di, kind, C.byref(a), C.byref(b)) == 1
    asm.generate_mesh(3, 3)
    assert L.pa_condensed_patches(asm.ctx.h, di, 2, ptr.data_ptr(), rows.data_ptr()) == 1
    assert L.pa_condensed_patches(asm.ctx.h, di, capi.PATCH_CELL, None, rows.data_ptr()) == 1
    slab.synchronize(); asm.synchronize()
    assert bool((ptr == -5).all()) and bool((rows == -7).all())


# ---- 2. factor + apply against the twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.case_table(), ids=P.case_id)
def test_factor_and_apply(asm, case):
    """z = M r of both test vectors at the gate; r1 . M r2 = r2 . M r1 at the gate; two calls give the same bits; so does a permuted
    patch order that keeps every row's order of patches"""
    import torch
    sy, pt = P.system(case), P.patches(case)
    dv, dp = _upload(asm, sy, pt)
    pre = asm.patch_precond_factor(dv[0], dv[1], dv[2], dp)
    assert pre["failed"] == 0 and int(pre["info"].abs().sum()) == 0
    assert pre["sizes"].max_patch_rows == min(case.maxm, case.n) and pre["sizes"].lanes_per_patch == (4 if min(case.maxm, case.n) <= 4 else 8 if case.maxm <= 8 else 16)
    g = P.gate(P.apply_e_ref(case))
    zs = []
    for w in (0, 1):
        r = _dev(asm, P.test_vectors(case)[w])
        keep = r.clone()
        z = asm.patch_precond_apply(pre, r)
        z2 = asm.patch_precond_apply(pre, r, torch.full_like(r, float("nan")))
        asm.synchronize()
        assert torch.equal(z, z2) and torch.equal(r, keep)
        e = P.scaled_error(case, z.cpu().numpy(), P.apply_truth(case, w))
        say("apply %-16s vector %d: e_gpu %.3e e_ref %.3e gate %.3e ratio %.3f" % (P.case_id(case), w, e, P.apply_e_ref(case), g, e / g))
        assert e <= g
        zs.append(z)
    sym = P.symmetry_defect(case, zs[0].cpu().numpy(), zs[1].cpu().numpy())
    say("apply %-16s |r1.Mr2 - r2.Mr1| / sqrt(r1.Mr1 r2.Mr2) = %.3e" % (P.case_id(case), sym))
    assert sym <= g
    # a second factor gives the same factors; the permuted table the same z
    pre2 = asm.patch_precond_factor(dv[0], dv[1], dv[2], dp)
    assert torch.equal(pre["factors"], pre2["factors"]) and torch.equal(pre["slots"], pre2["slots"])
    perm, other = P.order_preserving_permutation(pt)
    if not np.array_equal(perm, np.arange(perm.size)):
        pre3 = asm.patch_precond_factor(dv[0], dv[1], dv[2], (_dev(asm, other.ptr), _dev(asm, other.rows)))
        z3 = asm.patch_precond_apply(pre3, _dev(asm, P.test_vectors(case)[0]))
        asm.synchronize()
        assert torch.equal(z3, zs[0])


# ---- 3. the solver, iterate by iterate --------------------------------------------------------------------------------------------
def _pcg(a, dv, dp, x=None, **kw):
    import torch
    if x is None:
        x = torch.full_like(dv[3], float("nan"))
    x, reason, iters, rr = a.conjugated_gradient_patch(dv[0], dv[1], dv[2], dv[3], dp, x=x, **kw)
    a.synchronize()
    return x.cpu().numpy(), reason, iters, rr


@pytest.mark.parametrize("case", P.case_table(), ids=P.case_id)
def test_every_iterate(asm, case):
    """x_m, the reported residual, the exit reason and the count for m = 1..min(8, n) (div = 0, then max_iter = 0, 1, ...: the way
    tests/test_gpu_cg_twin.py sees iterates) against the twin"""
    sy, pt = P.system(case), P.patches(case)
    dv, dp = _upload(asm, sy, pt)
    tr, er = P.truth(case), P.e_ref(case)
    assert P.judged(case) == list(range(1, len(tr.rr) + 1))
    for m in range(1, len(tr.rr) + 1):
        kw, want = P.iterate_call(case, m)
        x, reason, iters, rr = _pcg(asm, dv, dp, **kw)
        assert (reason, iters) == want, (m, reason, iters, want)
        g = P.gate(er[m - 1])
        e = T.scaled_error(x, tr.x[m - 1], sy.diag)
        t = tr.rr[m - 1]
        drr = abs(rr - t) / t if t >= T.EXACT else rr
        say("pcg   %-16s m %d: e_gpu %.3e rr %.3e e_ref %.3e gate %.3e ratio %.3f" % (P.case_id(case), m, e, drr, er[m - 1], g, max(e, drr) / g))
        assert e <= g and drr <= g


@pytest.mark.parametrize("n", [257, 4097])
def test_one_row_patches_are_jacobi(asm, n):
    """patches of one row each: every iterate at cg_twin's gate for the Jacobi case, and on exits placed between two residuals of
    the truth the same reason and count as pa_conjugated_gradient(precond = 1), x within the gate of its x"""
    case = T.Case(n, True, False)
    sy = T.system(case)
    dv, dp = _upload(asm, sy, P.jacobi_patches(n))
    tr, er = T.truth(case), T.e_ref(case)
    for m in T.judged(case):
        kw, want = T.iterate_call(case, m)
        x, reason, iters, rr = _pcg(asm, dv, dp, **kw)
        assert (reason, iters) == want
        assert T.scaled_error(x, tr.x[m - 1], sy.diag) <= T.gate(er[m - 1])
    calls = T.threshold_calls(case)
    assert calls
    for kw, want in calls:
        x, reason, iters, rr = _pcg(asm, dv, dp, **kw)
        xj, rj, ij, rrj = asm.conjugated_gradient(dv[0], dv[1], dv[2], dv[3], precond=True, **kw)
        asm.synchronize()
        assert (reason, iters) == (rj, ij) == want[:2]
        assert T.scaled_error(x, xj.cpu().numpy().astype(np.longdouble), sy.diag) <= T.gate(er[want[2]])


# ---- 4. contract ------------------------------------------------------------------------------------------------------------------
def test_contract_of_the_solver(asm):
    """x is the only output, the inputs are read only, two calls give the same bits whatever x held; n = 0 and b = 0 as
    pa_conjugated_gradient has them"""
    import torch
    case = P.Case(257)
    dv, dp = _upload(asm, P.system(case), P.patches(case))
    keep = [t.clone() for t in dv + dp]
    kw = dict(tol=0.0, div=T.HUGE, max_iter=5)
    x0, *s0 = _pcg(asm, dv, dp, **kw)
    x1, *s1 = _pcg(asm, dv, dp, **kw)
    x2, *s2 = _pcg(asm, dv, dp, x=torch.full_like(dv[3], 1e300), **kw)
    assert s0 == s1 == s2 and s0[:2] == [2, 6] and np.isfinite(x0).all()
    assert np.array_equal(x0, x1) and np.array_equal(x0, x2)
    assert all(torch.equal(a, b) for a, b in zip(keep, dv + dp))
    x = torch.full((4,), 7.0, dtype=torch.float64, device=asm.device)
    res = asm.ctx.conjugated_gradient_patch(0, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), x.data_ptr(), 0,
                                            dp[0].data_ptr(), dp[1].data_ptr())
    asm.synchronize()
    assert tuple(res) == (0, 0, 0.0) and bool((x == 7.0).all())
    xz, *sz = _pcg(asm, (dv[0], dv[1], dv[2], torch.zeros_like(dv[3])), dp, tol=1e-9, div=100.0, max_iter=1000)
    assert sz == [0, 0, 0.0] and (xz == 0.0).all() and not np.signbit(xz).any()


def _bad_tables(n, pt):
    """(name, ptr, rows, word of pa_last_error) for every refusal of the validation"""
    ptr, rows = pt.ptr.copy(), pt.rows.copy()
    out = []
    r = rows.copy(); r[5] = n
    out.append(("index = n", ptr, r, "outside"))
    r = rows.copy(); r[int(ptr[-1]) - 1] = -1
    out.append(("index < 0", ptr, r, "outside"))
    p = int(np.nonzero(np.diff(ptr) >= 2)[0][0])
    r = rows.copy(); r[ptr[p] + 1] = r[ptr[p]]
    out.append(("repeated row", ptr, r, "twice"))
    jp = P.jacobi_patches(n)
    out.append(("uncovered row", jp.ptr[:-1].copy(), jp.rows[:-1].copy(), "no patch"))
    big = np.concatenate([[0, 17], 17 + jp.ptr[1:n - 16]])
    out.append(("17 rows", big, jp.rows.copy(), "1 to 16"))
    empty = np.concatenate([[0, 0], jp.ptr[1:]])
    out.append(("0 rows", empty, jp.rows.copy(), "1 to 16"))
    out.append(("ptr[0] != 0", jp.ptr + 1, np.concatenate([[0], jp.rows]).astype(np.int32), "start at 0"))
    back = ptr.copy(); back[3] = back[2] - 1
    out.append(("descending ptr", back, rows, "1 to 16"))
    return out


def test_refusals_touch_no_output(asm):
    """every refusal of the table validation: PA_ERR_INVALID_ARG with text, x / the factors / the slots / the info words untouched;
    the validation runs before anything is indexed with the table"""
    import torch
    from proton_amd import capi
    L = capi.lib()
    case = P.Case(257)
    sy, pt = P.system(case), P.patches(case)
    dv, dp = _upload(asm, sy, pt)
    sz = asm.ctx.patch_precond_query(sy.n, pt.ptr.size - 1, dp[0].data_ptr())
    x = torch.full_like(dv[3], 7.0)
    factors = torch.full((int(sz.factor_doubles) + 4096,), 1.5, dtype=torch.float64, device=asm.device)
    slots = torch.full((int(sz.slot_ints) + 4096,), -3, dtype=torch.int32, device=asm.device)
    info = torch.full((4096,), 9, dtype=torch.int32, device=asm.device)
    scratch = torch.zeros(int(sz.scratch_bytes) + (1 << 16), dtype=torch.uint8, device=asm.device)
    p = lambda t: t.data_ptr()
    for name, ptr, rows, word in _bad_tables(sy.n, pt):
        dptr, drows = _dev(asm, ptr.astype(np.int64)), _dev(asm, rows.astype(np.int32))
        npat = ptr.size - 1
        st = L.pa_conjugated_gradient_patch(asm.ctx.h, sy.n, p(dv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(x), npat, p(dptr), p(drows), 1e-9, 100.0,
                                            10, None, None, None)
        text = L.pa_last_error(asm.ctx.h).decode()
        assert st == 1 and word in text, (name, st, text)
        st = L.pa_patch_precond_factor(asm.ctx.h, sy.n, p(dv[0]), p(dv[1]), p(dv[2]), npat, p(dptr), p(drows), p(factors), p(slots), p(scratch),
                                       p(info), None)
        assert st == 1 and word in L.pa_last_error(asm.ctx.h).decode(), (name, st)
        asm.synchronize()
        assert bool((x == 7.0).all()) and bool((factors == 1.5).all()) and bool((slots == -3).all()) and bool((info == 9).all()), name
    # NULL pointers
    assert L.pa_conjugated_gradient_patch(asm.ctx.h, sy.n, p(dv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(x), 3, None, p(dp[1]), 1e-9, 100.0, 10,
                                          None, None, None) == 1
    assert L.pa_patch_precond_factor(asm.ctx.h, sy.n, p(dv[0]), p(dv[1]), p(dv[2]), pt.ptr.size - 1, p(dp[0]), p(dp[1]), p(factors), None,
                                     p(scratch), p(info), None) == 1
    asm.synchronize()
    assert bool((x == 7.0).all()) and bool((factors == 1.5).all())


def test_an_indefinite_patch_is_reported(asm):
    """one diagonal entry flipped: PA_ERR_NOT_SPD before the first iteration, x untouched; the factor entry names exactly the
    patches that hold the row"""
    import torch
    from proton_amd import capi
    case = P.Case(257)
    sy, pt = P.system(case), P.patches(case)
    row = 100
    vals = sy.values.copy()
    k = int(sy.rowptr[row] + np.nonzero(sy.colind[sy.rowptr[row]:sy.rowptr[row + 1]] == row)[0][0])
    vals[k] = -vals[k]
    dv, dp = _upload(asm, sy._replace(values=vals), pt)
    pre = asm.patch_precond_factor(dv[0], dv[1], dv[2], dp)
    holders = [q for q in range(pt.ptr.size - 1) if row in pt.rows[pt.ptr[q]:pt.ptr[q + 1]]]
    info = pre["info"].cpu().numpy()
    assert pre["failed"] == len(holders) >= 1 and np.nonzero(info)[0].tolist() == holders
    for q in holders:                                   # the first non-positive pivot is at or before the flipped row's position
        pos = int(np.nonzero(pt.rows[pt.ptr[q]:pt.ptr[q + 1]] == row)[0][0])
        assert 1 <= info[q] <= pos + 1
    x = torch.full_like(dv[3], 7.0)
    with pytest.raises(capi.ProtonAmdError) as e:
        asm.conjugated_gradient_patch(dv[0], dv[1], dv[2], dv[3], dp, x=x)
    asm.synchronize()
    assert e.value.status == 6 and bool((x == 7.0).all())


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,cell_ratio,face_ratio", [(20, 2, 2, None), (32, 2, 3, 2)])
def test_fictdom_condensed_solve_with_patches(asm, oracle, N, k, cell_ratio, face_ratio):
    """fictdom_condensed_solve(patches = "cell" / "face") at 1e-13: the recovered vector against spsolve of the full system within
    1e-8 max|ref| (what tests/test_gpu_fictdom_condensed.py asks of the Jacobi solve); iterations against the Jacobi solve of the
    same call sequence: cell <= Jacobi / 2 at (20, 2), cell <= Jacobi / 3 and face <= Jacobi / 2 at (32, 2); the energy error at
    (20, 2) against cuthho.xlsx as that file's test has it"""
    import scipy.sparse.linalg as spla

    import test_gpu_fictdom_condensed as F
    asm.cut_preprocess(N, refsteps=4)
    op = F.operators(asm, k, F.NEG)
    K, b, _ = F.full_system(asm, k, F.NEG, op)
    ref = spla.spsolve(K.tocsc(), b)
    iters = {}
    for patches in (None, "face", "cell"):
        full, iters[patches], reason = asm.fictdom_condensed_solve(k, F.NEG, tol=F.CG_TOL, patches=patches)
        asm.synchronize()
        assert reason == 0
        err = np.abs(full.cpu().numpy() - ref).max() / np.abs(ref).max()
        say("fictdom (%d, %d) patches %-5s: %4d iterations, against spsolve %.3e of max|ref|" % (N, k, patches, iters[patches], err))
        assert err <= 1e-8
        if (N, k) == (20, 2) and patches is not None:
            e = F.energy_error(oracle, oracle.CutMesh(N, refsteps=4), k, full.cpu().numpy())
            say("fictdom (%d, %d) patches %-5s: energy error %.10e (xlsx %.6e)" % (N, k, patches, e, F.XLSX[(k, N)]))
            assert abs(e - F.XLSX[(k, N)]) / F.XLSX[(k, N)] < 6e-6
    assert cell_ratio * iters["cell"] <= iters[None]
    if face_ratio:
        assert face_ratio * iters["face"] <= iters[None]


def test_poisson_on_general_quadrilaterals(asm, oracle):
    """plain Poisson on a 16 x 16 mesh of general quadrilaterals, k = 3 (cell patches of 16 rows): Jacobi, face blocks and cell
    patches converge to the same solution within 1e-8 of its largest entry; the iteration counts are printed"""
    import proton_amd as pa
    N, cd, fd = 16, 4, 3
    mp, points, ptids = oracle.make_mesh(N, N)
    rng = np.random.default_rng(11)
    ij = np.arange(points.shape[0])
    interior = (ij % (N + 1) > 0) & (ij % (N + 1) < N) & (ij // (N + 1) > 0) & (ij // (N + 1) < N)
    points[interior] += rng.uniform(-0.2 / N, 0.2 / N, size=points.shape)[interior]
    o = oracle.Assembler(mp, points, ptids, oracle.degrees(cd, fd))
    asm.set_mesh(points, ptids)
    asm.set_faces(o.cell_faces, o.faces, o.is_dir)
    rhs = asm.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS, pa.QUAD_TENSOR)
    g = asm.dirichlet_data(fd, pa.capi.FN_SIN_SIN_SOL)
    rec = asm.condensed_ops(cd, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, rhs=rhs)
    ptr, _ = asm.condensed_patches(cd, fd, "cell")
    assert int((ptr[1:] - ptr[:-1]).max()) == 16
    sol, iters = {}, {}
    for patches in (None, "face", "cell"):
        x, reason, iters[patches], rr = asm.condensed_solve(cd, fd, rec, g, tol=1e-13, patches=patches)
        asm.synchronize()
        assert reason == 0
        sol[patches] = x.cpu().numpy()
    say("poisson 16 x 16 general quadrilaterals, k = 3: Jacobi %d, face blocks %d, cell patches %d iterations" % (iters[None], iters["face"], iters["cell"]))
    for patches in ("face", "cell"):
        assert np.abs(sol[patches] - sol[None]).max() <= 1e-8 * np.abs(sol[None]).max()
    asm.generate_mesh(4, 4)                          # leave a generated mesh behind


def test_zz_report():
    """the lines of the run (with -s); written to the file PATCH_PCG_PROFILE names, if it names one"""
    path = os.environ.get("PATCH_PCG_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_patch_pcg.py on one MI355X: the device's error against the truth of tests/patch_pcg_twin.py (mpmath at 50\n"
                    "digits up to 257 rows, longdouble above), e_ref = the same computation in IEEE double on the CPU, gate = max(2^-45, 10 e_ref);\n"
                    "cases: n rows, m = the largest patch, hard = a patch matrix of condition beyond 1e8.\n")
            f.write("\n".join(REPORT) + "\n")
