"""pa_conjugated_gradient_rows_patch_coarse and the tables of a slab (proton_amd/csrc/rows_precond.hip) on the device.  The ranks
are threads of one process behind tests/cg_transport.py, each with its own context, as in tests/test_gpu_cg_rows.py.  What pins the
call: one rank is pa_conjugated_gradient_patch_coarse bit for bit; the slab tables are the whole-mesh tables cut by the rule of
tests/rows_pcg_twin.py; every iterate x_m, m <= 8, on 2, 3 and 4 ranks against the twin's truth (gate max(2^-45, 10 e_ref), measured
on the CPU: tests/test_rows_pcg_cpu.py); the full solves against the one-rank call with the same preconditioner; and every local
failure ends the solve on every rank with d_x as it was.  One run: profiles/rows_pcg_parity.txt (ROWS_PCG_PROFILE=that file python -m
pytest tests/test_gpu_rows_pcg.py -m gpu -s)."""
import os
import threading

import numpy as np
import pytest

import cg_twin as T
import coarse_twin as CT
import patch_pcg_twin as PT
import rows_pcg_twin as RT
from cg_transport import ThreadTransport

pytestmark = pytest.mark.gpu

REPORT = []
JOIN = 120                                 # seconds a rank may take: a defect fails the test, it does not hang it


def say(line):
    print(line)
    REPORT.append(line)


def _asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def _dev(a, v):
    import torch
    return torch.tensor(np.ascontiguousarray(v)).to(a.device)


def _ranks(R, body, fail_rank=None, fail_at=None):
    """body(r, transport) on R daemon threads -> what each returned or raised; the barrier is aborted on any exception"""
    tt = ThreadTransport(R, fail_rank, fail_at)
    out, keep = [None] * R, []

    def run(r):
        def transport(ctx):
            made = tt.make(r, ctx)
            keep.append(made)                  # (the thunks live as long as the solve)
            return made[0]
        try:
            out[r] = body(r, transport)
        except BaseException as e:      # noqa: BLE001  (a failed rank must not leave the others at a barrier)
            out[r] = e
            tt.bar.abort()

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN)
    assert all(not t.is_alive() for t in th), "a rank is still inside the solve"
    return out


# ---- the slabs of a mesh ------------------------------------------------------------------------------------------------------------
def _slab_system(N, cd, fd, rows, halo):
    import proton_amd as pa
    a = _asm()
    a.generate_mesh(N, N, rows=rows)
    rhs = a.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS, pa.QUAD_TENSOR)
    g = a.dirichlet_data(fd, pa.capi.FN_SIN_SIN_SOL)
    rec = a.condensed_ops(cd, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, rhs=rhs)
    info = a.condensed_info(cd, fd)
    rp, ci = a.condensed_csr_pattern(cd, fd)
    va, b = a.condensed_csr_fill(cd, fd, rec, g, halo_below=halo)
    out = a.condensed_halo_pack(cd, fd, rec, g).clone() if rows[1] < N else None
    a.synchronize()
    return a, info, rp, ci, va, b, out


def _slabs(N, cd, fd, parts):
    slabs, halo = [], None
    for r0, r1 in zip(parts[:-1], parts[1:]):
        s = _slab_system(N, cd, fd, (r0, r1), halo)
        halo = s[6]
        slabs.append(s)
    return slabs


def _random_rhs(n, seed, device):
    import torch
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5).to(device)


def _solve_slabs(slabs, b, H, kind="cell", jacobi=False, tables=None, fail_rank=None, fail_at=None, **kw):
    """every slab's rows of the common right-hand side b solved on its thread -> per rank ((reason, iterations, rr), x) or what the
    call raised as (status, text, x)"""
    import torch
    from proton_amd.capi import ProtonAmdError
    cd, fd = kw.pop("cd"), kw.pop("fd")

    def body(r, transport):
        s, inf, rp, ci, va, _, _ = slabs[r]
        tp = transport(s.ctx)
        bs = b[inf.row_begin:inf.row_end].to(s.device).clone()
        x = torch.full_like(bs, 7.0)
        try:
            if jacobi:
                res = s.ctx.conjugated_gradient_rows(tp, inf.row_begin, inf.row_end, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), bs.data_ptr(),
                                                     x.data_ptr(), **kw)
            else:
                pt, tb = tables[r] if tables else (s.condensed_rows_patches(cd, fd, kind), s.condensed_rows_coarse(cd, fd, H) if H else None)
                _, *res = s.conjugated_gradient_rows_patch_coarse(tp, inf.row_begin, inf.row_end, rp, ci, va, bs, pt, tb, x=x, **kw)
            s.synchronize()
            return tuple(res), x.cpu()
        except ProtonAmdError as e:
            s.synchronize()
            return e.status, str(e), x.cpu()
    return _ranks(len(slabs), body, fail_rank, fail_at)


# ---- 1. one rank ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cd,fd,H", [(12, 2, 1, 4), (8, 3, 2, 2)])
def test_one_rank_is_the_one_rank_solver_bit_for_bit(N, cd, fd, H):
    """no transport, row_begin = 0, whole tables: pa_conjugated_gradient_patch_coarse (ncoarse = 0: pa_conjugated_gradient_patch) in x,
    exit reason, count and residual; the tables of the slab of all rows are the whole-mesh tables"""
    import torch
    a, info, rp, ci, va, b, _ = _slab_system(N, cd, fd, (0, N), None)
    n = b.numel()
    b = b + _random_rhs(n, 1234 + N, a.device)
    for kind in ("face", "cell"):
        pt, tb = a.condensed_patches(cd, fd, kind), a.condensed_coarse(cd, fd, H)
        ptr, tbr = a.condensed_rows_patches(cd, fd, kind), a.condensed_rows_coarse(cd, fd, H)
        assert all(torch.equal(u, v) for u, v in zip(pt, ptr)) and all(torch.equal(u, v) for u, v in zip(tb[:3], tbr[:3])) and tb[3] == tbr[3]
        x0, *r0 = a.conjugated_gradient_patch_coarse(rp, ci, va, b, pt, tb, tol=1e-10, max_iter=5000)
        x1, *r1 = a.conjugated_gradient_rows_patch_coarse(None, 0, n, rp, ci, va, b, pt, tb, tol=1e-10, max_iter=5000)
        a.synchronize()
        assert r0[0] == 0 and r1 == r0 and torch.equal(x0, x1), (kind, r0, r1)
        y0, *s0 = a.conjugated_gradient_patch(rp, ci, va, b, pt, tol=1e-10, max_iter=5000)
        y1, *s1 = a.conjugated_gradient_rows_patch_coarse(None, 0, n, rp, ci, va, b, pt, None, tol=1e-10, max_iter=5000)
        a.synchronize()
        assert s0[0] == 0 and s1 == s0 and torch.equal(y0, y1), (kind, s0, s1)
        say("one rank (%d, %d, %d) H %d %s: %d iterations with the coarse level, %d without, both bit for bit" % (N, cd, fd, H, kind, r0[1], s0[1]))


# ---- 2. the tables of a slab ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("N,H,parts", [(12, 4, (0, 5, 12)), (9, 3, (0, 2, 5, 9)), (4, 2, (0, 1, 2, 3, 4))])
def test_slab_tables_are_the_whole_mesh_tables_cut(N, H, parts, k):
    """face tables concatenate to the whole-mesh table, cell tables to it with every row outside the patch's slab deleted, the coarse
    rows are the whole table's bit for bit with the pointer rebased"""
    cd, fd, fbs = k + 1, k, k + 1
    whole = _asm()
    whole.generate_mesh(N, N)
    face, cell = (PT.Patches(*(t.cpu().numpy() for t in whole.condensed_patches(cd, fd, kind))) for kind in ("face", "cell"))
    p, c, v, nc = whole.condensed_coarse(cd, fd, H)
    one = CT.Table(p.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy(), nc)
    bnds = RT.bounds(N, N, parts, fbs)
    want_face = RT.truncate_patches(face, RT.row_owner(face, bnds), bnds)
    want_cell = RT.truncate_patches(cell, RT.cell_owner(N, parts, cell.ptr.size - 1), bnds)
    for s, (r0, r1) in enumerate(zip(parts[:-1], parts[1:])):
        a = _asm()
        a.generate_mesh(N, N, rows=(r0, r1))
        inf = a.condensed_info(cd, fd)
        assert (inf.row_begin, inf.row_end) == bnds[s]
        for kind, want in (("face", want_face[s]), ("cell", want_cell[s])):
            ptr, rows = (t.cpu().numpy() for t in a.condensed_rows_patches(cd, fd, kind))
            assert ptr.dtype == np.int64 and rows.dtype == np.int32
            assert np.array_equal(ptr, want.ptr) and np.array_equal(rows, want.rows), (s, kind)
        p, c, v, nc = a.condensed_rows_coarse(cd, fd, H)
        want = RT.slab_coarse(one, *bnds[s])
        assert nc == one.ncoarse and np.array_equal(p.cpu().numpy(), want.ptr) and np.array_equal(c.cpu().numpy(), want.cols)
        assert np.array_equal(v.cpu().numpy().view(np.int64), want.vals.view(np.int64))                     # bit for bit


def test_slab_table_refusals():
    """the whole-mesh entries still refuse a slab; the slab entries refuse the parts of a cut mesh and an H without an interior node"""
    import ctypes as C
    from proton_amd import capi
    from proton_amd.capi import ProtonAmdError
    a = _asm()
    a.generate_mesh(4, 4, rows=(1, 3))
    for call in (lambda: a.condensed_patches(2, 1, "cell"), lambda: a.condensed_coarse(2, 1, 2)):
        with pytest.raises(ProtonAmdError) as e:
            call()
        assert e.value.status == 1 and "whole-mesh" in str(e.value)
    di, _ = capi.degree_info(2, 1)
    na, nb = C.c_size_t(0), C.c_size_t(0)
    L = capi.lib()
    assert L.pa_condensed_rows_coarse_query(a.ctx.h, di, 2, capi.COARSE_BY_SIDE, C.byref(na), C.byref(nb)) == 1
    assert "PA_COARSE_ONE only" in L.pa_last_error(a.ctx.h).decode()
    assert L.pa_condensed_rows_coarse_query(a.ctx.h, di, 4, capi.COARSE_ONE, C.byref(na), C.byref(nb)) == 1          # lines 0, 4: no node
    assert "coarse columns" in L.pa_last_error(a.ctx.h).decode()
    assert L.pa_condensed_rows_coarse_query(a.ctx.h, di, 0, capi.COARSE_ONE, C.byref(na), C.byref(nb)) == 1
    assert L.pa_condensed_rows_patches_query(a.ctx.h, di, 2, C.byref(na), C.byref(nb)) == 1                          # no such kind
    assert L.pa_condensed_rows_coarse_query(a.ctx.h, di, 2, capi.COARSE_ONE, C.byref(na), C.byref(nb)) == 0 and na.value == 1


# ---- 3. every iterate against the twin --------------------------------------------------------------------------------------------------
def _generic_ranks(parts, coarse=True):
    """the generic case cut at parts: per rank (context, row range, CSR rows, right-hand side, patch table, rows of P)"""
    sy = RT.generic_system()
    slabs, _, tb = RT.generic_tables(parts, coarse)
    out = []
    for (r0, r1), pt in zip(RT.generic_bounds(parts), slabs):
        a = _asm()
        rp, ci, va, b = (_dev(a, v) for v in RT.slab_rows(sy, r0, r1))
        t = RT.slab_coarse(tb, r0, r1) if coarse else None
        dc = (_dev(a, t.ptr.astype(np.int64)), _dev(a, t.cols.astype(np.int32)), _dev(a, t.vals.astype(np.float64)), t.ncoarse) if coarse else None
        out.append((a, r0, r1, rp, ci, va, b, (_dev(a, pt.ptr), _dev(a, pt.rows)), dc))
    return out


def _generic_solve(ranks, use_transport=True, **kw):
    import torch

    def body(r, transport):
        a, r0, r1, rp, ci, va, b, dp, dc = ranks[r]
        x = torch.full_like(b, float("nan"))
        _, *res = a.conjugated_gradient_rows_patch_coarse(transport(a.ctx) if use_transport else None, r0, r1, rp, ci, va, b, dp, dc, x=x, **kw)
        a.synchronize()
        return tuple(res), x.cpu().numpy()
    out = _ranks(len(ranks), body)
    for o in out:
        assert not isinstance(o, BaseException), o
    return out


@pytest.mark.parametrize("coarse", [True, False], ids=["two-level", "patches"])
@pytest.mark.parametrize("parts", RT.PARTITIONS, ids=lambda p: "%dranks" % (len(p) - 1))
def test_every_iterate(parts, coarse):
    """x_m for m = 1..8 (the call with max_iter = m - 2), the exit reason, the count and the residual, identical on every rank"""
    sy = RT.generic_system()
    tr, er = RT.truth(parts, coarse), RT.e_ref(parts, coarse)
    ranks = _generic_ranks(parts, coarse)
    worst = 0.0
    for m in range(1, len(tr.rr) + 1):
        kw, want = RT.iterate_call(parts, m, coarse)
        out = _generic_solve(ranks, **kw)
        assert len({o[0] for o in out}) == 1, [o[0] for o in out]              # reason, count and residual: the same bits everywhere
        reason, iters, rr = out[0][0]
        assert (reason, iters) == want, (m, reason, iters, want)
        x = np.concatenate([o[1] for o in out])
        g = RT.gate(er[m - 1])
        e = T.scaled_error(x, tr.x[m - 1], sy.diag)
        drr = abs(rr - tr.rr[m - 1]) / tr.rr[m - 1]
        worst = max(worst, e / g, drr / g)
        print("iterate %d ranks %s m %d: e_gpu %.3e rr %.3e e_ref %.3e gate %.3e" % (len(parts) - 1, "two-level" if coarse else "patches", m, e,
                                                                                      drr, er[m - 1], g))
        assert e <= g and drr <= g
    say("iterates  %d ranks, %-9s: largest error / gate over m = 1..8: %.3f" % (len(parts) - 1, "two-level" if coarse else "patches", worst))


# ---- 4. full solves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cd,fd,H,parts", [(12, 2, 1, 4, (0, 5, 12)), (9, 3, 2, 3, (0, 2, 5, 9)), (4, 2, 1, 2, (0, 1, 2, 3, 4))])
def test_ranks_reproduce_the_one_rank_solve_with_their_tables(N, cd, fd, H, parts):
    """the slabs' solve against the ONE-rank call given the concatenated slab tables, the same preconditioner: the count within 3 (the
    sums are grouped by rank: a step more or less at the threshold), x within 1e-7 of its scale"""
    import torch
    a, info, rp, ci, va, b, _ = _slab_system(N, cd, fd, (0, N), None)
    n = b.numel()
    b = b + _random_rhs(n, 1234 + N, a.device)
    slabs = _slabs(N, cd, fd, parts)
    tables = [(s[0].condensed_rows_patches(cd, fd, "cell"), s[0].condensed_rows_coarse(cd, fd, H)) for s in slabs]
    pt = RT.concat([PT.Patches(t[0][0].cpu().numpy(), t[0][1].cpu().numpy()) for t in tables])
    xw, *rw = a.conjugated_gradient_rows_patch_coarse(None, 0, n, rp, ci, va, b, (_dev(a, pt.ptr), _dev(a, pt.rows)), a.condensed_coarse(cd, fd, H),
                                                      tol=1e-11, max_iter=10000)
    a.synchronize()
    out = _solve_slabs(slabs, b.cpu(), H, tables=tables, cd=cd, fd=fd, tol=1e-11, max_iter=10000)
    for o in out:
        assert not isinstance(o, BaseException) and len(o) == 2, o
    assert rw[0] == 0 and all(o[0][0] == 0 for o in out) and len({o[0] for o in out}) == 1
    x = torch.cat([o[1] for o in out])
    scale = float(xw.abs().max())
    err = float((x - xw.cpu()).abs().max()) / scale
    say("solve (%d, %d, %d) H %d slabs %s: %d iterations on %d ranks, %d on one; |dx| / |x| %.2e" % (N, cd, fd, H, parts, out[0][0][1], len(slabs),
                                                                                                    rw[1], err))
    assert abs(out[0][0][1] - rw[1]) <= 3 and x.numel() == n and err < 1e-7


def test_count_against_the_point_jacobi_on_the_same_slabs():
    """the mesh tests/test_rows_pcg_cpu.py chose: the device's count is at most the twin's (textbook PCG in double on the device's own
    matrix with the slabs' tables) plus 3, and the twin's at most half of Jacobi's"""
    N, k, H, parts = RT.SOLVE_MESH
    cd, fd = k + 1, k
    a, info, rp, ci, va, b, _ = _slab_system(N, cd, fd, (0, N), None)
    n = b.numel()
    b = b + _random_rhs(n, 1234 + N, a.device)
    slabs = _slabs(N, cd, fd, parts)
    tables = [(s[0].condensed_rows_patches(cd, fd, "cell"), s[0].condensed_rows_coarse(cd, fd, H)) for s in slabs]
    two = _solve_slabs(slabs, b.cpu(), H, tables=tables, cd=cd, fd=fd, tol=1e-11, max_iter=10000)
    jac = _solve_slabs(slabs, b.cpu(), H, jacobi=True, cd=cd, fd=fd, tol=1e-11, max_iter=10000)
    for o in two + jac:
        assert not isinstance(o, BaseException) and len(o) == 2 and o[0][0] == 0, o
    pt = RT.concat([PT.Patches(t[0][0].cpu().numpy(), t[0][1].cpu().numpy()) for t in tables])
    p, c, v, nc = a.condensed_coarse(cd, fd, H)
    host = CT.Condensed(rp.cpu().numpy(), ci.cpu().numpy(), va.cpu().numpy(), b.cpu().numpy(), None, None, None, None, N, fd + 1)
    twin = CT.two_level_iterations(host, pt, CT.Table(p.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy(), nc), tol=1e-11)
    twin_jac = PT.pcg_iterations(host, "jacobi", tol=1e-11)
    say("count (%d, %d, %d) H %d slabs %s: two-level %d on the device, %d the twin's; Jacobi rows %d on the device, %d the twin's" %
        (N, cd, fd, H, parts, two[0][0][1], twin, jac[0][0][1], twin_jac))
    assert 2 * twin <= twin_jac and two[0][0][1] <= twin + 3


# ---- 5. a failure on one rank ends the solve on all of them ---------------------------------------------------------------------------
def _three_slabs():
    N, cd, fd, parts = 12, 2, 1, (0, 4, 8, 12)
    slabs = _slabs(N, cd, fd, parts)
    n = int(slabs[-1][1].row_end)
    tables = [(s[0].condensed_rows_patches(cd, fd, "face"), s[0].condensed_rows_coarse(cd, fd, 4)) for s in slabs]
    return slabs, tables, _random_rhs(n, 99, "cpu"), dict(cd=cd, fd=fd, tol=1e-13, max_iter=10000)


def _check_failure(out, bad, status_bad, error_bad):
    for r, o in enumerate(out):
        assert isinstance(o, tuple) and len(o) == 3, (r, o)
        status, text, x = o
        if r == bad:
            assert status == error_bad and "transport status %d" % status_bad in text, (r, o)
        else:
            assert status == 7 and "transport status 3" in text, (r, o)          # PA_ERR_COMM: another rank failed
        assert bool((x == 7.0).all()), r                                       # d_x as it was


def test_an_indefinite_block_on_one_rank():
    slabs, tables, b, kw = _three_slabs()
    s = list(slabs[1])
    s[4] = -s[4]                                                              # rank 1's rows negated: its patches have no Cholesky factor
    out = _solve_slabs([slabs[0], tuple(s), slabs[2]], b, 4, tables=tables, **kw)
    _check_failure(out, 1, 6, 6)                                              # PA_ERR_NOT_SPD


@pytest.mark.parametrize("defect", ["outside", "uncovered"])
def test_a_refused_table_on_one_rank(defect):
    slabs, tables, b, kw = _three_slabs()
    (ptr, rows), tb = tables[1]
    if defect == "outside":
        rows = rows.clone()
        rows[-1] = int(slabs[1][1].row_end)                                   # the first row of the rank above
    else:
        ptr, rows = ptr[:-1].clone(), rows[:int(ptr[-2])].clone()             # the last patch gone: its rows lie in no patch
    tables[1] = ((ptr, rows), tb)
    out = _solve_slabs(slabs, b, 4, tables=tables, **kw)
    _check_failure(out, 1, 5, 1)                                              # PA_ERR_INVALID_ARG
    assert ("outside the system" if defect == "outside" else "lies in no patch") in out[1][1]


@pytest.mark.parametrize("fail_rank,fail_at", [(1, 1), (0, 1), (2, 4)])
def test_a_failed_exchange_on_one_rank(fail_rank, fail_at):
    """the halo callback fails at its first call -- the exchange of P's rows -- or in the iteration"""
    slabs, tables, b, kw = _three_slabs()
    out = _solve_slabs(slabs, b, 4, tables=tables, fail_rank=fail_rank, fail_at=fail_at, **kw)
    _check_failure(out, fail_rank, 1, 7)


# ---- 6. repeatability, and the RCCL transport -----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    ranks = _generic_ranks(RT.PARTITIONS[1])
    a, b = (_generic_solve(ranks, tol=1e-12, div=T.HUGE, max_iter=400) for _ in range(2))
    assert all(u[0] == v[0] and np.array_equal(u[1], v[1]) for u, v in zip(a, b)) and a[0][0][0] == 0
    say("repeat    3 ranks: two runs of %d iterations, the same bits" % a[0][0][1])


def test_rccl_transport_of_one_rank():
    """pa_comm_cg_transport over a communicator of one rank with ncoarse = 33 > 8 values through its all-reduce: the NULL-transport call"""
    from proton_amd import capi
    ranks = _generic_ranks((0, 257))
    a = ranks[0][0]
    comm = capi.Comm(a.ctx, 1, 0, capi.comm_unique_id())
    tp = comm.cg_transport()
    a0, r0, r1, rp, ci, va, b, dp, dc = ranks[0]
    x0, *s0 = a.conjugated_gradient_rows_patch_coarse(None, r0, r1, rp, ci, va, b, dp, dc, tol=1e-12, div=T.HUGE, max_iter=400)
    x1, *s1 = a.conjugated_gradient_rows_patch_coarse(tp, r0, r1, rp, ci, va, b, dp, dc, tol=1e-12, div=T.HUGE, max_iter=400)
    a.synchronize()
    import torch
    assert s0[0] == 0 and s1 == s0 and torch.equal(x0, x1)
    comm.close()


def test_zz_report():
    """the lines of the run (with -s); written to the file ROWS_PCG_PROFILE names, if it names one"""
    path = os.environ.get("ROWS_PCG_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_rows_pcg.py on one MI355X, the ranks threads of one process: the device's error against the truth of\n"
                    "tests/rows_pcg_twin.py (longdouble), gate = max(2^-45, 10 e_ref) with e_ref the same computation in IEEE double on the\n"
                    "CPU; and the iteration counts of the full solves.\n")
            f.write("\n".join(REPORT) + "\n")
