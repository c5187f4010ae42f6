"""pa_conjugated_gradient, pa_conjugated_gradient_rows: every iterate against the twin of tests/cg_twin.py.

The converged solution cannot tell a solver with a lost partial sum, a dropped row entry or a half-applied preconditioner from a right
one -- CG corrects itself.  The m-th iterate can, and the public entry point returns it: div = 0 leaves after the first update,
max_iter = m - 2 with tol = 0 after the m-th (solver_cg.hpp:113-126).  Each x_m, m = 1..min(8, n), is compared with the 50-digit
(n <= 4097) or longdouble truth in the norm max |dx_i| sqrt(A_ii) / max |x_i| sqrt(A_ii); the gate is max(floor, 10 e_ref), e_ref the
error of the same recurrences in IEEE double (worst of the sequential and the device's summation order), floor = 2^-45 the largest
e_ref of the preconditioned cases -- all of it measured on the CPU (tests/test_cg_twin_cpu.py, which also shows that the sizes of the
table are the ones at which planted defects show).  Pairs with e_ref > 1e-10 are shown, not judged.  One run: profiles/cg_twin_parity.txt."""
import os
import threading

import numpy as np
import pytest

import cg_twin as T
from cg_transport import ThreadTransport

pytestmark = pytest.mark.gpu

DEVICE, DEVICE_RR = {}, {}     # (case, m) -> the device's error; the residual's error over the gate (judged pairs): for the report


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def _upload(a, sy, rows=None):
    """the system (or its rows [r0, r1) with a local rowptr and global columns) on a's device"""
    import torch
    r0, r1 = rows or (0, sy.n)
    k0, k1 = int(sy.rowptr[r0]), int(sy.rowptr[r1])
    dev = lambda v: torch.tensor(np.ascontiguousarray(v)).to(a.device)
    return dev(sy.rowptr[r0:r1 + 1] - k0), dev(sy.colind[k0:k1]), dev(sy.values[k0:k1]), dev(sy.b[r0:r1])


def _cg(a, dv, x=None, rows=None, transport=False, **kw):
    """one call -> (x on the host, reason, iterations, relative residual); x starts as NaN unless given"""
    import torch
    rp, ci, va, b = dv
    if x is None:
        x = torch.full_like(b, float("nan"))
    p = lambda t: t.data_ptr()
    precond = kw.pop("precond")
    if rows is None and transport is False:
        res = a.ctx.conjugated_gradient(b.numel(), p(rp), p(ci), p(va), p(b), p(x), precond=precond, **kw)
    else:
        r0, r1 = rows
        res = a.ctx.conjugated_gradient_rows(transport or None, r0, r1, p(rp), p(ci), p(va), p(b), p(x), precond=precond, **kw)
    a.synchronize()
    return (x.cpu().numpy(),) + tuple(res)


def _judge(case, m, x, rr, what=""):
    """x_m and the relative residual against truth at the pair's gate -> the error (asserted only where the pair is judged)"""
    tr, er = T.truth(case), T.e_ref(case)
    g = T.gate(er[m - 1])
    e = T.scaled_error(x, tr.x[m - 1], T.system(case).diag)
    t = tr.rr[m - 1]
    # the residual relative to its own size; where CG has terminated exactly (truth's residual is zero) to |r_0|, the largest before it
    drr = abs(rr - t) / t if t >= T.EXACT else rr
    kept = er[m - 1] <= T.CAP
    print("%s%s m %d: e_gpu %.3e rr %.3e e_ref %.3e gate %.3e ratio %.3f%s" % (what, T.case_id(case), m, e, drr, er[m - 1], g, max(e, drr) / g,
                                                                              "" if kept else "  (not judged)"))
    if kept:
        if not what:
            DEVICE_RR[(case, m)] = drr / g
        assert e <= g, (T.case_id(case), m, e, g)
        assert drr <= g, (T.case_id(case), m, drr, g)
    return e


@pytest.mark.parametrize("case", T.case_table(), ids=T.case_id)
def test_every_iterate_and_every_exit(asm, case):
    sy = T.system(case)
    dv = _upload(asm, sy)
    tr = T.truth(case)
    xs = {}
    for m in range(1, len(tr.rr) + 1):
        kw, want = T.iterate_call(case, m)
        x, reason, iters, rr = _cg(asm, dv, precond=case.precond, **kw)
        assert (reason, iters) == want, (m, reason, iters, want)
        DEVICE[(case, m)] = _judge(case, m, x, rr)
        xs[m] = x
    # tol and div between two successive residuals of truth: the exit order of solver_cg.hpp:113-126 on truth's history, exactly;
    # and the iterate it leaves with is the one the other route to it gave, bit for bit
    for kw, want in T.threshold_calls(case):
        x, reason, iters, rr = _cg(asm, dv, precond=case.precond, **kw)
        assert (reason, iters) == want[:2], (kw, reason, iters, want)
        assert np.array_equal(x, xs[want[2] + 1], equal_nan=True)


def test_contract_of_the_entry_point(asm):
    """deterministic run to run; x is an output only; the system is read only; n = 0 and b = 0 are solved by x = 0 without a step;
    a row without its diagonal entry under Jacobi leaves through the NaN test as DIVERGED at iteration 0"""
    import torch
    case = T.Case(257, True, True)
    sy = T.system(case)
    dv = _upload(asm, sy)
    keep = [t.clone() for t in dv]
    kw = dict(precond=True, tol=0.0, div=T.HUGE, max_iter=5)
    x0, *s0 = _cg(asm, dv, **kw)
    x1, *s1 = _cg(asm, dv, **kw)
    x2, *s2 = _cg(asm, dv, x=torch.zeros_like(dv[3]), **kw)
    x3, *s3 = _cg(asm, dv, x=torch.full_like(dv[3], 1e300), **kw)
    assert s0 == s1 == s2 == s3 and s0[:2] == [2, 6] and np.isfinite(x0).all()
    assert np.array_equal(x0, x1) and np.array_equal(x0, x2) and np.array_equal(x0, x3)
    assert all(torch.equal(a, b) for a, b in zip(keep, dv))
    # n = 0: nothing is read or written
    x = torch.full((4,), 7.0, dtype=torch.float64, device=asm.device)
    res = asm.ctx.conjugated_gradient(0, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), x.data_ptr())
    asm.synchronize()
    assert tuple(res) == (0, 0, 0.0) and bool((x == 7.0).all())
    # b = 0
    for precond in (True, False):
        xz, *sz = _cg(asm, (dv[0], dv[1], dv[2], torch.zeros_like(dv[3])), precond=precond, tol=1e-9, div=100.0, max_iter=1000)
        assert sz == [0, 0, 0.0] and (xz == 0.0).all() and not np.signbit(xz).any()
    # row 3 without its diagonal entry
    k = int(sy.rowptr[3] + np.nonzero(sy.colind[sy.rowptr[3]:sy.rowptr[4]] == 3)[0][0])
    rp = sy.rowptr.copy()
    rp[4:] -= 1
    cut = T.System(sy.n, rp, np.delete(sy.colind, k), np.delete(sy.values, k), sy.b, sy.diag, sy.scale)
    xd, *sd = _cg(asm, _upload(asm, cut), precond=True, tol=1e-9, div=100.0, max_iter=1000)
    assert sd[:2] == [1, 0] and np.isnan(sd[2])
    # (without the preconditioner the diagonal is not looked for: an ordinary solve of another matrix, which need not converge)
    xd, *sd = _cg(asm, _upload(asm, cut), precond=False, tol=0.0, div=T.HUGE, max_iter=0)
    assert sd[:2] == [2, 1] and np.isfinite(xd).all()


@pytest.mark.parametrize("case", [T.Case(n, precond, arrow) for n in (257, 4097, 65537) for arrow in (False, True) for precond in (True, False)],
                         ids=T.case_id)
def test_rows_solver_of_one_rank(asm, case):
    """pa_conjugated_gradient_rows without a transport (the kernels with the window view CgRowsWindow and by-value scalars,
    cg_reduce_kernel in mode 3): every iterate at the twin's gate, and the bits of pa_conjugated_gradient -- at 257 rows, at 4097 (second trip over the SpMV partials) and 65537 (over the vector's)"""
    sy = T.system(case)
    dv = _upload(asm, sy)
    for m in range(1, len(T.truth(case).rr) + 1):
        kw, want = T.iterate_call(case, m)
        x, reason, iters, rr = _cg(asm, dv, rows=(0, sy.n), precond=case.precond, **kw)
        assert (reason, iters) == want
        _judge(case, m, x, rr, "rows ")
        x0, *s0 = _cg(asm, dv, precond=case.precond, **kw)
        assert np.array_equal(x, x0) and s0 == [reason, iters, rr]


@pytest.mark.parametrize("precond", [True, False], ids=["jacobi", "plain"])
def test_rows_solver_of_three_ranks(precond):
    """4500 rows of the band over three thread-ranks (three contexts), parts (0, 17, 300, 4500): the first rank is exactly as tall as
    the band, so all of it travels to its neighbour and its whole window beyond arrives from there; the last rank's 4200 rows make
    263 SpMV partials, a second trip of cg_reduce_kernel.  The sums are grouped by rank, so these are not the one-rank bits: the judge
    is the twin (truth in longdouble), every iterate at its gate, every exit as truth's history gives it, on every rank."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    case = T.Case(4500, precond, False)
    sy = T.system(case)
    parts = (0, 17, 300, 4500)
    R = len(parts) - 1
    calls = [T.iterate_call(case, m) + (m,) for m in range(1, len(T.truth(case).rr) + 1)]
    calls += [(kw, want[:2], want[2] + 1) for kw, want in T.threshold_calls(case)]
    asms = [BatchAssembler(0) for _ in range(R)]
    dvs = [_upload(asms[r], sy, (parts[r], parts[r + 1])) for r in range(R)]
    tt = ThreadTransport(R)
    out, keep = [None] * R, []

    def run(r):
        try:
            tp, cbs = tt.make(r, asms[r].ctx)
            keep.append(cbs)
            out[r] = [_cg(asms[r], dvs[r], rows=(parts[r], parts[r + 1]), transport=tp, precond=precond, **kw) for kw, _, _ in calls]
        except BaseException as e:      # noqa: BLE001  (a failed rank must not leave the others at a barrier)
            out[r] = e
            tt.bar.abort()

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert all(not t.is_alive() for t in th)
    for o in out:
        assert not isinstance(o, BaseException), o
    assert len(T.judged(case)) >= 4
    for k, (kw, want, m) in enumerate(calls):
        res = [out[r][k] for r in range(R)]
        assert all(tuple(o[1:3]) == want for o in res), (kw, [o[1:] for o in res], want)
        assert len({o[3] for o in res}) == 1
        _judge(case, m, np.concatenate([o[0] for o in res]), res[0][3], "3 ranks ")


def test_zz_report():
    """the table of the run (with -s); written to the file CG_TWIN_PROFILE names, if it names one"""
    lines = T.table_lines(DEVICE or None, DEVICE_RR or None)
    print("\n".join(lines))
    path = os.environ.get("CG_TWIN_PROFILE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
