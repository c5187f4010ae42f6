"""The judge of tests/test_gpu_cg_twin.py, judged without a device (tests/cg_twin.py): its two routes to the truth agree, the table
of e_ref meets the cap, the exit thresholds are clear of every residual they are compared with, and the defects the case table
is there to catch -- planted in the numpy restatement of the device's summation order -- fail the gate at exactly the sizes
the table names and pass it one size below."""
import math
import os

import numpy as np

import cg_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fails(case, **defect):
    """does the device-order restatement with this defect miss the gate of a judged pair of the case?"""
    errs = T.errors(case, T.recurrences(case, "dev", **defect)[0])
    er = T.e_ref(case)
    assert T.judged(case)
    return any(errs[m - 1] > T.gate(er[m - 1]) for m in T.judged(case))


def _variants(n, **kw):
    return [T.Case(n, precond, arrow, **kw) for arrow in (False, True) for precond in (True, False)]


def test_generator_keeps_its_promises():
    """symmetric, strictly dominant before the scaling (so positive definite after it), exactly L entries per row where asked, the
    columns of a row ascending or descending, the last row with the largest scale and |b| >= 1"""
    for c in T.case_table():
        if c.n > 4097:
            continue
        sy = T.system(c)
        n = c.n
        A = np.zeros((n, n)) if n <= 257 else None
        rows = np.repeat(np.arange(n), np.diff(sy.rowptr))
        lens = np.diff(sy.rowptr)
        assert sy.rowptr[0] == 0 and sy.rowptr[-1] == sy.colind.size and (lens >= 1).all()
        if c.L:
            assert (lens == c.L).all()
        if c.arrow and n > 17:
            assert lens[0] == n
        step = np.diff(sy.colind.astype(np.int64))
        inside = np.ones(sy.colind.size - 1, dtype=bool)
        inside[sy.rowptr[1:-1] - 1] = False
        assert ((step < 0) if c.reverse else (step > 0))[inside].all()
        offd = np.abs(np.where(sy.colind == rows, 0.0, sy.values)) / (sy.scale[rows] * sy.scale[sy.colind])
        assert (sy.diag / sy.scale ** 2 > 1.2 * np.add.reduceat(offd, sy.rowptr[:-1])).all()
        assert sy.scale[n - 1] == sy.scale.max()
        assert np.array_equal(sy.values[sy.colind == rows], sy.diag)
        assert abs(sy.b[n - 1]) >= 1.0
        if A is not None:
            A[rows, sy.colind] = sy.values
            assert np.array_equal(A, A.T)
    c = T.Case(257, True, False)
    pos = lambda case: int(np.nonzero(T.system(case).colind[T.system(case).rowptr[100]:T.system(case).rowptr[101]] == 100)[0][0])
    assert pos(c) == 3 and pos(c._replace(reverse=True)) == 3 and pos(c._replace(arrow=True)) == 4 and pos(c._replace(arrow=True, reverse=True)) == 3
    assert pos(T.Case(257, True, False, 16)) == 7 and T.system(T.Case(257, True, False, 16)).values.tolist().count(0.0) == 1


def test_truth_by_two_routes_agrees():
    """mpmath at 50 digits against numpy.longdouble on every case of n <= 4097.  longdouble carries 11 bits more than double, so it
    leaves the exact trajectory 2^-11 as far as the double recurrences do (e_ref), one rounding sequence's luck apart: asserted is
    max(2^-58, 2^-5 e_ref) per judged pair.  Measured: at most 2.7e-19 on the preconditioned pairs (expected near 1e-18), at most
    0.0043 e_ref on any judged pair, and the residuals of the judged pairs within one ulp (1.7e-16) of each other.
    Above 4097 rows longdouble is the truth: its error is to the gate 10 e_ref as 2^-11 is to 10."""
    worst_pre, worst_ratio, worst_rr = 0.0, 0.0, 0.0
    for c in T.case_table():
        if c.n > T.MP_ROWS:
            continue
        mp, ld, er, diag = T.truth(c, "mp"), T.truth(c, "ld"), T.e_ref(c), T.system(c).diag
        assert len(mp.rr) == len(ld.rr) == len(er)
        for j in range(len(er)):
            e = T.scaled_error(ld.x[j], mp.x[j], diag)
            if er[j] > T.CAP:              # not judged: the error saturates, its ratio to e_ref says nothing
                continue
            assert e <= max(2.0 ** -58, 2.0 ** -5 * er[j]), (T.case_id(c), j + 1, e, er[j])
            worst_ratio = max(worst_ratio, e / er[j])
            if c.precond:
                worst_pre = max(worst_pre, e)
            if mp.rr[j] >= T.EXACT and er[j] <= T.CAP:
                drr = abs(ld.rr[j] - mp.rr[j]) / mp.rr[j]
                assert drr <= max(2.0 ** -51, 2.0 ** -5 * er[j]), (T.case_id(c), j + 1, drr)
                worst_rr = max(worst_rr, drr)
            elif mp.rr[j] < T.EXACT:
                assert ld.rr[j] < 1e-17
    print("truth, longdouble against mpmath: preconditioned pairs <= %.3e, every judged pair <= %.3e e_ref, residuals <= %.3e relative"
          % (worst_pre, worst_ratio, worst_rr))


def test_table_meets_the_cap():
    """A pair is judged only where e_ref <= 1e-10.  At most 5 % of the pairs are left out, none with m <= 3, none with the
    preconditioner on; the floor is the largest preconditioned e_ref rounded up to a power of two, and the committed table says so."""
    print("\n".join(T.table_lines()))
    pairs = [(c, m, e) for c in T.case_table() for m, e in enumerate(T.e_ref(c), 1)]
    out = [(c, m, e) for c, m, e in pairs if e > T.CAP]
    assert len(out) <= 0.05 * len(pairs), (len(out), len(pairs))
    assert all(m > 3 and not c.precond for c, m, e in out), out
    for c in T.case_table():
        M = len(T.truth(c).rr)
        assert M == min(T.M_MAX, c.n) or (c.L == 1 and c.precond and M == 1)      # a diagonal matrix under Jacobi: done in one step
        assert len(T.e_ref(c)) == M
    worst = max(e for c, m, e in pairs if c.precond)
    assert worst <= T.FLOOR == T.pow2_ceil(T.FLOOR) and T.FLOOR < 4.0 * worst, worst      # the recorded power of two still is the one above it
    with open(os.path.join(ROOT, "profiles", "cg_twin_parity.txt")) as f:
        text = f.read()
    assert "floor 2^%d" % round(math.log2(T.FLOOR)) in text
    for c, m, e in out:
        assert "%s m %d" % (T.case_id(c), m) in text.split("left out:")[1].split("\n")[0]


def test_thresholds_are_clear_of_the_residuals():
    """every call of the device test has its exit defined by truth's residual history, and no residual within 1e-3 (relative) of a
    threshold it is compared with"""
    ncalls = 0
    for c in T.case_table():
        rr = T.truth(c).rr
        for m in range(1, len(rr) + 1):
            kw, want = T.iterate_call(c, m)
            assert want == ((0, 0) if m == 1 and rr[0] < T.EXACT else (1, 0) if m == 1 else (2, m - 1))
        calls = T.threshold_calls(c)
        assert calls or len(rr) < 2 or c.n == 2
        for kw, want in calls:
            assert want is not None and T.thresholds_clear(c, kw), (T.case_id(c), kw)
            ncalls += 1
    assert ncalls > 200


# ---- the planted defects ---------------------------------------------------------------------------------------------------------
def test_unplanted_restatement_passes_everywhere():
    for c in T.case_table():
        assert not _fails(c)


def test_lost_vector_partials_show_at_65537():
    """only the first 256 per-block partials of r . r and r . M^-1 r summed: 65537 rows make 257"""
    for c in _variants(65537):
        assert _fails(c, vec_parts=RB), T.case_id(c)
    for c in _variants(65536):
        assert not _fails(c, vec_parts=RB), T.case_id(c)


def test_lost_spmv_partials_show_at_4097():
    """only the first 256 per-block partials of d . A d summed: 16 lanes a row, 4097 rows make 257"""
    for c in _variants(4097):
        assert _fails(c, spmv_parts=RB), T.case_id(c)
    for c in _variants(4096):
        assert not _fails(c, spmv_parts=RB), T.case_id(c)


def test_rows_cut_at_their_16th_entry_show_at_17():
    for precond in (True, False):
        assert _fails(T.Case(257, precond, False, 17), row_cap=T.ROW_LANES)
        assert _fails(T.Case(257, precond, False, 33), row_cap=T.ROW_LANES)
        assert _fails(T.Case(257, precond, True), row_cap=T.ROW_LANES)
        assert not _fails(T.Case(257, precond, False, 16), row_cap=T.ROW_LANES)
        assert not _fails(T.Case(257, precond, False, 15), row_cap=T.ROW_LANES)
        assert not _fails(T.Case(257, precond, False), row_cap=T.ROW_LANES)


def test_preconditioner_in_one_place_only_shows_everywhere():
    """1 / diag in rho and not in the search direction: wrong from x_1 on wherever the preconditioner is on (from x_2 on for one
    row, where x_1 is the solution whatever the step length's numerator), the same bits where it is off"""
    for c in T.case_table():
        if c.n > T.MP_ROWS:
            continue
        if c.precond:
            errs = T.errors(c, T.recurrences(c, "dev", precond_in_d=False)[0])
            assert errs[0] > 1e-3, (T.case_id(c), errs[0])
            assert _fails(c, precond_in_d=False)
        else:
            a, b = T.recurrences(c, "dev", precond_in_d=False), T.recurrences(c, "dev")
            assert all(np.array_equal(u, v) for u, v in zip(a[0], b[0]))


RB = T.RB
