"""What tests/golden/make_golden_post.py, tests/test_oracle_hard_post.py and tests/test_gpu_hard_post.py share: the test
function f_c of a cell, the names of the judged quantities, their floors and the gate.

f_c(x, y) = 2 + sin(3 (x - x0) / hs) cos(2 (y - y0) / hs), with (x0, y0) the lower left corner of the cell's bounding box
and hs the power of two nearest to the box's larger side.  Its values lie in [1, 3]: it vanishes nowhere (sin pi x sin pi y
vanishes at every quadrature point of a cell with integer vertices, and its mean vanishes on the rotated square), and it
varies by O(1) across a cell of any size, so a projection of it has an honest relative norm.  x0, y0 and hs are doubles
taken from the double vertex list; the 50-digit evaluation uses the same three numbers, so both sides project one
function."""
import math

import numpy as np

# the projection blocks, then the recovery of the eliminated cell unknowns
QUANTITIES = ("proj0_cell", "proj0_face", "proj1_cell", "proj1_face", "sin_cell", "sin_face", "R", "r0", "uT")
# the project's floors (make_golden_hard.FLOOR): a projection is a mass solve of a right-hand side, as `rhs`; R, r0 and uT
# sit behind one solve with A_TT, as `S` and `g`
FLOOR = {"proj0_cell": 1e-12, "proj0_face": 1e-12, "proj1_cell": 1e-12, "proj1_face": 1e-12, "sin_cell": 1e-12,
         "sin_face": 1e-12, "R": 1e-11, "r0": 1e-11, "uT": 1e-11}
DROP_ABOVE = 1e-7          # e_ref beyond this: stored, not gated
STORED = ("proj0", "proj1", "proj_sin", "fT", "uF", "R", "r0", "uT")


def fc_params(pts):
    """(x0, y0, hs) of the double vertex list pts[4][2]"""
    p = np.asarray(pts, dtype=np.float64)
    x0, y0 = float(p[:, 0].min()), float(p[:, 1].min())
    ext = max(float(p[:, 0].max()) - x0, float(p[:, 1].max()) - y0)
    return x0, y0, 2.0 ** round(math.log2(ext))


def fc(params, x, y, sin=np.sin, cos=np.cos):
    """f_c at (x, y): numpy arrays, floats (sin=math.sin, cos=math.cos) or mpmath numbers (sin=mp.sin, cos=mp.cos)"""
    x0, y0, hs = params
    return 2 + sin(3 * (x - x0) / hs) * cos(2 * (y - y0) / hs)


def fc_host(pts):
    """f_c of the cell as a double function of two doubles (the oracle's callback)"""
    prm = fc_params(pts)
    return lambda x, y: fc(prm, x, y, math.sin, math.cos)


def gate(q, e_ref):
    """as tests/test_gpu_hard_cells.judge"""
    return max(FLOOR[q], 10.0 * e_ref)


def blocks(cd):
    """slices of the cell part and of the face part of a projection (cell part first, then the four faces in local order)"""
    cbs = (cd + 2) * (cd + 1) // 2
    return slice(0, cbs), slice(cbs, None)


def nerr(got, truth, at_least=1e-300):
    """max-norm error over the max-norm of the truth"""
    return float(np.abs(np.asarray(got) - truth).max() / max(np.abs(truth).max(), at_least))


def check(cases, quantities, e_ref, dropped, log=print):
    """The conditions on the inputs the generator enforces before it writes, and tests/test_oracle_hard_post.py on the stored
    file -> list of violations.  NaN marks a pair that is not applicable (listed by the caller in `na`)."""
    bad = []
    quantities = list(quantities)
    dropped = set(dropped)
    gated = above = 0
    for j, q in enumerate(quantities):
        nq = nd = na = 0
        for i, c in enumerate(cases):
            e = float(e_ref[i, j])
            key = "%s|%s" % (c, q)
            if np.isnan(e):
                na += 1
                if key in dropped:
                    bad.append("%s: not applicable, yet listed as dropped" % key)
                continue
            nq += 1
            if not np.isfinite(e) or e < 0:
                bad.append("%s: e_ref %r" % (key, e))
                continue
            if (e > DROP_ABOVE) != (key in dropped):
                bad.append("%s: e_ref %.2e and the dropped list disagree" % (key, e))
            if e > DROP_ABOVE:
                nd += 1
                continue
            gated += 1
            above += 10.0 * e > FLOOR[q]
        log("%-10s cases %3d, not applicable %2d, dropped %2d (%.1f %%)" % (q, nq, na, nd, 100.0 * nd / max(nq, 1)))
        if 100 * nd > 12 * nq:
            bad.append("%s: %d of %d cases dropped: more than 12 %%" % (q, nd, nq))
    log("gated (case, quantity) pairs: %d, of which 10 e_ref is above the floor on %d (%.1f %%); dropped: %d"
        % (gated, above, 100.0 * above / max(gated, 1), len(dropped)))
    if 3 * above > gated:
        bad.append("10 e_ref is above the floor on %d of %d gated pairs: more than one third" % (above, gated))
    return bad
