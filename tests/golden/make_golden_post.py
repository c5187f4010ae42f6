#!/usr/bin/env python3
"""Generate tests/golden/hard_cells_post.npz: on the 155 cases of hard_cells.npz (same cases, same order), the 50-digit
evaluation of what turns the local operators into the numbers a user reads -- the L2 projections of project_function on the
cell and on its four faces (which are also the Dirichlet data of a boundary face), and the recovery of the eliminated cell
unknowns -- together with e_ref, the error of the CPU oracle (the reference's operation order in double precision) against
that truth, worst over the cell's eight relabelings.

Geometry, rules, bases and local_ops are make_golden's (imported); the cases, the relabelings and the oracle's operators
are make_golden_hard's (imported).  make_golden.gauss stops at five nodes and the pair (4,3) with a degree increase of one
needs six, so gauss() below adds a 50-digit Gauss-Legendre rule for more nodes (inside this process only:
local_ops.npz and hard_cells.npz never see it).

The projected function is f_c of tests/hard_post.py, rebuilt from the vertex list of every relabeling.

Per case, base labelling, key `name|cd|fd|kind|what`:
  proj0, proj1  [msize]     project_function of f_c with dinc = 0, 1: mass matrix and right-hand side at the rule of degree
                            2 (cd + dinc) / 2 (fd + dinc), exact solve; the cell part, then the four faces in local order, the
                            face bases running from the lower-id endpoint.  No proj1 where the rule does not exist in the
                            reference (the fan at degree 8: rules[8] is empty; that is (3,2) fan)
  proj_sin      [msize]     the same with dinc = 0 for sin(pi x) sin(pi y), the drivers' boundary function
  fT            [cbs]       the cell right-hand side int f_c phi_i at the rule of degree 2 cd, rounded to double
  uF            [nf]        the face part of proj0, rounded to double
  R             [cbs, nf]   -A_TT^-1 A_TF of the 50-digit lc = data + fancy
  r0, uT        [cbs]       A_TT^-1 fT and r0 + R uF, the stored doubles fT and uF taken as exact inputs
and
  cases, quantities, e_ref [ncase, nq], dropped   as in hard_cells.npz; e_ref is NaN where a quantity does not apply

Every error is the max-norm error of the block over the max-norm of its truth, except sin_cell / sin_face, which are
normalised by max(|truth|, 1): sup |sin sin| = 1, and the function is small or zero on some cells.

The oracle's values: oracle_lib.project_function with f_c (or the built-in function 2) for the projections;
oracle_lib.static_condensation(the oracle's lc_fancy, fT, cbs) for R (columns 1.. of its rec) and r0 (column 0); numpy's
rec[:, 0] + rec[:, 1:] @ uF for uT.

The gates of tests/test_gpu_hard_post.py are max(floor, 10 e_ref) with the floors of tests/hard_post.py.  The file is not
written unless hard_post.check() passes (tests/test_oracle_hard_post.py asserts the same on the stored file): status 0 and
finite values on all eight relabelings, `dropped` exactly the pairs with e_ref > 1e-7, at most 12 % of a quantity's cases
dropped, 10 e_ref above the floor on at most a third of the gated pairs.  Were a quantity to miss a cap, whole shapes
would leave that quantity through REMOVED, with the reason written there -- never single cells.

Run:  python tests/golden/make_golden_post.py [processes]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

import hard_post as HP  # noqa: E402

# quantity -> shape names taken out of it (whole shapes; e_ref NaN, not gated).  Empty: every cap holds on the full lists.
REMOVED = {}

_gl_cache = {}


def gauss_legendre(n):
    """n-point Gauss-Legendre rule to the working precision: roots of P_n by Newton from the Chebyshev-like guesses,
    weights 2 / ((1 - x^2) P_n'(x)^2)"""
    import mpmath as mp
    import make_golden  # noqa: F401  (sets the working precision)
    assert mp.mp.dps >= 50
    if n not in _gl_cache:
        P = lambda t: mp.legendre(n, t)                                              # noqa: E731
        dP = lambda t: n * (t * mp.legendre(n, t) - mp.legendre(n - 1, t)) / (t * t - 1)   # noqa: E731
        rule = []
        for k in range(1, n + 1):
            x = mp.findroot(P, mp.cos(mp.pi * (k - mp.mpf(1) / 4) / (n + mp.mpf(1) / 2)), df=dP, solver="newton")
            x -= P(x) / dP(x)                      # findroot stops at its tolerance; one more step reaches the working precision
            rule.append((x, 2 / ((1 - x * x) * dP(x) ** 2)))
        rule.sort(key=lambda r: r[0])
        assert all(rule[i + 1][0] - rule[i][0] > mp.mpf(1) / (4 * n * n) for i in range(n - 1))     # n distinct roots
        assert abs(sum(w for _, w in rule) - 2) < mp.mpf(10) ** (-40)
        assert abs(sum(w * x ** (2 * n - 2) for x, w in rule) - mp.mpf(2) / (2 * n - 1)) < mp.mpf(10) ** (-40)
        _gl_cache[n] = rule
    return _gl_cache[n]


def golden():
    """make_golden with its gauss() extended beyond five nodes"""
    import make_golden as G
    if not getattr(G.gauss, "extended", False):
        five = G.gauss

        def gauss(degree):
            n = ((degree | 1) + 1) // 2
            return five(degree) if n <= 5 else gauss_legendre(n)
        gauss.extended = True
        G.gauss = gauss
    return G


def mp_points(pts):
    import mpmath as mp
    return [(mp.mpf(float(pts[i, 0])), mp.mpf(float(pts[i, 1]))) for i in range(4)]


def f_truth(pts, what):
    """the 50-digit function of two mpmath numbers: f_c of the vertex list, or sin(pi x) sin(pi y)"""
    import mpmath as mp
    if what == "sin":
        return lambda x, y: mp.sin(mp.pi * x) * mp.sin(mp.pi * y)
    prm = HP.fc_params(pts)
    return lambda x, y: HP.fc(prm, x, y, mp.sin, mp.cos)


def project_truth(pts, ids, cd, fd, kind, f, dinc, swap_face=None):
    """project_function in 50 digits -> (coefficients [msize], cell right-hand side [cbs]) as lists of mpmath numbers, or
    None where the cell rule does not exist.  swap_face: that local face's basis runs from the HIGHER-id endpoint (what a
    kernel with (lo, hi) swapped would compute; the negative control of tests/test_oracle_hard_post.py)"""
    import mpmath as mp
    G = golden()
    P = mp_points(pts)
    cbs, fbs = (cd + 2) * (cd + 1) // 2, fd + 1
    bar, h = G.barycenter(P), G.diameter(P)
    qps = G.cell_qps(P, kind, 2 * (cd + dinc))
    if not qps:
        return None
    M, b = mp.zeros(cbs, cbs), mp.zeros(cbs, 1)
    for (x, y, w) in qps:
        ph = G.cell_phi(bar, h, cd, x, y)
        fv = f(x, y)
        for i in range(cbs):
            b[i] += w * ph[i] * fv
            for j in range(cbs):
                M[i, j] += w * ph[i] * ph[j]
    out = list(G.solve(M, b))
    for lf in range(4):
        a, c = G.face_pts(P, tuple(int(i) for i in ids), lf)
        if lf == swap_face:
            a, c = c, a
        Mf, bf = mp.zeros(fbs, fbs), mp.zeros(fbs, 1)
        for (x, y, w) in G.face_qps(a, c, 2 * (fd + dinc)):
            ph = G.face_phi(a, c, fd, x, y)
            fv = f(x, y)
            for i in range(fbs):
                bf[i] += w * ph[i] * fv
                for j in range(fbs):
                    Mf[i, j] += w * ph[i] * ph[j]
        out += list(G.solve(Mf, bf))
    return out, list(b)


def to_vec(v):
    return np.array([float(x) for x in v], dtype=np.float64)


def truth_eval(pts, ids, cd, fd, kind):
    """-> dict of the stored arrays of one labelling (proj1 None where it does not exist)"""
    import mpmath as mp
    G = golden()
    cbs = (cd + 2) * (cd + 1) // 2
    fc = f_truth(pts, "fc")
    p0, rhs = project_truth(pts, ids, cd, fd, kind, fc, 0)
    p1 = project_truth(pts, ids, cd, fd, kind, fc, 1)
    ps, _ = project_truth(pts, ids, cd, fd, kind, f_truth(pts, "sin"), 0)
    t = {"proj0": to_vec(p0), "proj1": None if p1 is None else to_vec(p1[0]), "proj_sin": to_vec(ps), "fT": to_vec(rhs)}
    t["uF"] = t["proj0"][cbs:].copy()
    ops = G.local_ops(mp_points(pts), tuple(int(i) for i in ids), cd, fd, kind)
    lc = ops["data"] + ops["fancy"]
    inv = mp.inverse(lc[0:cbs, 0:cbs])
    R = -inv * lc[0:cbs, cbs:]
    r0 = inv * mp.matrix([mp.mpf(float(v)) for v in t["fT"]])
    uT = r0 + R * mp.matrix([mp.mpf(float(v)) for v in t["uF"]])
    t.update(R=G.to_np(R), r0=to_vec(r0), uT=to_vec(uT))
    return t


def oracle_eval(O, H, pts, ids, cd, fd, kind, fT, uF):
    """the oracle's values of the same -> (status, dict); fT and uF are the truth's doubles"""
    di = O.degrees(cd, fd)
    quad = O.QUAD_TENSOR if kind == "tensor" else O.QUAD_FAN
    fc = HP.fc_host(pts)
    st0, p0 = O.project_function(pts, ids, di, fc, quad, 0)
    st1, p1 = O.project_function(pts, ids, di, fc, quad, 1)
    sts, ps = O.project_function(pts, ids, di, 2, quad, 0)                      # hho_builtin_fn(2): sin(pi x) sin(pi y)
    stl, ops = H.oracle_eval(O, pts, ids, cd, fd, kind)
    stc, _, _, rec = O.static_condensation(ops["lc_fancy"], fT, di.cbs)
    got = {"proj0": p0, "proj1": p1, "proj_sin": ps, "R": rec[:, 1:], "r0": rec[:, 0], "uT": rec[:, 0] + rec[:, 1:] @ uF}
    return {"proj0": st0, "proj1": st1, "proj_sin": sts, "rec": stl or stc}, got


def errors(got, t, cd):
    """the nine error quantities of one labelling; NaN where proj1 does not exist"""
    cell, face = HP.blocks(cd)
    e = {}
    for key, name, floor in (("proj0", "proj0", 1e-300), ("proj1", "proj1", 1e-300), ("sin", "proj_sin", 1.0)):
        for blk, sl in (("cell", cell), ("face", face)):
            e["%s_%s" % (key, blk)] = np.nan if t[name] is None else HP.nerr(got[name][sl], t[name][sl], floor)
    for q in ("R", "r0", "uT"):
        e[q] = HP.nerr(got[q], t[q])
    return e


def one_case(case):
    """-> (stored arrays of the base labelling, e_ref row, worst status, all finite)"""
    import make_golden_hard as H
    import oracle_lib as O
    group, name, pts, ids, cd, fd, kind = case
    e_ref = np.zeros(len(HP.QUANTITIES))
    base, status, finite = None, 0, True
    for img, p in enumerate(H.relabelings(pts)):
        t = truth_eval(p, ids, cd, fd, kind)
        st, got = oracle_eval(O, H, p, ids, cd, fd, kind, t["fT"], t["uF"])
        for k, v in st.items():
            if k == "proj1" and t["proj1"] is None:
                continue                   # the rule does not exist: whatever the oracle returns is not looked at
            status = status or v
            names = ("R", "r0", "uT") if k == "rec" else (k,)
            finite = finite and all(np.isfinite(got[n]).all() for n in names)
        e = errors(got, t, cd)
        e_ref = np.where(np.isnan([e[q] for q in HP.QUANTITIES]), np.nan, np.fmax(e_ref, [e[q] for q in HP.QUANTITIES]))
        if img == 0:
            base = t
    for q, shapes in REMOVED.items():
        if name in shapes:
            e_ref[HP.QUANTITIES.index(q)] = np.nan
    return base, e_ref, status, finite


def main():
    import multiprocessing
    import time
    import make_golden_hard as H
    import oracle_lib as O
    O.lib()                                  # build the oracle once, before the workers load it
    assert all(HP.FLOOR[q] == H.FLOOR["rhs"] for q in HP.QUANTITIES[:6]) and all(HP.FLOOR[q] == H.FLOOR["S"] for q in HP.QUANTITIES[6:])
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1)
    cl = H.case_list()
    names = ["%s|%d|%d|%s" % (c[1], c[4], c[5], c[6]) for c in cl]
    hard = np.load(os.path.join(HERE, "hard_cells.npz"))
    assert names == [str(c) for c in hard["cases"]], "the cases are not those of hard_cells.npz"
    t0 = time.time()
    with multiprocessing.Pool(nproc) as pool:
        results = pool.map(one_case, cl, chunksize=1)
    out = {}
    e_ref = np.zeros((len(cl), len(HP.QUANTITIES)))
    fail = []
    for i, (cname, (base, e, status, finite)) in enumerate(zip(names, results)):
        if status != 0 or not finite:
            fail.append("%s: oracle status %d, finite %s on one of the eight relabelings" % (cname, status, finite))
        e_ref[i] = e
        for k in HP.STORED:
            if base[k] is not None:
                out["%s|%s" % (cname, k)] = base[k]
        print(cname, " ".join("%s %.1e" % (q, x) for q, x in zip(HP.QUANTITIES, e)), flush=True)
    dropped = ["%s|%s" % (c, q) for i, c in enumerate(names) for j, q in enumerate(HP.QUANTITIES) if e_ref[i, j] > HP.DROP_ABOVE]
    fail += HP.check(names, HP.QUANTITIES, e_ref, dropped)
    na = ["%s|%s" % (c, q) for i, c in enumerate(names) for j, q in enumerate(HP.QUANTITIES) if np.isnan(e_ref[i, j])]
    print("not applicable:", " ".join(na))
    if fail:
        print("\n".join(fail))
        raise SystemExit("conditions on the inputs do not hold: nothing written")
    out.update(cases=np.array(names), quantities=np.array(HP.QUANTITIES), e_ref=e_ref, dropped=np.array(dropped, dtype=str))
    path = os.path.join(HERE, "hard_cells_post.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "hard_cells.npz"))
    print("all conditions on the inputs hold; wrote", path, os.path.getsize(path), "bytes in %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
