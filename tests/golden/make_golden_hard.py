#!/usr/bin/env python3
"""Generate tests/golden/hard_cells.npz: the 50-digit evaluations of make_golden.py (imported, not copied) on cells that
are hard for the local operators -- extreme aspect ratios, near-degenerate quadrilaterals, tiny and huge scales, every
achievable orientation pattern of the four face bases -- together with e_ref, the error of the CPU oracle (the
reference's operation order in double precision) against that truth on the same cell.

Per (shape, cd, fd, quad) the file holds oper, data, naive, fancy, rhs, S, g of the BASE labelling under the key scheme of
local_ops.npz, `name|cd|fd|kind|what`, and next to them

  cases       [ncase]        "name|cd|fd|kind", the order of every per-case array below
  case_group  [ncase]        "good", "orientation" or "graded"
  case_pts    [ncase, 4, 2]  the vertices, counter-clockwise
  case_ids    [ncase, 4]     the point ids, a permutation of 0..3: ids decide the face-basis orientation
  quantities  [nq]           oper, data, naive, fancy, rhs, S, g, lc_fancy, lc_naive (lc_* = data + stabilization)
  e_ref       [ncase, nq]    the oracle's normwise error, WORST OVER THE EIGHT RELABELINGS of the cell: four cyclic rolls of
                             the vertex list times a mirror image, the id tuple staying with the positions (so that every
                             relabeling has a fresh orientation of its faces); the truth is recomputed for every relabeling.
                             g is normalised by max(|g|, |rhs|) as tests/test_gpu_condensed.py does.
  dropped     [ndrop]        "name|cd|fd|kind|what" with e_ref > 1e-7: stored, not gated

e_ref is recorded output of the reference-order algorithm: the gates of tests/test_gpu_hard_cells.py are
max(floor, 10 * e_ref).  The generator refuses to write the file unless the conditions on the INPUTS hold (check()), which
tests/test_oracle_hard_cells.py asserts again on the stored file.

Shapes and configs are the lists below.  Two configs of the first plan are left out because they miss a condition on
the inputs (REMOVED): on the kite at (4,3) the oracle's fancy stabilization is 1.14e-13 from the truth on its worst
relabeling, not below 1e-13; on the 5-degree parallelogram at (4,3) the oracle returns status 3 (a pivot that is not
positive) and NaN on one of the eight relabelings.

Run:  python tests/golden/make_golden_hard.py [processes]      (40 s on 16 processes, 3 minutes of CPU time)
"""
import itertools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

QUANTITIES = ("oper", "data", "naive", "fancy", "rhs", "S", "g", "lc_fancy", "lc_naive")
STORED = ("oper", "data", "naive", "fancy", "rhs", "S", "g")
DROP_ABOVE = 1e-7
FLOOR = {"oper": 1e-12, "data": 1e-12, "naive": 1e-12, "fancy": 1e-12, "rhs": 1e-12, "lc_fancy": 1e-12, "lc_naive": 1e-12,
         "S": 1e-11, "g": 1e-11}
BASE_IDS = (0, 1, 3, 2)


def rot(P, a):
    c, s = math.cos(a), math.sin(a)
    return P @ np.array([[c, -s], [s, c]]).T


SQ = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
DISTORTED = np.array([[0.10, 0.05], [0.62, 0.11], [0.55, 0.58], [0.02, 0.47]])       # cases.CELLS["distorted"]
COT5 = 1.0 / math.tan(math.radians(5.0))

GOOD_SHAPES = {
    "aspect1000": SQ * [1.0, 1e-3],
    "neartri": np.array([[0.0, 0.0], [1.0, 0.0], [0.5 + 1e-6, 0.5 + 1e-6], [0.0, 1.0]]),      # three nearly collinear vertices
    "trapezoid1e-3": np.array([[0.0, 0.0], [1.0, 0.0], [0.5005, 1.0], [0.4995, 1.0]]),
    "kite": np.array([[0.0, 0.0], [1.0, 0.45], [1.1, 1.1], [0.45, 1.0]]),
    "distorted_x1e-7": DISTORTED * 1e-7,
    "distorted_x1e5": DISTORTED * 1e5,
    "square_rot45": rot(SQ, math.pi / 4) * 0.25,
}
TENSOR7 = [(2, 1), (3, 2), (4, 3), (0, 1), (0, 0), (1, 0), (2, 2)]
FAN_GOOD = [(2, 1), (3, 2)]
ORIENT_CONFIGS = [(2, 1, "tensor"), (3, 2, "tensor"), (0, 1, "tensor"), (2, 2, "fan")]
GRADED = [
    ("aspect10_rot", rot(SQ * [1.0, 0.1], 0.3), TENSOR7),
    ("aspect100_rot", rot(SQ * [1.0, 0.01], 0.3), [c for c in TENSOR7 if c != (4, 3)]),
    ("aspect1000_rot", rot(SQ * [1.0, 1e-3], 0.3), [(2, 1), (0, 1), (0, 0), (1, 0)]),
    ("shear5deg", np.array([[0.0, 0.0], [1.0, 0.0], [1.0 + COT5, 1.0], [COT5, 1.0]]), TENSOR7),
    ("far", SQ * 1e-3 + 1000.0, TENSOR7),
    ("tiny_offset", SQ * 1e-7 + 0.3, TENSOR7),
]


REMOVED = {("kite", 4, 3, "tensor"), ("shear5deg", 4, 3, "tensor")}


def flip_pattern(ids):
    """face f of a cell runs from vertex f to f+1; its basis is flipped (F) when the id of f exceeds that of f+1"""
    return "".join("F" if ids[f] > ids[(f + 1) % 4] else "N" for f in range(4))


def orientation_perms():
    """the 14 achievable patterns (NNNN and FFFF would need a cyclically increasing numbering), one permutation each"""
    pats = {}
    for perm in itertools.permutations(range(4)):
        pats.setdefault(flip_pattern(perm), perm)
    return dict(sorted(pats.items()))


def case_list():
    """-> [(group, name, pts, ids, cd, fd, kind)]"""
    out = []
    for name, pts in GOOD_SHAPES.items():
        for cd, fd in TENSOR7:
            out.append(("good", name, pts, BASE_IDS, cd, fd, "tensor"))
        for cd, fd in FAN_GOOD:
            out.append(("good", name, pts, BASE_IDS, cd, fd, "fan"))
    for pat, perm in orientation_perms().items():
        for cd, fd, kind in ORIENT_CONFIGS:
            out.append(("orientation", "distorted_" + pat, DISTORTED, perm, cd, fd, kind))
    for name, pts, cfgs in GRADED:
        for cd, fd in cfgs:
            out.append(("graded", name, pts, BASE_IDS, cd, fd, "tensor"))
    return [c for c in out if (c[1], c[4], c[5], c[6]) not in REMOVED]


def relabelings(pts):
    """the eight equivalent vertex lists of one cell: four cyclic rolls, times a mirror image (reversed order, y -> -y: still
    counter-clockwise)"""
    out = []
    for img in range(8):
        p = np.roll(pts, -(img % 4), axis=0)
        if img >= 4:
            p = p[::-1].copy() * [1.0, -1.0]
        out.append(np.ascontiguousarray(p))
    return out


def nerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def single_cell(pts, ids):
    P = np.zeros((4, 2))
    P[list(ids)] = pts
    return P, np.array([ids], dtype=np.uint64)


def oracle_eval(O, pts, ids, cd, fd, kind):
    """the oracle on one cell -> (status, dict of the nine quantities), matrices in (row, col) orientation"""
    P, I = single_cell(pts, ids)
    di = O.degrees(cd, fd)
    q = O.QUAD_TENSOR if kind == "tensor" else O.QUAD_FAN
    st1, f = O.local_ops_batch(P, I, di, q, O.STAB_FANCY, fn=1, want=("oper", "data", "stab", "lc"))
    st2, n = O.local_ops_batch(P, I, di, q, O.STAB_NAIVE, want=("stab", "lc"))
    st3, S, g, _ = O.static_condensation(f["lc"][0], f["rhs"][0], di.cbs)
    return st1 or st2 or st3, {"oper": f["oper"][0], "data": f["data"][0], "naive": n["stab"][0], "fancy": f["stab"][0],
                               "rhs": f["rhs"][0][:, None], "S": S, "g": g[:, None], "lc_fancy": f["lc"][0], "lc_naive": n["lc"][0]}


def errors(got, truth):
    """normwise errors of the nine quantities; g as tests/test_gpu_condensed.py normalises it"""
    e = {}
    for q in QUANTITIES:
        if q == "g":
            e[q] = np.abs(got["g"] - truth["g"]).max() / max(np.abs(truth["g"]).max(), np.abs(truth["rhs"]).max(), 1e-300)
        else:
            e[q] = nerr(got[q], truth[q])
    return e


def truth_eval(pts, ids, cd, fd, kind):
    import mpmath as mp
    import make_golden as G
    P = [(mp.mpf(float(pts[i, 0])), mp.mpf(float(pts[i, 1]))) for i in range(4)]
    res = {k: G.to_np(v) for k, v in G.local_ops(P, tuple(int(i) for i in ids), cd, fd, kind).items()}
    res["lc_fancy"] = res["data"] + res["fancy"]
    res["lc_naive"] = res["data"] + res["naive"]
    return res


def one_case(case):
    """-> (stored arrays of the base labelling, e_ref row, worst status, all finite)"""
    import oracle_lib as O
    group, name, pts, ids, cd, fd, kind = case
    e_ref = np.zeros(len(QUANTITIES))
    base, status, finite = None, 0, True
    for img, p in enumerate(relabelings(pts)):
        truth = truth_eval(p, ids, cd, fd, kind)
        st, got = oracle_eval(O, p, ids, cd, fd, kind)
        status = status or st
        finite = finite and all(np.isfinite(v).all() for v in got.values())
        e = errors(got, truth)
        e_ref = np.fmax(e_ref, [e[q] for q in QUANTITIES]) if finite else np.full(len(QUANTITIES), np.nan)
        if img == 0:
            base = {k: truth[k] for k in STORED}
    return base, e_ref, status, finite


def check(cases, groups, quantities, e_ref, dropped, log=print):
    """the conditions on the inputs -> list of violations (empty: the file may be written / the stored file is sound)"""
    bad = []
    quantities = list(quantities)
    dropped = set(dropped)
    gated = above = 0
    for i, c in enumerate(cases):
        for j, q in enumerate(quantities):
            e = float(e_ref[i, j])
            key = "%s|%s" % (c, q)
            if not np.isfinite(e):
                bad.append("%s: e_ref is not finite" % key)
                continue
            if (e > DROP_ABOVE) != (key in dropped):
                bad.append("%s: e_ref %.2e and the dropped list disagree" % (key, e))
            if key in dropped:
                continue
            gated += 1
            above += 10.0 * e > FLOOR[q]
            if groups[i] in ("good", "orientation") and q not in ("rhs", "g") and not e < 1e-13:
                bad.append("%s (%s): e_ref %.2e is not below 1e-13" % (key, groups[i], e))
    log("gated (case, quantity) pairs: %d, of which 10 e_ref is above the floor on %d (%.1f %%); dropped: %d"
        % (gated, above, 100.0 * above / max(gated, 1), len(dropped)))
    if 3 * above > gated:
        bad.append("10 e_ref is above the floor on %d of %d gated pairs: more than one third" % (above, gated))
    return bad


def main():
    import multiprocessing
    import time
    import oracle_lib as O
    O.lib()                                  # build the oracle once, before the workers load it
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1)
    cl = case_list()
    t0 = time.time()
    with multiprocessing.Pool(nproc) as pool:
        results = pool.map(one_case, cl, chunksize=1)
    out, names, groups = {}, [], []
    e_ref = np.zeros((len(cl), len(QUANTITIES)))
    fail = []
    for i, (case, (base, e, status, finite)) in enumerate(zip(cl, results)):
        group, name, pts, ids, cd, fd, kind = case
        cname = "%s|%d|%d|%s" % (name, cd, fd, kind)
        if status != 0 or not finite:
            fail.append("%s: oracle status %d, finite %s on one of the eight relabelings" % (cname, status, finite))
        names.append(cname)
        groups.append(group)
        e_ref[i] = e
        for k, v in base.items():
            out["%s|%s" % (cname, k)] = v
        print(cname, " ".join("%s %.1e" % (q, x) for q, x in zip(QUANTITIES, e)), flush=True)
    dropped = ["%s|%s" % (c, q) for i, c in enumerate(names) for j, q in enumerate(QUANTITIES) if e_ref[i, j] > DROP_ABOVE]
    fail += check(names, groups, QUANTITIES, e_ref, dropped)
    if fail:
        print("\n".join(fail))
        raise SystemExit("conditions on the inputs do not hold: nothing written")
    out.update(cases=np.array(names), case_group=np.array(groups), case_pts=np.array([c[2] for c in cl], dtype=np.float64),
               case_ids=np.array([c[3] for c in cl], dtype=np.int64), quantities=np.array(QUANTITIES), e_ref=e_ref,
               dropped=np.array(dropped, dtype=str))
    path = os.path.join(HERE, "hard_cells.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes in %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
