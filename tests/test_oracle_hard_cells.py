"""tests/golden/hard_cells.npz (tests/golden/make_golden_hard.py): 50-digit truth of the local operators on cells that are
hard -- aspect 1000, three nearly collinear vertices, a 1e-3 top side, scales 1e-7 and 1e5, every achievable orientation
pattern of the four face bases, and graded shapes on which the reference's own operation order loses digits -- with
e_ref, the CPU oracle's error against that truth, worst over the eight equivalent relabelings of each cell.

Checked here without a GPU: the oracle on the stored labelling stays within e_ref; the conditions on the inputs the
generator enforces; the 14 patterns; and, where mpmath is there, that three entries regenerate to the stored bits.
tests/test_gpu_hard_cells.py derives its gates from the same e_ref."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HARD = np.load(os.path.join(GOLDEN, "hard_cells.npz"))

QUANTITIES = [str(q) for q in HARD["quantities"]]
CASES = [str(c) for c in HARD["cases"]]
GROUPS = [str(g) for g in HARD["case_group"]]
DROPPED = set(str(d) for d in HARD["dropped"])
FLOOR = {"oper": 1e-12, "data": 1e-12, "naive": 1e-12, "fancy": 1e-12, "rhs": 1e-12, "lc_fancy": 1e-12, "lc_naive": 1e-12,
         "S": 1e-11, "g": 1e-11}          # test_gpu_parity.TOL, test_gpu_condensed.TOL
BASE_IDS = (0, 1, 3, 2)


def nerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def flip_pattern(ids):
    return "".join("F" if ids[f] > ids[(f + 1) % 4] else "N" for f in range(4))


def split(case):
    name, cd, fd, kind = case.split("|")
    return name, int(cd), int(fd), kind


def truth(case):
    """the stored arrays of one case plus lc_fancy / lc_naive = data + stabilization"""
    t = {k: HARD["%s|%s" % (case, k)] for k in ("oper", "data", "naive", "fancy", "rhs", "S", "g")}
    t["lc_fancy"] = t["data"] + t["fancy"]
    t["lc_naive"] = t["data"] + t["naive"]
    return t


def oracle_quantities(oracle, pts, ids, cd, fd, kind):
    P = np.zeros((4, 2))
    P[list(ids)] = pts
    I = np.array([ids], dtype=np.uint64)
    di = oracle.degrees(cd, fd)
    q = oracle.QUAD_TENSOR if kind == "tensor" else oracle.QUAD_FAN
    st1, f = oracle.local_ops_batch(P, I, di, q, oracle.STAB_FANCY, fn=1, want=("oper", "data", "stab", "lc"))
    st2, n = oracle.local_ops_batch(P, I, di, q, oracle.STAB_NAIVE, want=("stab", "lc"))
    st3, S, g, _ = oracle.static_condensation(f["lc"][0], f["rhs"][0], di.cbs)
    return st1 or st2 or st3, {"oper": f["oper"][0], "data": f["data"][0], "naive": n["stab"][0], "fancy": f["stab"][0],
                               "rhs": f["rhs"][0][:, None], "S": S, "g": g[:, None], "lc_fancy": f["lc"][0], "lc_naive": n["lc"][0]}


def error_of(q, got, t):
    if q == "g":           # normalised as tests/test_gpu_condensed.py does
        return np.abs(got["g"] - t["g"]).max() / max(np.abs(t["g"]).max(), np.abs(t["rhs"]).max(), 1e-300)
    return nerr(got[q], t[q])


def test_file_layout_and_size():
    assert os.path.getsize(os.path.join(GOLDEN, "hard_cells.npz")) < 1_000_000
    n = len(CASES)
    assert HARD["e_ref"].shape == (n, len(QUANTITIES)) and HARD["case_pts"].shape == (n, 4, 2) and HARD["case_ids"].shape == (n, 4)
    assert QUANTITIES == ["oper", "data", "naive", "fancy", "rhs", "S", "g", "lc_fancy", "lc_naive"]
    assert len(set(CASES)) == n
    for i, case in enumerate(CASES):
        name, cd, fd, kind = split(case)
        assert sorted(HARD["case_ids"][i].tolist()) == [0, 1, 2, 3]              # cell c of a batch owns points 4c .. 4c+3
        cbs, fbs, nr = (cd + 2) * (cd + 1) // 2, fd + 1, (fd + 3) * (fd + 2) // 2 - 1
        ms = cbs + 4 * fbs
        t = truth(case)
        assert t["oper"].shape == (nr, ms) and t["data"].shape == t["naive"].shape == t["fancy"].shape == (ms, ms)
        assert t["rhs"].shape == (cbs, 1) and t["S"].shape == (4 * fbs, 4 * fbs) and t["g"].shape == (4 * fbs, 1)
        assert all(np.isfinite(v).all() for v in t.values())


def test_the_lists_of_the_issue_are_all_there():
    by_name = {}
    for case, group in zip(CASES, GROUPS):
        name, cd, fd, kind = split(case)
        by_name.setdefault((group, name), set()).add((cd, fd, kind))
    tensor7 = {(2, 1), (3, 2), (4, 3), (0, 1), (0, 0), (1, 0), (2, 2)}
    t = lambda s: {(cd, fd, "tensor") for cd, fd in s}  # noqa: E731
    good = ["aspect1000", "neartri", "trapezoid1e-3", "kite", "distorted_x1e-7", "distorted_x1e5", "square_rot45"]
    # left out by the generator for missing a condition on the inputs (make_golden_hard.REMOVED): kite and shear5deg at (4,3)
    for name in good:
        assert by_name[("good", name)] == t(tensor7 - ({(4, 3)} if name == "kite" else set())) | {(2, 1, "fan"), (3, 2, "fan")}, name
    graded = {"aspect10_rot": tensor7, "aspect100_rot": tensor7 - {(4, 3)}, "aspect1000_rot": {(2, 1), (0, 1), (0, 0), (1, 0)},
              "shear5deg": tensor7 - {(4, 3)}, "far": tensor7, "tiny_offset": tensor7}
    for name, cfgs in graded.items():
        assert by_name[("graded", name)] == t(cfgs), name
    assert len(by_name) == 7 + 14 + 6


def test_all_14_orientation_patterns_are_present():
    seen = {}
    for i, (case, group) in enumerate(zip(CASES, GROUPS)):
        ids = HARD["case_ids"][i].tolist()
        if group != "orientation":
            assert tuple(ids) == BASE_IDS
            continue
        name, cd, fd, kind = split(case)
        assert name == "distorted_" + flip_pattern(ids)                  # the pattern string in the name is the ids' pattern
        seen.setdefault(flip_pattern(ids), set()).add((cd, fd, kind))
    every = {"".join(p) for p in __import__("itertools").product("NF", repeat=4)} - {"NNNN", "FFFF"}
    assert set(seen) == every and len(every) == 14
    for pat, cfgs in seen.items():
        assert cfgs == {(2, 1, "tensor"), (3, 2, "tensor"), (0, 1, "tensor"), (2, 2, "fan")}, pat
    # all on the one shape: the patterns differ by signs of face functions and by nothing else
    pts = [HARD["case_pts"][i] for i, g in enumerate(GROUPS) if g == "orientation"]
    assert all(np.array_equal(p, pts[0]) for p in pts)


def test_conditions_on_the_inputs():
    """what make_golden_hard.check() enforced when the file was written, restated on the stored numbers"""
    e_ref = HARD["e_ref"]
    assert np.isfinite(e_ref).all() and (e_ref >= 0).all()
    gated = above = 0
    for i, case in enumerate(CASES):
        for j, q in enumerate(QUANTITIES):
            key = "%s|%s" % (case, q)
            assert (e_ref[i, j] > 1e-7) == (key in DROPPED), key          # dropped: exactly the pairs beyond 1e-7
            if key in DROPPED:
                continue
            gated += 1
            above += 10.0 * e_ref[i, j] > FLOOR[q]
            if GROUPS[i] in ("good", "orientation") and q not in ("rhs", "g"):
                assert e_ref[i, j] < 1e-13, (key, e_ref[i, j])
    print("gated pairs %d, 10 e_ref above the floor on %d, dropped %d" % (gated, above, len(DROPPED)))
    assert 3 * above <= gated
    assert len(DROPPED) < gated // 10                                       # a margin of the lists, not their substance


@pytest.mark.parametrize("group", ["good", "orientation", "graded"])
def test_oracle_is_within_e_ref_on_the_stored_labelling(oracle, group):
    worst = {}
    for i, case in enumerate(CASES):
        if GROUPS[i] != group:
            continue
        name, cd, fd, kind = split(case)
        st, got = oracle_quantities(oracle, HARD["case_pts"][i], tuple(HARD["case_ids"][i].tolist()), cd, fd, kind)
        assert st == 0 and all(np.isfinite(v).all() for v in got.values()), case
        t = truth(case)
        for j, q in enumerate(QUANTITIES):
            if "%s|%s" % (case, q) in DROPPED:
                continue
            e = error_of(q, got, t)
            assert e <= HARD["e_ref"][i, j], (case, q, e, HARD["e_ref"][i, j])
            if e > worst.get(q, (0.0,))[0]:
                worst[q] = (e, HARD["e_ref"][i, j], case)
    for q, (e, er, case) in worst.items():
        print("%-12s %-9s worst oracle error %.2e (e_ref %.2e) on %s" % (group, q, e, er, case))


def test_three_entries_regenerate_to_the_stored_bits():
    """one good shape, one pattern, one graded shape: make_golden_hard.py on the spot gives the stored arrays exactly"""
    pytest.importorskip("mpmath")
    sys.path.insert(0, GOLDEN)
    import make_golden_hard as H
    want = ["neartri|2|1|tensor", "distorted_FNNF|0|1|tensor", "aspect100_rot|1|0|tensor"]
    cl = {"%s|%d|%d|%s" % (c[1], c[4], c[5], c[6]): c for c in H.case_list()}
    assert list(cl) == CASES                                                # the generator's lists are the stored ones
    for case in want:
        group, name, pts, ids, cd, fd, kind = cl[case]
        i = CASES.index(case)
        assert GROUPS[i] == group
        assert np.array_equal(HARD["case_pts"][i], pts) and tuple(HARD["case_ids"][i].tolist()) == tuple(ids)
        res = H.truth_eval(pts, ids, cd, fd, kind)
        for k in H.STORED:
            assert np.array_equal(res[k], HARD["%s|%s" % (case, k)]), (case, k)
