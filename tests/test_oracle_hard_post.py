"""tests/golden/hard_cells_post.npz (tests/golden/make_golden_post.py): on the cases of hard_cells.npz, the 50-digit truth of
project_function (cell and face blocks, degree increase 0 and 1, the test function f_c of tests/hard_post.py and the
drivers' sin(pi x) sin(pi y)) and of the recovery of the eliminated cell unknowns (R = -A_TT^-1 A_TF, r0 = A_TT^-1 fT,
uT = r0 + R uF), with e_ref, the CPU oracle's error against that truth, worst over the eight relabelings of each cell.

Checked here without a GPU: the layout; the conditions on the inputs the generator enforces; on a fixed sample -- the first
case of every (group, cell degree) -- that the truth regenerates to the stored bits and that the oracle reproduces its
stored e_ref within a factor of 2; and a negative control: the stored face projection, judged against the truth of the same
cell with one face's endpoints swapped, is beyond the gate, so the judge of tests/test_gpu_hard_post.py would catch a face
basis that runs from the wrong endpoint."""
import os
import sys

import numpy as np
import pytest

import hard_post as HP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HARD = np.load(os.path.join(GOLDEN, "hard_cells.npz"))
POST = np.load(os.path.join(GOLDEN, "hard_cells_post.npz"))
CASES = [str(c) for c in POST["cases"]]
GROUPS = [str(g) for g in HARD["case_group"]]
QUANTITIES = [str(q) for q in POST["quantities"]]
DROPPED = [str(d) for d in POST["dropped"]]
E_REF = POST["e_ref"]


def split(case):
    name, cd, fd, kind = case.split("|")
    return name, int(cd), int(fd), kind


def _sample():
    """the first case, in fixture order, of every (group, cell degree): 5 good, 3 orientation (cell degrees 0, 2, 3), 5 graded"""
    seen = {}
    for i, case in enumerate(CASES):
        seen.setdefault((GROUPS[i], split(case)[1]), case)
    return list(seen.values())


SAMPLE = _sample()


def generator():
    pytest.importorskip("mpmath")
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_post as MP
    return MP


def test_file_layout_and_size():
    assert os.path.getsize(os.path.join(GOLDEN, "hard_cells_post.npz")) < os.path.getsize(os.path.join(GOLDEN, "hard_cells.npz"))
    assert CASES == [str(c) for c in HARD["cases"]] and len(CASES) == 155             # the same cases in the same order
    assert QUANTITIES == list(HP.QUANTITIES) and E_REF.shape == (len(CASES), len(QUANTITIES))
    assert len(SAMPLE) == 13 and {split(c)[1] for c in SAMPLE} == {0, 1, 2, 3, 4}
    for i, case in enumerate(CASES):
        name, cd, fd, kind = split(case)
        cbs, nf = (cd + 2) * (cd + 1) // 2, 4 * (fd + 1)
        no_proj1 = kind == "fan" and 2 * (cd + 1) >= 8                               # rules[8] is empty in the reference
        assert ("%s|proj1" % case in POST.files) == (not no_proj1), case
        for j, q in enumerate(QUANTITIES):
            assert np.isnan(E_REF[i, j]) == (no_proj1 and q in ("proj1_cell", "proj1_face")), (case, q)
        for k in ("proj0", "proj_sin") + (() if no_proj1 else ("proj1",)):
            assert POST["%s|%s" % (case, k)].shape == (cbs + nf,)
        for k in ("fT", "r0", "uT"):
            assert POST["%s|%s" % (case, k)].shape == (cbs,)
        assert POST["%s|R" % case].shape == (cbs, nf)
        assert np.array_equal(POST["%s|uF" % case], POST["%s|proj0" % case][cbs:])      # uF IS the face part of proj0
        assert all(np.isfinite(POST["%s|%s" % (case, k)]).all() for k in HP.STORED if "%s|%s" % (case, k) in POST.files)
        # f_c lies in [1, 3], and so does its mean: the projection on constants
        p0 = POST["%s|proj0" % case]
        assert cd > 0 or 1.0 <= p0[0] <= 3.0, case
        assert fd > 0 or all(1.0 <= p0[cbs + lf] <= 3.0 for lf in range(4)), case
    assert sum(1 for c in CASES if "%s|proj1" % c not in POST.files) == 7               # (3,2) fan of the seven good shapes


def test_conditions_on_the_inputs():
    """what make_golden_post.py enforced when the file was written, on the stored numbers: dropped = exactly the pairs with
    e_ref > 1e-7, at most 12 % of any quantity's cases dropped, 10 e_ref above the floor on at most a third of the gated pairs"""
    assert HP.FLOOR == {q: (1e-12 if i < 6 else 1e-11) for i, q in enumerate(HP.QUANTITIES)}    # rhs's floor, S and g's floor
    assert HP.DROP_ABOVE == 1e-7
    assert len(set(DROPPED)) == len(DROPPED)
    bad = HP.check(CASES, QUANTITIES, E_REF, DROPPED)
    assert not bad, "\n".join(bad)
    # the finding the fixture records: the reference order loses the recovery operator on the rotated thin cells while S is kept
    for case, s_below in (("aspect100_rot|3|2|tensor", 1e-7), ("aspect1000_rot|2|1|tensor", 1e-7)):
        i = CASES.index(case)
        assert E_REF[i, QUANTITIES.index("R")] > 1e-1 and "%s|R" % case in DROPPED
        assert HARD["e_ref"][i, [str(q) for q in HARD["quantities"]].index("S")] < s_below


def test_six_node_rule():
    """the 50-digit Gauss-Legendre rule the generator adds beyond make_golden's five nodes, against numpy's"""
    MP = generator()
    for n in (6, 7):
        rule = MP.gauss_legendre(n)
        x, w = np.polynomial.legendre.leggauss(n)
        # numpy's rule is a double computation, good to a few units in the last place; a wrong node or weight is off by 1e-2
        assert np.abs(np.array([float(r[0]) for r in rule]) - x).max() < 1e-14
        assert np.abs(np.array([float(r[1]) for r in rule]) - w).max() < 1e-14
    G = MP.golden()
    assert len(G.gauss(10)) == 6 and len(G.gauss(8)) == 5 and len(G.gauss(0)) == 1


@pytest.mark.parametrize("case", SAMPLE)
def test_truth_regenerates_and_the_oracle_reproduces_e_ref(case):
    """make_golden_post.one_case on the spot: the stored arrays exactly, and e_ref (the worst of eight relabelings) within a
    factor of 2.  An error of a few units in the last place is quantised, so the comparison allows 4 eps on top."""
    MP = generator()
    import make_golden_hard as H
    cl = {"%s|%d|%d|%s" % (c[1], c[4], c[5], c[6]): c for c in H.case_list()}
    assert list(cl) == CASES
    i = CASES.index(case)
    assert np.array_equal(HARD["case_pts"][i], cl[case][2]) and tuple(HARD["case_ids"][i].tolist()) == tuple(cl[case][3])
    base, e_ref, status, finite = MP.one_case(cl[case])
    assert status == 0 and finite
    for k in HP.STORED:
        key = "%s|%s" % (case, k)
        if base[k] is None:
            assert key not in POST.files
        else:
            assert np.array_equal(base[k], POST[key]), key
    tiny = 4 * np.finfo(np.float64).eps
    for j, q in enumerate(QUANTITIES):
        want = E_REF[i, j]
        if np.isnan(want):
            assert np.isnan(e_ref[j])
            continue
        print("%-28s %-10s e_ref stored %.3e now %.3e" % (case, q, want, e_ref[j]))
        assert 0.5 * want - tiny <= e_ref[j] <= 2.0 * want + tiny, (case, q, want, e_ref[j])


# face degree 1 on two orientation patterns, 2 on a third, and 3 -- which no case of the orientation group has -- on the same
# quadrilateral at another scale (no face of it lies on x = x0, where f_c is the constant 2 and has no odd coefficient to flip)
@pytest.mark.parametrize("case", ["distorted_FNNF|2|1|tensor", "distorted_NFNF|0|1|tensor", "distorted_NNFN|3|2|tensor",
                                  "distorted_x1e-7|4|3|tensor"])
def test_a_swapped_face_endpoint_is_beyond_the_gate(case):
    """negative control: the truth with the basis of ONE face running from the higher-id endpoint differs from the stored
    face projection by far more than the gate -- the odd coefficients of that face change sign -- for each of the four faces"""
    MP = generator()
    i = CASES.index(case)
    name, cd, fd, kind = split(case)
    assert fd >= 1
    pts, ids = HARD["case_pts"][i], tuple(int(v) for v in HARD["case_ids"][i])
    j = QUANTITIES.index("proj0_face")
    assert "%s|proj0_face" % case not in DROPPED
    g = HP.gate("proj0_face", float(E_REF[i, j]))
    cell, face = HP.blocks(cd)
    stored = POST["%s|proj0" % case]
    fc = MP.f_truth(pts, "fc")
    right = MP.to_vec(MP.project_truth(pts, ids, cd, fd, kind, fc, 0)[0])
    assert HP.nerr(stored[face], right[face]) <= g                           # the judge accepts the stored projection
    for lf in range(4):
        wrong = MP.to_vec(MP.project_truth(pts, ids, cd, fd, kind, fc, 0, swap_face=lf)[0])
        assert np.array_equal(wrong[cell], right[cell])                      # the cell block does not see the face bases
        e = HP.nerr(stored[face], wrong[face])
        print("%-28s face %d swapped: error %.2e, gate %.1e, error / gate %.1e" % (case, lf, e, g, e / g))
        assert e > g, (case, lf, e, g)
