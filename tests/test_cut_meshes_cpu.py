"""What makes tests/cut_meshes.py a valid judge of the cutHHO side, asserted on the CPU oracle and its binary128 side alone (no device):
a later edit of a mesh that turned it symmetric, emptied it of cut cells, or moved a cell into (or out of) the indefinite regime
would fail here instead of hollowing out tests/test_gpu_cut_general.py."""
import numpy as np
import pytest

import cut_meshes as cm

NOT_SPD = 3                      # HHO_ERR_NOT_SPD (oracle/hho_oracle.h)
LEVELS = [(n, 4) for n in cm.CATALOGUE] + [("A", r) for r in cm.A_REFSTEPS if r != 4]
CLEAN_LEVELS = [(n, r) for n, r in LEVELS if n in cm.CLEAN]


def test_catalogue_stays_small_and_off_the_square():
    for m in cm.CATALOGUE.values():
        assert m.Nx * m.Ny <= cm.MAX_CELLS and m.Nx != m.Ny
    boxes = {(m.lo, m.hi) for m in cm.CATALOGUE.values()}
    assert any(lo[0] != 0.0 and lo[1] != 0.0 for lo, _ in boxes)                          # both origins non-zero somewhere
    assert any(abs((m.hi[0] - m.lo[0]) / m.Nx - (m.hi[1] - m.lo[1]) / m.Ny) > 1e-3 for m in cm.CATALOGUE.values())   # hx != hy


@pytest.mark.parametrize("name,r", LEVELS)
def test_every_mesh_has_cut_cells_and_no_transpose_symmetry(oracle, name, r):
    msh = cm.oracle_mesh(name, r)
    assert (msh.Nx, msh.Ny, msh.nc) == (cm.CATALOGUE[name].Nx, cm.CATALOGUE[name].Ny, msh.Nx * msh.Ny)
    cut = cm.cut_cells(msh)
    assert len(cut) > 0
    assert np.any(msh.cell_loc == oracle.CUT_NEG) and np.any(msh.cell_loc == oracle.CUT_POS)
    if msh.Nx == msh.Ny:         # none today: a square mesh added later must not be its own transpose
        tags = msh.cell_loc.reshape(msh.Ny, msh.Nx)
        assert not np.array_equal(tags, tags.T)
    cut_faces = msh.face_loc == oracle.CUT_ON_INTERFACE
    dirs = cm.face_direction(msh)
    assert np.any(cut_faces & (dirs == 1))                                                 # cut vertical faces everywhere
    if name in cm.CIRCLES:
        assert np.any(cut_faces & (dirs == 0))                                             # and cut horizontal ones on the circles


def test_cut_cell_counts_of_the_catalogue(oracle):
    want = {"A": 24, "At": 24, "B": 28, "C": 20, "E": 9, "G": 32, "D": 26}
    assert {n: len(cm.cut_cells(cm.oracle_mesh(n))) for n in cm.CATALOGUE} == want


def test_At_is_A_transposed(oracle):
    A, At = cm.oracle_mesh("A"), cm.oracle_mesh("At")
    assert np.array_equal(At.cell_loc.reshape(At.Ny, At.Nx), A.cell_loc.reshape(A.Ny, A.Nx).T)
    assert not np.array_equal(At.cell_loc, A.cell_loc)


@pytest.mark.parametrize("name,r", CLEAN_LEVELS)
def test_clean_meshes_factor_everywhere_within_the_covered_conditioning(oracle, name, r):
    """binary128 and the oracle factor every cut cell at k = 0, 1, 2: the one-sided problem on the negative side and the interface
    problem at both kappa pairs; no condition number beyond what the 1e-12 gate already covers on the square meshes"""
    msh = cm.oracle_mesh(name, r)
    worst = 0.0
    for k in (0, 1, 2):
        di = oracle.degrees(k + 1, k)
        for c in cm.cut_cells(msh):
            c = int(c)
            assert msh.truth_laplacian(c, di)[0] == 0 and msh.laplacian(c, di)[0] == 0, (name, r, k, c)
            worst = max(worst, msh.truth_cond(c, di))
            for kappa in cm.KAPPAS:
                assert msh.truth_laplacian_interface(c, di, *kappa)[0] == 0, (name, r, k, c, kappa)
                assert msh.laplacian_interface(c, di, *kappa)[0] == 0, (name, r, k, c, kappa)
    assert 0.0 < worst <= cm.COND_GATE, worst


def test_D_is_refused_on_exactly_its_four_small_fractions(oracle):
    """k = 2 on D: the negative-side area fraction of cells 25, 34, 49, 58 is 0.097 and eta / measure(cl) does not make their
    reconstruction systems positive definite -- binary128 says so for the one-sided and for the interface system, the oracle's llt for
    the one-sided one; nothing is refused at k <= 1"""
    msh = cm.oracle_mesh("D")
    cut = [int(c) for c in cm.cut_cells(msh)]
    assert set(cm.D_REFUSED) <= set(cut)
    for c in cm.D_REFUSED:
        frac = msh.cell_quadrature(c, 2, oracle.CUT_NEG)[2].sum() * msh.Nx * msh.Ny
        assert 0.09 < frac < 0.105, (c, frac)
    for k in (0, 1, 2):
        di = oracle.degrees(k + 1, k)
        one = {c: msh.truth_laplacian(c, di)[0] for c in cut}
        orc = {c: msh.laplacian(c, di)[0] for c in cut}
        two = {c: msh.truth_laplacian_interface(c, di, *kappa)[0] for c in cut for kappa in cm.KAPPAS[:1]}
        want = set(cm.D_REFUSED) if k == 2 else set()
        assert {c for c, st in one.items() if st != 0} == want and all(one[c] == NOT_SPD for c in want), (k, one)
        assert {c for c, st in orc.items() if st != 0} == want and all(orc[c] == NOT_SPD for c in want), (k, orc)
        assert {c for c, st in two.items() if st != 0} == want and all(two[c] == NOT_SPD for c in want), (k, two)
        assert max(msh.truth_cond(c, di) for c in cut if c not in want) <= cm.COND_GATE


@pytest.mark.parametrize("name", list(cm.CATALOGUE))
def test_the_positive_side_is_refused_on_every_cut_cell(oracle, name):
    """where = POSITIVE of the one-sided operators: the reference's normal flip is commented out (cuthho_square.cpp:352-355), the
    Nitsche terms enter with the wrong sign and the reconstruction system is indefinite on every cut cell"""
    msh = cm.oracle_mesh(name)
    for k in (0, 1, 2):
        di = oracle.degrees(k + 1, k)
        for c in cm.cut_cells(msh):
            assert msh.truth_laplacian(int(c), di, oracle.CUT_POS)[0] == NOT_SPD, (name, k, int(c))
            assert msh.laplacian(int(c), di, oracle.CUT_POS)[0] == NOT_SPD, (name, k, int(c))
