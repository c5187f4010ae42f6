"""The cutHHO side judged off the centred circle on the square mesh (tests/cut_meshes.py: Nx != Ny, shifted and stretched boxes,
circles off the centre, a line far from the origin): preprocessing, the one-sided and the interface operators of every cut cell
against the oracle and its binary128 side, and the failure report -- `info` of a cut cell whose reconstruction system is not positive
definite (mesh D at k = 2; where = PA_LOC_POSITIVE on every cut cell).  tests/test_cut_meshes_cpu.py asserts on the CPU that the
catalogue is the judge these tests take it for.  The global systems, row slabs, preconditioner tables and end-to-end runs on the same
meshes: tests/test_gpu_cut_general_systems.py."""
import numpy as np
import pytest

import cut_meshes as cm
from test_gpu_cuthho import TOL, judge_cut_cells, nerr

pytestmark = pytest.mark.gpu

NEG, POS, CUT = 0, 1, 2
LEVELS = [(n, 4) for n in cm.CATALOGUE] + [("A", r) for r in cm.A_REFSTEPS if r != 4]


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def query_tags(asm, ref):
    from proton_amd import capi
    node = np.zeros(ref.np_, dtype=np.int8)
    face = np.zeros(ref.nf, dtype=np.int8)
    pts = np.zeros((ref.np_, 2))
    assert capi.lib().pa_cut_query_tags(asm.ctx.h, node.ctypes.data, face.ctypes.data, pts.ctypes.data) == 0
    return node, face, pts


# ---- preprocessing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", LEVELS)
def test_preprocessing_equals_the_oracles(asm, oracle, name, r):
    """cell, node and face tags, cut_index, the displaced points and the three quadrature lists of both sides: bit for bit"""
    ref = cm.oracle_mesh(name, r)
    ncut = cm.preprocess(asm, name, r)
    cut = cm.cut_cells(ref)
    assert asm.ncells == ref.nc and ncut == len(cut) > 0
    assert np.array_equal(asm.cell_loc, ref.cell_loc)
    want_index = np.full(ref.nc, -1, dtype=np.int64)
    want_index[cut] = np.arange(len(cut))
    assert np.array_equal(np.asarray(asm.cut_index, dtype=np.int64), want_index)
    node, face, pts = query_tags(asm, ref)
    assert np.array_equal(node, ref.node_loc) and np.array_equal(face, ref.face_loc)
    assert np.array_equal(pts, ref.points)
    for k in (0, 1, 2):
        for where in (oracle.CUT_NEG, oracle.CUT_POS):
            for which, fn, deg in ((0, ref.cell_quadrature, 2 * (k + 1)), (1, ref.interface_quadrature, 2 * (k + 1)),
                                   (2, ref.interface_quadrature, k + 1)):
                off, xyw = asm.ctx.cut_quadrature_points(k, where, which)
                assert len(off) == len(cut) + 1 and off[-1] == len(xyw)
                for i, c in enumerate(cut):
                    want = np.array(fn(int(c), deg, where)).T.reshape(-1, 3)
                    assert np.array_equal(xyw[off[i]:off[i + 1]], want), (k, where, which, int(c))


@pytest.mark.parametrize("name", ["A", "At", "B"])
def test_agglomeration_branch_equals_the_oracles(asm, oracle, name):
    ref = cm.oracle_mesh(name, 4, agglomeration=True)
    ncut = cm.preprocess(asm, name, 4, agglomeration=True)
    assert ncut == len(cm.cut_cells(ref)) > 0
    assert np.array_equal(asm.cell_loc, ref.cell_loc)
    node, face, pts = query_tags(asm, ref)
    assert np.array_equal(node, ref.node_loc) and np.array_equal(face, ref.face_loc) and np.array_equal(pts, ref.points)
    agglo, nb = asm.ctx.cut_agglo_query()
    assert np.array_equal(agglo, ref.agglo_set())
    assert np.array_equal(nb, ref.neighbors())


# ---- one-sided operators ----------------------------------------------------------------------------------------------------
def one_sided(asm, k, where=NEG):
    from proton_amd.batch import to_rowcol
    out = asm.cut_local_ops(k, where=where)
    asm.synchronize()
    return {"info": out["info"].cpu().numpy(), "rhs": out["rhs"].cpu().numpy(),
            **{key: to_rowcol(out[key]) for key in ("oper", "data", "stab", "lc")}}


def check_stab_and_rhs(ref, di, cells, got, where):
    """stabilization and right-hand side involve no factorization: 1e-12 against binary128 and against the oracle on every cell"""
    for i, c in enumerate(cells):
        c = int(c)
        st, o_stab = ref.cut_stabilization(c, di, where)
        assert st == 0
        st, t_stab = ref.truth_stabilization(c, di, where)
        assert st == 0
        st, o_rhs = ref.rhs(c, di.cell_deg, where)
        assert st == 0
        st, t_rhs = ref.truth_rhs(c, di.cell_deg, where)
        assert st == 0
        assert nerr(got["stab"][i], o_stab) < TOL and nerr(got["stab"][i], t_stab) < TOL, (c, where)
        assert np.abs(got["rhs"][i] - o_rhs).max() < 1e-12 * max(1.0, np.abs(o_rhs).max()), (c, where)
        assert np.abs(got["rhs"][i] - t_rhs).max() < 1e-12 * max(1.0, np.abs(t_rhs).max()), (c, where)


ONE_SIDED = ([(n, 4, k) for n in ("A", "At", "B", "E", "G") for k in (0, 1, 2)] + [("D", 4, 0), ("D", 4, 1)] +
             [("A", r, 2) for r in (0, 1, 6)])


@pytest.mark.parametrize("name,r,k", ONE_SIDED)
def test_one_sided_operators_negative_side(asm, oracle, name, r, k):
    ref = cm.oracle_mesh(name, r)
    cm.preprocess(asm, name, r)
    assert np.array_equal(asm.cell_loc, ref.cell_loc)
    cut = cm.cut_cells(ref)
    di = oracle.degrees(k + 1, k)
    got = one_sided(asm, k)
    assert got["info"].shape == (len(cut),) and not got["info"].any()
    for i, c in enumerate(cut):
        st, o_oper, _ = ref.laplacian(int(c), di)
        assert st == 0 and o_oper.shape == got["oper"][i].shape
    check_stab_and_rhs(ref, di, cut, got, oracle.CUT_NEG)
    judge_cut_cells(ref, oracle, di, cut, got["lc"], got["oper"], got["data"], label="%s r=%d k=%d:" % (name, r, k))


# ---- interface operators ----------------------------------------------------------------------------------------------------
def judge_interface(asm, oracle, ref, k, kappa, label, refused=()):
    """the assertions of test_gpu_cuthho.test_interface_operators_match_oracle on the context's current mesh; `refused`: cut cells
    whose matrices are not judged (their info_cut must be non-zero, every other cell's zero)"""
    import cuthho_driver as cd
    from proton_amd.batch import to_rowcol
    di = oracle.degrees(k + 1, k)
    out = asm.interface_local_ops(k, kappa=kappa, want_oper=True)
    asm.synchronize()
    info = out["info_cut"].cpu().numpy()
    want = cd.oracle_interface_provider(ref, di, kappa)
    lc, rhs = to_rowcol(out["lc"]), out["rhs"].cpu().numpy()
    lcc, rhsc = to_rowcol(out["lc_cut"]), out["rhs_cut"].cpu().numpy()
    datac, operc = to_rowcol(out["data_cut"]), to_rowcol(out["oper_cut"])
    cut = cm.cut_cells(ref)
    assert asm.ncut == len(cut) == info.size
    flagged = {int(cut[i]) for i in np.nonzero(info)[0]}
    assert flagged == set(refused), (flagged, refused)
    rbs = di.rbs
    rows = []
    for c in range(ref.nc):
        w_lc, w_rhs = want[c]
        if ref.cell_loc[c] != oracle.CUT_ON_INTERFACE:
            assert nerr(lc[c], w_lc) < TOL and np.abs(rhs[c] - w_rhs).max() < 1e-12 * max(1.0, np.abs(w_rhs).max()), c
            continue
        i = int(asm.cut_index[c])
        for side, where in enumerate((oracle.CUT_NEG, oracle.CUT_POS)):
            st, t_rhs = ref.truth_rhs_side(int(c), di.cell_deg, where)
            assert st == 0
            assert np.abs(rhsc[i][side * di.cbs:(side + 1) * di.cbs] - t_rhs).max() < 1e-12 * max(1.0, np.abs(t_rhs).max()), c
        assert np.abs(rhsc[i] - w_rhs).max() < 1e-12 * max(1.0, np.abs(w_rhs).max()), c
        if c in refused:
            continue
        st, o_oper, o_data = ref.laplacian_interface(int(c), di, kappa[0], kappa[1])
        assert st == 0 and o_oper.shape == operc[i].shape
        st, t_oper, t_data = ref.truth_laplacian_interface(int(c), di, kappa[0], kappa[1])
        assert st == 0
        d = operc[i] - o_oper                          # must be (row 0 + row rbs) * const per column
        shift = d[0].copy()
        d[0] -= shift; d[rbs] -= shift
        assert np.abs(operc[i][0]).max() == 0.0        # the pinned unknown
        rows.append((nerr(datac[i], t_data), nerr(o_data, t_data), nerr(operc[i], t_oper), np.abs(d).max() / np.abs(o_oper).max(),
                     nerr(lcc[i] - datac[i], w_lc - o_data), ref.last_interface_cond))
    e_gpu, e_orc, e_oper, e_oper_mod, e_stab, cond = np.array(rows).T
    print("interface %s kappa=%s: cut cells %d judged %d | cond (pinned two-sided system) median %.1e max %.1e | data vs binary128: GPU median "
          "%.1e max %.1e, oracle median %.1e max %.1e | beyond 1e-12: GPU %d, oracle %d | oper vs binary128 max %.1e"
          % (label, kappa, len(cut), len(rows), np.median(cond), cond.max(), np.median(e_gpu), e_gpu.max(), np.median(e_orc), e_orc.max(),
             (e_gpu > TOL).sum(), (e_orc > TOL).sum(), e_oper.max()))
    assert np.all(e_stab < TOL)
    assert np.all(e_gpu < TOL), (int((e_gpu >= TOL).sum()), e_gpu.max())
    assert np.all(e_oper < TOL), e_oper.max()
    assert np.all(e_oper_mod < TOL + 1e-13 * cond)


INTERFACE = [(n, k, kappa) for n in ("A", "At", "B", "G") for k in (0, 1, 2) for kappa in cm.KAPPAS] + [("E", 1, (1.0, 1.0))]


@pytest.mark.parametrize("name,k,kappa", INTERFACE, ids=["%s-k%d-kappa%g" % (n, k, kp[1]) for n, k, kp in INTERFACE])
def test_interface_operators(asm, oracle, name, k, kappa):
    ref = cm.oracle_mesh(name)
    cm.preprocess(asm, name)
    assert np.array_equal(asm.cell_loc, ref.cell_loc)
    judge_interface(asm, oracle, ref, k, kappa, "%s k=%d" % (name, k))


# ---- the failure report -----------------------------------------------------------------------------------------------------
def test_D_reports_its_four_indefinite_cells(asm, oracle):
    """D at k = 2: eta / measure(cl) leaves the reconstruction system of the cells with a negative-side area fraction of 0.097
    indefinite (binary128 and the oracle refuse them: tests/test_cut_meshes_cpu.py).  The reference's llt() would hand back NaNs
    in silence; the product reports info = failed pivot + 1 on exactly these cells -- and every other cut cell, and stab and rhs of
    the flagged ones (no factorization), stay within the 1e-12 gate.  oper / data / lc of a flagged cell are not judged."""
    k = 2
    ref = cm.oracle_mesh("D")
    cm.preprocess(asm, "D")
    assert np.array_equal(asm.cell_loc, ref.cell_loc)
    cut = cm.cut_cells(ref)
    di = oracle.degrees(k + 1, k)
    got = one_sided(asm, k)
    flagged = {int(cut[i]) for i in np.nonzero(got["info"])[0]}
    print("D k=2: info != 0 on cells %s, values %s (rbs %d)" % (sorted(flagged), got["info"][got["info"] != 0].tolist(), di.rbs))
    assert flagged == set(cm.D_REFUSED)
    bad = got["info"][got["info"] != 0]
    assert np.all((bad >= 1) & (bad <= di.rbs))
    check_stab_and_rhs(ref, di, cut, got, oracle.CUT_NEG)
    keep = np.array([i for i, c in enumerate(cut) if int(c) not in cm.D_REFUSED])
    assert keep.size == len(cut) - 4
    judge_cut_cells(ref, oracle, di, cut[keep], got["lc"][keep], got["oper"][keep], got["data"][keep], label="D k=2 (22 of 26 cells):")
    # the interface system: flagged where binary128 refuses, everything else judged as everywhere
    refused = {int(c) for c in cut if ref.truth_laplacian_interface(int(c), di)[0] != 0}
    assert refused == set(cm.D_REFUSED)
    judge_interface(asm, oracle, ref, k, (1.0, 1.0), "D k=2", refused=refused)


@pytest.mark.parametrize("name", ["A", "D"])
def test_positive_side_is_reported_on_every_cut_cell(asm, oracle, name):
    """where = PA_LOC_POSITIVE of the one-sided operators: the reference's normal flip is commented out (cuthho_square.cpp:352-355),
    the product follows it, and the reconstruction system is indefinite on every cut cell -- reported through info; stab and rhs of
    that side are still the reference's"""
    k = 1
    ref = cm.oracle_mesh(name)
    cm.preprocess(asm, name)
    cut = cm.cut_cells(ref)
    di = oracle.degrees(k + 1, k)
    got = one_sided(asm, k, where=POS)
    print("%s k=1 where=POSITIVE: info %s" % (name, got["info"].tolist()))
    assert got["info"].shape == (len(cut),)
    assert np.all((got["info"] >= 1) & (got["info"] <= di.rbs))
    check_stab_and_rhs(ref, di, cut, got, oracle.CUT_POS)
