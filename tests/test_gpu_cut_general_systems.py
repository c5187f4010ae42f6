"""The cutHHO side's global systems, row slabs, preconditioner tables and end-to-end runs off the centred circle on the square mesh
(tests/cut_meshes.py; the per-cell half: tests/test_gpu_cut_general.py).  Every closed form in Nx, Ny, row0 and the box behind these
entry points is exercised with Nx != Ny, hx != hy and a box away from the origin: what is bit for bit on the square meshes
(interface_assembler's index maps, the direct CSR gathers against the sorted triplet path, the slabs against the whole mesh, the patch
and coarse tables against their twins) is bit for bit here."""
import numpy as np
import pytest

import cut_meshes as cm
import interface_helpers as ih

pytestmark = pytest.mark.gpu

NEG, POS, CUT = 0, 1, 2
CG_TOL = 1e-13
SYSTEMS = [(n, k) for n in ("A", "At", "B") for k in (0, 1, 2)]


def say(line):
    print(line)                          # (python -m pytest -s: the lines of profiles/cut_general_parity.txt)


def new_asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


@pytest.fixture(scope="module")
def asm():
    return new_asm()


def interface_ops(asm, name, k):
    return ih.real_ops(asm, cm.CATALOGUE[name].Nx, k, **cm.kwargs(name))


# ---- global systems: the interface problem -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", SYSTEMS)
def test_interface_assembler_index_maps_and_triplets(asm, oracle, name, k):
    """test_gpu_cuthho.test_interface_assembler_bit_exact on the catalogue: tables, cell offsets and every cell's triplets"""
    from proton_amd.batch import to_rowcol
    ref = cm.oracle_mesh(name)
    ops, g = interface_ops(asm, name, k)
    assert np.array_equal(asm.cell_loc, ref.cell_loc)
    di = oracle.degrees(k + 1, k)
    ct, ft, num_all_cells, num_other = ref.interface_tables()
    info = asm.ctx.interface_info(k)
    assert (info.num_all_cells, info.num_other_faces) == (num_all_cells, num_other)
    assert info.system_size == di.cbs * num_all_cells + di.fbs * num_other
    offs = asm.interface_cell_offsets(k).cpu().numpy()
    t = {kk: v.cpu().numpy() for kk, v in asm.interface_triplets(k, ops, g).items()}
    lc, rhs, lcc, rhsc = to_rowcol(ops["lc"]), ops["rhs"].cpu().numpy(), to_rowcol(ops["lc_cut"]), ops["rhs_cut"].cpu().numpy()
    gh = g.cpu().numpy()
    assert gh.shape == (ref.nf, di.fbs)
    cbs, fbs = di.cbs, di.fbs
    for c in range(ref.nc):
        for where in (oracle.CUT_NEG, oracle.CUT_POS):
            assert offs[c, where] == oracle.lib().cut_interface_cell_offset(ref.h, di, c, oracle._i64p(ct), where)
        if ref.cell_loc[c] == oracle.CUT_ON_INTERFACE:
            i = int(asm.cut_index[c])
            tr, tc, tv, rr, rv = ref.interface_assemble(di, c, ct, ft, num_all_cells, lcc[i], rhsc[i], np.zeros(2 * di.msize))
            R, Cc, V, RR, RV = t["rows_cut"][i], t["cols_cut"][i], t["vals_cut"][i], t["rhs_rows_cut"][i], t["rhs_vals_cut"][i]
            assert np.all(t["rows"][c] == -1) and np.all(t["rhs_rows"][c] == -1)
        else:
            dd = np.zeros(di.msize)
            for lf in range(4):
                dd[cbs + lf * fbs: cbs + (lf + 1) * fbs] = gh[int(ref.cell_faces[c, lf])]
            tr, tc, tv, rr, rv = ref.interface_assemble(di, c, ct, ft, num_all_cells, lc[c], rhs[c], dd)
            R, Cc, V, RR, RV = t["rows"][c], t["cols"][c], t["vals"][c], t["rhs_rows"][c], t["rhs_vals"][c]
        keep = R >= 0
        assert np.array_equal(R[keep], tr) and np.array_equal(Cc[keep], tc) and np.array_equal(V[keep], tv), c
        assert np.array_equal(RR.astype(np.int64), rr), c
        assert np.abs(RV - rv).max() <= 1e-13 * max(1.0, np.abs(rv).max()), c


@pytest.mark.parametrize("name,k", SYSTEMS)
def test_interface_direct_csr_equals_the_sorted_path(asm, name, k):
    """pa_interface_csr_* and pa_interface_condensed_csr_* against pa_csr_from_triplets of their triplets in cell order, bit for bit;
    the condensed pattern is the face block of the full one"""
    cbs, ms = ih.full_sizes(k)
    nf = ih.condensed_sizes(k)[2]
    ops, g = interface_ops(asm, name, k)
    assert asm.ncut > 0
    info = asm.ctx.interface_info(k)
    full = ih.sorted_path(asm, asm.interface_triplets(k, ops, g), ms, info.system_size)
    rp, ci, _, _ = ih.check_bit_identical(asm, full, lambda: asm.interface_csr_pattern(k), lambda: asm.interface_csr_fill(k, ops, g))
    rec = asm.interface_condensed_ops(k, ops)
    assert int(rec["info"].abs().sum()) == 0 and int(rec["info_cut"].abs().sum()) == 0
    cond = ih.sorted_path(asm, asm.interface_condensed_triplets(k, rec, g), nf, asm.ctx.interface_condensed_query(k).system_size)
    crp, cci, _, _ = ih.check_bit_identical(asm, cond, lambda: asm.interface_condensed_csr_pattern(k),
                                            lambda: asm.interface_condensed_csr_fill(k, rec, g))
    rp, ci, crp, cci = rp.cpu().numpy(), ci.cpu().numpy(), crp.cpu().numpy(), cci.cpu().numpy()
    c0 = cbs * info.num_all_cells
    sub_rp, sub_ci = [0], []
    for r in range(c0, rp.size - 1):
        cols = ci[rp[r]:rp[r + 1]]
        cols = cols[cols >= c0] - c0
        sub_ci.append(cols)
        sub_rp.append(sub_rp[-1] + cols.size)
    assert np.array_equal(crp, np.asarray(sub_rp)) and np.array_equal(cci, np.concatenate(sub_ci))


@pytest.mark.parametrize("name,k", SYSTEMS)
def test_interface_condensed_solve_matches_a_direct_solve(asm, name, k):
    """the face-only solve (Jacobi, 1e-13) and the recovery against spsolve of the full system: 1e-8 max|ref|, the square meshes'
    tolerance (test_gpu_interface_condensed.test_condensed_solve_matches_a_direct_solve_of_the_full_system)"""
    import scipy.sparse.linalg as spla
    import test_gpu_interface_condensed as T
    ops, g = interface_ops(asm, name, k)
    K, b = T.full_csr(asm, k, ops, g)
    ref = spla.spsolve(K.tocsc(), b)
    full = T.condensed_solve(asm, k, ops, g, CG_TOL)
    asm.synchronize()
    err = np.abs(full.cpu().numpy() - ref).max() / np.abs(ref).max()
    say("interface %s k %d: condensed solve + recovery against spsolve %.3e of max|ref|" % (name, k, err))
    assert err <= 1e-8


# ---- global systems: the fictitious domain -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", SYSTEMS)
def test_fictdom_csr_assemble_equals_the_merged_fill(asm, name, k):
    """pa_fictdom_csr_assemble == pa_assembler_csr_fill of the merged local matrices, bit for bit
    (test_gpu_fictdom_csr.test_real_operators_bit_for_bit), with boundary data that vanish nowhere"""
    import torch
    import test_gpu_fictdom_csr as F
    assert cm.preprocess(asm, name) > 0
    g = F.boundary_data(asm, k)
    rhs = F.uncut_rhs(asm, k)
    cut = asm.cut_local_ops(k, NEG, want=("lc", "rhs"))
    va, RHS, lc, _ = F.two_step(asm, k, NEG, rhs, g, cut["lc"], cut["rhs"])
    out = asm.fictdom_csr_scatter(k, NEG, rhs, g, cut["lc"], cut["rhs"], want=("lc",))
    asm.synchronize()
    assert torch.equal(out["values"], va) and torch.equal(out["RHS"], RHS) and torch.equal(out["lc"], lc)
    assert torch.equal(out["lc"][F.cut_rows(asm)], cut["lc"])
    conv = asm.fictdom_csr_assemble(k, NEG, g=g)
    asm.synchronize()
    assert torch.equal(conv["values"], va) and torch.equal(conv["RHS"], RHS)


@pytest.mark.parametrize("name,k", SYSTEMS)
def test_fictdom_condensed_records_and_solve(asm, name, k):
    """the cut cells' condensed records against the exact elimination of the GPU's own cut matrices at fictdom_condensed_judge's gate;
    the condensed solve plus recovery against spsolve of the full system at 1e-8 max|ref|"""
    import scipy.sparse.linalg as spla
    import fictdom_condensed_judge as judge
    import test_gpu_fictdom_condensed as F
    from proton_amd.batch import to_rowcol
    cbs, fbs, nf, ntri = F.sizes(k)
    assert cm.preprocess(asm, name) > 0
    op = F.operators(asm, k, NEG)
    rec = F.records(asm, k, NEG, op)
    asm.synchronize()
    assert int(rec["info"].abs().sum()) == 0 and int(rec["info_cut"].abs().sum()) == 0
    rows = F.cut_rows(asm)
    assert rows.size == asm.ncut
    cond = rec["cond"].cpu().numpy()
    worst = judge.worst_record_error(to_rowcol(op["cut_lc"]), op["cut_rhs"].cpu().numpy(), cond[rows, :ntri], cond[rows, ntri:], cbs)
    K, b, _ = F.full_system(asm, k, NEG, op)
    ref = spla.spsolve(K.tocsc(), b)
    full, iters, reason = asm.fictdom_condensed_solve(k, NEG, tol=CG_TOL)
    asm.synchronize()
    err = np.abs(full.cpu().numpy() - ref).max() / np.abs(ref).max()
    say("fictdom %s k %d: %d cut cells, records against exact elimination %.3e; condensed solve (%d iterations) against spsolve %.3e of max|ref|"
        % (name, k, asm.ncut, worst, iters, err))
    assert worst <= judge.RECORD_GATE
    assert reason == 0 and err <= 1e-8


# ---- row slabs -------------------------------------------------------------------------------------------------------------------
SLABS = {"A": (0, 1, 4, 5, 10), "At": (0, 3, 9, 14), "E": (0, 2, 3, 5)}


def test_the_slabs_hold_the_hard_cases(oracle):
    """A with (0, 1, 4, 5, 10): slab (0, 1) has no cut cell, slab (4, 5) is one cell row with cut horizontal faces on both of its
    boundaries; pa_cut_preprocess_rows' counts partition the whole mesh's on all three sets"""
    a = new_asm()
    ref = cm.oracle_mesh("A")
    face_loc, dirs = ref.face_loc, cm.face_direction(ref)
    pts = ref.points[ref.faces.astype(np.int64)]
    hy = (ref.hi[1] - ref.lo[1]) / ref.Ny
    for j in (4, 5):                                    # the horizontal faces on node row j
        on_row = (dirs == 0) & (np.abs(pts[:, :, 1].mean(axis=1) - (ref.lo[1] + j * hy)) < 0.25 * hy)
        assert on_row.sum() == ref.Nx and np.any(face_loc[on_row] == oracle.CUT_ON_INTERFACE), j
    for name, bounds in SLABS.items():
        ref = cm.oracle_mesh(name)
        assert bounds[0] == 0 and bounds[-1] == ref.Ny
        whole = cm.preprocess(a, name)
        loc, idx = a.cell_loc.copy(), np.asarray(a.cut_index).copy()
        counts, seen = [], 0
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            counts.append(cm.preprocess(a, name, rows=(r0, r1)))
            assert a.ncells == (r1 - r0) * ref.Nx
            assert np.array_equal(a.cell_loc, loc[r0 * ref.Nx:r1 * ref.Nx])
            mine = idx[r0 * ref.Nx:r1 * ref.Nx]
            assert np.array_equal(np.asarray(a.cut_index) >= 0, mine >= 0)
            assert np.array_equal(np.asarray(a.cut_index)[mine >= 0], mine[mine >= 0] - seen)
            seen += counts[-1]
        assert sum(counts) == whole == len(cm.cut_cells(ref))
        if name == "A":
            assert counts[0] == 0 and all(c > 0 for c in counts[1:])


@pytest.mark.parametrize("name", list(SLABS))
@pytest.mark.parametrize("k", [0, 1, 2])
def test_slabs_equal_the_whole_mesh(name, k):
    """the slab records are the whole-mesh rows, the stacked pa_interface_rows_* system and the recovered cell blocks the whole mesh's,
    bit for bit; pa_interface_rows_partition_info agrees with the context's query (inside assemble_slabs)"""
    import torch
    import test_gpu_interface_rows as R
    m, bounds = cm.CATALOGUE[name], SLABS[name]
    kw = cm.kwargs(name)
    w = R.whole_mesh(m.Nx, k, tuple(kw.items()))
    slabs = R.assemble_slabs(m.Nx, k, bounds, kw, w, synthetic=False)
    for s in slabs:
        ref, _, (k0, k1) = R.slices_of(w, m.Nx, k, s["rows"], m.Ny)
        assert s["asm"].ncut == k1 - k0
        assert torch.equal(s["rec"]["cond"], ref["cond"]) and torch.equal(s["rec"]["cond_cut"], ref["cond_cut"])
        assert int(s["rec"]["info"].abs().sum()) == 0 and int(s["rec"]["info_cut"].abs().sum()) == 0
    R.check_stacked(slabs, w)
    # the recovery: a seeded random face vector (the recovery is the same arithmetic on any face vector)
    a = w["asm"]
    cbs = ih.condensed_sizes(k)[0]
    gen = torch.Generator().manual_seed(91 + k)
    xF = (torch.rand(w["RH"].numel(), generator=gen, dtype=torch.float64) - 0.5).to(a.device)
    full = a.interface_condensed_recover(k, w["ops"], xF, w["g"]).clone()
    a.synchronize()
    blocks = 0
    for s in slabs:
        i = s["info"]
        assert i.cell_block_begin == blocks
        uT = s["asm"].interface_rows_recover(k, s["ops"], xF[i.row_begin:i.col_end].clone(), s["g"])
        s["asm"].synchronize()
        assert torch.equal(uT, full[i.cell_block_begin * cbs:i.cell_block_end * cbs])
        blocks = i.cell_block_end
    assert blocks * cbs + xF.numel() == full.numel()


# ---- preconditioner tables -------------------------------------------------------------------------------------------------------
TABLES = ("A", "At", "B")
HS = (3, 4)                              # neither divides both 14 and 10 (nor 15 and 11)


def _same_table(got, want, what):
    ptr, cols, vals, nc = got
    assert want is not None and nc == want.ncoarse, what
    ptr, cols, vals = ptr.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
    assert np.array_equal(ptr, want.ptr) and np.array_equal(cols, want.cols), what
    assert np.array_equal(vals.view(np.int64), want.vals.view(np.int64)), what              # bit for bit


@pytest.mark.parametrize("name", TABLES)
def test_interface_tables_equal_the_twins(asm, oracle, name):
    """pa_interface_condensed_patches (face, cell) against interface_patch_twin and pa_interface_condensed_coarse (one, side; H = 3, 4)
    against interface_coarse_twin at k = 1"""
    import interface_coarse_twin as IC
    import interface_patch_twin as I
    k = 1
    msh = cm.oracle_mesh(name)
    assert cm.preprocess(asm, name) > 0
    n = asm.ctx.interface_condensed_query(k).system_size
    face, cell, nrows = I.mesh_tables(msh, k, device_numbering=True)
    assert nrows == n
    assert np.array_equal(I.device_face_table(msh.bnd, msh.face_loc)[0], msh.interface_tables()[1])      # no cut face on the boundary
    for kind, want in (("face", face), ("cell", cell)):
        ptr, rows = asm.interface_condensed_patches(k, kind)
        asm.synchronize()
        assert np.array_equal(ptr.cpu().numpy(), want.ptr) and np.array_equal(rows.cpu().numpy(), want.rows), (name, kind)
    faces, _ = oracle.mesh_faces(msh.mesh_params())
    assert np.array_equal(faces, msh.faces)
    for H in HS:
        assert msh.Nx % H or msh.Ny % H
        for parts in ("one", "side"):
            want = IC.mesh_table(msh, faces, k, H, parts, device_numbering=True)
            got = asm.interface_condensed_coarse(k, H, parts)
            asm.synchronize()
            assert got[0].numel() == n + 1
            _same_table(got, want, (name, H, parts))
            say("tables %s k 1 H %d %-4s: %d rows, %d columns, %d entries: equal to the twin" % (name, H, parts, n, want.ncoarse, want.cols.size))


@pytest.mark.parametrize("name", TABLES)
def test_plain_tables_on_the_cut_mesh_equal_the_twins(asm, oracle, name):
    """pa_condensed_patches against the oracle's numbering, pa_condensed_coarse (one part; by side with both values of `where`)
    against coarse_twin, and the _rows_ variants of a slab partition against rows_pcg_twin's cut of the whole-mesh tables, at k = 1"""
    import coarse_twin as CT
    import patch_pcg_twin as PT
    import rows_pcg_twin as RT
    k, cd, fd, fbs = 1, 2, 1, 2
    m = cm.CATALOGUE[name]
    msh = cm.oracle_mesh(name)
    assert cm.preprocess(asm, name) > 0
    o = oracle.Assembler(msh.mesh_params(), msh.points, msh.ptids, oracle.degrees(cd, fd))
    assert asm.condensed_info(cd, fd).system_size == o.num_other * fbs
    face, cell = PT.numbering_patches(o.compress, o.cell_faces, o.num_other, fbs)
    for kind, want in (("face", face), ("cell", cell)):
        ptr, rows = asm.condensed_patches(cd, fd, kind)
        asm.synchronize()
        assert np.array_equal(ptr.cpu().numpy(), want.ptr) and np.array_equal(rows.cpu().numpy(), want.rows), (name, kind)
    one = {}
    for H in HS:
        one[H] = CT.table(m.Nx, m.Ny, H, fbs, o.compress, o.faces, o.num_other)
        _same_table(asm.condensed_coarse(cd, fd, H), one[H], (name, H, "one"))
        for where in (NEG, POS):
            want = CT.table(m.Nx, m.Ny, H, fbs, o.compress, o.faces, o.num_other, msh.face_loc, where)
            _same_table(asm.condensed_coarse(cd, fd, H, "side", where), want, (name, H, "side", where))
            assert want.ncoarse > one[H].ncoarse                 # some hat is split
    # the slabs of a partition with a one-row slab
    parts = (0, 3, 4, m.Ny)
    bnds = RT.bounds(m.Nx, m.Ny, parts, fbs)
    want_face = RT.truncate_patches(face, RT.row_owner(face, bnds), bnds)
    want_cell = RT.truncate_patches(cell, RT.cell_owner(m.Nx, parts, cell.ptr.size - 1), bnds)
    slab = new_asm()
    for s, (r0, r1) in enumerate(zip(parts[:-1], parts[1:])):
        cm.preprocess(slab, name, rows=(r0, r1))
        inf = slab.condensed_info(cd, fd)
        assert (inf.row_begin, inf.row_end) == bnds[s]
        for kind, want in (("face", want_face[s]), ("cell", want_cell[s])):
            ptr, rows = (t.cpu().numpy() for t in slab.condensed_rows_patches(cd, fd, kind))
            assert np.array_equal(ptr, want.ptr) and np.array_equal(rows, want.rows), (name, s, kind)
        for H in HS:
            _same_table(slab.condensed_rows_coarse(cd, fd, H), RT.slab_coarse(one[H], *bnds[s]), (name, s, H))
    assert bnds[-1][1] == o.num_other * fbs


@pytest.mark.parametrize("name", TABLES)
def test_two_level_solves_match_the_jacobi_solves(asm, name):
    """one two-level solve per numbering (cell patches + coarse H = 3 by side, 1e-13) against the Jacobi solve of the same system:
    1e-8 max|ref|, the end-to-end tolerance of the square meshes' two-level tests"""
    k = 1
    assert cm.preprocess(asm, name) > 0
    jac, it_j, r_j = asm.fictdom_condensed_solve(k, NEG, tol=CG_TOL)
    two, it_t, r_t = asm.fictdom_condensed_solve(k, NEG, tol=CG_TOL, patches="cell", coarse=3)
    asm.synchronize()
    e = float((two - jac).abs().max() / jac.abs().max())
    say("two-level %s k 1 fictdom: Jacobi %d iterations, cell + coarse H 3 side %d; difference %.3e of max|ref|" % (name, it_j, it_t, e))
    assert r_j == 0 and r_t == 0 and e <= 1e-8
    ops, g = interface_ops(asm, name, k)
    jac, it_j, r_j = asm.interface_condensed_solve(k, ops, g, tol=CG_TOL)
    two, it_t, r_t = asm.interface_condensed_solve(k, ops, g, tol=CG_TOL, patches="cell", coarse=3, coarse_parts="side")
    asm.synchronize()
    e = float((two - jac).abs().max() / jac.abs().max())
    say("two-level %s k 1 interface: Jacobi %d iterations, cell + coarse H 3 side %d; difference %.3e of max|ref|" % (name, it_j, it_t, e))
    assert r_j == 0 and r_t == 0 and e <= 1e-8


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _gate(e_oracle, e_truth):
    """what separates the oracle-provider run from the truth-provider run is the oracle's own cut-cell error passed through the
    solve; the GPU matches binary128 per cell, so its run may differ from the truth run by no more than ten times that (floor 1e-9)"""
    return max(1e-9, 10.0 * abs(e_oracle - e_truth) / e_truth)


@pytest.mark.parametrize("name,k", [(n, k) for n in ("A", "B") for k in (1, 2)])
def test_fictdom_end_to_end(asm, oracle, name, k):
    """cuthho_square -f restated (tests/cuthho_driver.py) with sin(pi x) sin(pi y) on the mesh's own box -- non-zero boundary values --
    and three providers of the local matrices: the GPU, the oracle, binary128 on the cut cells"""
    import cuthho_driver as cd
    from proton_amd.batch import to_rowcol
    m = cm.CATALOGUE[name]

    def gpu_provider(msh, di):
        cm.preprocess(asm, name)
        assert np.array_equal(asm.cell_loc, msh.cell_loc)
        lc, rhs = asm.fictdom_local_ops(k)
        asm.synchronize()
        L, R = to_rowcol(lc), rhs.cpu().numpy()
        return [(L[c], R[c]) for c in range(msh.nc)]

    e_gpu, e_orc, e_tru = (cd.run_fictdom(m.Nx, k, 4, provider=p, **cm.kwargs(name))[0]
                           for p in (gpu_provider, cd.oracle_cut_provider, cd.truth_cut_provider))
    gate = _gate(e_orc, e_tru)
    say("end to end fictdom   %-2s k %d: energy error GPU %.12e oracle %.12e truth %.12e | GPU against truth %.3e, gate %.3e"
        % (name, k, e_gpu, e_orc, e_tru, abs(e_gpu - e_tru) / e_tru, gate))
    assert 0.0 < e_tru < 0.1
    assert abs(e_gpu - e_tru) / e_tru <= gate


@pytest.mark.parametrize("name", ["A", "B"])
def test_interface_end_to_end(asm, oracle, name):
    """cuthho_square -i restated, k = 1, the same three providers"""
    import cuthho_driver as cd
    from proton_amd.batch import to_rowcol
    k, m = 1, cm.CATALOGUE[name]

    def gpu_provider(msh, di, kappa=(1.0, 1.0)):
        cm.preprocess(asm, name)
        assert np.array_equal(asm.cell_loc, msh.cell_loc)
        out = asm.interface_local_ops(k, kappa=kappa)
        asm.synchronize()
        lc, rhs, lcc, rhsc = to_rowcol(out["lc"]), out["rhs"].cpu().numpy(), to_rowcol(out["lc_cut"]), out["rhs_cut"].cpu().numpy()
        res = []
        for c in range(msh.nc):
            i = int(asm.cut_index[c])
            res.append((lcc[i], rhsc[i]) if i >= 0 else (lc[c], rhs[c]))
        return res

    e_gpu, e_orc, e_tru = (cd.run_interface(m.Nx, k, 4, provider=p, **cm.kwargs(name))[0]
                           for p in (gpu_provider, cd.oracle_interface_provider, cd.truth_interface_provider))
    gate = _gate(e_orc, e_tru)
    say("end to end interface %-2s k %d: energy error GPU %.12e oracle %.12e truth %.12e | GPU against truth %.3e, gate %.3e"
        % (name, k, e_gpu, e_orc, e_tru, abs(e_gpu - e_tru) / e_tru, gate))
    assert 0.0 < e_tru < 0.1
    assert abs(e_gpu - e_tru) / e_tru <= gate
