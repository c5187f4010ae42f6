"""The kernels that turn the local operators into the numbers a user reads -- cell_project_kernel and face_project_kernel
(pa_project_function_batch), dirichlet_data_kernel (pa_dirichlet_data_batch), the recovery of the eliminated cell unknowns
(pa_condensed_recover_batch, the rec output of pa_static_condensation_batch) and energy_form_kernel -- on the hard cells of
tests/golden/hard_cells.npz, against the 50-digit truth of tests/golden/hard_cells_post.npz (tests/golden/make_golden_post.py,
checked without a GPU by tests/test_oracle_hard_post.py).

The gate of a (cell, quantity) is max(floor, 10 e_ref) as in tests/test_gpu_hard_cells.py: the project's floors (1e-12 for the
projections, 1e-11 behind the A_TT solve), e_ref the CPU oracle's error against the same truth, worst over the cell's eight
relabelings; pairs with e_ref > 1e-7 (`dropped`) are not gated.  Errors are max-norm over the max-norm of the truth of the block;
the projections of sin(pi x) sin(pi y) are normalised by max(|truth|, 1).  The projected function of the sampled paths is f_c of
tests/hard_post.py, evaluated here on the host at the points the library returns.

All fixture cells of one (cd, fd, quadrature) go up as one mesh, cell c owning points 4c .. 4c+3 (test_gpu_hard_cells.mesh_of),
with explicit face tables: face (c, lf) joins the points of vertices lf and lf+1 of cell c, stored (lo, hi), all faces sorted
by (lo, hi) -- so the 14 orientation patterns reach the Dirichlet kernel and the face projection through the tables a
general mesh has.  Every face is a Dirichlet face but two, which pa_dirichlet_data_batch must leave zero.

The energy form needs no fixture: the quadratic form of the doubles the kernel reads is evaluated in exact rational
arithmetic, and the kernel is held to 32 * 2^-53 * sum |A_ij| |d_i| |d_j| per cell.  Where that comes from: one rounding in
each of d_i and d_j, two in the product A_ij d_i d_j, at most ceil(31^2 / 64) = 16 sequential additions in a lane and six
shuffle levels: 26 roundings; 32 leaves room for the compiler's choice of contractions.

Every test prints, per quantity and group of cells, the worst e_gpu / gate with its e_ref before it asserts, and every dropped
pair with the kernel's and the oracle's error (pytest -s; one run is kept in profiles/hard_post_parity.txt).

MEASURED ON AN MI355X.  Every kernel is inside its gate on every cell, e_gpu / gate at most 0.73 (the face projection of f_c on
`far` at face degree 2, 7.39e-11 against e_ref 1.02e-11); all 14 orientation patterns at <= 3.4e-14, their face blocks and Dirichlet
data at <= 1e-15, so no endpoint is swapped anywhere; R, r0 and uT at most 0.26 of their gates; on the dropped pairs the kernels are
closer to the truth than the oracle's worst relabeling on 42 of 45 (R of the rotated aspect-1000 cell: 3.2e-2 against 1.1e+1); the
energy form within 0.08 of its bound on every cell; placement and the tiled batch bit-identical throughout.

WHAT THE FIRST RUN FOUND, AND THE FIX.  One cell failed, `far` (side 1e-3 at (1000, 1000)), in the face blocks of the sampled
paths: proj0_face 1.061e-10 at (2,1) and (0,1) through project_function and through dirichlet_data (gate 3.531e-11), proj1_face
6.145e-11 at (0,0) and (1,0) (gate 3.531e-11) and 1.823e-10 at (4,3) (gate 5.045e-11).  pa_face_quadrature_points returned -- and the
built-in paths of dirichlet_data_kernel and face_project_kernel used -- the points 0.5 (1 - t) a + 0.5 (1 + t) b, contracted to one
fused multiply-add: up to two ulps of the offset along the face, 2e-10 of the cell, and f_c varies by O(1) across the cell.  The three
kernels now take the point from the endpoint a, a + 0.5 (1 + t) (b - a) (face_point in hho_aux.hpp, what S1 of the operator kernel
does): within half an ulp.  After it the same five figures are 3.53e-12, 3.53e-12 and 2.64e-11; a double evaluation of both formulas
on the host reproduces the figures before and after."""
import os
from fractions import Fraction

import numpy as np
import pytest

import hard_post as HP
from test_gpu_hard_cells import CASES, CONFIGS, GROUPS, HARD, batch, cells_of, mesh_of

pytestmark = pytest.mark.gpu

POST = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard_cells_post.npz"))
assert [str(c) for c in POST["cases"]] == CASES
QUANTITIES = [str(q) for q in POST["quantities"]]
DROPPED = set(str(d) for d in POST["dropped"])
E_REF = POST["e_ref"]
PLACEMENT = [(2, 1, "tensor"), (2, 2, "fan")]      # both hold the 14 orientation patterns


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def dev(a, asm):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(asm.device)


def gated(i, q):
    return not np.isnan(E_REF[i, QUANTITIES.index(q)]) and "%s|%s" % (CASES[i], q) not in DROPPED


def judge(label, idx, q, errs, failures):
    """errs[k]: the GPU's error of quantity q on cell idx[k].  Prints, for each group of cells, the worst e_gpu / gate of the gated
    cells with its e_ref; appends every cell beyond its gate to `failures`."""
    j = QUANTITIES.index(q)
    worst = {}
    for k, i in enumerate(idx):
        if not gated(i, q):
            if not np.isnan(E_REF[i, j]):          # dropped: the oracle is beyond 1e-7; shown, not judged
                print("%-40s %-10s %-11s e_gpu %.2e  e_ref %.2e  not gated  %s" % (label, q, "dropped", float(errs[k]), E_REF[i, j], CASES[i]))
            continue
        e_ref = float(E_REF[i, j])
        g = HP.gate(q, e_ref)
        e = float(errs[k])
        if not e <= g:
            failures.append("%s %s %s: e_gpu %.3e beyond the gate %.3e (e_ref %.3e)" % (label, CASES[i], q, e, g, e_ref))
        group = GROUPS[i]
        if group not in worst or not e / g <= worst[group][0]:
            worst[group] = (e / g, e, e_ref, g, CASES[i])
    for group, (r, e, e_ref, g, case) in worst.items():
        print("%-40s %-10s %-11s e_gpu %.2e  e_ref %.2e  gate %.1e  e_gpu/gate %.3f  %s" % (label, q, group, e, e_ref, g, r, case))


class Batch:
    """one config's cells as a mesh with explicit face tables"""

    def __init__(self, asm, cd, fd, kind, order=None):
        import proton_amd as pa
        self.cd, self.fd, self.kind = cd, fd, kind
        self.quad = pa.QUAD_TENSOR if kind == "tensor" else pa.QUAD_FAN
        self.idx = batch(cd, fd, kind)
        if order is not None:
            self.idx = [self.idx[k] for k in order]
        self.n = n = len(self.idx)
        self.cbs, self.fbs = (cd + 2) * (cd + 1) // 2, fd + 1
        self.nf, self.ms = 4 * self.fbs, self.cbs + 4 * self.fbs
        points, ptids = mesh_of(cells_of(self.idx))
        # face (c, lf) joins vertices lf and lf+1 of cell c; (lo, hi); all faces sorted by (lo, hi)
        ends = np.stack([ptids, np.roll(ptids, -1, axis=1)], axis=2).reshape(4 * n, 2).astype(np.int64)
        lohi = np.sort(ends, axis=1)
        order_f = np.lexsort((lohi[:, 1], lohi[:, 0]))
        self.face_pts = lohi[order_f].astype(np.uint32)
        self.face_cell, self.face_lf = order_f // 4, order_f % 4          # face f is local face face_lf[f] of cell face_cell[f]
        self.cell_faces = np.zeros((n, 4), dtype=np.uint32)
        self.cell_faces[self.face_cell, self.face_lf] = np.arange(4 * n)
        assert (np.diff(self.face_pts[:, 0].astype(np.int64)) >= 0).all() and (self.face_pts[:, 0] < self.face_pts[:, 1]).all()
        # every face Dirichlet but two: the second face of the config's first fixture cell and the third of its last (chosen by
        # the cell, not by its place in the batch, so that a batch in another order frees the same two)
        self.is_dir = np.ones(4 * n, dtype=np.uint8)
        self.free = [int(self.cell_faces[int(np.argmin(self.idx)), 1]), int(self.cell_faces[int(np.argmax(self.idx)), 2])]
        self.is_dir[self.free] = 0
        asm.set_mesh(points, ptids)
        asm.set_faces(self.cell_faces, self.face_pts, self.is_dir)
        self.prm = [HP.fc_params(HARD["case_pts"][i]) for i in self.idx]

    def truth(self, k, what):
        a = POST["%s|%s" % (CASES[self.idx[k]], what)]
        a.setflags(write=False)
        return a

    def has(self, k, what):
        return "%s|%s" % (CASES[self.idx[k]], what) in POST.files

    def fc_cells(self, xyw):
        """f_c of each cell at its own points xyw[n, nq, 3] (host, double)"""
        xyw = xyw.cpu().numpy()
        return np.stack([HP.fc(self.prm[c], xyw[c, :, 0], xyw[c, :, 1]) for c in range(self.n)])

    def fc_faces(self, xyw):
        """f_c of the owning cell at the points of every face, xyw[nfaces, nfq, 3]"""
        xyw = xyw.cpu().numpy()
        return np.stack([HP.fc(self.prm[int(self.face_cell[f])], xyw[f, :, 0], xyw[f, :, 1]) for f in range(4 * self.n)])

    def by_cell(self, g):
        """face-indexed Dirichlet data g[nfaces, fbs] -> [n, 4 fbs] in local face order"""
        return g[self.cell_faces.astype(np.int64)].reshape(self.n, self.nf)

    def dirichlet_mask(self):
        """[n, 4 fbs]: True on the coefficients of Dirichlet faces"""
        return np.repeat(self.is_dir[self.cell_faces.astype(np.int64)].astype(bool), self.fbs, axis=1)


def block_errors(B, got, what, sin=False, mask=None):
    """-> (cell errors, face errors) of the projections got[n, ms] against the stored `what`; cells without that array get NaN.
    mask[n, nf]: the face coefficients that are looked at (the block's norm stays that of the whole truth block)"""
    cell, face = HP.blocks(B.cd)
    floor = 1.0 if sin else 1e-300
    ec, ef = [], []
    for k in range(B.n):
        if not B.has(k, what):
            ec.append(np.nan), ef.append(np.nan)
            continue
        t = B.truth(k, what)
        ec.append(HP.nerr(got[k][cell], t[cell], floor))
        d = np.abs(got[k][face] - t[face])
        if mask is not None:
            d = d[mask[k]]
        ef.append(float(d.max() / max(np.abs(t[face]).max(), floor)))
    return ec, ef


def sampled_projection(asm, B, dinc, first=0, n=None):
    import proton_amd as pa
    nq = asm.quadrature_points(2 * (B.cd + dinc), B.quad)
    fq = asm.face_quadrature_points(B.fd + dinc)
    last = B.n if n is None else first + n
    cv, fv = dev(B.fc_cells(nq)[first:last], asm), dev(B.fc_faces(fq), asm)
    assert cv.shape == (last - first, nq.shape[1]) and fv.shape == (4 * B.n, B.fd + dinc + 1)
    out, info = asm.project_function(B.cd, B.fd, pa.capi.FN_SAMPLED, quad=B.quad, dinc=dinc, cell_fvals=cv, face_fvals=fv,
                                     first=first, n=n, want_info=True)
    asm.synchronize()
    return out, info


def sampled_dirichlet(asm, B):
    import proton_amd as pa
    fv = dev(B.fc_faces(asm.face_quadrature_points(B.fd)), asm)
    assert fv.shape == (4 * B.n, B.fd + 1)
    g = asm.dirichlet_data(B.fd, pa.capi.FN_SAMPLED, fvals=fv)
    asm.synchronize()
    return g


def no_rule(cd, kind, dinc):
    """the fan at degree 8: rules[8] is empty in the reference; the fixture holds no truth there"""
    return kind == "fan" and 2 * (cd + dinc) >= 8


@pytest.mark.parametrize("cd,fd,kind", CONFIGS)
def test_projection_sampled(asm, cd, fd, kind):
    """project_function(FN_SAMPLED) of f_c with degree increase 0 and 1: the cell block and the face block against truth"""
    B = Batch(asm, cd, fd, kind)
    failures = []
    for dinc in (0, 1):
        if no_rule(cd, kind, dinc):
            assert not any(B.has(k, "proj1") for k in range(B.n))
            continue
        out, info = sampled_projection(asm, B, dinc)
        got, info = out.cpu().numpy(), info.cpu().numpy()
        label = "project sampled (%d,%d) %s dinc %d" % (cd, fd, kind, dinc)
        ec, ef = block_errors(B, got, "proj%d" % dinc)
        judge(label, B.idx, "proj%d_cell" % dinc, ec, failures)
        judge(label, B.idx, "proj%d_face" % dinc, ef, failures)
        flagged = [(CASES[i], int(info[k])) for k, i in enumerate(B.idx) if info[k] and gated(i, "proj%d_cell" % dinc)]
        if flagged:
            failures.append("%s: the cell mass matrix of a gated cell is flagged: %s" % (label, flagged))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cd,fd,kind", CONFIGS)
def test_projection_and_dirichlet_data_builtin(asm, cd, fd, kind):
    """the built-in sin(pi x) sin(pi y): project_function and dirichlet_data against proj_sin; the two faces that are not
    Dirichlet faces keep zeros"""
    import proton_amd as pa
    B = Batch(asm, cd, fd, kind)
    failures = []
    got = asm.project_function(cd, fd, pa.capi.FN_SIN_SIN_SOL, quad=B.quad, dinc=0).cpu().numpy()
    label = "project built-in (%d,%d) %s" % (cd, fd, kind)
    ec, ef = block_errors(B, got, "proj_sin", sin=True)
    judge(label, B.idx, "sin_cell", ec, failures)
    judge(label, B.idx, "sin_face", ef, failures)
    g = asm.dirichlet_data(fd, pa.capi.FN_SIN_SIN_SOL).cpu().numpy()
    assert g.shape == (4 * B.n, B.fbs) and not g[B.free].any() and np.isfinite(g).all()
    full = np.zeros((B.n, B.ms))
    full[:, B.cbs:] = B.by_cell(g)
    _, ef = block_errors(B, full, "proj_sin", sin=True, mask=B.dirichlet_mask())
    judge("dirichlet built-in (%d,%d) %s" % (cd, fd, kind), B.idx, "sin_face", ef, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cd,fd,kind", CONFIGS)
def test_dirichlet_data_sampled(asm, cd, fd, kind):
    """dirichlet_data(FN_SAMPLED) of f_c against the face block of proj0, through the face -> (cell, local face) map"""
    B = Batch(asm, cd, fd, kind)
    g = sampled_dirichlet(asm, B).cpu().numpy()
    assert g.shape == (4 * B.n, B.fbs) and not g[B.free].any() and np.isfinite(g).all()
    full = np.zeros((B.n, B.ms))
    full[:, B.cbs:] = B.by_cell(g)
    failures = []
    _, ef = block_errors(B, full, "proj0", mask=B.dirichlet_mask())
    judge("dirichlet sampled (%d,%d) %s" % (cd, fd, kind), B.idx, "proj0_face", ef, failures)
    assert not failures, "\n".join(failures)


def recovery(asm, B, first=0, n=None):
    """-> uT of condensed_recover, rec of static_condensation of the GPU's own lc (cells [first, first + n))"""
    import proton_amd as pa
    last = B.n if n is None else first + n
    fT = dev(np.stack([B.truth(k, "fT") for k in range(first, last)]), asm)
    uF = dev(np.stack([B.truth(k, "uF") for k in range(first, last)]), asm)
    uT = asm.condensed_recover(B.cd, B.fd, uF, B.quad, pa.STAB_FANCY, rhs=fT, first=first, n=n)
    out = asm.local_ops(B.cd, B.fd, B.quad, pa.STAB_FANCY, first=first, n=n, want=("lc", "info"))
    S, g, rec, info = asm.static_condensation(B.cd, B.fd, out["lc"], fT)
    asm.synchronize()
    return uT, rec, out["info"], info


@pytest.mark.parametrize("cd,fd,kind", CONFIGS)
def test_recovery(asm, cd, fd, kind):
    """u_T = A_TT^-1 (f_T - A_TF u_F) of the fused pass, and r0 = A_TT^-1 f_T, R = -A_TT^-1 A_TF of the two-kernel route,
    against truth; f_T and u_F are the fixture's doubles"""
    B = Batch(asm, cd, fd, kind)
    uT, rec, info_lc, info_sc = recovery(asm, B)
    uT, rec = uT.cpu().numpy(), rec.cpu().numpy()                        # rec[c, col, :]: column col of [r0 | R]
    assert uT.shape == (B.n, B.cbs) and rec.shape == (B.n, B.nf + 1, B.cbs)
    failures = []
    label = "recovery (%d,%d) %s" % (cd, fd, kind)
    judge(label, B.idx, "uT", [HP.nerr(uT[k], B.truth(k, "uT")) for k in range(B.n)], failures)
    judge(label, B.idx, "r0", [HP.nerr(rec[k, 0], B.truth(k, "r0")) for k in range(B.n)], failures)
    judge(label, B.idx, "R", [HP.nerr(rec[k, 1:].T, B.truth(k, "R")) for k in range(B.n)], failures)
    flags = info_lc.cpu().numpy() | info_sc.cpu().numpy()
    flagged = [(CASES[i], int(flags[k])) for k, i in enumerate(B.idx) if flags[k] and gated(i, "R")]
    if flagged:
        failures.append("%s: a gated cell is flagged: %s" % (label, flagged))
    assert not failures, "\n".join(failures)


def placement_outputs(asm, B, first=0, n=None):
    """per CELL (so that batches in another order compare): built-in and sampled projections, built-in and sampled Dirichlet
    data in local face order, the recovered uT -- of cells [first, first + n)"""
    import proton_amd as pa
    last = B.n if n is None else first + n
    out = {"project built-in": asm.project_function(B.cd, B.fd, pa.capi.FN_SIN_SIN_SOL, quad=B.quad, dinc=0, first=first, n=n).cpu().numpy(),
           "project sampled dinc 1": sampled_projection(asm, B, 1, first, n)[0].cpu().numpy(),
           "uT": recovery(asm, B, first, n)[0].cpu().numpy()}
    # pa_dirichlet_data_batch has no sub-range: every call covers the context's faces
    out["dirichlet built-in"] = B.by_cell(asm.dirichlet_data(B.fd, pa.capi.FN_SIN_SIN_SOL).cpu().numpy())[first:last]
    out["dirichlet sampled"] = B.by_cell(sampled_dirichlet(asm, B).cpu().numpy())[first:last]
    return out


@pytest.mark.parametrize("cd,fd,kind", PLACEMENT)
def test_placement(asm, cd, fd, kind):
    """a cell's projection, Dirichlet data and recovered unknowns do not depend on where it stands in the batch (the batch
    reversed: other point ids, other face numbers) nor on the range of the call (two sub-ranges): bit for bit"""
    B = Batch(asm, cd, fd, kind)
    base = placement_outputs(asm, B)
    bad = []

    def compare(what, got, cells):
        """got[name][k] belongs to base cell cells[k]"""
        for name, a in got.items():
            want = base[name][cells]
            a = np.ascontiguousarray(a)
            assert a.shape == want.shape
            for k in np.nonzero((a.view(np.int64) != want.view(np.int64)).reshape(len(cells), -1).any(axis=1))[0]:
                bad.append("%s: %s of %s differs (relative %.2e)" % (what, name, CASES[B.idx[cells[k]]],
                                                                     np.abs(a[k] - want[k]).max() / np.abs(want[k]).max()))
        print("placement (%d,%d) %s %s: %d cells, %d outputs each, %d differences so far" % (cd, fd, kind, what, len(cells), len(got), len(bad)))

    rev = np.arange(B.n)[::-1]
    Br = Batch(asm, cd, fd, kind, order=rev)
    assert Br.idx == B.idx[::-1] and not np.array_equal(Br.cell_faces, B.cell_faces)       # other orientations at every place
    compare("reversed", placement_outputs(asm, Br), rev)
    B = Batch(asm, cd, fd, kind)
    split = B.n // 3
    for first, n in ((0, split), (split, B.n - split)):
        compare("first=%d n=%d" % (first, n), placement_outputs(asm, B, first, n), np.arange(first, first + n))
    assert not bad, "\n".join(bad[:20])


def exact_forms(A, d):
    """-> (sum_ij A_ij d_i d_j, sum_ij |A_ij| |d_i| |d_j|) in exact rational arithmetic; A[ms, ms] doubles, d a list of Fractions"""
    ms = len(d)
    FA = [[Fraction(float(A[i, j])) for j in range(ms)] for i in range(ms)]
    ad = [abs(x) for x in d]
    q = sum(d[i] * sum(FA[i][j] * d[j] for j in range(ms)) for i in range(ms))
    b = sum(ad[i] * sum(abs(FA[i][j]) * ad[j] for j in range(ms)) for i in range(ms))
    return q, b


@pytest.mark.parametrize("cd,fd,kind", CONFIGS)
def test_energy_form_exact(asm, cd, fd, kind):
    """(u - v)^T lc (u - v) per cell, with the GPU's own lc_fancy of the batch, against the exact value of the quadratic form of the
    same doubles: (a) u random, v = 0; (b) v the GPU's projection of f_c and u = v (1 + 1e-9 xi), nine digits cancelling in u - v.
    Every cell within 32 * 2^-53 * sum |A_ij| |d_i| |d_j|.  Then the batch tiled to 32 CUs + 37 cells, past one pass of the grid-stride
    loop: every tiled cell bit-identical to its first occurrence."""
    import torch
    import proton_amd as pa
    B = Batch(asm, cd, fd, kind)
    lc = asm.local_ops(cd, fd, B.quad, pa.STAB_FANCY, want=("lc",))["lc"]
    proj, _ = sampled_projection(asm, B, 0)
    rng = np.random.default_rng(1000 * cd + 10 * fd + (kind == "fan"))
    v = proj.cpu().numpy()
    # a cell whose mass matrix the projection flags (not gated: the oracle loses it too) may hold no finite value: take the truth
    v = np.where(np.isfinite(v), v, np.stack([B.truth(k, "proj0") for k in range(B.n)]))
    ua = rng.standard_normal((B.n, B.ms))
    ub = v * (1.0 + 1e-9 * rng.standard_normal((B.n, B.ms)))
    A = lc.cpu().numpy()                                    # A[c, j, i] = lc(i, j); the form does not care
    assert np.isfinite(A).all()
    failures = []
    runs = {}
    for name, u, vv in (("a: u random, v = 0", ua, None), ("b: u = v (1 + 1e-9 xi)", ub, v)):
        du, dv = dev(u, asm), (None if vv is None else dev(vv, asm))
        e = asm.energy_form(cd, fd, lc, du, dv).cpu().numpy()
        runs[name] = (du, dv, e)
        worst = 0.0
        for c in range(B.n):
            d = [Fraction(float(u[c, i])) - (Fraction(float(vv[c, i])) if vv is not None else 0) for i in range(B.ms)]
            q, b = exact_forms(A[c], d)
            bound = 32 * Fraction(1, 2 ** 53) * b
            err = abs(Fraction(float(e[c])) - q)
            if b > 0:
                worst = max(worst, float(err / bound))
            if not err <= bound:
                failures.append("energy %s, %s: e_gpu %.17g, exact %.17g, error %.3e beyond the bound %.3e"
                                % (name, CASES[B.idx[c]], e[c], float(q), float(err), float(bound)))
        print("energy (%d,%d) %s %-24s %d cells, worst error / bound %.3f" % (cd, fd, kind, name, B.n, worst))
    # the grid is min(n, 32 * CUs) blocks: with 32 CUs + 37 cells the first 37 blocks take a second cell
    ntile = 32 * torch.cuda.get_device_properties(asm.device).multi_processor_count + 37
    src = torch.arange(ntile, device=asm.device) % B.n
    lct = lc[src].contiguous()
    for name, (du, dv, e) in runs.items():
        et = asm.energy_form(cd, fd, lct, du[src].contiguous(), None if dv is None else dv[src].contiguous()).cpu().numpy()
        assert et.shape == (ntile,)
        diff = np.nonzero(et != e[src.cpu().numpy()])[0]
        print("energy (%d,%d) %s %-24s tiled to %d cells: %d differ from their first occurrence" % (cd, fd, kind, name, ntile, len(diff)))
        if len(diff):
            failures.append("energy %s tiled: %d of %d cells differ from their first occurrence, the first at %d" % (name, len(diff), ntile, diff[0]))
    assert not failures, "\n".join(failures[:20])
