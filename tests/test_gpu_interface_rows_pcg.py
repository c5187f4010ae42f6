"""The two-level preconditioned CG on the interface problem's row slabs: the slab tables of pa_interface_rows_patches /
pa_interface_rows_coarse (patch_precond.hip, coarse_precond.hip) bit for bit against the twin of tests/interface_rows_pcg_twin.py
and against the slices of the device's own whole-mesh tables, their refusals, and pa_conjugated_gradient_rows_patch_coarse through
them: thread-ranks (tests/cg_transport.py) against the one-process solver with the slabs' patch tables stacked -- the same
preconditioner in exact arithmetic --, bit identity of the one-slab case and of a repeat, a jump in kappa on a shifted box, and the
slab path end to end against the xlsx Interface table.  One run: profiles/interface_rows_pcg_parity.txt
(INTERFACE_ROWS_PCG_PROFILE=that file python -m pytest tests/test_gpu_interface_rows_pcg.py -m gpu -s)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import interface_rows_pcg_twin as T
import patch_pcg_twin as PT
from cg_transport import ThreadTransport

pytestmark = pytest.mark.gpu

REPORT = []
JOIN = 120                                 # seconds a rank may take: a defect fails the test, it does not hang it
KINDS = ("face", "cell")
PARTS = ("one", "side")
HS = (3, 4)
RANKS = {2: (0, 7, 12), 3: (0, 3, 8, 12), 4: (0, 1, 5, 6, 12)}
COARSE = {"none": None, "one-4": ("one", 4), "side-3": ("side", 3)}


def say(line):
    print(line)
    REPORT.append(line)


def new_asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def host(t):
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in t)


def patches_of(t):
    return PT.Patches(*host(t))


# ---- 1. the tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CASES))
def test_slab_tables_equal_the_twin_and_the_whole_mesh_slices(oracle, name):
    """face degrees 0..3, both kinds, H = 3 and 4, both parts, on every slab: the twin's tables bit for bit; the slices of the
    device's own whole-mesh tables; ncoarse the whole mesh's on every slab; the query's sizes the tables'; a repeat the same bits;
    and the one-slab context exactly pa_interface_condensed_patches / _coarse"""
    from proton_amd import capi
    N, bounds, kw = T.case(name)
    msh = T.oracle_mesh(oracle, name)
    w = new_asm()
    w.cut_preprocess(N, **kw)
    slabs = []
    for rows in zip(bounds[:-1], bounds[1:]):
        a = new_asm()
        a.cut_preprocess(N, rows=rows, **kw)
        slabs.append(a)
    for k in (0, 1, 2, 3):
        fbs = k + 1
        rg = T.ranges(msh, bounds, fbs)
        want_p = T.slab_patches(msh, k, bounds)
        dev_whole = {kind: patches_of(w.interface_condensed_patches(k, kind)) for kind in KINDS}
        wf, wc, _ = T.whole_patches(msh, k)
        assert T.same_patches(dev_whole["face"], wf) and T.same_patches(dev_whole["cell"], wc)
        got_p = []
        for s, a in enumerate(slabs):
            inf = a.interface_rows_info(k)
            assert (inf.row_begin, inf.row_end) == rg[s]
            got = [patches_of(a.interface_rows_patches(k, kind)) for kind in KINDS]
            a.synchronize()
            for i, kind in enumerate(KINDS):
                assert got[i].ptr.dtype == np.int64 and got[i].rows.dtype == np.int32
                assert T.same_patches(got[i], want_p[s][i]), (name, k, s, kind)
                assert a.ctx.interface_rows_patches_query(k, {"face": capi.PATCH_FACE, "cell": capi.PATCH_CELL}[kind]) == \
                    (got[i].ptr.size - 1, got[i].rows.size)
                assert T.same_patches(patches_of(a.interface_rows_patches(k, kind)), got[i])
            got_p.append(got)
        # the device's own whole-mesh tables: the face patches concatenate to it; the cell table cut by the twin's rule
        assert T.same_patches(T.stacked([g[0] for g in got_p]), dev_whole["face"])
        if len(slabs) == 1:
            assert T.same_patches(got_p[0][1], dev_whole["cell"])
        for H in HS:
            for parts in PARTS:
                whole = host(w.interface_condensed_coarse(k, H, parts))
                assert T.same_table(whole, T.whole_coarse(msh, k, H, parts))
                want = T.slab_coarse(msh, k, H, parts, bounds)
                for s, a in enumerate(slabs):
                    got = host(a.interface_rows_coarse(k, H, parts))
                    a.synchronize()
                    r0, r1 = rg[s]
                    assert got[0].size == r1 - r0 + 1 and got[3] == whole[3]
                    assert T.same_table(got, want[s]), (name, k, H, parts, s)
                    assert np.array_equal(got[2].view(np.int64), want[s].vals.view(np.int64))
                    e0, e1 = whole[0][r0], whole[0][r1]
                    assert np.array_equal(got[0], whole[0][r0:r1 + 1] - e0) and np.array_equal(got[1], whole[1][e0:e1])
                    assert np.array_equal(got[2].view(np.int64), whole[2][e0:e1].view(np.int64))
                    assert a.ctx.interface_rows_coarse_query(k, H, {"one": capi.COARSE_ONE, "side": capi.COARSE_BY_SIDE}[parts]) == \
                        (got[3], got[1].size)
                    assert T.same_table(host(a.interface_rows_coarse(k, H, parts)), got)
    say("tables %-18s %d slab(s), k 0..3, face / cell, H 3 / 4, one / side: equal to the twin and to the whole-mesh slices" % (name, len(slabs)))


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_no_buffer():
    """what pa_interface_rows_* refuses in its order (face degree, no cut mesh), then the kind / H / parts and the NULL outputs, then
    the column count with H in pa_last_error(); canary-filled outputs and the queries' sizes stay as they were; the whole-mesh entry
    points still refuse a slab context"""
    import torch
    from proton_amd import capi
    L = capi.lib()
    a = new_asm()
    ptr = torch.full((1 << 12,), -5, dtype=torch.int64, device=a.device)
    idx = torch.full((1 << 14,), -7, dtype=torch.int32, device=a.device)
    vals = torch.full((1 << 14,), -9.0, dtype=torch.float64, device=a.device)
    na, nb = C.c_size_t(7), C.c_size_t(9)
    P, I_, V = ptr.data_ptr(), idx.data_ptr(), vals.data_ptr()

    def patch_calls(h, fd, kind=capi.PATCH_CELL):
        return [L.pa_interface_rows_patches_query(h, fd, kind, C.byref(na), C.byref(nb)), L.pa_interface_rows_patches(h, fd, kind, P, I_)]

    def coarse_calls(h, fd, H=4, parts=capi.COARSE_BY_SIDE):
        return [L.pa_interface_rows_coarse_query(h, fd, H, parts, C.byref(na), C.byref(nb)), L.pa_interface_rows_coarse(h, fd, H, parts, P, I_, V)]

    def calls(h, fd):
        return patch_calls(h, fd) + coarse_calls(h, fd)

    def untouched():
        a.synchronize()
        return (na.value, nb.value) == (7, 9) and bool((ptr == -5).all()) and bool((idx == -7).all()) and bool((vals == -9.0).all())

    assert calls(None, 1) == [1] * 4
    assert calls(a.ctx.h, 1) == [5] * 4                          # no mesh
    assert calls(a.ctx.h, 4) == [2] * 4                          # the face degree comes first
    a.generate_mesh(8, 8)
    assert calls(a.ctx.h, 1) == [5] * 4                          # a plain mesh, no cut mesh
    a.cut_preprocess(12, rows=(5, 6))                            # cut cells and a row below: neither cut-cell arrays nor a halo are asked for
    assert a.ncut > 0
    h = a.ctx.h
    for fd in (-1, 4):
        assert calls(h, fd) == [2] * 4
        assert patch_calls(h, fd, 7) == [2, 2] and coarse_calls(h, fd, 0, 7) == [2, 2]      # ... before the kind, H and the parts
    for kind in (-1, 2):
        assert patch_calls(h, 1, kind) == [1, 1]
    for H in (0, -3):
        assert coarse_calls(h, 1, H) == [1, 1]
    for parts in (-1, 2):
        assert coarse_calls(h, 1, 4, parts) == [1, 1]
    assert L.pa_interface_rows_patches_query(h, 1, capi.PATCH_CELL, None, C.byref(nb)) == 1
    assert L.pa_interface_rows_patches_query(h, 1, capi.PATCH_CELL, C.byref(na), None) == 1
    assert L.pa_interface_rows_patches(h, 1, capi.PATCH_CELL, None, I_) == 1
    assert L.pa_interface_rows_patches(h, 1, capi.PATCH_CELL, P, None) == 1
    assert L.pa_interface_rows_coarse_query(h, 1, 4, capi.COARSE_ONE, None, C.byref(nb)) == 1
    assert L.pa_interface_rows_coarse_query(h, 1, 4, capi.COARSE_ONE, C.byref(na), None) == 1
    assert L.pa_interface_rows_coarse(h, 1, 4, capi.COARSE_ONE, None, I_, V) == 1
    assert L.pa_interface_rows_coarse(h, 1, 4, capi.COARSE_ONE, P, None, V) == 1
    assert L.pa_interface_rows_coarse(h, 1, 4, capi.COARSE_ONE, P, I_, None) == 1
    for H in (12, 13, 100):                                      # H >= N: no interior node
        for parts in (capi.COARSE_ONE, capi.COARSE_BY_SIDE):
            assert coarse_calls(h, 1, H, parts) == [1, 1]
            msg = L.pa_last_error(h).decode()
            assert "H = %d" % H in msg and " 0 coarse columns" in msg
    assert untouched()
    a.cut_preprocess(66, rows=(30, 33))
    h = a.ctx.h
    assert coarse_calls(h, 0, 1, capi.COARSE_ONE) == [1, 1]      # 65 x 65 nodes: the WHOLE mesh's count on a three-row slab
    msg = L.pa_last_error(h).decode()
    assert "H = 1" in msg and "4225" in msg
    assert coarse_calls(h, 0, 1, capi.COARSE_BY_SIDE) == [1, 1]
    assert untouched()
    # the whole-mesh entry points still refuse the slab, after the slab's own have run on it
    assert coarse_calls(h, 0, 2, capi.COARSE_BY_SIDE) == [0, 0] and patch_calls(h, 0) == [0, 0]
    a.synchronize()
    assert L.pa_interface_condensed_patches_query(h, 0, capi.PATCH_CELL, C.byref(na), C.byref(nb)) == 1
    assert "whole mesh" in L.pa_last_error(h).decode()
    assert L.pa_interface_condensed_coarse_query(h, 0, 2, capi.COARSE_ONE, C.byref(na), C.byref(nb)) == 1
    assert L.pa_interface_condensed_patches(h, 0, capi.PATCH_CELL, P, I_) == 1
    assert L.pa_interface_condensed_coarse(h, 0, 2, capi.COARSE_ONE, P, I_, V) == 1


# ---- the systems of the solves ----------------------------------------------------------------------------------------------------------
_systems = {}


def system(name, k, bounds, kappa=(1.0, 1.0)):
    """once per case: the whole-mesh face-only system with the assembled right-hand side plus a seeded random vector, scipy's direct
    solve, the slabs (each in its own context, the real halo handed up), and the Jacobi rows solve's count; never modified"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import torch
    import proton_amd as pa
    key = (name, k, bounds, kappa)
    if key in _systems:
        return _systems[key]
    N, _, kw = T.case(name)
    Ny = kw.get("Ny", N)

    def ops_of(a, rows=None):
        a.cut_preprocess(N, rows=rows, **kw)
        return a.interface_local_ops(k, kappa=kappa), a.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    a = new_asm()
    ops, g = ops_of(a)
    rec = a.interface_condensed_ops(k, ops)
    rp, ci = a.interface_condensed_csr_pattern(k)
    va, RH = a.interface_condensed_csr_fill(k, rec, g)
    n = RH.numel()
    gen = torch.Generator().manual_seed(1234 + N + k)
    b = (RH.cpu() + torch.rand(n, generator=gen, dtype=torch.float64) - 0.5).to(a.device)
    a.synchronize()
    A = sp.csr_matrix((va.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n, n))
    sy = {"asm": a, "rp": rp, "ci": ci, "va": va, "b": b, "n": n, "direct": spla.spsolve(A.tocsc(), b.cpu().numpy()), "slabs": []}
    halo, row = None, 0
    for rows in zip(bounds[:-1], bounds[1:]):
        s = new_asm()
        sops, sg = ops_of(s, rows)
        srec = s.interface_rows_ops(k, sops)
        inf = s.interface_rows_info(k)
        srp, sci = s.interface_rows_csr_pattern(k)
        sva, _ = s.interface_rows_csr_fill(k, srec, sg, halo_below=halo)
        halo = s.interface_rows_halo_pack(k, srec, sg).clone() if rows[1] < Ny else None
        s.synchronize()
        assert inf.row_begin == row and inf.system_size == n
        row = inf.row_end
        sy["slabs"].append({"asm": s, "info": inf, "rp": srp, "ci": sci, "va": sva})
    assert row == n
    out = solve_by_ranks(sy, None, None, 1e-11, jacobi=True)
    assert all(o[0][0] == 0 for o in out) and len({o[0][1] for o in out}) == 1
    sy["jacobi"] = out[0][0][1]
    _systems[key] = sy
    return sy


def slab_tables(sy, k, kind, coarse):
    """per slab (patches, coarse or None) on the slab's device"""
    out = []
    for s in sy["slabs"]:
        a = s["asm"]
        out.append((a.interface_rows_patches(k, kind), a.interface_rows_coarse(k, coarse[1], coarse[0]) if coarse else None))
        a.synchronize()
    return out


def solve_by_ranks(sy, tables, k, tol, jacobi=False, div=100.0):
    """rank r = a thread with slab r's context -> [((reason, iterations, residual), x on the host)]"""
    import torch
    slabs = sy["slabs"]
    R = len(slabs)
    tt = ThreadTransport(R)
    out, keep = [None] * R, []

    def run(r):
        s, inf = slabs[r], slabs[r]["info"]
        a = s["asm"]
        tp, cbs = tt.make(r, a.ctx)
        keep.append(cbs)
        bs = sy["b"][inf.row_begin:inf.row_end].clone()
        x = torch.zeros_like(bs)
        try:
            if jacobi:
                res = a.ctx.conjugated_gradient_rows(tp, inf.row_begin, inf.row_end, s["rp"].data_ptr(), s["ci"].data_ptr(), s["va"].data_ptr(),
                                                     bs.data_ptr(), x.data_ptr(), tol=tol, max_iter=10000)
            else:
                _, *res = a.conjugated_gradient_rows_patch_coarse(tp, inf.row_begin, inf.row_end, s["rp"], s["ci"], s["va"], bs, tables[r][0],
                                                                  tables[r][1], tol=tol, div=div, max_iter=10000, x=x)
            a.synchronize()
            out[r] = (tuple(res), x.cpu())
        except BaseException as e:      # noqa: BLE001  (a failed rank must not leave the others at a barrier)
            out[r] = e
            tt.bar.abort()

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN)
    assert all(not t.is_alive() for t in th), "a rank is still inside the solve"
    for o in out:
        assert not isinstance(o, BaseException), o
    return out


def stacked_patches(tables, device):
    """the slabs' patch tables one after the other on `device`: a valid whole-mesh table"""
    import torch
    ptrs, rows, off = [torch.zeros(1, dtype=torch.int64)], [], 0
    for (ptr, r), _ in tables:
        ptrs.append(ptr.cpu()[1:] + off)
        rows.append(r.cpu())
        off += r.numel()
    return torch.cat(ptrs).to(device), torch.cat(rows).to(device)


def judge(label, name, k, bounds, kind, coarse, kappa=(1.0, 1.0), tol=1e-11):
    """the checks of the preconditioner agreement: every rank exits with reason 0 in the same iteration, within 3 of the one-process
    solve with the slabs' patch tables stacked and the whole coarse table, the solution within 10 e_ref of scipy's direct solve
    (e_ref: that one-process solution's distance), and fewer iterations than the Jacobi rows solve of the same system"""
    sy = system(name, k, bounds, kappa)
    a = sy["asm"]
    tables = slab_tables(sy, k, kind, coarse)
    pt = stacked_patches(tables, a.device)
    if coarse:
        tb = a.interface_condensed_coarse(k, coarse[1], coarse[0])
        xw, reason, iters, _ = a.conjugated_gradient_patch_coarse(sy["rp"], sy["ci"], sy["va"], sy["b"], pt, tb, tol=tol, max_iter=10000)
    else:
        xw, reason, iters, _ = a.conjugated_gradient_patch(sy["rp"], sy["ci"], sy["va"], sy["b"], pt, tol=tol, max_iter=10000)
    a.synchronize()
    assert reason == 0
    e_ref = float(np.abs(xw.cpu().numpy() - sy["direct"]).max())
    out = solve_by_ranks(sy, tables, k, tol)
    x = np.concatenate([o[1].numpy() for o in out])
    err = float(np.abs(x - sy["direct"]).max())
    got = out[0][0][1]
    say("%s: e_ref %.3e, ranks %.3e, iterations %d / %d one process, Jacobi rows %d" % (label, e_ref, err, got, iters, sy["jacobi"]))
    assert all(o[0][0] == 0 for o in out)
    assert len({o[0][1] for o in out}) == 1
    assert abs(got - iters) <= 3
    assert x.size == sy["n"] and e_ref > 0.0
    assert err <= 10.0 * e_ref
    assert got < sy["jacobi"]
    return e_ref, err, got, iters, sy["jacobi"]


# ---- 3. the preconditioner agreement with one rank ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("coarse", list(COARSE))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", list(RANKS))
@pytest.mark.parametrize("k", [1, 2])
def test_ranks_agree_with_the_stacked_one_process_solve(k, R, kind, coarse):
    """N = 12, real operators, tolerance 1e-11, the assembled right-hand side plus the seeded random vector (as
    test_gpu_interface_rows.test_ranks_reproduce_the_whole_mesh_solve); 2, 3 and 4 thread-ranks.  The margins 3 (the dot products are
    grouped by rank) and 10 e_ref are that test's own.  Measured on an MI355X: MEASURED below."""
    judge("k %d, %d ranks, %s, coarse %s" % (k, R, kind, coarse), "circle-12", k, RANKS[R], kind, COARSE[coarse])


# test_ranks_agree_with_the_stacked_one_process_solve as measured on an MI355X: (k, ranks, kind, coarse) ->
# (e_ref, distance of the ranks' solution to the direct solve, iterations of the ranks, of the one-process solve, of the Jacobi rows solve)
MEASURED = {
    (1, 2, "face", "none"): (4.634e-12, 4.634e-12, 90, 90, 157),
    (1, 2, "face", "one-4"): (6.040e-12, 6.028e-12, 75, 75, 157),
    (1, 2, "face", "side-3"): (4.465e-12, 4.471e-12, 60, 60, 157),
    (1, 2, "cell", "none"): (1.291e-11, 1.291e-11, 80, 80, 157),
    (1, 2, "cell", "one-4"): (9.672e-12, 9.665e-12, 64, 64, 157),
    (1, 2, "cell", "side-3"): (6.914e-12, 6.918e-12, 53, 53, 157),
    (1, 3, "face", "none"): (4.634e-12, 4.633e-12, 90, 90, 157),
    (1, 3, "face", "one-4"): (6.040e-12, 6.027e-12, 75, 75, 157),
    (1, 3, "face", "side-3"): (4.465e-12, 4.462e-12, 60, 60, 157),
    (1, 3, "cell", "none"): (6.906e-12, 6.906e-12, 85, 85, 157),
    (1, 3, "cell", "one-4"): (1.366e-11, 1.366e-11, 62, 62, 157),
    (1, 3, "cell", "side-3"): (7.698e-12, 7.696e-12, 53, 53, 157),
    (1, 4, "face", "none"): (4.634e-12, 4.633e-12, 90, 90, 157),
    (1, 4, "face", "one-4"): (6.040e-12, 6.023e-12, 75, 75, 157),
    (1, 4, "face", "side-3"): (4.465e-12, 4.477e-12, 60, 60, 157),
    (1, 4, "cell", "none"): (1.362e-11, 1.362e-11, 85, 85, 157),
    (1, 4, "cell", "one-4"): (6.388e-12, 6.389e-12, 65, 65, 157),
    (1, 4, "cell", "side-3"): (5.558e-12, 5.558e-12, 56, 56, 157),
    (2, 2, "face", "none"): (3.564e-10, 3.552e-10, 87, 87, 554),
    (2, 2, "face", "one-4"): (4.499e-10, 4.480e-10, 73, 73, 554),
    (2, 2, "face", "side-3"): (3.328e-10, 3.328e-10, 57, 57, 554),
    (2, 2, "cell", "none"): (2.593e-10, 2.563e-10, 80, 80, 554),
    (2, 2, "cell", "one-4"): (4.728e-10, 4.709e-10, 62, 62, 554),
    (2, 2, "cell", "side-3"): (3.126e-10, 3.124e-10, 52, 52, 554),
    (2, 3, "face", "none"): (3.564e-10, 3.550e-10, 87, 87, 554),
    (2, 3, "face", "one-4"): (4.499e-10, 4.424e-10, 73, 73, 554),
    (2, 3, "face", "side-3"): (3.328e-10, 3.322e-10, 57, 57, 554),
    (2, 3, "cell", "none"): (2.873e-10, 2.863e-10, 84, 84, 554),
    (2, 3, "cell", "one-4"): (2.668e-10, 2.646e-10, 63, 63, 554),
    (2, 3, "cell", "side-3"): (4.298e-10, 4.281e-10, 54, 54, 554),
    (2, 4, "face", "none"): (3.564e-10, 3.539e-10, 87, 87, 554),
    (2, 4, "face", "one-4"): (4.499e-10, 4.522e-10, 73, 73, 554),
    (2, 4, "face", "side-3"): (3.328e-10, 3.339e-10, 57, 57, 554),
    (2, 4, "cell", "none"): (2.924e-10, 2.957e-10, 85, 85, 554),
    (2, 4, "cell", "one-4"): (6.022e-10, 5.432e-10, 68, 68, 554),
    (2, 4, "cell", "side-3"): (2.478e-10, 2.344e-10, 57, 57, 554),
}


# ---- 4. bit identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,coarse", [("cell", "side-3"), ("face", "one-4"), ("cell", "none")])
def test_one_slab_without_transport_is_the_one_process_solver(kind, coarse):
    """the one-slab context, transport = NULL: pa_conjugated_gradient_patch_coarse with the whole-mesh tables bit for bit in x,
    iterations and residual"""
    import torch
    k = 2
    sy = system("circle-12", k, (0, 12))
    a, s = sy["asm"], sy["slabs"][0]
    (pt, tb), = slab_tables(sy, k, kind, COARSE[coarse])
    wpt = a.interface_condensed_patches(k, kind)
    assert all(torch.equal(u.cpu(), v.cpu()) for u, v in zip(pt, wpt))
    if tb is not None:
        wtb = a.interface_condensed_coarse(k, COARSE[coarse][1], COARSE[coarse][0])
        assert all(torch.equal(u.cpu(), v.cpu()) for u, v in zip(tb[:3], wtb[:3])) and tb[3] == wtb[3]
        x0, *r0 = a.conjugated_gradient_patch_coarse(sy["rp"], sy["ci"], sy["va"], sy["b"], wpt, wtb, tol=1e-11, max_iter=10000)
    else:
        x0, *r0 = a.conjugated_gradient_patch(sy["rp"], sy["ci"], sy["va"], sy["b"], wpt, tol=1e-11, max_iter=10000)
    a.synchronize()
    b = sy["b"].to(s["asm"].device)
    x1, *r1 = s["asm"].conjugated_gradient_rows_patch_coarse(None, 0, sy["n"], s["rp"], s["ci"], s["va"], b, pt, tb, tol=1e-11, max_iter=10000)
    s["asm"].synchronize()
    assert r0[0] == 0 and r1 == r0 and torch.equal(x0.cpu(), x1.cpu()), (r0, r1)
    say("one slab, no transport, k %d %s coarse %s: %d iterations, x, count and residual bit for bit" % (k, kind, coarse, r0[1]))


def test_two_runs_of_three_ranks_give_the_same_bits():
    import torch
    k = 2
    sy = system("circle-12", k, RANKS[3])
    runs = []
    for _ in range(2):
        out = solve_by_ranks(sy, slab_tables(sy, k, "cell", COARSE["side-3"]), k, 1e-11)
        runs.append(([o[0] for o in out], torch.cat([o[1] for o in out])))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


# ---- 5. a jump in kappa on the shifted box ---------------------------------------------------------------------------------------------
def test_kappa_jump_on_the_shifted_box():
    """mesh B of tests/cut_meshes.py (15 x 11, both origins non-zero), k = 1, kappa = (1, 7.5), slabs (0, 4, 5, 11), cell patches and
    the table by side (H = 3): the checks of the preconditioner agreement.  Measured on an MI355X: MEASURED_KAPPA"""
    _, bounds, _ = T.case("B")
    judge("B kappa (1, 7.5) k 1, 3 ranks, cell, coarse side-3", "B", 1, bounds, "cell", COARSE["side-3"], kappa=(1.0, 7.5))


MEASURED_KAPPA = (2.830e-11, 2.830e-11, 44, 44, 144)      # as the values of MEASURED


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
def test_slab_path_with_both_levels_reproduces_xlsx(oracle):
    """operators per slab -> records -> halo -> CSR -> the two-level rows solve -> pa_interface_rows_recover: the slab path's xlsx check
    (test_gpu_interface_rows.test_slab_path_reproduces_xlsx: N = 20, k = 1, two slabs, threshold 1e-9) with its helpers and its gate"""
    import torch
    import test_gpu_interface_rows as G
    N, k, bounds, ref = 20, 1, (0, 7, 20), 5.22389e-3
    w = G.whole_mesh(N, k)
    slabs = G.assemble_slabs(N, k, bounds, {}, w, synthetic=False)
    sy = {"slabs": slabs, "b": w["RH"]}
    tables = slab_tables(sy, k, "cell", ("side", 4))
    out = solve_by_ranks(sy, tables, k, 1e-9)
    assert all(o[0][0] == 0 for o in out) and len({o[0][1] for o in out}) == 1
    xF = torch.cat([o[1] for o in out])
    assert xF.numel() == slabs[0]["info"].system_size
    cells = []
    for s in slabs:
        i, a = s["info"], s["asm"]
        cells.append(a.interface_rows_recover(k, s["ops"], xF[i.row_begin:i.col_end].to(a.device), s["g"]).cpu())
        a.synchronize()
    sol = torch.cat(cells + [xF]).numpy()
    err = G.energy_error(oracle, sol, N, k)
    say("slab path (%d, %d), 2 ranks, cell + side H 4 at 1e-9: %d iterations, energy error %.10e (xlsx %.6e)" % (N, k, out[0][0][1], err, ref))
    assert abs(err - ref) / ref < 6e-6, err


# ---- the report -----------------------------------------------------------------------------------------------------------------------
def test_zz_report():
    """the lines of the run (with -s); written to the file INTERFACE_ROWS_PCG_PROFILE names, if it names one"""
    path = os.environ.get("INTERFACE_ROWS_PCG_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_interface_rows_pcg.py on one MI355X: the slab tables of pa_interface_rows_patches / pa_interface_rows_coarse\n"
                    "against the numpy twin of tests/interface_rows_pcg_twin.py and the device's whole-mesh tables (bit for bit), and\n"
                    "pa_conjugated_gradient_rows_patch_coarse through them on 2, 3 and 4 thread-ranks against the one-process solver with the\n"
                    "slabs' patch tables stacked, scipy's direct solve and the Jacobi rows solve of the same system.\n")
            f.write("\n".join(REPORT) + "\n")
