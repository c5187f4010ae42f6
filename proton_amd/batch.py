"""Torch-tensor convenience layer over the C ABI (device memory + streams only).

All compute happens inside libproton_amd.so; torch provides allocations and the stream.
"""
import numpy as np
import torch

from . import capi


def _ptr(t):
    return None if t is None else t.data_ptr()


class BatchAssembler:
    """Batched counterpart of the reference's per-cell loop (convergence_test.cpp:202-213):
    make_hho_laplacian + stabilization (+ make_rhs) for a block of cells, on one GPU."""

    def __init__(self, device=0, use_torch_stream=True):
        if not torch.cuda.is_available():
            raise RuntimeError("proton_amd needs a GPU: torch.cuda.is_available() is False (no CPU fallback)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        if use_torch_stream:      # enqueue on torch's current stream (0 = the default stream)
            self.ctx = capi.Context(device, torch.cuda.current_stream(self.device).cuda_stream)
        else:
            self.ctx = capi.Context(device, own_stream=True)
        self._keep = []

    # ---- mesh -----------------------------------------------------------------------
    def set_mesh(self, points, ptids):
        points = np.ascontiguousarray(points, dtype=np.float64)
        ptids = np.ascontiguousarray(ptids)
        assert ptids.max() < 2 ** 32
        self.ctx.mesh_upload(points, ptids.astype(np.uint32))

    def generate_mesh(self, Nx, Ny, lo=(0.0, 0.0), hi=(1.0, 1.0), rows=None):
        self.ctx.mesh_generate(Nx, Ny, lo, hi, rows)

    @property
    def ncells(self):
        return self.ctx.mesh_counts()[1]

    # ---- hot path -------------------------------------------------------------------
    def local_ops(self, cd, fd, quad=capi.QUAD_TENSOR, stab=capi.STAB_FANCY, first=0, n=None,
                  want=("lc",), out=None):
        """Returns dict of cell-major torch tensors [n, cols, rows] (column-major matrices:
        entry (i, j) is t[c, j, i]); `out` may carry preallocated tensors to reuse."""
        di, _ = capi.degree_info(cd, fd)
        sz = capi.sizes_for(di, quad)
        if n is None:
            n = self.ncells - first
        out = dict(out or {})
        shapes = {"oper": (n, sz.msize, sz.oper_rows), "data": (n, sz.msize, sz.msize),
                  "stab": (n, sz.msize, sz.msize), "lc": (n, sz.msize, sz.msize)}
        for k in want:
            if k == "info":
                if "info" not in out:
                    out["info"] = torch.empty(n, dtype=torch.int32, device=self.device)
            elif k not in out:
                out[k] = torch.empty(shapes[k], dtype=torch.float64, device=self.device)
        self.ctx.local_ops(di, quad, stab, first, n, _ptr(out.get("oper")), _ptr(out.get("data")),
                           _ptr(out.get("stab")), _ptr(out.get("lc")), _ptr(out.get("info")))
        return out

    def cell_rhs(self, degree, fn, quad=capi.QUAD_TENSOR, dinc=0, first=0, n=None, fvals=None, out=None):
        if n is None:
            n = self.ncells - first
        cbs = (degree + 2) * (degree + 1) // 2
        if out is None:
            out = torch.empty((n, cbs), dtype=torch.float64, device=self.device)
        self.ctx.cell_rhs(degree, dinc, quad, fn, first, n, out.data_ptr(), _ptr(fvals))
        return out

    def quadrature_points(self, degree, quad=capi.QUAD_TENSOR, first=0, n=None):
        if n is None:
            n = self.ncells - first
        nq = self.ctx.cell_quadrature_points(degree, quad, first, n, None)
        out = torch.empty((n, nq, 3), dtype=torch.float64, device=self.device)
        self.ctx.cell_quadrature_points(degree, quad, first, n, out.data_ptr())
        return out

    def static_condensation(self, cd, fd, lc, rhs=None):
        di, _ = capi.degree_info(cd, fd)
        sz = capi.sizes_for(di, capi.QUAD_TENSOR)
        n, nf = lc.shape[0], 4 * sz.fbs
        S = torch.empty((n, nf, nf), dtype=torch.float64, device=self.device)
        g = torch.empty((n, nf), dtype=torch.float64, device=self.device)
        rec = torch.empty((n, nf + 1, sz.cbs), dtype=torch.float64, device=self.device)
        info = torch.empty(n, dtype=torch.int32, device=self.device)
        self.ctx.static_condensation(di, n, lc.data_ptr(), _ptr(rhs), S.data_ptr(), g.data_ptr(), rec.data_ptr(),
                                     info.data_ptr())
        return S, g, rec, info

    # ---- condensed mode (static condensation fused into the local-operator pass) ------
    def condensed_ops(self, cd, fd, quad=capi.QUAD_TENSOR, stab=capi.STAB_FANCY, rhs=None, first=0, n=None, out=None, want_info=False):
        """-> packed records [n, nf(nf+1)/2 + nf]: upper triangle of the Schur complement (column-packed), then g."""
        di, _ = capi.degree_info(cd, fd)
        n = self.ncells - first if n is None else n
        nf = 4 * (di.face_deg + 1)
        if out is None:
            out = torch.empty((n, nf * (nf + 1) // 2 + nf), dtype=torch.float64, device=self.device)
        info = torch.empty(n, dtype=torch.int32, device=self.device) if want_info else None
        self.ctx.condensed_ops(di, quad, stab, first, n, _ptr(rhs), out.data_ptr(), _ptr(info))
        return (out, info) if want_info else out

    def condensed_recover(self, cd, fd, uF, quad=capi.QUAD_TENSOR, stab=capi.STAB_FANCY, rhs=None, first=0, n=None):
        """u_T = A_TT^-1 (f_T - A_TF u_F) for cells [first, first+n) -> [n, cbs]."""
        di, _ = capi.degree_info(cd, fd)
        n = self.ncells - first if n is None else n
        cbs = (di.cell_deg + 1) * (di.cell_deg + 2) // 2
        uT = torch.empty((n, cbs), dtype=torch.float64, device=self.device)
        self.ctx.condensed_recover(di, quad, stab, first, n, _ptr(rhs), uF.data_ptr(), uT.data_ptr(), None)
        return uT

    def condensed_info(self, cd, fd):
        di, _ = capi.degree_info(cd, fd)
        return self.ctx.condensed_query(di)

    def condensed_triplets(self, cd, fd, cond, g=None, first=0):
        di, _ = capi.degree_info(cd, fd)
        n, nf = cond.shape[0], 4 * (di.face_deg + 1)
        rows = torch.empty((n, nf * nf), dtype=torch.int32, device=self.device)
        cols = torch.empty((n, nf * nf), dtype=torch.int32, device=self.device)
        vals = torch.empty((n, nf * nf), dtype=torch.float64, device=self.device)
        rhs_rows = torch.empty((n, nf), dtype=torch.int32, device=self.device)
        rhs_vals = torch.empty((n, nf), dtype=torch.float64, device=self.device)
        self.ctx.condensed_triplets(di, first, n, cond.data_ptr(), _ptr(g), rows.data_ptr(), cols.data_ptr(), vals.data_ptr(),
                                    rhs_rows.data_ptr(), rhs_vals.data_ptr())
        return rows, cols, vals, rhs_rows, rhs_vals

    def condensed_csr_pattern(self, cd, fd):
        """symbolic phase -> (rowptr int64 [rows+1], colind int32 [nnz]) of the rows this context owns"""
        di, _ = capi.degree_info(cd, fd)
        ci = self.ctx.condensed_query(di)
        rowptr = torch.empty(ci.row_end - ci.row_begin + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(ci.nnz_owned, 1), dtype=torch.int32, device=self.device)
        self.ctx.condensed_csr_pattern(di, rowptr.data_ptr(), colind.data_ptr())
        return rowptr, colind[:ci.nnz_owned]

    def condensed_csr_fill(self, cd, fd, cond, g=None, halo_below=None, values=None, rhs=None):
        """numeric phase -> (values [nnz], rhs [rows])"""
        di, _ = capi.degree_info(cd, fd)
        ci = self.ctx.condensed_query(di)
        if values is None:
            values = torch.empty(max(ci.nnz_owned, 1), dtype=torch.float64, device=self.device)
        if rhs is None:
            rhs = torch.empty(max(ci.row_end - ci.row_begin, 1), dtype=torch.float64, device=self.device)
        self.ctx.condensed_csr_fill(di, cond.data_ptr(), _ptr(g), _ptr(halo_below), values.data_ptr(), rhs.data_ptr())
        return values[:ci.nnz_owned], rhs[:ci.row_end - ci.row_begin]

    def condensed_halo_pack(self, cd, fd, cond, g=None, out=None):
        di, _ = capi.degree_info(cd, fd)
        ci = self.ctx.condensed_query(di)
        if out is None:
            out = torch.empty((max(ci.halo_cells, 1), ci.halo_doubles), dtype=torch.float64, device=self.device)
        self.ctx.condensed_halo_pack(di, cond.data_ptr(), _ptr(g), out.data_ptr())
        return out[:ci.halo_cells]

    def condensed_take_faces(self, cd, fd, solution, g=None, first=0, n=None):
        di, _ = capi.degree_info(cd, fd)
        n = self.ncells - first if n is None else n
        uF = torch.empty((n, 4 * (di.face_deg + 1)), dtype=torch.float64, device=self.device)
        self.ctx.condensed_take_faces(di, first, n, solution.data_ptr(), _ptr(g), uF.data_ptr())
        return uF

    def condensed_expand_solution(self, cd, fd, uT, xF, full=None):
        di, _ = capi.degree_info(cd, fd)
        info = self.ctx.assembler_query(di)
        if full is None:
            full = torch.zeros(info.system_size, dtype=torch.float64, device=self.device)
        self.ctx.condensed_expand_solution(di, uT.data_ptr(), _ptr(xF), full.data_ptr())
        return full

    # ---- assembler (hho.hpp:252-463) -------------------------------------------------
    def set_faces(self, cell_faces, face_pts, face_is_dirichlet):
        self.ctx.mesh_set_faces(cell_faces, face_pts, face_is_dirichlet)

    def assembler_info(self, cd, fd):
        di, _ = capi.degree_info(cd, fd)
        return self.ctx.assembler_query(di)

    def dirichlet_data(self, fd, fn, fvals=None):
        info = self.assembler_info(fd, fd)
        g = torch.empty((info.nfaces_local, fd + 1), dtype=torch.float64, device=self.device)
        self.ctx.dirichlet_data(fd, fn, g.data_ptr(), _ptr(fvals))
        return g

    def face_quadrature_points(self, fd):
        info = self.assembler_info(0, 0)
        out = torch.empty((info.nfaces_local, fd + 1, 3), dtype=torch.float64, device=self.device)
        self.ctx.face_quadrature_points(fd, out.data_ptr())
        return out

    def triplets(self, cd, fd, lc, rhs=None, g=None, first=0):
        """assembler::assemble for the cells lc covers -> (rows, cols, vals, rhs_rows, rhs_vals)."""
        di, _ = capi.degree_info(cd, fd)
        n, ms = lc.shape[0], lc.shape[1]
        rows = torch.empty((n, ms * ms), dtype=torch.int32, device=self.device)
        cols = torch.empty((n, ms * ms), dtype=torch.int32, device=self.device)
        vals = torch.empty((n, ms * ms), dtype=torch.float64, device=self.device)
        rhs_rows = torch.empty((n, ms), dtype=torch.int32, device=self.device)
        rhs_vals = torch.empty((n, ms), dtype=torch.float64, device=self.device)
        self.ctx.triplets(di, first, n, lc.data_ptr(), _ptr(rhs), _ptr(g), rows.data_ptr(), cols.data_ptr(),
                          vals.data_ptr(), rhs_rows.data_ptr(), rhs_vals.data_ptr())
        return rows, cols, vals, rhs_rows, rhs_vals

    def assembler_csr_pattern(self, cd, fd):
        """assembler<Mesh>'s own system (cell + face unknowns) directly in CSR, symbolic phase -> (rowptr int64 [nrows+1], colind int32 [nnz])"""
        di, _ = capi.degree_info(cd, fd)
        info = self.ctx.assembler_csr_query(di)
        rowptr = torch.empty(info.nrows + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(info.nnz, 1), dtype=torch.int32, device=self.device)
        self.ctx.assembler_csr_pattern(di, rowptr.data_ptr(), colind.data_ptr())
        return rowptr, colind[:info.nnz]

    def assembler_csr_fill(self, cd, fd, lc, rhs=None, g=None, values=None, RHS=None):
        """numeric phase of the same -> (values [nnz], RHS [nrows])"""
        di, _ = capi.degree_info(cd, fd)
        info = self.ctx.assembler_csr_query(di)
        if values is None:
            values = torch.empty(max(info.nnz, 1), dtype=torch.float64, device=self.device)
        if RHS is None:
            RHS = torch.empty(max(info.nrows, 1), dtype=torch.float64, device=self.device)
        self.ctx.assembler_csr_fill(di, lc.data_ptr(), _ptr(rhs), _ptr(g), values.data_ptr(), RHS.data_ptr())
        return values[:info.nnz], RHS[:info.nrows]

    def assembler_csr_assemble(self, cd, fd, quad=capi.QUAD_TENSOR, stab=capi.STAB_FANCY, rhs=None, g=None, values=None, RHS=None,
                               want=()):
        """local operators + numeric phase fused: the local-operator kernel writes the CSR values of assembler_csr_pattern from its
        on-chip image of lc (no [ncells, msize, msize] buffer unless "lc" is in `want`) -> dict(values [nnz], RHS [nrows]
        [, lc [ncells, msize, msize]] [, info [ncells]]); bit-identical to assembler_csr_fill of that lc"""
        di, _ = capi.degree_info(cd, fd)
        sz = capi.sizes_for(di, quad)
        info = self.ctx.assembler_csr_query(di)
        if values is None:
            values = torch.empty(max(info.nnz, 1), dtype=torch.float64, device=self.device)
        if RHS is None:
            RHS = torch.empty(max(info.nrows, 1), dtype=torch.float64, device=self.device)
        lc = torch.empty((self.ncells, sz.msize, sz.msize), dtype=torch.float64, device=self.device) if "lc" in want else None
        cinfo = torch.empty(self.ncells, dtype=torch.int32, device=self.device) if "info" in want else None
        self.ctx.assembler_csr_assemble(di, quad, stab, _ptr(rhs), _ptr(g), values.data_ptr(), RHS.data_ptr(), _ptr(lc), _ptr(cinfo))
        out = {"values": values[:info.nnz], "RHS": RHS[:info.nrows]}
        if lc is not None:
            out["lc"] = lc
        if cinfo is not None:
            out["info"] = cinfo
        return out

    def csr_from_triplets(self, rows, cols, vals, nrows):
        """setFromTriplets on the device -> (rowptr int64 [nrows+1], colind int32 [nnz], values [nnz])."""
        rows, cols, vals = rows.reshape(-1), cols.reshape(-1), vals.reshape(-1)
        n = rows.numel()
        rowptr = torch.empty(nrows + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        values = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        nnz = self.ctx.csr_from_triplets(n, rows.data_ptr(), cols.data_ptr(), vals.data_ptr(), nrows, rowptr.data_ptr(),
                                         colind.data_ptr(), values.data_ptr())
        return rowptr, colind[:nnz], values[:nnz]

    def conjugated_gradient(self, rowptr, colind, values, b, tol=1e-9, div=100.0, max_iter=1000, precond=True):
        """solver_cg.hpp:63-144 on the device -> (x, exit_reason, iterations, relative residual)"""
        x = torch.empty_like(b)
        reason, iters, rr = self.ctx.conjugated_gradient(b.numel(), rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(),
                                                         b.data_ptr(), x.data_ptr(), tol, div, max_iter, precond)
        return x, reason, iters, rr

    # ---- the patch preconditioner (patch_precond.hip) -----------------------------------
    def condensed_patches(self, cd, fd, kind):
        """the patch table of the face-only system of condensed_csr_pattern: kind "face" (one patch per non-Dirichlet face) or
        "cell" (one per cell, the rows of its non-Dirichlet faces) -> (patch_ptr int64 [npatches + 1], patch_rows int32)"""
        di, _ = capi.degree_info(cd, fd)
        kind = {"face": capi.PATCH_FACE, "cell": capi.PATCH_CELL}.get(kind, kind)
        npatches, entries = self.ctx.condensed_patches_query(di, kind)
        ptr = torch.empty(npatches + 1, dtype=torch.int64, device=self.device)
        rows = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        self.ctx.condensed_patches(di, kind, ptr.data_ptr(), rows.data_ptr())
        return ptr, rows[:entries]

    def patch_precond_factor(self, rowptr, colind, values, patches):
        """pa_patch_precond_query + pa_patch_precond_factor -> dict(factors, slots, scratch, info [npatches], failed, sizes,
        patches): what patch_precond_apply takes.  failed > 0: some patch has a non-positive pivot (info says which)."""
        ptr, rows = patches
        n, npatches = rowptr.numel() - 1, ptr.numel() - 1
        sz = self.ctx.patch_precond_query(n, npatches, ptr.data_ptr())
        factors = torch.empty(max(sz.factor_doubles, 1), dtype=torch.float64, device=self.device)
        slots = torch.empty(max(sz.slot_ints, 1), dtype=torch.int32, device=self.device)
        scratch = torch.empty(max(sz.scratch_bytes, 1), dtype=torch.uint8, device=self.device)
        info = torch.empty(max(npatches, 1), dtype=torch.int32, device=self.device)
        failed = self.ctx.patch_precond_factor(n, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), npatches, ptr.data_ptr(),
                                               rows.data_ptr(), factors.data_ptr(), slots.data_ptr(), scratch.data_ptr(), info.data_ptr())
        return {"factors": factors, "slots": slots, "scratch": scratch, "info": info[:npatches], "failed": failed, "sizes": sz,
                "patches": (ptr, rows), "n": n}

    def patch_precond_apply(self, pre, r, z=None):
        """z = sum_p R_p^T A_p^-1 R_p r with what patch_precond_factor returned"""
        ptr, rows = pre["patches"]
        if z is None:
            z = torch.empty_like(r)
        self.ctx.patch_precond_apply(pre["n"], ptr.numel() - 1, ptr.data_ptr(), rows.data_ptr(), pre["factors"].data_ptr(),
                                     pre["slots"].data_ptr(), pre["scratch"].data_ptr(), r.data_ptr(), z.data_ptr())
        return z

    def conjugated_gradient_patch(self, rowptr, colind, values, b, patches, tol=1e-9, div=100.0, max_iter=1000, x=None):
        """solver_cg.hpp:63-144 with the patch preconditioner -> (x, exit_reason, iterations, relative residual)"""
        ptr, rows = patches
        if x is None:
            x = torch.empty_like(b)
        reason, iters, rr = self.ctx.conjugated_gradient_patch(b.numel(), rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), b.data_ptr(),
                                                               x.data_ptr(), ptr.numel() - 1, ptr.data_ptr(), rows.data_ptr(), tol, div, max_iter)
        return x, reason, iters, rr

    # ---- the Galerkin coarse level (coarse_precond.hip) ----------------------------------
    def condensed_coarse(self, cd, fd, H, parts="one", where=capi.LOC_NEGATIVE):
        """the coarse table of the face-only system of condensed_csr_pattern: bilinear hats on every H-th mesh line, parts "one" or
        "side" (every hat split at the interface; needs the cut preprocessing) -> (p_ptr int64 [rows + 1], p_cols int32, p_vals
        float64, ncoarse)"""
        di, _ = capi.degree_info(cd, fd)
        parts = {"one": capi.COARSE_ONE, "side": capi.COARSE_BY_SIDE}.get(parts, parts)
        ncoarse, entries = self.ctx.condensed_coarse_query(di, H, parts, where)
        nrows = self.ctx.assembler_query(di).num_other_faces * (fd + 1)
        ptr = torch.empty(nrows + 1, dtype=torch.int64, device=self.device)
        cols = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        vals = torch.empty(max(entries, 1), dtype=torch.float64, device=self.device)
        self.ctx.condensed_coarse(di, H, parts, where, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr())
        return ptr, cols[:entries], vals[:entries], ncoarse

    def coarse_precond_factor(self, rowptr, colind, values, coarse, want_matrix=False):
        """pa_coarse_precond_query + pa_coarse_precond_factor on the table `coarse` = (p_ptr, p_cols, p_vals, ncoarse) -> dict(pt,
        factor, scratch, pivot, sizes, coarse, n [, matrix]): what coarse_precond_apply takes.  pivot > 0: the coarse matrix has its
        first non-positive pivot at pivot - 1."""
        ptr, cols, vals, ncoarse = coarse
        n = rowptr.numel() - 1
        sz = self.ctx.coarse_precond_query(n, ncoarse, ptr.data_ptr())
        pt = torch.zeros(max(sz.pt_bytes, 1), dtype=torch.uint8, device=self.device)       # (its parts are padded to 256 bytes)
        factor = torch.empty(max(sz.factor_doubles, 1), dtype=torch.float64, device=self.device)
        scratch = torch.empty(max(sz.scratch_bytes, 1), dtype=torch.uint8, device=self.device)
        matrix = torch.empty((ncoarse, ncoarse), dtype=torch.float64, device=self.device) if want_matrix else None
        pivot = self.ctx.coarse_precond_factor(n, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), ncoarse, ptr.data_ptr(),
                                               cols.data_ptr(), vals.data_ptr(), pt.data_ptr(), factor.data_ptr(), scratch.data_ptr(),
                                               _ptr(matrix))
        out = {"pt": pt, "factor": factor, "scratch": scratch, "pivot": pivot, "sizes": sz, "coarse": coarse, "n": n}
        if want_matrix:
            out["matrix"] = matrix
        return out

    def coarse_precond_apply(self, pre, r, z=None, accumulate=False):
        """z = (accumulate ? z : 0) + P (P^T A P)^-1 P^T r with what coarse_precond_factor returned"""
        ptr, cols, vals, ncoarse = pre["coarse"]
        if z is None:
            z = torch.zeros_like(r) if accumulate else torch.empty_like(r)
        self.ctx.coarse_precond_apply(pre["n"], ncoarse, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), pre["pt"].data_ptr(),
                                      pre["factor"].data_ptr(), pre["scratch"].data_ptr(), accumulate, r.data_ptr(), z.data_ptr())
        return z

    def conjugated_gradient_patch_coarse(self, rowptr, colind, values, b, patches, coarse, tol=1e-9, div=100.0, max_iter=1000, x=None):
        """solver_cg.hpp:63-144 with z = (patch sum) + (coarse term) -> (x, exit_reason, iterations, relative residual)"""
        ptr, rows = patches
        cptr, ccols, cvals, ncoarse = coarse
        if x is None:
            x = torch.empty_like(b)
        reason, iters, rr = self.ctx.conjugated_gradient_patch_coarse(
            b.numel(), rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), b.data_ptr(), x.data_ptr(), ptr.numel() - 1, ptr.data_ptr(),
            rows.data_ptr(), ncoarse, cptr.data_ptr(), ccols.data_ptr(), cvals.data_ptr(), tol, div, max_iter)
        return x, reason, iters, rr

    # ---- smoothed levels (multilevel_precond.hip) and the conjugate gradient with patches, smoothed levels and an exact level ----
    def smoothed_level_setup(self, rowptr, colind, values, coarse):
        """pa_smoothed_level_query + pa_smoothed_level_setup on the table `coarse` = (p_ptr, p_cols, p_vals, ncoarse) -> dict(pt,
        dinv, scratch, column, sizes, coarse, n): what smoothed_level_apply takes.  column > 0: d_j of column - 1 is not a positive
        finite number (dinv is then not written)."""
        ptr, cols, vals, ncoarse = coarse
        n = rowptr.numel() - 1
        sz = self.ctx.smoothed_level_query(n, ncoarse, ptr.data_ptr())
        pt = torch.zeros(max(sz.pt_bytes, 1), dtype=torch.uint8, device=self.device)       # (its parts are padded to 256 bytes)
        dinv = torch.zeros(max(sz.dinv_doubles, 1), dtype=torch.float64, device=self.device)
        scratch = torch.empty(max(sz.scratch_bytes, 1), dtype=torch.uint8, device=self.device)
        column = self.ctx.smoothed_level_setup(n, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), ncoarse, ptr.data_ptr(),
                                               cols.data_ptr(), vals.data_ptr(), pt.data_ptr(), dinv.data_ptr(), scratch.data_ptr())
        return {"pt": pt, "dinv": dinv[:ncoarse], "scratch": scratch, "column": column, "sizes": sz, "coarse": coarse, "n": n}

    def smoothed_level_apply(self, pre, r, z=None, accumulate=False):
        """z = (accumulate ? z : 0) + P diag(P^T A P)^-1 P^T r with what smoothed_level_setup returned"""
        ptr, cols, vals, ncoarse = pre["coarse"]
        if z is None:
            z = torch.zeros_like(r) if accumulate else torch.empty_like(r)
        self.ctx.smoothed_level_apply(pre["n"], ncoarse, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), pre["pt"].data_ptr(),
                                      pre["dinv"].data_ptr(), pre["scratch"].data_ptr(), accumulate, r.data_ptr(), z.data_ptr())
        return z

    def conjugated_gradient_multilevel(self, rowptr, colind, values, b, patches, levels, exact=None, tol=1e-9, div=100.0, max_iter=1000,
                                       x=None):
        """solver_cg.hpp:63-144 with z = (patch sum) + (the smoothed levels in their order) + (the exact level, if any); levels: a
        sequence of tables (p_ptr, p_cols, p_vals, ncoarse), exact: one or None -> (x, exit_reason, iterations, relative residual)"""
        ptr, rows = patches
        tup = lambda t: (t[3], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        if x is None:
            x = torch.empty_like(b)
        reason, iters, rr = self.ctx.conjugated_gradient_multilevel(
            b.numel(), rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), b.data_ptr(), x.data_ptr(), ptr.numel() - 1, ptr.data_ptr(),
            rows.data_ptr(), [tup(t) for t in levels], None if exact is None else tup(exact), tol, div, max_iter)
        return x, reason, iters, rr

    @staticmethod
    def _nested_levels(coarse_levels, coarse, patches):
        """the H of the smoothed levels as a list: each divides the next, the last divides `coarse`"""
        hs = [int(h) for h in coarse_levels]
        if patches is None:
            raise ValueError("coarse_levels needs patches")
        if len(hs) > capi.MULTILEVEL_MAX_LEVELS or any(h < 1 or h != g for h, g in zip(hs, coarse_levels)):
            raise ValueError("coarse_levels: up to %d integers >= 1" % capi.MULTILEVEL_MAX_LEVELS)
        for a, nxt in zip(hs, hs[1:] + ([int(coarse)] if coarse is not None else [])):
            if nxt % a:
                raise ValueError("coarse_levels: %d does not divide %d (the hat spaces must be nested)" % (a, nxt))
        return hs

    def _multilevel_solve(self, rowptr, colind, values, b, patches, hs, coarse, table, **kw):
        """conjugated_gradient_multilevel on the tables table(H) of hs and of coarse (None: no exact level); the context's table cap
        is raised for the smoothed levels' tables and put back"""
        cap = self.ctx.coarse_table_cap
        self.ctx.set_coarse_table_cap(capi.SMOOTHED_MAX_NODES)
        try:
            levels = [table(h) for h in hs]
        finally:
            self.ctx.set_coarse_table_cap(cap)
        exact = table(int(coarse)) if coarse is not None else None
        return self.conjugated_gradient_multilevel(rowptr, colind, values, b, patches, levels, exact, **kw)

    # ---- both levels on the row-partitioned system (rows_precond.hip): the tables of this context's slab ----
    def condensed_rows_patches(self, cd, fd, kind):
        """condensed_patches for the rows this context's slab owns (generate_mesh(.., rows=..); a whole mesh is the slab of all
        rows), the rows as global indices; a cell patch keeps the slab's own rows only -> (patch_ptr, patch_rows)"""
        di, _ = capi.degree_info(cd, fd)
        kind = {"face": capi.PATCH_FACE, "cell": capi.PATCH_CELL}.get(kind, kind)
        npatches, entries = self.ctx.condensed_rows_patches_query(di, kind)
        ptr = torch.empty(npatches + 1, dtype=torch.int64, device=self.device)
        rows = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        self.ctx.condensed_rows_patches(di, kind, ptr.data_ptr(), rows.data_ptr())
        return ptr, rows[:entries]

    def condensed_rows_coarse(self, cd, fd, H):
        """rows [row_begin, row_end) of condensed_coarse(cd, fd, H, "one") of the whole mesh for this context's slab: the same
        columns, p_ptr from 0 -> (p_ptr, p_cols, p_vals, ncoarse)"""
        di, _ = capi.degree_info(cd, fd)
        ncoarse, entries = self.ctx.condensed_rows_coarse_query(di, H, capi.COARSE_ONE)
        info = self.condensed_info(cd, fd)
        ptr = torch.empty(info.row_end - info.row_begin + 1, dtype=torch.int64, device=self.device)
        cols = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        vals = torch.empty(max(entries, 1), dtype=torch.float64, device=self.device)
        self.ctx.condensed_rows_coarse(di, H, capi.COARSE_ONE, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr())
        return ptr, cols[:entries], vals[:entries], ncoarse

    def conjugated_gradient_rows_patch_coarse(self, transport, row_begin, row_end, rowptr, colind, values, b, patches, coarse=None, tol=1e-9,
                                              div=100.0, max_iter=1000, x=None):
        """pa_conjugated_gradient_rows_patch_coarse on this rank's rows with its tables (condensed_rows_patches,
        condensed_rows_coarse or None) -> (x, exit_reason, iterations, relative residual)"""
        ptr, rows = patches
        cptr, ccols, cvals, ncoarse = coarse if coarse is not None else (None, None, None, 0)
        if x is None:
            x = torch.zeros_like(b)
        reason, iters, rr = self.ctx.conjugated_gradient_rows_patch_coarse(
            transport, row_begin, row_end, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), b.data_ptr(), x.data_ptr(),
            ptr.numel() - 1, ptr.data_ptr(), rows.data_ptr(), ncoarse, _ptr(cptr), _ptr(ccols), _ptr(cvals), tol, div, max_iter)
        return x, reason, iters, rr

    def condensed_solve(self, cd, fd, cond, g=None, tol=1e-9, div=100.0, max_iter=None, precond=True, patches=None, coarse=None,
                        coarse_levels=None):
        """the face-only system of the records `cond` (condensed_ops) assembled (condensed_csr_pattern / condensed_csr_fill) and
        solved: patches None = conjugated_gradient (precond: Jacobi), "face" / "cell" = conjugated_gradient_patch on that table;
        coarse = H (needs patches): conjugated_gradient_patch_coarse with the table condensed_coarse(H, "one") as well;
        coarse_levels = (H_0, H_1, ..) (needs patches; each divides the next, the last divides coarse): conjugated_gradient_multilevel
        with a smoothed level on each of these tables below the exact one (coarse = None: no exact level)
        -> (xF, exit_reason, iterations, relative residual).  Whole-mesh contexts."""
        if coarse is not None and patches is None:
            raise ValueError("coarse needs patches")
        hs = None if coarse_levels is None else self._nested_levels(coarse_levels, coarse, patches)
        rowptr, colind = self.condensed_csr_pattern(cd, fd)
        values, b = self.condensed_csr_fill(cd, fd, cond, g)
        if max_iter is None:
            max_iter = 4 * b.numel()
        if patches is None:
            return self.conjugated_gradient(rowptr, colind, values, b, tol=tol, div=div, max_iter=max_iter, precond=precond)
        if hs is not None:
            return self._multilevel_solve(rowptr, colind, values, b, self.condensed_patches(cd, fd, patches), hs, coarse,
                                          lambda H: self.condensed_coarse(cd, fd, H, "one"), tol=tol, div=div, max_iter=max_iter)
        if coarse is not None:
            return self.conjugated_gradient_patch_coarse(rowptr, colind, values, b, self.condensed_patches(cd, fd, patches),
                                                         self.condensed_coarse(cd, fd, int(coarse), "one"), tol=tol, div=div,
                                                         max_iter=max_iter)
        return self.conjugated_gradient_patch(rowptr, colind, values, b, self.condensed_patches(cd, fd, patches), tol=tol, div=div,
                                              max_iter=max_iter)

    def take_local_data(self, cd, fd, solution, g=None, first=0, n=None):
        """assembler::take_local_data (hho.hpp:408-449) for cells [first, first+n) -> n x msize."""
        di, _ = capi.degree_info(cd, fd)
        n = self.ncells - first if n is None else n
        ms = (cd + 1) * (cd + 2) // 2 + 4 * (fd + 1)
        out = torch.empty((n, ms), dtype=torch.float64, device=self.device)
        self.ctx.take_local_data(di, first, n, solution.data_ptr(), _ptr(g), out.data_ptr())
        return out

    def project_function(self, cd, fd, fn, quad=capi.QUAD_TENSOR, dinc=0, cell_fvals=None, face_fvals=None, first=0, n=None,
                         want_info=False):
        """project_function(msh, cl, hdi, f, di) (utils.hpp:199-227) -> n x msize [, info: n, the cell mass matrix's pivot flag]."""
        di, _ = capi.degree_info(cd, fd)
        n = self.ncells - first if n is None else n
        ms = (di.cell_deg + 1) * (di.cell_deg + 2) // 2 + 4 * (di.face_deg + 1)
        out = torch.empty((n, ms), dtype=torch.float64, device=self.device)
        info = torch.empty(n, dtype=torch.int32, device=self.device) if want_info else None
        self.ctx.project_function(di, quad, dinc, fn, _ptr(cell_fvals), _ptr(face_fvals), first, n, out.data_ptr(), _ptr(info))
        return (out, info) if want_info else out

    def energy_form(self, cd, fd, lc, u, v=None):
        """per-cell (u - v)^T lc (u - v)."""
        di, _ = capi.degree_info(cd, fd)
        out = torch.empty(lc.shape[0], dtype=torch.float64, device=self.device)
        self.ctx.energy_form(di, lc.shape[0], lc.data_ptr(), u.data_ptr(), _ptr(v), out.data_ptr())
        return out

    # ---- obstacle_assembler (hho.hpp:471-751) -------------------------------------------
    def obstacle_tables(self, in_A):
        """-> (A_ct, B_ct, num_I, num_A) for the uint8 flags in_A (hho.hpp:538-578)."""
        A_ct = torch.empty(self.ncells, dtype=torch.int32, device=self.device)
        B_ct = torch.empty(self.ncells, dtype=torch.int32, device=self.device)
        num_I, num_A = self.ctx.obstacle_tables(in_A.data_ptr(), A_ct.data_ptr(), B_ct.data_ptr())
        return A_ct, B_ct, num_I, num_A

    def obstacle_triplets(self, cd, fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I, first=0):
        """obstacle_assembler::assemble -> (rows, cols, vals) n x (msize^2 + 1), rhs_rows, rhs_vals n x msize."""
        di, _ = capi.degree_info(cd, fd)
        n, ms = lc.shape[0], lc.shape[1]
        rows = torch.empty((n, ms * ms + 1), dtype=torch.int32, device=self.device)
        cols = torch.empty((n, ms * ms + 1), dtype=torch.int32, device=self.device)
        vals = torch.empty((n, ms * ms + 1), dtype=torch.float64, device=self.device)
        rhs_rows = torch.empty((n, ms), dtype=torch.int32, device=self.device)
        rhs_vals = torch.empty((n, ms), dtype=torch.float64, device=self.device)
        self.ctx.obstacle_triplets(di, first, n, lc.data_ptr(), _ptr(rhs), _ptr(g), gamma.data_ptr(), in_A.data_ptr(),
                                   A_ct.data_ptr(), B_ct.data_ptr(), num_I, rows.data_ptr(), cols.data_ptr(),
                                   vals.data_ptr(), rhs_rows.data_ptr(), rhs_vals.data_ptr())
        return rows, cols, vals, rhs_rows, rhs_vals

    def obstacle_expand_solution(self, cd, fd, solution, g, gamma, in_A, A_ct, B_ct, num_I, nfaces):
        """obstacle_assembler::expand_solution -> (alpha, beta)."""
        di, _ = capi.degree_info(cd, fd)
        cbs = (cd + 1) * (cd + 2) // 2
        alpha = torch.empty(self.ncells * cbs + nfaces * (fd + 1), dtype=torch.float64, device=self.device)
        beta = torch.empty(self.ncells * cbs, dtype=torch.float64, device=self.device)
        self.ctx.obstacle_expand_solution(di, solution.data_ptr(), _ptr(g), gamma.data_ptr(), in_A.data_ptr(),
                                          A_ct.data_ptr(), B_ct.data_ptr(), num_I, alpha.data_ptr(), beta.data_ptr())
        return alpha, beta

    def obstacle_take_local_data(self, cd, fd, expanded, first=0, n=None):
        """free take_local_data(msh, cl, di, expanded_solution) (hho.hpp:753-782) -> n x msize."""
        di, _ = capi.degree_info(cd, fd)
        n = self.ncells - first if n is None else n
        ms = (cd + 1) * (cd + 2) // 2 + 4 * (fd + 1)
        out = torch.empty((n, ms), dtype=torch.float64, device=self.device)
        self.ctx.obstacle_take_local_data(di, first, n, expanded.data_ptr(), out.data_ptr())
        return out

    def obstacle_csr_assemble(self, fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I):
        """obstacle_assembler::assemble + finalize for cell degree 0, directly in CSR (pa_obstacle_csr_assemble): bit-identical to
        csr_from_triplets(obstacle_triplets(0, fd, ..)) -> (rowptr int64 [nrows+1], colind int32 [nnz], values [nnz], RHS [nrows])"""
        di = capi.DegreeInfo(0, fd, fd + 1)      # cell degree 0 as it is: degree_info(0, fd) reverts to equal order for fd > 1
        info = self.ctx.assembler_csr_query(di)
        rowptr = torch.empty(info.nrows + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(info.nnz, 1), dtype=torch.int32, device=self.device)
        values = torch.empty(max(info.nnz, 1), dtype=torch.float64, device=self.device)
        RHS = torch.empty(max(info.nrows, 1), dtype=torch.float64, device=self.device)
        nnz = self.ctx.obstacle_csr_assemble(di, lc.data_ptr(), _ptr(rhs), _ptr(g), gamma.data_ptr(), in_A.data_ptr(), A_ct.data_ptr(),
                                             B_ct.data_ptr(), num_I, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(),
                                             RHS.data_ptr())
        return rowptr, colind[:nnz], values[:nnz], RHS[:info.nrows]

    def obstacle_block_solve(self, fd, rowptr, colind, values, RHS, in_A, A_ct, B_ct, num_I, tol=1e-13, div=100.0, max_iter=None,
                             precond=True):
        """the solve of obstacle_csr_assemble's system (obstacle.cpp:170-175) in place: conjugated_gradient on the SPD block of the
        inactive cells and the faces through a row map, then the multipliers from the active cells' rows (pa_obstacle_block_solve)
        -> (x [nrows] in the layout obstacle_expand_solution reads, exit_reason, iterations, relative residual)"""
        di = capi.DegreeInfo(0, fd, fd + 1)
        nrows = rowptr.numel() - 1
        if max_iter is None:
            max_iter = 20 * (nrows - (self.ncells - num_I))
        x = torch.empty(max(nrows, 1), dtype=torch.float64, device=self.device)
        reason, iters, rr = self.ctx.obstacle_block_solve(di, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), RHS.data_ptr(),
                                                          in_A.data_ptr(), A_ct.data_ptr(), B_ct.data_ptr(), num_I, x.data_ptr(), tol, div,
                                                          max_iter, precond)
        return x[:nrows], reason, iters, rr

    def obstacle_active_set_update(self, fd, alpha, beta, gamma, c=1.0, alpha_prev=None, in_A_prev=None, in_A=None):
        """obstacle.cpp:133-142 and :193 in one pass (pa_obstacle_active_set_update): in_A = beta + c (alpha - gamma) < 0, unfused
        -> (in_A uint8 [ncells], num_A, cells whose flag differs from in_A_prev, || alpha_prev - alpha ||_2)"""
        di = capi.DegreeInfo(0, fd, fd + 1)
        if in_A is None:
            in_A = torch.empty(self.ncells, dtype=torch.uint8, device=self.device)
        num_A, changed, norm = self.ctx.obstacle_active_set_update(di, c, alpha.data_ptr(), beta.data_ptr(), gamma.data_ptr(),
                                                                   _ptr(alpha_prev), _ptr(in_A_prev), in_A.data_ptr())
        return in_A, num_A, changed, norm

    def obstacle_solve(self, fd, lc, rhs, g, gamma, c=1.0, max_outer=50, outer_tol=1e-7, tol=1e-13, div=100.0, cg_max_iter=0,
                       precond=True):
        """the primal-dual active set loop of obstacle.cpp:117-197 on the device (pa_obstacle_solve)
        -> dict(alpha [ncells + fbs nfaces], beta [ncells], in_A uint8 [ncells], info = capi.ObstacleSolveInfo, num_A = [per system],
        cg_iterations = [per system])"""
        di = capi.DegreeInfo(0, fd, fd + 1)
        nfaces = self.ctx.assembler_query(di).nfaces_local
        alpha = torch.empty(self.ncells + (fd + 1) * nfaces, dtype=torch.float64, device=self.device)
        beta = torch.empty(self.ncells, dtype=torch.float64, device=self.device)
        in_A = torch.empty(self.ncells, dtype=torch.uint8, device=self.device)
        params = capi.ObstacleSolveParams(c, max_outer, outer_tol, tol, div, cg_max_iter, precond)
        info, hist_a, hist_cg = self.ctx.obstacle_solve(di, lc.data_ptr(), _ptr(rhs), _ptr(g), gamma.data_ptr(), params, alpha.data_ptr(),
                                                        beta.data_ptr(), in_A.data_ptr())
        return {"alpha": alpha, "beta": beta, "in_A": in_A, "info": info, "num_A": hist_a, "cg_iterations": hist_cg}

    # ---- cutHHO fictitious domain (cuthho_square -f) ------------------------------------
    def cut_preprocess(self, N, radius=0.35, center=(0.5, 0.5), refsteps=4, rows=None, line_y=None, Ny=None, lo=(0.0, 0.0), hi=(1.0, 1.0),
                       agglomeration=False):
        """cuthho_square.cpp:2026-2052: the N x Ny mesh (Ny = None: N x N) of the box [lo, hi], circle level set (or, line_y given,
        line_level_set y - line_y, :91-124), default (-D) preprocessing or, agglomeration set, the `-A` branch
        (pa_cut_preprocess_agglomeration: no node displacement).  rows = (row_begin, row_end): the context keeps that slab of cell
        rows (pa_cut_preprocess_rows)."""
        self.level_set = capi.LevelSet(0, radius, center[0], center[1], 0.0) if line_y is None else capi.LevelSet(1, 0.0, 0.0, 0.0, line_y)
        self.Nx, self.Ny = int(N), int(N if Ny is None else Ny)
        self.lo, self.hi = (float(lo[0]), float(lo[1])), (float(hi[0]), float(hi[1]))
        if agglomeration:
            if rows is not None:
                raise ValueError("the agglomeration branch numbers the whole mesh: no row slab")
            self.ctx.cut_preprocess_agglomeration(self.Nx, self.Ny, self.level_set, refsteps, lo=self.lo, hi=self.hi)
        else:
            self.ctx.cut_preprocess(self.Nx, self.Ny, self.level_set, refsteps, lo=self.lo, hi=self.hi, rows=rows)
        self.ncut, self.cell_loc, self.cut_index = self.ctx.cut_query()
        return self.ncut

    def cut_local_ops(self, fd, where=capi.LOC_NEGATIVE, rhs_fn=capi.FN_SIN_SIN_RHS, bcs_fn=capi.FN_SIN_SIN_SOL,
                      want=("oper", "data", "stab", "lc", "rhs", "info")):
        cbs = (fd + 3) * (fd + 2) // 2
        ms = cbs + 4 * (fd + 1)
        n = self.ncut
        shapes = {"oper": (n, ms, cbs), "data": (n, ms, ms), "stab": (n, ms, ms), "lc": (n, ms, ms), "rhs": (n, cbs)}
        out = {}
        for k in want:
            out[k] = torch.empty(n, dtype=torch.int32, device=self.device) if k == "info" else \
                torch.empty(shapes[k], dtype=torch.float64, device=self.device)
        self.ctx.cut_local_ops(fd, self.level_set, where, rhs_fn, bcs_fn, _ptr(out.get("oper")), _ptr(out.get("data")),
                               _ptr(out.get("stab")), _ptr(out.get("lc")), _ptr(out.get("rhs")), _ptr(out.get("info")))
        return out

    def fictdom_local_ops(self, fd, where=capi.LOC_NEGATIVE, rhs_fn=capi.FN_SIN_SIN_RHS, bcs_fn=capi.FN_SIN_SIN_SOL,
                          overlap=False):
        """The whole loop body of cuthho_square.cpp:883-900 for every cell: uncut cells through the
        fan-quadrature / naive-stabilization kernel, cut cells through the cut kernel, merged.
        overlap: the cut cells' kernel first, on the context's side stream (pa_context_set_cut_overlap), next to
        the uncut cells' kernels.  -> (lc [n, ms, ms], rhs [n, cbs]) device tensors."""
        cd = fd + 1
        cut = None
        if overlap:
            self.ctx.set_cut_overlap(True)
            if self.ncut:
                cut = self.cut_local_ops(fd, where, rhs_fn, bcs_fn, want=("lc", "rhs"))
        out = self.local_ops(cd, fd, capi.QUAD_FAN, capi.STAB_NAIVE, want=("lc",))
        rhs = self.cell_rhs(cd, rhs_fn, capi.QUAD_FAN)
        if self.ncut:
            if cut is None:
                cut = self.cut_local_ops(fd, where, rhs_fn, bcs_fn, want=("lc", "rhs"))
            self.ctx.cut_merge(fd, where, cut["lc"].data_ptr(), cut["rhs"].data_ptr(), out["lc"].data_ptr(), rhs.data_ptr())
        else:
            self.ctx.cut_merge(fd, where, None, None, None, rhs.data_ptr())
        if overlap:
            self.ctx.set_cut_overlap(False)
        return out["lc"], rhs

    def fictdom_csr_scatter(self, fd, where=capi.LOC_NEGATIVE, rhs=None, g=None, cut_lc=None, cut_rhs=None, values=None, RHS=None,
                            want=()):
        """pa_fictdom_csr_assemble on caller tensors: rhs [ncells, cbs] (uncut cells; those outside `where` count as zero),
        cut_lc [ncut, msize, msize] / cut_rhs [ncut, cbs] (cut cells), g the boundary data -> dict(values [nnz], RHS [nrows]
        [, lc [ncells, msize, msize]] [, info [ncells]]) on the pattern of assembler_csr_pattern(fd + 1, fd)"""
        cd = fd + 1
        di, _ = capi.degree_info(cd, fd)
        ms = (cd + 1) * (cd + 2) // 2 + 4 * (fd + 1)
        info = self.ctx.assembler_csr_query(di)
        if values is None:
            values = torch.empty(max(info.nnz, 1), dtype=torch.float64, device=self.device)
        if RHS is None:
            RHS = torch.empty(max(info.nrows, 1), dtype=torch.float64, device=self.device)
        lc = torch.empty((self.ncells, ms, ms), dtype=torch.float64, device=self.device) if "lc" in want else None
        cinfo = torch.empty(self.ncells, dtype=torch.int32, device=self.device) if "info" in want else None
        self.ctx.fictdom_csr_assemble(fd, where, _ptr(rhs), _ptr(g), _ptr(cut_lc), _ptr(cut_rhs), values.data_ptr(), RHS.data_ptr(),
                                      _ptr(lc), _ptr(cinfo))
        out = {"values": values[:info.nnz], "RHS": RHS[:info.nrows]}
        if lc is not None:
            out["lc"] = lc
        if cinfo is not None:
            out["info"] = cinfo
        return out

    def fictdom_csr_assemble(self, fd, where=capi.LOC_NEGATIVE, rhs_fn=capi.FN_SIN_SIN_RHS, bcs_fn=capi.FN_SIN_SIN_SOL, g=None,
                             values=None, RHS=None, want=(), overlap=False):
        """The assembly loop of cuthho_square.cpp:881-905 without the [ncells, msize, msize] buffer: the uncut cells' right-hand
        sides (pa_cut_uncut_rhs_batch), the cut cells' operators (pa_cut_local_ops_batch; overlap: on the context's side stream)
        and pa_fictdom_csr_assemble -> fictdom_csr_scatter's dict, plus "rhs" [ncells, cbs] and "cut_lc" / "cut_rhs" (None
        without cut cells)"""
        cd = fd + 1
        cut = None
        if overlap:
            self.ctx.set_cut_overlap(True)
        try:
            if self.ncut:
                cut = self.cut_local_ops(fd, where, rhs_fn, bcs_fn, want=("lc", "rhs"))
            rhs = torch.empty((self.ncells, (cd + 1) * (cd + 2) // 2), dtype=torch.float64, device=self.device)
            self.ctx.cut_uncut_rhs(cd, where, rhs_fn, rhs.data_ptr())
            out = self.fictdom_csr_scatter(fd, where, rhs, g, None if cut is None else cut["lc"], None if cut is None else cut["rhs"],
                                           values, RHS, want)
        finally:
            if overlap:
                self.ctx.set_cut_overlap(False)
        out["rhs"] = rhs
        out["cut_lc"] = None if cut is None else cut["lc"]
        out["cut_rhs"] = None if cut is None else cut["rhs"]
        return out

    def fictdom_condensed_ops(self, fd, where=capi.LOC_NEGATIVE, rhs_fn=capi.FN_SIN_SIN_RHS, bcs_fn=capi.FN_SIN_SIN_SOL):
        """The same loop body in condensed mode: packed records [n, nf(nf+1)/2 + nf] of every cell of the context -- the fused
        pass with the uncut formulas (fan quadrature, naive stabilization), the cut cells' records from the stand-alone
        condensation of their cut operators (pa_static_condensation_packed_batch + pa_cut_merge_condensed).
        -> (records, rhs [n, cbs])."""
        cd = fd + 1
        di, _ = capi.degree_info(cd, fd)
        nf = 4 * (fd + 1)
        f64 = dict(dtype=torch.float64, device=self.device)
        rhs = torch.empty((self.ncells, (cd + 1) * (cd + 2) // 2), **f64)
        self.ctx.cut_uncut_rhs(cd, where, rhs_fn, rhs.data_ptr())
        cut = None
        if self.ncut:
            cut = self.cut_local_ops(fd, where, rhs_fn, bcs_fn, want=("lc", "rhs"))
            Sp = torch.empty((self.ncut, nf * (nf + 1) // 2), **f64)
            g = torch.empty((self.ncut, nf), **f64)
            self.ctx.static_condensation_packed(di, self.ncut, cut["lc"].data_ptr(), cut["rhs"].data_ptr(), Sp.data_ptr(), g.data_ptr(), None)
        self.ctx.cut_merge(fd, where, None, None if cut is None else cut["rhs"].data_ptr(), None, rhs.data_ptr())
        rec = self.condensed_ops(cd, fd, capi.QUAD_FAN, capi.STAB_NAIVE, rhs=rhs)
        if self.ncut:
            self.ctx.cut_merge_condensed(fd, Sp.data_ptr(), g.data_ptr(), rec.data_ptr())
        return rec, rhs

    def fictdom_condensed_records(self, fd, where=capi.LOC_NEGATIVE, rhs=None, cut_lc=None, cut_rhs=None, out=None):
        """pa_fictdom_condensed_ops_batch on caller tensors: rhs [ncells, cbs] (uncut cells; those outside `where` count as
        zero), cut_lc [ncut, msize, msize] / cut_rhs [ncut, cbs] (cut cells, eliminated in double-double)
        -> dict(cond [ncells, nf(nf+1)/2 + nf] in condensed_ops' layout, info [ncells], info_cut [ncut])"""
        nf = 4 * (fd + 1)
        if out is None:
            out = torch.empty((self.ncells, nf * (nf + 1) // 2 + nf), dtype=torch.float64, device=self.device)
        info = torch.empty(max(self.ncells, 1), dtype=torch.int32, device=self.device)
        info_cut = torch.empty(max(self.ncut, 1), dtype=torch.int32, device=self.device)
        self.ctx.fictdom_condensed_ops(fd, where, _ptr(rhs), _ptr(cut_lc), _ptr(cut_rhs), out.data_ptr(), info.data_ptr(),
                                       info_cut.data_ptr())
        return {"cond": out, "info": info[:self.ncells], "info_cut": info_cut[:self.ncut]}

    def fictdom_condensed_recover(self, fd, xF, where=capi.LOC_NEGATIVE, rhs=None, cut_lc=None, cut_rhs=None, g=None, full=None):
        """pa_fictdom_condensed_recover: u_T of every cell of the context from the face solution xF (Dirichlet faces: g)
        -> the full solution vector [cbs ncells_global + system_size], cells first (a slab fills its own cells)"""
        di, _ = capi.degree_info(fd + 1, fd)
        if full is None:
            full = torch.zeros(self.ctx.assembler_query(di).system_size, dtype=torch.float64, device=self.device)
        self.ctx.fictdom_condensed_recover(fd, where, _ptr(rhs), _ptr(cut_lc), _ptr(cut_rhs), _ptr(g), xF.data_ptr(), full.data_ptr())
        return full

    def fictdom_condensed_solve(self, fd, where=capi.LOC_NEGATIVE, rhs_fn=capi.FN_SIN_SIN_RHS, bcs_fn=capi.FN_SIN_SIN_SOL, tol=1e-13,
                                g=None, max_iter=None, precond=True, overlap=False, patches=None, coarse=None, coarse_levels=None,
                                coarse_parts="side"):
        """cuthho_square.cpp:881-919 and :959-962 on the face-only system: the operators (pa_cut_uncut_rhs_batch,
        pa_cut_local_ops_batch; overlap: on the context's side stream), the records, condensed_csr_pattern / condensed_csr_fill,
        conjugated_gradient and the recovery -> (full solution vector, iterations, exit reason).  g: the boundary data
        (default: dirichlet_data of bcs_fn).  patches "face" / "cell": conjugated_gradient_patch on that table of condensed_patches
        in place of conjugated_gradient; coarse = H (needs patches): conjugated_gradient_patch_coarse with the table
        condensed_coarse(H, "side") as well; coarse_levels = (H_0, H_1, ..) (needs patches; each divides the next, the last divides
        coarse): conjugated_gradient_multilevel with a smoothed level on each of these tables of condensed_coarse(H, coarse_parts)
        below the exact one (coarse = None: no exact level; coarse_parts is read with coarse_levels only).  Whole-mesh contexts."""
        cd = fd + 1
        if coarse is not None and patches is None:
            raise ValueError("coarse needs patches")
        hs = None if coarse_levels is None else self._nested_levels(coarse_levels, coarse, patches)
        if g is None:
            g = self.dirichlet_data(fd, bcs_fn)
        cut = None
        if overlap:
            self.ctx.set_cut_overlap(True)
        try:
            if self.ncut:
                cut = self.cut_local_ops(fd, where, rhs_fn, bcs_fn, want=("lc", "rhs"))
            rhs = torch.empty((self.ncells, (cd + 1) * (cd + 2) // 2), dtype=torch.float64, device=self.device)
            self.ctx.cut_uncut_rhs(cd, where, rhs_fn, rhs.data_ptr())
            cut_lc, cut_rhs = (None, None) if cut is None else (cut["lc"], cut["rhs"])
            rec = self.fictdom_condensed_records(fd, where, rhs, cut_lc, cut_rhs)
        finally:
            if overlap:
                self.ctx.set_cut_overlap(False)
        rowptr, colind = self.condensed_csr_pattern(cd, fd)
        values, b = self.condensed_csr_fill(cd, fd, rec["cond"], g)
        if max_iter is None:
            max_iter = 4 * b.numel()
        if patches is None:
            xF, reason, iters, _ = self.conjugated_gradient(rowptr, colind, values, b, tol=tol, max_iter=max_iter, precond=precond)
        elif hs is not None:
            xF, reason, iters, _ = self._multilevel_solve(rowptr, colind, values, b, self.condensed_patches(cd, fd, patches), hs, coarse,
                                                          lambda H: self.condensed_coarse(cd, fd, H, coarse_parts, where), tol=tol,
                                                          max_iter=max_iter)
        elif coarse is not None:
            xF, reason, iters, _ = self.conjugated_gradient_patch_coarse(rowptr, colind, values, b, self.condensed_patches(cd, fd, patches),
                                                                         self.condensed_coarse(cd, fd, int(coarse), "side", where), tol=tol,
                                                                         max_iter=max_iter)
        else:
            xF, reason, iters, _ = self.conjugated_gradient_patch(rowptr, colind, values, b, self.condensed_patches(cd, fd, patches), tol=tol,
                                                                  max_iter=max_iter)
        full = self.fictdom_condensed_recover(fd, xF, where, rhs, cut_lc, cut_rhs, g)
        return full, iters, reason

    # ---- cutHHO two-sided interface problem (cuthho_square -i) ------------------------------
    def interface_local_ops(self, fd, kappa=(1.0, 1.0), eta=5.0, rhs_fn=capi.FN_SIN_SIN_RHS, want_oper=False):
        """-> dict(lc, rhs: all cells, uncut formulas; lc_cut, rhs_cut [, oper_cut, data_cut]: cut cells)."""
        parms = capi.InterfaceParams(kappa[0], kappa[1], eta)
        cbs = (fd + 3) * (fd + 2) // 2
        ms = cbs + 4 * (fd + 1)
        n, nc = self.ncut, self.ncells
        f64 = dict(dtype=torch.float64, device=self.device)
        out = {"lc": torch.empty((nc, ms, ms), **f64), "rhs": torch.empty((nc, cbs), **f64),
               "lc_cut": torch.empty((n, 2 * ms, 2 * ms), **f64), "rhs_cut": torch.empty((n, 2 * cbs), **f64),
               "info_cut": torch.empty(n, dtype=torch.int32, device=self.device)}
        if want_oper:
            out["oper_cut"] = torch.empty((n, 2 * ms, 2 * cbs), **f64)
            out["data_cut"] = torch.empty((n, 2 * ms, 2 * ms), **f64)
        self.ctx.cut_interface_uncut(fd, parms, rhs_fn, out["lc"].data_ptr(), out["rhs"].data_ptr(), None)
        self.ctx.cut_interface_ops(fd, self.level_set, parms, rhs_fn, _ptr(out.get("oper_cut")), _ptr(out.get("data_cut")),
                                   out["lc_cut"].data_ptr(), out["rhs_cut"].data_ptr(), out["info_cut"].data_ptr())
        return out

    def interface_triplets(self, fd, ops, g=None):
        """interface_assembler::assemble / assemble_cut -> dict of device arrays."""
        cbs = (fd + 3) * (fd + 2) // 2
        ms = cbs + 4 * (fd + 1)
        n, nc = self.ncut, self.ncells
        i32 = dict(dtype=torch.int32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        t = {"rows": torch.empty((nc, ms * ms), **i32), "cols": torch.empty((nc, ms * ms), **i32), "vals": torch.empty((nc, ms * ms), **f64),
             "rows_cut": torch.empty((n, 4 * ms * ms), **i32), "cols_cut": torch.empty((n, 4 * ms * ms), **i32),
             "vals_cut": torch.empty((n, 4 * ms * ms), **f64),
             "rhs_rows": torch.empty((nc, ms), **i32), "rhs_vals": torch.empty((nc, ms), **f64),
             "rhs_rows_cut": torch.empty((n, 2 * ms), **i32), "rhs_vals_cut": torch.empty((n, 2 * ms), **f64)}
        self.ctx.interface_triplets(fd, ops["lc"].data_ptr(), ops["rhs"].data_ptr(), _ptr(g), ops["lc_cut"].data_ptr(),
                                    ops["rhs_cut"].data_ptr(), t["rows"].data_ptr(), t["cols"].data_ptr(), t["vals"].data_ptr(),
                                    t["rows_cut"].data_ptr(), t["cols_cut"].data_ptr(), t["vals_cut"].data_ptr(),
                                    t["rhs_rows"].data_ptr(), t["rhs_vals"].data_ptr(), t["rhs_rows_cut"].data_ptr(),
                                    t["rhs_vals_cut"].data_ptr())
        return t

    def interface_csr_pattern(self, fd):
        """interface_assembler's system directly in CSR, symbolic phase -> (rowptr int64 [nrows+1], colind int32 [nnz])"""
        info = self.ctx.interface_csr_query(fd)
        rowptr = torch.empty(info.nrows + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(info.nnz, 1), dtype=torch.int32, device=self.device)
        self.ctx.interface_csr_pattern(fd, rowptr.data_ptr(), colind.data_ptr())
        return rowptr, colind[:info.nnz]

    def interface_csr_fill(self, fd, ops, g=None, values=None, RHS=None):
        """numeric phase of the same from interface_local_ops' dict -> (values [nnz], RHS [nrows])"""
        info = self.ctx.interface_csr_query(fd)
        if values is None:
            values = torch.empty(max(info.nnz, 1), dtype=torch.float64, device=self.device)
        if RHS is None:
            RHS = torch.empty(max(info.nrows, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_csr_fill(fd, ops["lc"].data_ptr(), _ptr(ops.get("rhs")), _ptr(g), _ptr(ops.get("lc_cut")),
                                    _ptr(ops.get("rhs_cut")), values.data_ptr(), RHS.data_ptr())
        return values[:info.nnz], RHS[:info.nrows]

    def interface_condensed_ops(self, fd, ops):
        """static condensation of interface_local_ops' dict -> dict(cond [ncells * cond_doubles]: [S of every cell | g of every
        cell], cond_cut [ncut * cond_cut_doubles] the same for the cut cells (double-double), info, info_cut)"""
        qi = self.ctx.interface_condensed_query(fd)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        out = {"cond": torch.empty(max(self.ncells * qi.cond_doubles, 1), **f64),
               "cond_cut": torch.empty(max(self.ncut * qi.cond_cut_doubles, 1), **f64),
               "info": torch.empty(max(self.ncells, 1), **i32), "info_cut": torch.empty(max(self.ncut, 1), **i32)}
        self.ctx.interface_condensed_ops(fd, ops["lc"].data_ptr(), _ptr(ops.get("rhs")), _ptr(ops.get("lc_cut")), _ptr(ops.get("rhs_cut")),
                                         out["cond"].data_ptr(), out["cond_cut"].data_ptr(), out["info"].data_ptr(),
                                         out["info_cut"].data_ptr())
        out["cond"] = out["cond"][:self.ncells * qi.cond_doubles]
        out["cond_cut"] = out["cond_cut"][:self.ncut * qi.cond_cut_doubles]
        out["info"], out["info_cut"] = out["info"][:self.ncells], out["info_cut"][:self.ncut]
        return out

    def interface_condensed_triplets(self, fd, rec, g=None):
        """the records' assembly as triplets in the reference's push order -> dict of device arrays (as interface_triplets)"""
        nf, NF = 4 * (fd + 1), 8 * (fd + 1)
        n, nc = self.ncut, self.ncells
        i32 = dict(dtype=torch.int32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        t = {"rows": torch.empty((nc, nf * nf), **i32), "cols": torch.empty((nc, nf * nf), **i32), "vals": torch.empty((nc, nf * nf), **f64),
             "rows_cut": torch.empty((n, NF * NF), **i32), "cols_cut": torch.empty((n, NF * NF), **i32),
             "vals_cut": torch.empty((n, NF * NF), **f64),
             "rhs_rows": torch.empty((nc, nf), **i32), "rhs_vals": torch.empty((nc, nf), **f64),
             "rhs_rows_cut": torch.empty((n, NF), **i32), "rhs_vals_cut": torch.empty((n, NF), **f64)}
        self.ctx.interface_condensed_triplets(fd, rec["cond"].data_ptr(), rec["cond_cut"].data_ptr(), _ptr(g),
                                              *[t[k].data_ptr() for k in ("rows", "cols", "vals", "rows_cut", "cols_cut", "vals_cut",
                                                                          "rhs_rows", "rhs_vals", "rhs_rows_cut", "rhs_vals_cut")])
        return t

    def interface_condensed_csr_pattern(self, fd):
        """the face-only system directly in CSR, symbolic phase -> (rowptr int64 [nrows+1], colind int32 [nnz])"""
        qi = self.ctx.interface_condensed_query(fd)
        rowptr = torch.empty(qi.system_size + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(qi.nnz, 1), dtype=torch.int32, device=self.device)
        self.ctx.interface_condensed_csr_pattern(fd, rowptr.data_ptr(), colind.data_ptr())
        return rowptr, colind[:qi.nnz]

    def interface_condensed_csr_fill(self, fd, rec, g=None, values=None, RHS=None):
        """numeric phase of the same from interface_condensed_ops' dict -> (values [nnz], RHS [nrows])"""
        qi = self.ctx.interface_condensed_query(fd)
        if values is None:
            values = torch.empty(max(qi.nnz, 1), dtype=torch.float64, device=self.device)
        if RHS is None:
            RHS = torch.empty(max(qi.system_size, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_condensed_csr_fill(fd, rec["cond"].data_ptr(), _ptr(rec.get("cond_cut")), _ptr(g), values.data_ptr(),
                                              RHS.data_ptr())
        return values[:qi.nnz], RHS[:qi.system_size]

    def interface_condensed_recover(self, fd, ops, xF, g=None):
        """cell unknowns from the face-only solution -> the full solution vector in interface_assembler's numbering"""
        info = self.ctx.interface_info(fd)
        full = torch.empty(max(info.system_size, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_condensed_recover(fd, ops["lc"].data_ptr(), _ptr(ops.get("rhs")), _ptr(ops.get("lc_cut")),
                                             _ptr(ops.get("rhs_cut")), _ptr(g), xF.data_ptr(), full.data_ptr())
        return full[:info.system_size]

    def interface_condensed_patches(self, fd, kind):
        """the patch table of the face-only system of interface_condensed_csr_pattern: kind "face" (one patch per non-Dirichlet
        face: all rows of its one or two blocks) or "cell" (one per uncut cell and per side of a cut cell)
        -> (patch_ptr int64 [npatches + 1], patch_rows int32)"""
        kind = {"face": capi.PATCH_FACE, "cell": capi.PATCH_CELL}.get(kind, kind)
        npatches, entries = self.ctx.interface_condensed_patches_query(fd, kind)
        ptr = torch.empty(npatches + 1, dtype=torch.int64, device=self.device)
        rows = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        self.ctx.interface_condensed_patches(fd, kind, ptr.data_ptr(), rows.data_ptr())
        return ptr, rows[:entries]

    def interface_condensed_coarse(self, fd, H, parts="side"):
        """the coarse table of the face-only system of interface_condensed_csr_pattern: condensed_coarse's hats on every H-th mesh
        line, both blocks of a cut face with the face's values; parts "one", or "side" (an uncut face's block in the part of its
        side, a cut face's blocks one in each) -> (p_ptr int64 [rows + 1], p_cols int32, p_vals float64, ncoarse)"""
        parts = {"one": capi.COARSE_ONE, "side": capi.COARSE_BY_SIDE}.get(parts, parts)
        ncoarse, entries = self.ctx.interface_condensed_coarse_query(fd, H, parts)
        nrows = self.ctx.interface_condensed_query(fd).system_size
        ptr = torch.empty(nrows + 1, dtype=torch.int64, device=self.device)
        cols = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        vals = torch.empty(max(entries, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_condensed_coarse(fd, H, parts, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr())
        return ptr, cols[:entries], vals[:entries], ncoarse

    def interface_condensed_solve(self, fd, ops, g=None, tol=1e-9, div=100.0, max_iter=None, precond=True, patches=None, coarse=None,
                                  coarse_parts="side", coarse_levels=None):
        """cuthho_square.cpp:1664-1743 on the face-only system from interface_local_ops' dict: the records, the pattern, the fill,
        conjugated_gradient (precond: Jacobi) or, patches "face" / "cell", conjugated_gradient_patch on that table of
        interface_condensed_patches, and the recovery; coarse = H (needs patches): conjugated_gradient_patch_coarse with the table
        interface_condensed_coarse(H, coarse_parts) as well; coarse_levels = (H_0, H_1, ..) (needs patches; each divides the next,
        the last divides coarse): conjugated_gradient_multilevel with a smoothed level on each of these tables of
        interface_condensed_coarse(H, coarse_parts) below the exact one (coarse = None: no exact level)
        -> (full solution vector, iterations, exit reason)"""
        if coarse is not None and patches is None:
            raise ValueError("coarse needs patches")
        hs = None if coarse_levels is None else self._nested_levels(coarse_levels, coarse, patches)
        rec = self.interface_condensed_ops(fd, ops)
        rowptr, colind = self.interface_condensed_csr_pattern(fd)
        values, b = self.interface_condensed_csr_fill(fd, rec, g)
        if max_iter is None:
            max_iter = 20 * b.numel()
        if patches is None:
            xF, reason, iters, _ = self.conjugated_gradient(rowptr, colind, values, b, tol=tol, div=div, max_iter=max_iter, precond=precond)
        elif hs is not None:
            xF, reason, iters, _ = self._multilevel_solve(rowptr, colind, values, b, self.interface_condensed_patches(fd, patches), hs, coarse,
                                                          lambda H: self.interface_condensed_coarse(fd, H, coarse_parts), tol=tol, div=div,
                                                          max_iter=max_iter)
        elif coarse is not None:
            xF, reason, iters, _ = self.conjugated_gradient_patch_coarse(rowptr, colind, values, b, self.interface_condensed_patches(fd, patches),
                                                                         self.interface_condensed_coarse(fd, int(coarse), coarse_parts),
                                                                         tol=tol, div=div, max_iter=max_iter)
        else:
            xF, reason, iters, _ = self.conjugated_gradient_patch(rowptr, colind, values, b, self.interface_condensed_patches(fd, patches),
                                                                  tol=tol, div=div, max_iter=max_iter)
        return self.interface_condensed_recover(fd, ops, xF, g), iters, reason

    # ---- the same by row slabs: a context of cut_preprocess(rows=...), or the whole mesh as one slab ----
    def interface_rows_info(self, fd):
        """pa_interface_rows_query: the slab's owned rows, column window, cell blocks and halo sizes"""
        return self.ctx.interface_rows_query(fd)

    def interface_rows_ops(self, fd, ops):
        """interface_condensed_ops on the slab's cells (ops: interface_local_ops on the slab) -> the same dict"""
        qi = self.ctx.interface_rows_query(fd)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        out = {"cond": torch.empty(max(self.ncells * qi.cond_doubles, 1), **f64),
               "cond_cut": torch.empty(max(self.ncut * qi.cond_cut_doubles, 1), **f64),
               "info": torch.empty(max(self.ncells, 1), **i32), "info_cut": torch.empty(max(self.ncut, 1), **i32)}
        self.ctx.interface_rows_ops(fd, ops["lc"].data_ptr(), _ptr(ops.get("rhs")), _ptr(ops.get("lc_cut")), _ptr(ops.get("rhs_cut")),
                                    out["cond"].data_ptr(), out["cond_cut"].data_ptr(), out["info"].data_ptr(), out["info_cut"].data_ptr())
        out["cond"] = out["cond"][:self.ncells * qi.cond_doubles]
        out["cond_cut"] = out["cond_cut"][:self.ncut * qi.cond_cut_doubles]
        out["info"], out["info_cut"] = out["info"][:self.ncells], out["info_cut"][:self.ncut]
        return out

    def interface_rows_halo_pack(self, fd, rec, g=None, halo=None):
        """the top cell row's records and boundary values for the slab above -> [halo_send_doubles] (empty on the top slab)"""
        qi = self.ctx.interface_rows_query(fd)
        if halo is None:
            halo = torch.empty(max(qi.halo_send_doubles, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_rows_halo_pack(fd, rec["cond"].data_ptr(), _ptr(rec.get("cond_cut")), _ptr(g), halo.data_ptr())
        return halo[:qi.halo_send_doubles]

    def interface_rows_csr_pattern(self, fd):
        """the owned rows of the face-only system -> (rowptr int64 [nrows_owned+1] local, colind int32 [nnz_owned] global)"""
        qi = self.ctx.interface_rows_query(fd)
        rowptr = torch.empty(qi.row_end - qi.row_begin + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(max(qi.nnz_owned, 1), dtype=torch.int32, device=self.device)
        self.ctx.interface_rows_csr_pattern(fd, rowptr.data_ptr(), colind.data_ptr())
        return rowptr, colind[:qi.nnz_owned]

    def interface_rows_csr_fill(self, fd, rec, g=None, halo_below=None, values=None, RHS=None):
        """numeric phase of the same from interface_rows_ops' dict and the halo of the slab below -> (values [nnz_owned], RHS [nrows_owned])"""
        qi = self.ctx.interface_rows_query(fd)
        n = qi.row_end - qi.row_begin
        if values is None:
            values = torch.empty(max(qi.nnz_owned, 1), dtype=torch.float64, device=self.device)
        if RHS is None:
            RHS = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_rows_csr_fill(fd, rec["cond"].data_ptr(), _ptr(rec.get("cond_cut")), _ptr(g), _ptr(halo_below), values.data_ptr(),
                                         RHS.data_ptr())
        return values[:qi.nnz_owned], RHS[:n]

    def interface_rows_recover(self, fd, ops, xF, g=None):
        """the slab's cell unknowns from the face solution over [row_begin, col_end) -> [(cell_block_end - cell_block_begin) * cbs]"""
        qi = self.ctx.interface_rows_query(fd)
        n = (qi.cell_block_end - qi.cell_block_begin) * ((fd + 3) * (fd + 2) // 2)
        uT = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_rows_recover(fd, ops["lc"].data_ptr(), _ptr(ops.get("rhs")), _ptr(ops.get("lc_cut")), _ptr(ops.get("rhs_cut")),
                                        _ptr(g), xF.data_ptr(), uT.data_ptr())
        return uT[:n]

    def interface_rows_patches(self, fd, kind):
        """the slab's patch table for conjugated_gradient_rows_patch_coarse: kind "face" (the whole-mesh face patches of the owned
        rows) or "cell" (the patches of the slab's own cells and cell sides, rows outside the owned range deleted); rows are global
        -> (patch_ptr int64 [npatches + 1], patch_rows int32)"""
        kind = {"face": capi.PATCH_FACE, "cell": capi.PATCH_CELL}.get(kind, kind)
        npatches, entries = self.ctx.interface_rows_patches_query(fd, kind)
        ptr = torch.empty(npatches + 1, dtype=torch.int64, device=self.device)
        rows = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        self.ctx.interface_rows_patches(fd, kind, ptr.data_ptr(), rows.data_ptr())
        return ptr, rows[:entries]

    def interface_rows_coarse(self, fd, H, parts="side"):
        """the owned rows of interface_condensed_coarse's whole-mesh table, the same ncoarse and columns on every slab; parts "one"
        or "side" -> (p_ptr int64 [owned rows + 1] from 0, p_cols int32, p_vals float64, ncoarse)"""
        parts = {"one": capi.COARSE_ONE, "side": capi.COARSE_BY_SIDE}.get(parts, parts)
        ncoarse, entries = self.ctx.interface_rows_coarse_query(fd, H, parts)
        qi = self.ctx.interface_rows_query(fd)
        ptr = torch.empty(qi.row_end - qi.row_begin + 1, dtype=torch.int64, device=self.device)
        cols = torch.empty(max(entries, 1), dtype=torch.int32, device=self.device)
        vals = torch.empty(max(entries, 1), dtype=torch.float64, device=self.device)
        self.ctx.interface_rows_coarse(fd, H, parts, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr())
        return ptr, cols[:entries], vals[:entries], ncoarse

    def interface_cell_offsets(self, fd):
        out = torch.empty((self.ncells, 2), dtype=torch.int64, device=self.device)
        self.ctx.interface_cell_offsets(fd, out.data_ptr())
        return out

    def synchronize(self):
        self.ctx.synchronize()


def to_rowcol(t):
    """[n, cols, rows] device tensor of column-major matrices -> numpy [n, rows, cols]."""
    return t.detach().cpu().numpy().swapaxes(1, 2).copy()

