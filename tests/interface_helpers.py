"""What the tests of interface_assembler's system share (test_gpu_interface_csr.py: the full system; test_gpu_interface_condensed.py:
the face-only one): sizes, the local operators of a cut mesh, and the sorted triplet path both CSR gathers are pinned against."""
import numpy as np


def full_sizes(k):
    cbs = (k + 3) * (k + 2) // 2          # cell degree k + 1
    return cbs, cbs + 4 * (k + 1)


def condensed_sizes(k):
    cbs, fbs = full_sizes(k)[0], k + 1
    return cbs, fbs, 4 * fbs, 8 * fbs


def in_cell_order(asm, uncut, cut, per_cell):
    """[ncells, per_cell] uncut and [ncut, per_cut] cut slot arrays -> one flat array in the reference's push order: cells ascending,
    a cut cell's block in place of its (empty) uncut block"""
    import torch
    dev = asm.device
    nc = uncut.shape[0]
    ci = torch.from_numpy(np.asarray(asm.cut_index, dtype=np.int64)).to(dev)
    is_cut = ci >= 0
    per_cut = cut.shape[1] if cut.numel() else 0
    counts = torch.where(is_cut, per_cut, per_cell)
    base = torch.where(is_cut, nc * per_cell + ci.clamp(min=0) * per_cut, torch.arange(nc, device=dev) * per_cell)
    starts = torch.cumsum(counts, 0) - counts
    total = int(counts.sum())
    local = torch.arange(total, device=dev) - torch.repeat_interleave(starts, counts)
    src = torch.repeat_interleave(base, counts) + local
    return torch.cat([uncut.reshape(-1), cut.reshape(-1)])[src]


def sorted_path(asm, t, n, system_size):
    """the slots t of a triplet entry point (n unknowns per uncut cell) in cell order -> pa_csr_from_triplets; RHS = np.add.at of
    the per-row sums in cell order"""
    r = in_cell_order(asm, t["rows"], t["rows_cut"], n * n)
    c = in_cell_order(asm, t["cols"], t["cols_cut"], n * n)
    v = in_cell_order(asm, t["vals"], t["vals_cut"], n * n)
    rowptr, colind, values = asm.csr_from_triplets(r, c, v, system_size)
    rr = in_cell_order(asm, t["rhs_rows"], t["rhs_rows_cut"], n).cpu().numpy()
    rv = in_cell_order(asm, t["rhs_vals"], t["rhs_vals_cut"], n).cpu().numpy()
    RHS = np.zeros(system_size)
    keep = rr >= 0
    np.add.at(RHS, rr[keep], rv[keep])
    return rowptr, colind, values, RHS


def real_ops(asm, N, k, refsteps=4, **kw):
    """kw: BatchAssembler.cut_preprocess's further arguments (Ny, lo, hi, radius, center, line_y, rows)"""
    import proton_amd as pa
    asm.cut_preprocess(N, refsteps=refsteps, **kw)
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    return ops, g


def check_bit_identical(asm, sorted_csr, pattern, fill):
    """pattern() and fill() of a direct CSR against sorted_path's (rowptr, colind, values, RHS)"""
    import torch
    rowptr, colind, values, RHS = sorted_csr
    rp, ci = pattern()
    va, RH = fill()
    asm.synchronize()
    assert rp.numel() == rowptr.numel() and int(rp[-1]) == ci.numel() == colind.numel()
    assert torch.equal(rp, rowptr) and torch.equal(ci, colind)
    assert torch.equal(va, values)
    assert np.array_equal(RH.cpu().numpy(), RHS)
    return rp, ci, va, RH
