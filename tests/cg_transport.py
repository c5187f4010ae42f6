"""The transport of pa_conjugated_gradient_rows for ranks that are threads of one process (tests/test_gpu_cg_rows.py,
tests/test_gpu_cg_twin.py)."""
import threading


class ThreadTransport:
    """pa_cg_transport for R ranks that are threads of this process: mailboxes and barriers instead of messages"""

    def __init__(self, R, fail_rank=None, fail_at=None):
        """fail_rank / fail_at: that rank's halo callback returns an error at its fail_at-th call (a one-sided failure)"""
        self.R = R
        self.fail_rank, self.fail_at, self.calls = fail_rank, fail_at, 0
        self.bar = threading.Barrier(R)
        self.vals = [None] * R
        self.need = [None] * R
        self.mail = {}

    def make(self, r, ctx):
        import torch
        from proton_amd import capi
        R, me = self.R, self

        def allreduce(user, vals, n):
            me.vals[r] = [vals[i] for i in range(n)]
            me.bar.wait()
            tot = [sum(me.vals[q][i] for q in range(R)) for i in range(n)]      # rank order: the same bits on every rank
            me.bar.wait()
            for i in range(n):
                vals[i] = tot[i]
            return 0

        def counts(user, need_lo, need_hi, give_lo, give_hi):
            me.need[r] = (need_lo, need_hi)
            me.bar.wait()
            give_lo[0] = me.need[r - 1][1] if r > 0 else 0          # rank - 1 reads above its range: my first entries
            give_hi[0] = me.need[r + 1][0] if r + 1 < R else 0      # rank + 1 reads below its range: my last entries
            me.bar.wait()
            return 0

        def d2h(ptr, n):
            t = torch.empty(n, dtype=torch.float64)
            ctx.copy_to_host(t.data_ptr(), ptr, 8 * n)
            return t

        def halo(user, send_lo, n_send_lo, send_hi, n_send_hi, recv_lo, n_recv_lo, recv_hi, n_recv_hi, stream):
            if r == me.fail_rank:
                me.calls += 1
                if me.calls == me.fail_at:
                    # this rank's exchange fails before it posts anything; like an asynchronous send / recv the neighbours'
                    # exchanges still return (their data is stale -- the solver must not use it: everybody leaves at the reduction)
                    me.bar.wait(); me.bar.wait()
                    return 1
            ctx.synchronize()
            if r > 0 and n_send_lo:
                me.mail[(r, r - 1)] = d2h(send_lo, n_send_lo)
            if r + 1 < R and n_send_hi:
                me.mail[(r, r + 1)] = d2h(send_hi, n_send_hi)
            me.bar.wait()
            if r > 0 and n_recv_lo:
                t = me.mail.get((r - 1, r))                 # (after a neighbour's failure: its previous message, or none yet)
                if t is not None:
                    assert t.numel() == n_recv_lo
                    ctx.copy_to_device(recv_lo, t.data_ptr(), 8 * n_recv_lo)
            if r + 1 < R and n_recv_hi:
                t = me.mail.get((r + 1, r))
                if t is not None:
                    assert t.numel() == n_recv_hi
                    ctx.copy_to_device(recv_hi, t.data_ptr(), 8 * n_recv_hi)
            me.bar.wait()
            return 0

        cbs = (capi.CG_ALLREDUCE(allreduce), capi.CG_HALO(halo), capi.CG_COUNTS(counts))
        return capi.CgTransport(None, *cbs), cbs
