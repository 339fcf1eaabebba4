"""Torch emulation of the loss operators of morig_amd.native.NativeOps (csrc/losses.hip), for the CPU tests of the HOST logic of
morig_amd/losses.py: autograd wiring, batch-vector handling, the status word. Installed through ``runtime._test_ops``; the arithmetic is
tests/loss_oracle.py in float32. It keeps the contract of the kernels: wrong data sets status bits, indices are clamped, the loss is NaN."""
import torch

import loss_oracle as lo

ST_INDEX, ST_UNSORTED, ST_SEGMENT, ST_SIZE = 1, 2, 4, 8
FATAL = ST_UNSORTED | ST_SEGMENT


def _batch_of(ptr):
    return torch.repeat_interleave(torch.arange(ptr.numel() - 1), (ptr[1:] - ptr[:-1]).long())


class LossOps:
    NCE_WIDTH = 64
    CHAMFER_MAX_JOINTS = 1024

    def __init__(self):
        self.calls = []

    def loss_status(self, device):
        return torch.zeros(1, dtype=torch.int32, device=device)

    def segment_ptr(self, batch, n_segments, status):
        assert batch.dtype == torch.int64 and batch.dim() == 1
        if batch.numel() and bool(((batch < 0) | (batch >= n_segments)).any()):
            status |= ST_SEGMENT
        if batch.numel() > 1 and bool((batch[1:] < batch[:-1]).any()):
            status |= ST_UNSORTED
        if int(status) & FATAL:
            return torch.zeros(n_segments + 1, dtype=torch.int32)
        return torch.searchsorted(batch, torch.arange(n_segments + 1)).int()

    def gather_rows(self, src, idx, dst):
        dst.view().copy_(src.view()[idx.long()])

    # -- infoNCE
    def _nce_inputs(self, vtx, pts, corr_v2p, corr_p2v, ptrs, status):
        assert vtx.shape[1] == pts.shape[1] == self.NCE_WIDTH and corr_v2p.dtype == corr_p2v.dtype == torch.int64
        pv, pp, pcv, pcp = (p.long() for p in ptrs)
        out = []
        for corr, pc, pa, pk in ((corr_v2p, pcv, pv, pp), (corr_p2v, pcp, pp, pv)):
            cb = _batch_of(pc)
            na, nk = (pa[1:] - pa[:-1])[cb], (pk[1:] - pk[:-1])[cb]
            live = torch.ones_like(cb, dtype=torch.bool) if corr is corr_v2p else (pcv[1:] - pcv[:-1])[cb] > 0
            bad = ((corr[:, 0] < 0) | (corr[:, 0] >= na) | (corr[:, 1] < 0) | (corr[:, 1] >= nk)) & live
            if bool(bad.any()):
                status |= ST_INDEX
            c = torch.stack([torch.minimum(corr[:, 0].clamp(min=0), (na - 1).clamp(min=0)), torch.minimum(corr[:, 1].clamp(min=0), (nk - 1).clamp(min=0))], 1)
            out += [c, cb]
        return out[0], out[2], _batch_of(pv), _batch_of(pp), out[1], out[3]

    def infonce_forward(self, vtx, pts, corr_v2p, corr_p2v, ptrs, tau, status):
        self.calls.append("infonce_forward")
        rows = corr_v2p.shape[0] + corr_p2v.shape[0]
        if int(status) & FATAL:
            return torch.full((1,), float("nan")), torch.zeros(max(rows, 1))
        args = self._nce_inputs(vtx, pts, corr_v2p, corr_p2v, ptrs, status)
        loss = lo.infonce_loss(vtx, pts, *args, tau, ptrs[0].numel() - 1).reshape(1)
        return (torch.full((1,), float("nan")) if int(status) else loss), torch.zeros(max(rows, 1))

    def infonce_backward(self, vtx, pts, corr_v2p, corr_p2v, ptrs, tau, lse, upstream, groups, status):
        self.calls.append("infonce_backward")
        assert upstream.shape == (1,) and len(groups) == 4
        rp_v, ord_v, rp_p, ord_p = groups
        assert rp_v.numel() == vtx.shape[0] + 1 and ord_v.numel() == corr_v2p.shape[0] and int(rp_v[-1]) == corr_v2p.shape[0]
        assert rp_p.numel() == pts.shape[0] + 1 and ord_p.numel() == corr_p2v.shape[0] and int(rp_p[-1]) == corr_p2v.shape[0]
        if int(status):
            return torch.zeros_like(vtx), torch.zeros_like(pts)
        args = self._nce_inputs(vtx, pts, corr_v2p, corr_p2v, ptrs, status)
        _, gv, gp = lo.infonce(vtx, pts, *args, tau, ptrs[0].numel() - 1)
        return gv * upstream, gp * upstream

    # -- multi-positive
    def _multipos_ids(self, ids, S, status):
        if bool(((ids < 0) | (ids >= S)).any()):
            status |= ST_INDEX
        return ids.long().clamp(0, S - 1)

    def multipos_forward(self, F, pos_ids, neg_ids, n_meshes, n_sample, status):
        self.calls.append("multipos_forward")
        assert F.shape[0] == n_meshes * n_sample and F.shape[1] % 4 == 0 and F.shape[1] <= 128
        pos = self._multipos_ids(pos_ids, n_sample, status).reshape(n_meshes, n_sample, -1)
        neg = self._multipos_ids(neg_ids, n_sample, status).reshape(n_meshes, n_sample, -1)
        batch = torch.arange(n_meshes).repeat_interleave(n_sample)
        sid = torch.arange(n_sample).repeat(n_meshes, 1)
        loss = lo.multipos_loss(F, batch, sid, pos, neg, n_meshes).reshape(1)
        z = torch.zeros(F.shape[0])
        return (torch.full((1,), float("nan")) if int(status) else loss), z, z.clone()

    def multipos_backward(self, F, pos_ids, neg_ids, n_meshes, n_sample, neg_max, neg_sum, upstream, rows, n_total, status):
        self.calls.append("multipos_backward")
        pos = pos_ids.long().clamp(0, n_sample - 1).reshape(n_meshes, n_sample, -1)
        neg = neg_ids.long().clamp(0, n_sample - 1).reshape(n_meshes, n_sample, -1)
        batch = torch.arange(n_meshes).repeat_interleave(n_sample)
        sid = torch.arange(n_sample).repeat(n_meshes, 1)
        _, g = lo.multipos(F, batch, sid, pos, neg, n_meshes)
        grad = torch.zeros(n_total, F.shape[1])
        grad[rows.long()] = g * upstream
        return grad

    # -- chamfer
    def chamfer_forward(self, p, q, ptr_p, ptr_q, status):
        self.calls.append("chamfer_forward")
        B = ptr_p.numel() - 1
        nan = torch.full((1,), float("nan"))
        dummy = (torch.zeros(p.shape[0], dtype=torch.int32), torch.zeros(p.shape[0]), torch.zeros(q.shape[0], dtype=torch.int64))
        if int(status) & FATAL:
            return (nan,) + dummy
        if int((ptr_q[1:] - ptr_q[:-1]).max()) > self.CHAMFER_MAX_JOINTS:
            status |= ST_SIZE
            return (nan,) + dummy
        return (lo.chamfer_loss(p, _batch_of(ptr_p.long()), q, _batch_of(ptr_q.long()), B).reshape(1),) + dummy

    def chamfer_backward(self, p, q, ptr_p, ptr_q, arg1, d1, key2, upstream, status):
        self.calls.append("chamfer_backward")
        if int(status):
            return torch.zeros_like(p), torch.zeros_like(q)
        _, gp, gq = lo.chamfer(p, _batch_of(ptr_p.long()), q, _batch_of(ptr_q.long()), ptr_p.numel() - 1)
        return gp * upstream, gq * upstream
