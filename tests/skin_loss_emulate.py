"""Torch emulation of the skin-loss operators of morig_amd.native.NativeOps (csrc/losses_skin.hip), for the CPU tests of the HOST logic
of morig_amd/losses.py. The arithmetic is tests/skin_loss_oracle.py in float32; the contract of the kernels is kept: a sample outside its
mesh or repeated inside it sets the status bit and is clamped, the loss is NaN, the gradient of such a call stays zero."""
import torch

import skin_loss_oracle as so
from loss_emulate import FATAL, ST_INDEX, LossOps


class SkinLossOps(LossOps):
    def _sets(self, feat_all, feat_aggr):
        sets = [] if feat_all is None else [feat_all[:, t, :] for t in range(feat_all.shape[1])]
        return sets + ([] if feat_aggr is None else [feat_aggr])

    def _samples(self, ptr, samples, status):
        assert samples.dtype == torch.int32 and samples.dim() == 3 and samples.shape[1] == ptr.numel() - 1
        counts = (ptr[1:] - ptr[:-1]).long()[None, :, None]
        s = samples.long()
        live = (counts > 0).expand_as(s)                    # a mesh without vertices is skipped, its ids are not looked at
        bad = bool((((s < 0) | (s >= counts)) & live).any())
        s = torch.minimum(s.clamp(min=0), (counts - 1).clamp(min=0))
        srt = torch.sort(s, dim=2).values
        if bad or bool(((srt[:, :, 1:] == srt[:, :, :-1]) & live[:, :, 1:]).any()):
            status |= ST_INDEX
        return s

    @staticmethod
    def _meshes(ptr):
        return [(b, int(ptr[b])) for b in range(ptr.numel() - 1) if int(ptr[b + 1]) > int(ptr[b])]

    def logratio_forward(self, feat_all, feat_aggr, gt, ptr, samples, status):
        self.calls.append("logratio_forward")
        sets = self._sets(feat_all, feat_aggr)
        B, S = ptr.numel() - 1, samples.shape[2]
        assert len(sets) == samples.shape[0] and 3 <= S <= 64 and all(f.shape[1] % 4 == 0 and f.stride(1) == 1 for f in sets)
        tab = torch.zeros(len(sets), B, 2, S, S)
        nan = torch.full((1,), float("nan"))
        if int(status) & FATAL:
            return nan, tab
        s = self._samples(ptr, samples, status)
        if int(status):
            return nan, tab
        total = torch.zeros((), dtype=torch.float64)
        for k, f in enumerate(sets):
            per_set = torch.zeros((), dtype=torch.float64)
            for b, v0 in self._meshes(ptr):
                per_set = per_set + so.logratio_mesh_loss(f[v0 + s[k, b]], gt[v0 + s[k, b]]).double()
            total = total + per_set / B
        return total.float().reshape(1), tab

    def logratio_backward(self, feat_all, feat_aggr, gt, ptr, samples, tab, upstream, status):
        self.calls.append("logratio_backward")
        assert upstream.shape == (1,) and tab.shape[0] == samples.shape[0]
        sets = self._sets(feat_all, feat_aggr)
        B = ptr.numel() - 1
        grads = [torch.zeros(f.shape) for f in sets]
        if not int(status):
            for k, f in enumerate(sets):
                for b, v0 in self._meshes(ptr):
                    rows = v0 + samples[k, b].long()
                    grads[k][rows] = so.logratio_mesh(f[rows], gt[rows])[1] * (upstream / B)
        g_all = None if feat_all is None else torch.stack(grads[:feat_all.shape[1]], dim=1)
        return g_all, (None if feat_aggr is None else grads[-1])

    def skin_ce_forward(self, x, label, mask, K):
        self.calls.append("skin_ce_forward")
        assert 1 <= K <= 8 and x.shape[1] >= K and label.dtype == mask.dtype == torch.float32
        loss = so.skin_ce_loss(x[:, :K], label, mask, K)
        vm = torch.from_numpy(so.vert_mask_sequential(label.numpy(), mask.numpy(), K)).float()
        w = mask[:, :K] * vm[:, None]
        return loss.reshape(1), vm, torch.stack([loss.double() * w.sum().double(), w.sum().double()])

    def skin_ce_backward(self, x, label, mask, K, sums, upstream):
        self.calls.append("skin_ce_backward")
        assert sums.dtype == torch.float64 and upstream.shape == (1,)
        return so.skin_ce(x[:, :K], label, mask, K)[1] * upstream

    def ce_probs_forward(self, x, target, weight, reduction):
        self.calls.append("ce_probs_forward")
        assert x.shape == target.shape and (weight is None or weight.shape == x.shape) and x.shape[1] <= 128
        value = so.ce_probs(x, target, weight, reduction)[0]
        return value if reduction == "none" else value.reshape(1)

    def ce_probs_backward(self, x, target, weight, reduction, upstream):
        self.calls.append("ce_probs_backward")
        assert upstream.shape == (x.shape if reduction == "none" else (1,))
        return so.ce_probs(x, target, weight, reduction, upstream if reduction == "none" else upstream[0])[1]
