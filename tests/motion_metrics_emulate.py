"""Numpy emulation of the operators morig_amd/motion_metrics.py calls on morig_amd.native.NativeOps, for the CPU tests of its HOST logic:
ragged packing, the status word, the refusals, ratios and means. Installed through ``runtime._test_ops``. The two operators of
csrc/motion_metrics.hip (corr_hits, pr_counts) keep the contract of the kernels -- a row with an index outside its pair counts nothing and
sets MOTION_ST_INDEX, a bad batch vector leaves every count 0 -- with the arithmetic of tests/motion_metrics_oracle.py; segment_ptr,
cosine_nn and pose_traj_errors stand in for the existing kernels they name."""
import numpy as np
import torch

import motion_metrics_oracle as mo
import playback_oracle as po

ST_UNSORTED, ST_SEGMENT, MOTION_ST_INDEX = 2, 4, 16
FATAL = ST_UNSORTED | ST_SEGMENT


class MotionOps:
    CURVE_MAX_BINS = 32

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

    def cosine_nn(self, v, ptr_v, p, ptr_p, n_clouds, max_rows_per_cloud):
        """the float64 arg-max per pair, as rows of the point array (the tests' features are separated by far more than the kernel's error)"""
        self.calls.append("cosine_nn")
        vf, pf = v.view().numpy().astype(np.float64), p.view().numpy().astype(np.float64)
        assert vf.shape[1] == pf.shape[1] == 64 and ptr_v.numel() == ptr_p.numel() == n_clouds + 1 and max_rows_per_cloud >= 1
        nn, sim = np.full(len(vf), -1, dtype=np.int32), np.zeros(len(vf), dtype=np.float32)
        for b in range(n_clouds):
            v0, v1, p0, p1 = int(ptr_v[b]), int(ptr_v[b + 1]), int(ptr_p[b]), int(ptr_p[b + 1])
            if v1 > v0 and p1 > p0:
                s = vf[v0:v1] @ pf[p0:p1].T
                nn[v0:v1], sim[v0:v1] = p0 + s.argmax(axis=1), s.max(axis=1)
        return torch.from_numpy(nn), torch.from_numpy(sim)

    def corr_hits(self, pts, ptr_pts, nn, ptr_vtx, nn_global, corr, ptr_corr, tol, status):
        self.calls.append("corr_hits")
        assert pts.dtype == torch.float32 and nn.dtype == torch.int32 and corr.dtype == torch.int64 and tol.dtype == torch.float32
        assert 1 <= tol.numel() <= self.CURVE_MAX_BINS
        B = ptr_corr.numel() - 1
        hits = torch.zeros(B, tol.numel(), dtype=torch.int64)
        if int(status) & FATAL:
            return hits
        for b in range(B):
            p0, p1, v0, v1 = int(ptr_pts[b]), int(ptr_pts[b + 1]), int(ptr_vtx[b]), int(ptr_vtx[b + 1])
            rows = corr[int(ptr_corr[b]):int(ptr_corr[b + 1])].numpy()
            local = nn[v0:v1].numpy().astype(np.int64) - (p0 if nn_global else 0)
            ok = (rows[:, 0] >= 0) & (rows[:, 0] < v1 - v0) & (rows[:, 1] >= 0) & (rows[:, 1] < p1 - p0)
            ok[ok] &= (local[rows[ok, 0]] >= 0) & (local[rows[ok, 0]] < p1 - p0)
            if not ok.all():
                status |= MOTION_ST_INDEX
            if ok.any():
                hits[b] = torch.from_numpy(mo.corr_hits(pts[p0:p1].numpy(), local, rows[ok], tol.numpy()))
        return hits

    def pr_counts(self, pred, gt, ptr, thr, normalize, status):
        self.calls.append("pr_counts")
        assert pred.dtype == torch.float32 and gt.dtype == torch.uint8 and thr.dtype == torch.float32 and 1 <= thr.numel() <= self.CURVE_MAX_BINS
        B = ptr.numel() - 1
        tp, pp = torch.zeros(B, thr.numel(), dtype=torch.int64), torch.zeros(B, thr.numel(), dtype=torch.int64)
        gp = torch.zeros(B, dtype=torch.int64)
        if int(status) & FATAL:
            return tp, pp, gp
        for b in range(B):
            s, e = int(ptr[b]), int(ptr[b + 1])
            if e > s:
                t, p, g = mo.pr_counts(pred[s:e].numpy(), gt[s:e].numpy(), thr.numpy(), normalize)
                tp[b], pp[b], gp[b] = torch.from_numpy(t), torch.from_numpy(p), g
        return tp, pp, gp

    def pose_traj_errors(self, pred, gt, vis, vptr):
        self.calls.append("pose_traj_errors")
        assert pred.dtype == gt.dtype == torch.float64 and vis.dtype == torch.uint8 and pred.shape == gt.shape and tuple(vis.shape) == tuple(pred.shape[:2])
        B, T = vptr.numel() - 1, pred.shape[1]
        full, visible = np.zeros((B, T)), np.zeros((B, T))
        for b in range(B):
            rows = slice(int(vptr[b]), int(vptr[b + 1]))
            full[b], visible[b] = po.trajectory_errors(pred.numpy()[rows], gt.numpy()[rows], vis.numpy()[rows])
        return torch.from_numpy(full), torch.from_numpy(visible)
