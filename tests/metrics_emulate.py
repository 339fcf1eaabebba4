"""Torch / numpy emulation of the metric operators of morig_amd.native.NativeOps (csrc/metrics.hip), for the CPU tests of the HOST logic
of morig_amd/metrics.py: ptr handling, the invalid-mesh bookkeeping, the report, what is refused. Installed through ``runtime._test_ops``;
the arithmetic is tests/metrics_oracle.py. The contract of the kernels is kept: a mesh beyond the supported size gets its status word and
-1 / NaN pairs while the others are solved; a mesh with rows in a and none in b gets NaN and its flag; a NaN among a row's candidates
gives NaN (np.min); tables that do not describe a mesh give ASSIGN_ST_PTR with nothing of it written; non-finite joints follow
metrics_oracle.match_rule (ASSIGN_ST_INFEASIBLE when no finite assignment exists); a bone the kernel refuses counts 0."""
import numpy as np
import torch

import metrics_oracle as mo


class MetricOps:
    ASSIGN_MAX_SMALL, ASSIGN_MAX_LARGE, ASSIGN_ST_SIZE, ASSIGN_ST_PTR, ASSIGN_ST_INFEASIBLE = 128, 256, 1, 2, 4

    def __init__(self):
        self.calls = []

    def bone_sample_counts(self, joints, bones):
        self.calls.append("bone_sample_counts")
        assert joints.dtype == torch.float64 and bones.dtype == torch.int32 and bones.shape[1] == 2
        j = joints.numpy()
        return torch.tensor([self._count(j, p, c) for p, c in bones.tolist()], dtype=torch.int64)

    @staticmethod
    def _count(j, p, c):
        """the kernel's contract: 0 for a bone whose joints lie outside the array, hold a NaN, or give 2^24 steps or more"""
        if not (0 <= p < len(j) and 0 <= c < len(j)):
            return 0
        d = j[p] - j[c]
        with np.errstate(invalid="ignore", over="ignore"):
            steps = np.round(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / mo.STEP)
        return int(steps) + 1 if 0.0 <= steps < 16777216.0 else 0

    def bone_samples(self, joints, bones, off, n_samples):
        self.calls.append("bone_samples")
        assert off.dtype == torch.int64 and off.numel() == bones.shape[0] + 1 and int(off[-1]) == n_samples
        j = joints.numpy()
        parts = [mo.sample_bone(j[p], j[c]) for k, (p, c) in enumerate(bones.tolist()) if int(off[k + 1]) > int(off[k])]
        return torch.from_numpy(np.concatenate(parts, axis=0)) if parts else torch.zeros(0, 3, dtype=torch.float64)

    def nearest_distance(self, a, a_ptr, b, b_ptr, squared):
        self.calls.append("nearest_distance")
        assert a_ptr.dtype == b_ptr.dtype == torch.int32 and a_ptr.numel() == b_ptr.numel()
        out = torch.full((a.shape[0],), float("nan"), dtype=torch.float64)
        flags = torch.zeros(a_ptr.numel() - 1, dtype=torch.int32)
        for m in range(a_ptr.numel() - 1):
            s, e, q0, q1 = int(a_ptr[m]), int(a_ptr[m + 1]), int(b_ptr[m]), int(b_ptr[m + 1])
            if e > s and q1 <= q0:
                flags[m] = 1
            elif e > s:
                d = mo.nearest_sq(a[s:e].numpy(), b[q0:q1].numpy())
                out[s:e] = torch.from_numpy(d if squared else np.sqrt(d))
        return out, flags

    def segment_mean(self, x, ptr):
        self.calls.append("segment_mean")
        ok = lambda s, e: 0 <= s < e <= x.numel()                                                 # a segment that leaves x: no rows, NaN
        return torch.tensor([float(np.mean(x[int(ptr[m]):int(ptr[m + 1])].numpy())) if ok(int(ptr[m]), int(ptr[m + 1])) else float("nan")
                             for m in range(ptr.numel() - 1)], dtype=torch.float64)

    def assign_joints(self, pred, pred_ptr, gt, gt_ptr, match_ptr, n_match, cost_off, n_cost, out=None):
        """``out``: (row, col, dist, status) to write into, as the C entry point does -- a mesh with ASSIGN_ST_PTR leaves its part alone"""
        self.calls.append("assign_joints")
        nm = pred_ptr.numel() - 1
        if out is None:
            assert cost_off.dtype == torch.int64 and int(cost_off[-1]) == n_cost and int(match_ptr[-1]) == n_match
            out = (torch.full((n_match,), -1, dtype=torch.int32), torch.full((n_match,), -1, dtype=torch.int32),
                   torch.full((n_match,), float("nan"), dtype=torch.float64), torch.zeros(nm, dtype=torch.int32))
        row, col, dist, status = out
        for m in range(nm):
            p0, p1, g0, g1, m0, m1 = (int(t[m + k]) for t in (pred_ptr, gt_ptr, match_ptr) for k in (0, 1))
            if (p0 < 0 or p1 < p0 or p1 > pred.shape[0] or g0 < 0 or g1 < g0 or g1 > gt.shape[0] or m0 < 0 or m1 < m0 or m1 > n_match or
                    m1 - m0 != min(p1 - p0, g1 - g0)):
                status[m] = self.ASSIGN_ST_PTR
                continue
            p, g = pred[p0:p1].numpy(), gt[g0:g1].numpy()
            status[m] = 0
            if (min(len(p), len(g)) > self.ASSIGN_MAX_SMALL or max(len(p), len(g)) > self.ASSIGN_MAX_LARGE or int(cost_off[m]) < 0 or
                    int(cost_off[m + 1]) > n_cost or int(cost_off[m + 1]) - int(cost_off[m]) < len(p) * len(g)):
                status[m] = self.ASSIGN_ST_SIZE
                row[m0:m1], col[m0:m1], dist[m0:m1] = -1, -1, float("nan")
            elif m1 > m0:
                st, r, c, d = mo.match_rule(p, g)
                status[m] = st
                row[m0:m1], col[m0:m1], dist[m0:m1] = torch.from_numpy(r.astype(np.int32)), torch.from_numpy(c.astype(np.int32)), torch.from_numpy(d)
        return row, col, dist, status

    def joint_scores(self, row_ind, dist, match_ptr, pred_ptr, gt_ptr, fs, fs_ptr):
        self.calls.append("joint_scores")
        nm = match_ptr.numel() - 1
        hits, out = torch.zeros(nm, dtype=torch.int32), torch.zeros(3, nm, dtype=torch.float64)
        for m in range(nm):
            m0, m1, f0 = int(match_ptr[m]), int(match_ptr[m + 1]), int(fs_ptr[m])
            r = row_ind[m0:m1].long()
            ok = r >= 0
            h = int((dist[m0:m1][ok] < fs[f0 + r[ok]]).sum())
            n_p, n_g = np.float64(int(pred_ptr[m + 1]) - int(pred_ptr[m])), np.float64(int(gt_ptr[m + 1]) - int(gt_ptr[m]))
            hits[m] = h
            with np.errstate(divide="ignore", invalid="ignore"):
                out[0, m], out[1, m], out[2, m] = float(np.float64(2 * h) / (n_p + n_g)), float(np.float64(h) / n_p), float(np.float64(h) / n_g)
        return hits, out

    def valid_mean(self, x, valid):
        self.calls.append("valid_mean")
        assert x.dtype == torch.float64 and valid.dtype == torch.int32 and valid.numel() == x.shape[1]
        out = torch.zeros(x.shape[0], dtype=torch.float64)
        for r in range(x.shape[0]):
            s = 0.0
            for i in range(x.shape[1]):
                if int(valid[i]):
                    s += float(x[r, i])
            with np.errstate(divide="ignore", invalid="ignore"):
                out[r] = float(np.float64(s) / np.float64(int(valid.sum())))
        return out
