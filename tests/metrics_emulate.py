"""Torch / numpy emulation of the metric operators of morig_amd.native.NativeOps (csrc/metrics.hip), for the CPU tests of the HOST logic
of morig_amd/metrics.py: ptr handling, the invalid-mesh bookkeeping, the report, what is refused. Installed through ``runtime._test_ops``;
the arithmetic is tests/metrics_oracle.py. The contract of the kernels is kept: a mesh beyond the supported size gets its status word and
-1 / NaN pairs while the others are solved; a mesh with rows in a and none in b gets NaN and its flag."""
import numpy as np
import torch

import metrics_oracle as mo


class MetricOps:
    ASSIGN_MAX_SMALL, ASSIGN_MAX_LARGE, ASSIGN_ST_SIZE = 128, 256, 1

    def __init__(self):
        self.calls = []

    def bone_sample_counts(self, joints, bones):
        self.calls.append("bone_sample_counts")
        assert joints.dtype == torch.float64 and bones.dtype == torch.int32 and bones.shape[1] == 2
        j = joints.numpy()
        return torch.tensor([len(mo.sample_bone(j[p], j[c])) for p, c in bones.tolist()], dtype=torch.int64)

    def bone_samples(self, joints, bones, off, n_samples):
        self.calls.append("bone_samples")
        assert off.dtype == torch.int64 and off.numel() == bones.shape[0] + 1 and int(off[-1]) == n_samples
        j = joints.numpy()
        return torch.from_numpy(np.concatenate([mo.sample_bone(j[p], j[c]) for p, c in bones.tolist()], axis=0))

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
        return torch.tensor([float(np.mean(x[int(ptr[m]):int(ptr[m + 1])].numpy())) if int(ptr[m + 1]) > int(ptr[m]) else float("nan")
                             for m in range(ptr.numel() - 1)], dtype=torch.float64)

    def assign_joints(self, pred, pred_ptr, gt, gt_ptr, match_ptr, n_match, cost_off, n_cost):
        self.calls.append("assign_joints")
        nm = pred_ptr.numel() - 1
        assert cost_off.dtype == torch.int64 and int(cost_off[-1]) == n_cost and int(match_ptr[-1]) == n_match
        row, col = torch.full((n_match,), -1, dtype=torch.int32), torch.full((n_match,), -1, dtype=torch.int32)
        dist = torch.full((n_match,), float("nan"), dtype=torch.float64)
        status = torch.zeros(nm, dtype=torch.int32)
        for m in range(nm):
            p, g = pred[int(pred_ptr[m]):int(pred_ptr[m + 1])].numpy(), gt[int(gt_ptr[m]):int(gt_ptr[m + 1])].numpy()
            m0, m1 = int(match_ptr[m]), int(match_ptr[m + 1])
            assert m1 - m0 == min(len(p), len(g))
            if min(len(p), len(g)) > self.ASSIGN_MAX_SMALL or max(len(p), len(g)) > self.ASSIGN_MAX_LARGE:
                status[m] = self.ASSIGN_ST_SIZE
            elif m1 > m0:
                assert int(cost_off[m + 1]) - int(cost_off[m]) >= len(p) * len(g)
                r, c, d = mo.match(p, g)
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
