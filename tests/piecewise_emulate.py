"""NumPy emulation of the rig-free tracking operators of morig_amd.native.NativeOps (csrc/piecewise.hip), for the CPU tests of the HOST
logic of morig_amd/piecewise.py: the label renumbering, the handle CSR, the sample order, the slicing of the results, the error paths.
Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors; the arithmetic is that of
tests/piecewise_oracle.py."""
import numpy as np
import torch

import piecewise_oracle as po


class PiecewiseOps:
    RANSAC_SMALLEST_SUM, RANSAC_REFIT, RANSAC_NONE = 0, 1, 2
    KMEANS_OK, KMEANS_BAD_MESH, KMEANS_NO_CLUSTER = 0, 1, 2
    KMEANS_MAX_CLUSTERS, KMEANS_MAX_DIM = 64, 128

    def __init__(self):
        self.calls = []

    @staticmethod
    def _check(src, dst, handles, hptr, samples):
        assert src.dtype == dst.dtype == torch.float64 and src.shape == dst.shape and src.shape[1] == 3 and src.is_contiguous()
        assert handles.dtype == hptr.dtype == samples.dtype == torch.int32 and handles.dim() == 1 and hptr.dim() == 1
        P = hptr.numel() - 1
        assert samples.dim() == 3 and samples.shape[0] == P and samples.shape[2] == 3 and samples.is_contiguous()
        hp = hptr.numpy()
        assert hp[0] == 0 and hp[-1] == handles.numel() and np.all(np.diff(hp) >= po.MIN_HANDLES)
        h = handles.numpy()
        for p in range(P):                                                     # ascending vertex inside a problem
            assert np.all(np.diff(h[hp[p]:hp[p + 1]]) > 0)
        return P, samples.shape[1], h, hp

    def ransac_vote(self, src, dst, handles, hptr, samples, inlier_dist):
        self.calls.append("ransac_vote")
        P, n_iter, h, hp = self._check(src, dst, handles, hptr, samples)
        s, d, smp = src.numpy(), dst.numpy(), samples.numpy()
        count, dsum = np.zeros((P, n_iter), dtype=np.int32), np.zeros((P, n_iter))
        for p in range(P):
            rows = h[hp[p]:hp[p + 1]]
            for i in range(n_iter):
                R, t, _ = po.rigid_fit(s[rows][smp[p, i]], d[rows][smp[p, i]])
                dist = np.sqrt(np.sum((s[rows] @ R.T + t - d[rows]) ** 2, axis=1))
                count[p, i], dsum[p, i] = np.sum(dist < inlier_dist), dist.sum()
        return torch.from_numpy(count), torch.from_numpy(dsum)

    def ransac_fit(self, src, dst, handles, hptr, samples, count, dsum, inlier_dist, refit_share):
        self.calls.append("ransac_fit")
        P, n_iter, h, hp = self._check(src, dst, handles, hptr, samples)
        assert count.dtype == torch.int32 and dsum.dtype == torch.float64 and count.shape == dsum.shape == (P, n_iter)
        s, d, smp = src.numpy(), dst.numpy(), samples.numpy()
        chosen, best = np.zeros((P, 2), dtype=np.int32), np.zeros(P, dtype=np.int32)
        flag, Rt = np.zeros(P, dtype=np.int32), np.zeros((P, 12))
        for p in range(P):
            rows = h[hp[p]:hp[p + 1]]
            by_count, by_sum, top = po.select(count[p].numpy(), dsum[p].numpy())
            chosen[p], best[p] = (by_count, by_sum), top
            refit = by_count >= 0 and top > refit_share * len(rows)
            use = by_count if refit else by_sum
            if use < 0:
                flag[p], Rt[p, :9] = self.RANSAC_NONE, np.eye(3).reshape(-1)
                continue
            R, t, _ = po.rigid_fit(s[rows][smp[p, use]], d[rows][smp[p, use]])
            if refit:
                inl = np.sqrt(np.sum((s[rows] @ R.T + t - d[rows]) ** 2, axis=1)) < inlier_dist
                R, t, _ = po.rigid_fit(s[rows][inl], d[rows][inl])
            flag[p] = self.RANSAC_REFIT if refit else self.RANSAC_SMALLEST_SUM
            Rt[p, :9], Rt[p, 9:] = R.reshape(-1), t
        return torch.from_numpy(chosen), torch.from_numpy(best), torch.from_numpy(flag), torch.from_numpy(Rt)

    def ransac_apply(self, src, dst, problem_of, flag, Rt):
        self.calls.append("ransac_apply")
        assert problem_of.dtype == torch.int32 and problem_of.shape == (src.shape[0],) and Rt.shape == (flag.numel(), 12)
        s, d, po_, f, rt = src.numpy(), dst.numpy(), problem_of.numpy(), flag.numpy(), Rt.numpy()
        out = np.zeros_like(s)
        for v in range(len(s)):
            p = po_[v]
            if p < 0 or p >= len(f):
                out[v] = d[v]
            elif f[p] == self.RANSAC_NONE:
                out[v] = s[v]
            else:
                out[v] = s[v] @ rt[p, :9].reshape(3, 3).T + rt[p, 9:]
        return torch.from_numpy(out)

    def kernel_kmeans(self, X, pos, vptr, first, n_clusters, max_iter, w_euc, tol):
        self.calls.append("kernel_kmeans")
        assert X.dtype in (torch.float32, torch.float64) and X.is_contiguous() and pos.dtype == torch.float64 and pos.shape == (X.shape[0], 3)
        assert vptr.dtype == first.dtype == torch.int32 and first.numel() == vptr.numel() - 1
        if n_clusters > self.KMEANS_MAX_CLUSTERS or X.shape[1] > self.KMEANS_MAX_DIM:
            from morig_amd.abi import MorigNativeError
            raise MorigNativeError("morig_kernel_kmeans: unsupported width / shape")
        B, K, D = first.numel(), n_clusters, X.shape[1]
        vp = vptr.numpy()
        labels = np.full(X.shape[0], -1, dtype=np.int64)
        seeds, info, members = np.zeros((B, K), dtype=np.int32), np.zeros((B, 4), dtype=np.int32), np.zeros((B, K), dtype=np.int32)
        cemb, ceuc, fit = np.zeros((B, K, D)), np.zeros((B, K, 3)), np.zeros(B)
        for b in range(B):
            x, v = X.numpy()[vp[b]:vp[b + 1]], pos.numpy()[vp[b]:vp[b + 1]]
            lab, st = po.kernel_kmeans(x, v, K, max_iter, w_euc, tol, int(first[b]))
            if st["n_kept"] == 0:                                              # no cluster kept: the status, labels of -1
                info[b, 0] = self.KMEANS_NO_CLUSTER
                continue
            labels[vp[b]:vp[b + 1]] = lab
            seeds[b], members[b], cemb[b], ceuc[b], fit[b] = st["seeds"], st["members"], st["centres_emb"], st["centres_euc"], st["fit"]
            info[b] = (self.KMEANS_OK, st["n_iter"], st["n_kept"], 0)
        t = torch.from_numpy
        return dict(labels=t(labels), seeds=t(seeds), info=t(info), members=t(members), centres_emb=t(cemb), centres_euc=t(ceuc), fit=t(fit))
