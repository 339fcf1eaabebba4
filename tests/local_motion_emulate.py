"""NumPy emulation of the local-motion operators of morig_amd.native.NativeOps (csrc/local_motion.hip), for the CPU tests of the HOST
logic of morig_amd/local_motion.py: the ragged tables, the sorted one-ring keys and their row pointer, the two passes around the scan,
the status words and the refusals. Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on
CPU tensors: the candidates are the end points of the walks of exactly four edges over the one-ring it decodes from the keys the host
sorted, the arithmetic is that of tests/local_motion_oracle.py. ``transfer_keys`` is the emulation of tests/transfer_emulate.py."""
import numpy as np
import torch

import local_motion_oracle as lo
from transfer_emulate import NO_KEY, TransferOps


class LocalOps(TransferOps):
    LOCAL_MAX_VERTS, LOCAL_BAD_FACE, LOCAL_BAD_COORD, LOCAL_BAD_ID = 32768, 1, 2, 4

    def _members(self, verts, vptr, rowptr, keys, rungs):
        vp, v, rp, k = self._ptr(vptr), self._f64(verts, 3), self._ptr(rowptr), keys.numpy()
        assert keys.dtype == torch.int64 and np.all(np.diff(k) >= 0) and len(rp) == len(v) + 1                       # sorted
        assert np.array_equal(rp, np.searchsorted(k, np.arange(len(v) + 1, dtype=np.int64) << 32)) and np.all(k[rp[-1]:] == NO_KEY)
        assert tuple(rungs) == lo.RUNGS
        lists, rung, lone = [], np.zeros(len(v), dtype=np.int32), 0
        for b in range(len(vp) - 1):
            v0, nv = vp[b], vp[b + 1] - vp[b]
            ring = [np.unique(k[rp[v0 + i]:rp[v0 + i + 1]] & 0xffffffff) for i in range(nv)]
            for i in range(nv):
                walk = {i}
                for _ in range(4):
                    walk = {int(u) for w in walk for u in ring[w]}
                if len(ring[i]) == 0:
                    walk, lone = {i}, lone + 1
                cand = np.array(sorted(walk), dtype=np.int64)
                d = lo.dist_row(v[v0 + i], v[v0 + cand])
                c = [int(np.count_nonzero(d < r)) for r in rungs]
                r = 0 if c[0] >= 5 else (1 if c[1] >= 5 else 2)
                lists.append(cand[d < rungs[r]])
                rung[v0 + i] = r
        return lists, rung, lone, bool(len(v)) and not np.isfinite(v).all()

    def local_patches(self, verts, vptr, max_verts, rowptr, keys, rungs, status, ptr=None, rung=None, n_ids=0):
        self.calls.append("local_patches")
        assert status.dtype == torch.int32 and status.numel() == 3 and max_verts == np.diff(self._ptr(vptr)).max() <= self.LOCAL_MAX_VERTS
        lists, rungs_used, lone, bad = self._members(verts, vptr, rowptr, keys, rungs)
        if ptr is None:
            status[1] += lone
            if bad:
                status[0] |= self.LOCAL_BAD_COORD
            return torch.from_numpy(np.array([len(r) for r in lists], dtype=np.int32)), torch.from_numpy(rungs_used)
        want_ptr, ids = lo.flat(lists)
        assert np.array_equal(self._ptr(ptr), want_ptr) and n_ids == want_ptr[-1] and np.array_equal(rung.numpy(), rungs_used)
        return torch.from_numpy(ids)

    def local_fit(self, verts0, traj, vptr, patch_ptr, ids, status):
        self.calls.append("local_fit")
        vp, v, pp = self._ptr(vptr), self._f64(verts0, 3), self._ptr(patch_ptr)
        assert traj.dtype in (torch.float64, torch.float32) and traj.dim() == 3 and traj.shape[0] == len(v) and traj.shape[2] == 3 and traj.is_contiguous()
        assert ids.dtype == torch.int32 and pp[-1] == ids.numel() and len(pp) == len(v) + 1 and status.dtype == torch.int32 and status.numel() == 3
        tr, k = traj.numpy().astype(np.float64), ids.numpy().astype(np.int64)
        T = tr.shape[1]
        out = dict(rot6d=np.zeros((len(v), T, 6)), trans=np.zeros((len(v), T, 3)), gap=np.zeros((len(v), T)), residual=np.zeros((len(v), T)))
        for b in range(len(vp) - 1):
            s = slice(vp[b], vp[b + 1])
            lists = [k[pp[i]:pp[i + 1]] for i in range(vp[b], vp[b + 1])]
            nv = vp[b + 1] - vp[b]
            if any(len(r) and (r.min() < 0 or r.max() >= nv) for r in lists):
                status[0] |= self.LOCAL_BAD_ID
                lists = [np.clip(r, 0, nv - 1) for r in lists]
            status[2] += sum(len(r) == 0 for r in lists)
            res = lo.local_motion(v[s], tr[s], lists)
            for name in out:
                out[name][s] = res[name]
        return tuple(torch.from_numpy(out[name]) for name in ("rot6d", "trans", "gap", "residual"))
