"""NumPy emulation of the split operators of morig_amd.native.NativeOps (csrc/meshsplit.hip) on top of tests/repair_emulate.py, for the
CPU tests of the HOST logic of ``morig_amd.meshprep.split_nonmanifold`` / ``repair(split=True)`` / ``prepare_mesh(split=True)``: the sort
and its permutation, the round loop on the corner nodes, the new-fan flags and their prefix sum, the one table read, the list shapes and
the error texts. Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors, with
its own means (plain loops)."""
import numpy as np
import torch

import repair_emulate as re_

INT64_MAX = re_.INT64_MAX
INT32_MAX = 2 ** 31 - 1
T = torch.from_numpy


class ManifoldOps(re_.RepairOps):
    def meshsplit_links(self, keys, vals, order, n_faces):
        self.calls.append("meshsplit_links")
        k, val, o = self._vec(keys, torch.int64), self._vec(vals, torch.int32, keys.numel()), self._vec(order, torch.int64, keys.numel())
        assert np.all(np.diff(k) >= 0) and len(k) == 3 * n_faces and sorted(o.tolist()) == list(range(len(k)))
        links, nm = np.full(len(k), INT64_MAX, dtype=np.int64), np.zeros(len(k), dtype=np.int32)
        i = 0
        while i < len(k) and k[i] != INT64_MAX:
            j = i
            while j < len(k) and k[j] == k[i]:
                j += 1
            if j - i == 2:
                ends = []                                                        # per record (corner at lo, corner at hi)
                for p in (i, i + 1):
                    f, d, c = int(val[p] >> 1), int(val[p] & 1), int(o[p] % 3)
                    assert o[p] // 3 == f
                    ends.append((3 * f + (c if d else (c + 1) % 3), 3 * f + ((c + 1) % 3 if d else c)))
                assert ends[0][0] < ends[1][0]
                links[i] = (ends[0][0] << 32) | (ends[1][0] << 1)
                links[i + 1] = (ends[0][1] << 32) | (ends[1][1] << 1)
            elif j - i >= 3:
                nm[i] = 1
            i = j
        return T(links), T(nm)

    def meshsplit_fans(self, lab, tri, n_rows):
        self.calls.append("meshsplit_fans")
        t = tri.numpy().reshape(-1).astype(np.int64)
        l = self._vec(lab, torch.int32, len(t))
        first, nfans = np.full(n_rows, INT32_MAX, dtype=np.int32), np.zeros(n_rows, dtype=np.int32)
        for n in np.nonzero(l == np.arange(len(t)))[0][::-1]:                    # any order gives the same
            first[t[n]] = min(first[t[n]], n)
            nfans[t[n]] += 1
        return T(first), T(nfans)

    def meshsplit_apply(self, lab, tri, first, rank, fptr, vptr, aptr, verts, n_out_rows):
        self.calls.append("meshsplit_apply")
        v, t = self._verts(verts), tri.numpy().reshape(-1).astype(np.int64)
        vp, fp = self._ptr(vptr), self._ptr(fptr)
        l, fi = self._vec(lab, torch.int32, len(t)), self._vec(first, torch.int32, len(v))
        rk, ap = self._vec(rank, torch.int64, len(t)), self._vec(aptr, torch.int64, len(vp))
        new = (l == np.arange(len(t))) & (fi[t] != np.arange(len(t))) if len(t) else np.zeros(0, dtype=bool)
        assert np.array_equal(rk, np.cumsum(new)) and n_out_rows == len(v) + int(new.sum()) and ap[-1] == new.sum()
        out_f, source = np.empty(len(t), dtype=np.int64), np.full(n_out_rows, -7, dtype=np.int64)
        out_v = np.full((n_out_rows, 3), 123.0)
        for b in range(len(vp) - 1):
            for x in range(vp[b], vp[b + 1]):
                source[x + ap[b]], out_v[x + ap[b]] = x - vp[b], v[x]
            for n in range(3 * fp[b], 3 * fp[b + 1]):
                if fi[t[n]] == l[n]:
                    out_f[n] = t[n] - vp[b]
                    continue
                out_f[n] = (vp[b + 1] - vp[b]) + rk[l[n]] - 1 - ap[b]
                if l[n] == n:
                    row = vp[b + 1] + rk[n] - 1
                    source[row], out_v[row] = t[n] - vp[b], v[t[n]]
        assert (source >= 0).all()
        return T(out_f.reshape(-1, 3)), T(source), T(out_v)
