"""NumPy emulation of the mesh-diagnosis operators of morig_amd.native.NativeOps (csrc/meshcheck.hip), with ``mesh_bbox`` /
``mesh_affine`` for ``prepare_mesh``'s first stage, for the CPU tests of the HOST logic of ``morig_amd.meshprep.diagnose`` / ``clean``:
the sorts and prefix sums between the kernels, the round loop and its guard, the ``keep`` rules, the list shapes and the error texts.
Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors, with its own means
(plain loops); the area of a component is summed by tests/topology_oracle.py ``lane_sum``."""
import struct

import numpy as np
import torch

import topology_oracle as to

INT64_MAX = np.iinfo(np.int64).max
ROOT_NONE = (1 << 31) - 1


def coord_key(x: float) -> int:
    if x == 0.0:
        return 0
    b = struct.unpack("=q", struct.pack("=d", x))[0]
    return b if b >= 0 else b ^ 0x7fffffffffffffff


class TopologyOps:
    MESHCHECK_BAD_FACE, MESHCHECK_ROUND_GUARD = 1, 2
    EDGE_MANIFOLD, EDGE_BOUNDARY, EDGE_NONMANIFOLD, EDGE_CONFLICT = 1, 2, 3, 4
    MESH_NORMALIZE, MESH_GRID = 0, 1

    def __init__(self, stall_rounds=False):
        self.calls = []
        self.stall_rounds = stall_rounds                                         # a broken round that never settles: the guard's test

    @staticmethod
    def _vec(t, dtype, n=None):
        assert t.dtype == dtype and t.dim() == 1 and t.is_contiguous() and (n is None or t.numel() == n), (t.dtype, tuple(t.shape))
        return t.numpy()

    @staticmethod
    def _ptr(p):
        assert p.dtype == torch.int32 and p.dim() == 1 and p.is_contiguous()
        h = p.numpy().astype(np.int64)
        assert h[0] == 0 and np.all(np.diff(h) >= 0)
        return h

    @staticmethod
    def _verts(verts):
        assert verts.dtype == torch.float64 and verts.dim() == 2 and verts.shape[1] == 3 and verts.is_contiguous()
        return verts.numpy()

    # -- what prepare_mesh needs in front of the cleaning
    def mesh_bbox(self, verts, vptr):
        self.calls.append("mesh_bbox")
        v, vp = self._verts(verts), self._ptr(vptr)
        return torch.from_numpy(np.array([np.concatenate([v[vp[b]:vp[b + 1]].min(0), v[vp[b]:vp[b + 1]].max(0)]) for b in range(len(vp) - 1)]))

    def mesh_affine(self, verts, vptr, frame, mode, mul=1.0):
        self.calls.append("mesh_affine")
        v, vp, fr = self._verts(verts), self._ptr(vptr), frame.numpy()
        out = np.empty_like(v)
        for b in range(len(vp) - 1):
            d = v[vp[b]:vp[b + 1]] - fr[b, :3]
            out[vp[b]:vp[b + 1]] = d * fr[b, 3] if mode == self.MESH_NORMALIZE else d / fr[b, 3] * mul
        return torch.from_numpy(out)

    # -- the weld
    def meshcheck_coord_keys(self, verts):
        self.calls.append("meshcheck_coord_keys")
        v = self._verts(verts)
        keys = np.array([[coord_key(float(x)) for x in v[:, c]] for c in range(3)], dtype=np.int64).reshape(3, len(v))
        return torch.from_numpy(keys), torch.from_numpy((~np.isfinite(v).all(1)).astype(np.int32))

    def meshcheck_weld_mark(self, keys, nonfinite, order, vptr):
        self.calls.append("meshcheck_weld_mark")
        vp, n = self._ptr(vptr), nonfinite.numel()
        k, bad, o = keys.numpy(), self._vec(nonfinite, torch.int32), self._vec(order, torch.int64, n)
        assert tuple(k.shape) == (3, n) and sorted(o.tolist()) == list(range(n))
        mesh = np.searchsorted(vp[1:], np.arange(n), side="right")
        flags = np.ones(n, dtype=np.int32)
        for i in range(1, n):
            r, p = o[i], o[i - 1]
            flags[i] = 0 if (not bad[r] and not bad[p] and mesh[r] == mesh[p] and np.array_equal(k[:, r], k[:, p])) else 1
        return torch.from_numpy(flags)

    def meshcheck_run_rep(self, order, flags, rank, dead=None):
        self.calls.append("meshcheck_run_rep")
        n = order.numel()
        o, fl, rk = self._vec(order, torch.int64), self._vec(flags, torch.int32, n), self._vec(rank, torch.int64, n)
        assert np.array_equal(rk, np.cumsum(fl))
        dd = np.zeros(n, dtype=np.int32) if dead is None else self._vec(dead, torch.int32, n)
        rep, first = np.full(n, -1, dtype=np.int32), -1
        for i in range(n):
            if fl[i]:
                first = o[i]
            if not dd[o[i]]:
                assert first >= 0
                rep[o[i]] = first
        return torch.from_numpy(rep)

    # -- faces
    def meshcheck_face_keys(self, faces, fptr, vptr, rep, status):
        self.calls.append("meshcheck_face_keys")
        vp, fp = self._ptr(vptr), self._ptr(fptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.shape[0] == fp[-1] and len(fp) == len(vp)
        rp, f = self._vec(rep, torch.int32, vp[-1]), faces.numpy().astype(np.int64)
        F = len(f)
        tri, major, minor = np.full((F, 3), -1, dtype=np.int32), np.full(F, INT64_MAX, dtype=np.int64), np.full(F, INT64_MAX, dtype=np.int64)
        deg = np.ones(F, dtype=np.int32)
        mesh = np.searchsorted(fp[1:], np.arange(F), side="right")
        for i in range(F):
            b = mesh[i]
            if (f[i] < 0).any() or (f[i] >= vp[b + 1] - vp[b]).any():
                status[0] |= self.MESHCHECK_BAD_FACE
                continue
            t = rp[f[i] + vp[b]]
            tri[i] = t
            if len(set(t.tolist())) == 3:
                lo, mid, hi = sorted(int(x) for x in t)
                deg[i], major[i], minor[i] = 0, lo, (mid << 32) | hi
        return torch.from_numpy(tri), torch.from_numpy(major), torch.from_numpy(minor), torch.from_numpy(deg)

    def meshcheck_face_mark(self, major, minor, order):
        self.calls.append("meshcheck_face_mark")
        F = order.numel()
        ma, mi, o = self._vec(major, torch.int64, F), self._vec(minor, torch.int64, F), self._vec(order, torch.int64)
        pairs = [(int(ma[x]), int(mi[x]), int(x)) for x in o]
        assert pairs == sorted(pairs)                                            # sorted by (major, minor), stably
        flags = np.array([1 if pairs[i][0] != INT64_MAX and (i == 0 or pairs[i][:2] != pairs[i - 1][:2]) else 0 for i in range(F)], dtype=np.int32)
        return torch.from_numpy(flags)

    @staticmethod
    def _kept(tri, surv):
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and surv.dtype == torch.int32 and surv.numel() == tri.shape[0]
        t, s = tri.numpy().astype(np.int64), surv.numpy()
        return t, s, s == np.arange(len(s))

    def meshcheck_face_edges(self, verts, tri, surv):
        self.calls.append("meshcheck_face_edges")
        v = self._verts(verts)
        t, _, kept = self._kept(tri, surv)
        ref, zero = np.zeros(len(v), dtype=np.int32), np.zeros(len(t), dtype=np.int32)
        ek = np.full(3 * len(t), INT64_MAX, dtype=np.int64)
        for i in np.nonzero(kept)[0]:
            ref[t[i]] = 1
            zero[i] = 1 if all(x == 0.0 for x in to.normal(v, *t[i])) else 0
            for c in range(3):
                a, b = int(t[i][c]), int(t[i][(c + 1) % 3])
                ek[3 * i + c] = (a << 32) | (b << 1) | 1 if a < b else (b << 32) | (a << 1)
        return torch.from_numpy(ref), torch.from_numpy(zero), torch.from_numpy(ek)

    # -- components
    def meshcheck_cc_round(self, cur, nxt, ekeys, vptr, changed):
        self.calls.append("meshcheck_cc_round")
        vp, n = self._ptr(vptr), cur.numel()
        c, k = self._vec(cur, torch.int32).astype(np.int64), self._vec(ekeys, torch.int64)
        assert nxt.dtype == torch.int32 and nxt.numel() == n and changed.dtype == torch.int32 and changed.numel() == len(vp) - 1
        k = k[k != INT64_MAX]
        u, w = k >> 32, (k & 0xffffffff) >> 1
        gp = c[c]
        m = gp.copy()
        np.minimum.at(m, u, gp[w])
        np.minimum.at(m, w, gp[u])
        out = np.minimum(c, m)
        np.minimum.at(out, c, m)
        nxt.copy_(torch.from_numpy(out.astype(np.int32)))
        moved = np.array([int((out[vp[b]:vp[b + 1]] != c[vp[b]:vp[b + 1]]).any()) for b in range(len(vp) - 1)], dtype=np.int32)
        if self.stall_rounds:
            moved[:] = 1
        changed.copy_(torch.from_numpy(moved))

    def meshcheck_edge_classify(self, keys, label):
        self.calls.append("meshcheck_edge_classify")
        k, lab = self._vec(keys, torch.int64), self._vec(label, torch.int32)
        assert np.all(np.diff(k) >= 0)
        ec, rb = np.zeros(len(k), dtype=np.int32), np.zeros(len(lab), dtype=np.int32)
        i = 0
        while i < len(k) and k[i] != INT64_MAX:
            j = i
            while j < len(k) and k[j] >> 1 == k[i] >> 1:
                j += 1
            n, fw = j - i, int((k[i:j] & 1).sum())
            ec[i] = self.EDGE_BOUNDARY if n == 1 else self.EDGE_NONMANIFOLD if n >= 3 else self.EDGE_MANIFOLD if fw == 1 else self.EDGE_CONFLICT
            if n == 1:
                rb[lab[k[i] >> 32]] += 1
            i = j
        return torch.from_numpy(ec), torch.from_numpy(rb)

    def meshcheck_comp_counts(self, tri, surv, referenced, label):
        self.calls.append("meshcheck_comp_counts")
        t, _, kept = self._kept(tri, surv)
        ref, lab = self._vec(referenced, torch.int32), self._vec(label, torch.int32)
        rv, rf = np.zeros(len(lab), dtype=np.int32), np.zeros(len(lab), dtype=np.int32)
        np.add.at(rv, lab[ref != 0], 1)
        froot = np.full(len(t), ROOT_NONE, dtype=np.int64)
        froot[kept] = lab[t[kept, 0]]
        np.add.at(rf, froot[kept], 1)
        return torch.from_numpy(rv), torch.from_numpy(rf), torch.from_numpy(froot)

    def meshcheck_comp_area(self, verts, tri, order, kptr):
        self.calls.append("meshcheck_comp_area")
        v, t = self._verts(verts), tri.numpy().astype(np.int64)
        o, kp = self._vec(order, torch.int64, len(t)), self._vec(kptr, torch.int64)
        area = [to.lane_sum([to.face_area(v, t[f]) for f in o[kp[c]:kp[c + 1]]]) for c in range(len(kp) - 1)]
        return torch.from_numpy(np.array(area, dtype=np.float64))

    # -- compaction
    def meshcheck_keep_flags(self, rep, referenced, label, keep_root, drop_unreferenced, tri, surv):
        self.calls.append("meshcheck_keep_flags")
        t, _, kept = self._kept(tri, surv)
        rp, ref, lab, kr = (self._vec(x, torch.int32) for x in (rep, referenced, label, keep_root))
        vkeep = rp == np.arange(len(rp))
        if drop_unreferenced:
            vkeep &= (ref != 0) & (kr[lab] != 0)
        fkeep = kept.copy()
        fkeep[kept] = kr[lab[t[kept, 0]]] != 0
        return torch.from_numpy(vkeep.astype(np.int32)), torch.from_numpy(fkeep.astype(np.int32))

    def meshcheck_compact(self, verts, rep, vkeep, vrank, vptr, ovptr, tri, surv, fkeep, frank, fptr, ofptr, n_out_v, n_out_f):
        self.calls.append("meshcheck_compact")
        v, vp, fp = self._verts(verts), self._ptr(vptr), self._ptr(fptr)
        t, s, _ = self._kept(tri, surv)
        rp, vk, fk = self._vec(rep, torch.int32, len(v)), self._vec(vkeep, torch.int32, len(v)), self._vec(fkeep, torch.int32, len(t))
        vr, fr, ov, of = self._vec(vrank, torch.int64), self._vec(frank, torch.int64), self._vec(ovptr, torch.int64), self._vec(ofptr, torch.int64)
        assert np.array_equal(vr, np.cumsum(vk)) and np.array_equal(fr, np.cumsum(fk)) and n_out_v == vk.sum() and n_out_f == fk.sum()
        assert ov[-1] == n_out_v and of[-1] == n_out_f
        vmesh = np.searchsorted(vp[1:], np.arange(len(v)), side="right")
        fmesh = np.searchsorted(fp[1:], np.arange(len(t)), side="right")
        glob = np.where(vk[rp] != 0, vr[rp] - 1, -1)                              # the output row of every input row
        vmap = np.where(glob >= 0, glob - ov[vmesh], -1) if len(v) else np.zeros(0, dtype=np.int64)
        fmap = np.full(len(t), -1, dtype=np.int64)
        ok = s >= 0
        fmap[ok] = np.where(fk[s[ok]] != 0, fr[s[ok]] - 1 - of[fmesh[ok]], -1)
        out_f = np.array([glob[t[i]] - ov[fmesh[i]] for i in np.nonzero(fk)[0]], dtype=np.int64).reshape(-1, 3)
        return (torch.from_numpy(v[vk != 0].reshape(-1, 3).copy()), torch.from_numpy(out_f), torch.from_numpy(vmap.astype(np.int64)),
                torch.from_numpy(fmap))
