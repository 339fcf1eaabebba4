"""NumPy emulation of the mesh-repair operators of morig_amd.native.NativeOps (csrc/meshfix.hip) on top of tests/topology_emulate.py, for
the CPU tests of the HOST logic of ``morig_amd.meshprep.repair`` / ``prepare_mesh(repair=True)``: the sorts, prefix sums and searches
between the kernels, the cover's round loop, the fixed number of doubling rounds, the selection by ``fill_holes``, the list shapes and the
error texts. Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors, with its own
means (plain loops); the sums are tests/topology_oracle.py ``lane_sum``."""
import numpy as np
import torch

import repair_oracle as ro
import topology_emulate as te
import topology_oracle as to

INT64_MAX = te.INT64_MAX
T = torch.from_numpy


class RepairOps(te.TopologyOps):
    MESHFIX_ORIENTABLE, MESHFIX_NONORIENTABLE, MESHFIX_CLOSED, MESHFIX_INVERTED = 1, 2, 4, 8
    MESHFIX_REGULAR, MESHFIX_TANGLED = 1, 2

    def meshfix_edge_records(self, faces, fptr, vptr, n_rows, status):
        self.calls.append("meshfix_edge_records")
        vp, fp = self._ptr(vptr), self._ptr(fptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.shape[0] == fp[-1] and n_rows == vp[-1]
        f = faces.numpy().astype(np.int64)
        F = len(f)
        tri, keys, vals = np.full((F, 3), -1, dtype=np.int32), np.full(3 * F, INT64_MAX, dtype=np.int64), np.full(3 * F, -1, dtype=np.int32)
        mesh = np.searchsorted(fp[1:], np.arange(F), side="right")
        for i in range(F):
            b = mesh[i]
            if (f[i] < 0).any() or (f[i] >= vp[b + 1] - vp[b]).any() or len(set(f[i].tolist())) < 3:
                status[0] |= self.MESHCHECK_BAD_FACE
                continue
            t = f[i] + vp[b]
            tri[i] = t
            for c in range(3):
                a, d = int(t[c]), int(t[(c + 1) % 3])
                keys[3 * i + c], vals[3 * i + c] = (min(a, d) << 32) | max(a, d), (i << 1) | (1 if a < d else 0)
        return T(tri), T(keys), T(vals)

    def meshfix_links(self, keys, vals, n_faces):
        self.calls.append("meshfix_links")
        k, val = self._vec(keys, torch.int64), self._vec(vals, torch.int32, keys.numel())
        assert np.all(np.diff(k) >= 0)
        cover, bflag, fopen = np.full(len(k), INT64_MAX, dtype=np.int64), np.zeros(len(k), dtype=np.int32), np.zeros(n_faces, dtype=np.int32)
        i = 0
        while i < len(k) and k[i] != INT64_MAX:
            j = i
            while j < len(k) and k[j] == k[i]:
                j += 1
            assert list(val[i:j] >> 1) == sorted(val[i:j] >> 1)                  # a stable sort of face-major records
            if j - i == 2:
                f, g, p = int(val[i] >> 1), int(val[i + 1] >> 1), int((val[i] & 1) == (val[i + 1] & 1))
                assert f < g
                for s in (0, 1):
                    cover[i + s] = ((2 * f + s) << 32) | ((2 * g + (s ^ p)) << 1)
            else:
                fopen[val[i:j] >> 1] = 1
                bflag[i] = 1 if j - i == 1 else 0
            i = j
        return T(cover), T(fopen), T(bflag)

    def meshfix_orient_stats(self, lab, face_open):
        self.calls.append("meshfix_orient_stats")
        F = face_open.numel()
        l, fo = self._vec(lab, torch.int32, 2 * F), self._vec(face_open, torch.int32)
        root, parity = (l[0::2] >> 1).astype(np.int32), (l[0::2] & 1).astype(np.int32)
        ropen = np.zeros(F, dtype=np.int32)
        ropen[root[fo != 0]] = 1
        return T(root), T(parity), T(root.astype(np.int64)), T(ropen)

    def meshfix_signed_volume(self, verts, tri, parity, order, kptr, roots):
        self.calls.append("meshfix_signed_volume")
        v, t = self._verts(verts), tri.numpy().astype(np.int64)
        F = len(t)
        par, o = self._vec(parity, torch.int32, F), self._vec(order, torch.int64, F)
        kp, rt = self._vec(kptr, torch.int64, roots.numel() + 1), self._vec(roots, torch.int64)
        vol, cnt, cnt1 = np.zeros(F), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
        for c, r in enumerate(rt):
            members = o[kp[c]:kp[c + 1]]
            assert list(members) == sorted(members)
            with np.errstate(all="ignore"):
                vol[r] = to.lane_sum([-ro.term(v, t[f]) if par[f] else ro.term(v, t[f]) for f in members])
            cnt[r], cnt1[r] = len(members), int(par[members].sum())
        return T(vol), T(cnt), T(cnt1)

    def meshfix_orient_apply(self, tri, fptr, vptr, lab, root, parity, root_open, vol, cnt, cnt1):
        self.calls.append("meshfix_orient_apply")
        vp, fp, t = self._ptr(vptr), self._ptr(fptr), tri.numpy().astype(np.int64)
        F = len(t)
        l, rt, par, ro_, n, n1 = (self._vec(x, torch.int32) for x in (lab, root, parity, root_open, cnt, cnt1))
        s = self._vec(vol, torch.float64, F)
        mesh = np.searchsorted(fp[1:], np.arange(F), side="right")
        out, flipped, info = np.empty((F, 3), dtype=np.int64), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
        for f in range(F):
            r = rt[f]
            twisted, closed = l[2 * r] == l[2 * r + 1], not ro_[r]
            by_volume = (not twisted) and closed and (s[r] > 0 or s[r] < 0)
            cls = -1 if twisted else ((1 if s[r] > 0 else 0) if by_volume else (1 if n1[r] <= n[r] - n1[r] else 0))
            flipped[f] = int(cls >= 0 and par[f] == cls)
            out[f] = (t[f][[0, 2, 1]] if flipped[f] else t[f]) - vp[mesh[f]]
            if r == f:
                turned = n1[r] if cls == 1 else n[r] - n1[r]
                info[f] = 2 if twisted else 1 | (4 if closed else 0) | (8 if by_volume and turned == n[r] else 0)
        return T(out), T(flipped), T(info)

    def meshfix_boundary_init(self, keys, vals, bflag, flipped, n_rows):
        self.calls.append("meshfix_boundary_init")
        k, val, bf, fl = self._vec(keys, torch.int64), self._vec(vals, torch.int32), self._vec(bflag, torch.int32), self._vec(flipped, torch.int32)
        hfrom, hto = np.full(len(k), -1, dtype=np.int32), np.full(len(k), -1, dtype=np.int32)
        out, ind, nxt = np.zeros(n_rows, dtype=np.int64), np.zeros(n_rows, dtype=np.int64), np.full(n_rows, 2 ** 31 - 1, dtype=np.int64)
        for i in np.nonzero(bf)[0]:
            lo, hi = int(k[i] >> 32), int(k[i] & 0xffffffff)
            a, b = (lo, hi) if bool(val[i] & 1) != bool(fl[val[i] >> 1]) else (hi, lo)
            hfrom[i], hto[i] = a, b
            out[a] += 1
            ind[b] += 1
            nxt[a] = min(nxt[a], b)
        regular = (out == 1) & (ind == 1)
        rows = np.arange(n_rows)
        vclass = np.where(regular, 1, np.where((out > 0) | (ind > 0), 2, 0)).astype(np.int32)
        return (T(hfrom), T(hto), T(np.where(regular, nxt, rows).astype(np.int32)), T(np.where(regular, rows, -1).astype(np.int32)), T(vclass))

    def meshfix_loop_round(self, lab, nxt, lab2, nxt2):
        self.calls.append("meshfix_loop_round")
        l, n = self._vec(lab, torch.int32), self._vec(nxt, torch.int32, lab.numel())
        assert lab2.data_ptr() != lab.data_ptr() and nxt2.data_ptr() != nxt.data_ptr() and lab2.numel() == nxt2.numel() == lab.numel()
        lab2.copy_(T(np.minimum(l, l[n])))
        nxt2.copy_(T(n[n]))

    def meshfix_loop_centroid(self, verts, order, lptr, sel):
        self.calls.append("meshfix_loop_centroid")
        v = self._verts(verts)
        o, lp, s = self._vec(order, torch.int64, len(v)), self._vec(lptr, torch.int64), self._vec(sel, torch.int64)
        with np.errstate(all="ignore"):
            out = [[to.lane_sum([float(v[x, d]) for x in o[lp[c]:lp[c + 1]]]) / float(lp[c + 1] - lp[c]) for d in range(3)] for c in s]
        return T(np.array(out, dtype=np.float64).reshape(-1, 3))

    def meshfix_fill_mark(self, vclass, lab, slot):
        self.calls.append("meshfix_fill_mark")
        vc, l, sl = (self._vec(x, torch.int32, vclass.numel()) for x in (vclass, lab, slot))
        return T(((vc == 1) & (l >= 0) & (sl[np.maximum(l, 0)] >= 0)).astype(np.int32))

    def meshfix_fill_emit(self, nxt0, emit, erank, lab, slot, vptr, sptr, n_out):
        self.calls.append("meshfix_fill_emit")
        n0, em, l, sl = (self._vec(x, torch.int32, nxt0.numel()) for x in (nxt0, emit, lab, slot))
        er, vp, sp = self._vec(erank, torch.int64), self._ptr(vptr), self._vec(sptr, torch.int64)
        assert np.array_equal(er, np.cumsum(em)) and n_out == em.sum() and len(sp) == len(vp)
        mesh = np.searchsorted(vp[1:], np.arange(len(n0)), side="right")
        out = [(n0[x] - vp[mesh[x]], x - vp[mesh[x]], vp[mesh[x] + 1] - vp[mesh[x]] + sl[l[x]] - sp[mesh[x]]) for x in np.nonzero(em)[0]]
        return T(np.array(out, dtype=np.int64).reshape(-1, 3))
