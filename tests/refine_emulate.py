"""NumPy emulation of the mesh-refinement operators of morig_amd.native.NativeOps (csrc/refine.hip) on top of tests/repair_emulate.py, for
the CPU tests of the HOST logic of ``morig_amd.meshprep.refine`` / ``interpolate`` / ``prepare_mesh(refine_...)``: the sorts, prefix sums
and searches between the kernels, the phases of every mesh, the one size read per pass, the list shapes and the error texts. Installed
through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors, with its own means (plain loops,
Python floats); the children of a face are tests/refine_oracle.py ``split_face``."""
import math
import struct

import numpy as np
import torch

import refine_oracle as fo
import repair_emulate as re_

INT64_MAX = re_.INT64_MAX
T = torch.from_numpy


def bits(x: float) -> int:
    return struct.unpack("=q", struct.pack("=d", x))[0]


class RefineOps(re_.RepairOps):
    REFINE_IDLE, REFINE_LENGTH, REFINE_LONGEST = 0, 1, 2

    def tpl_edge_flags(self, keys):
        self.calls.append("tpl_edge_flags")
        k = self._vec(keys, torch.int64)
        assert np.all(np.diff(k) >= 0)
        first = np.ones(len(k), dtype=bool)
        first[1:] = k[1:] != k[:-1]
        return T((first & (k != INT64_MAX)).astype(np.int32))

    def refine_edge_records(self, verts, faces, fptr, vptr, status):
        self.calls.append("refine_edge_records")
        v, vp, fp = self._verts(verts), self._ptr(vptr), self._ptr(fptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.shape[0] == fp[-1] and len(v) == vp[-1]
        f = faces.numpy().astype(np.int64)
        F, B = len(f), len(vp) - 1
        keys, len2 = np.full(3 * F, INT64_MAX, dtype=np.int64), np.zeros(3 * F)
        top, degenerate = np.zeros(B, dtype=np.int64), np.zeros(F, dtype=np.int32)
        mesh = np.searchsorted(fp[1:], np.arange(F), side="right")
        for i in range(F):
            b = mesh[i]
            if (f[i] < 0).any() or (f[i] >= vp[b + 1] - vp[b]).any():
                status[0] |= self.MESHCHECK_BAD_FACE
                continue
            if len(set(f[i].tolist())) < 3:
                degenerate[i] = 1
                continue
            t = f[i] + vp[b]
            for c in range(3):
                lo, hi = sorted((int(t[c]), int(t[(c + 1) % 3])))
                with np.errstate(all="ignore"):
                    l2 = fo.sq(v[hi], v[lo])
                keys[3 * i + c], len2[3 * i + c] = (lo << 32) | hi, l2
                if math.isfinite(l2):
                    top[b] = max(top[b], bits(l2))
        return T(keys), T(len2), T(top), T(degenerate)

    def refine_mark(self, keys, order, flags, len2, vptr, mode, limit2, maxbits):
        self.calls.append("refine_mark")
        k, o, l2 = self._vec(keys, torch.int64), self._vec(order, torch.int64, keys.numel()), self._vec(len2, torch.float64, keys.numel())
        fl, vp = self._vec(flags, torch.int32, keys.numel()), self._ptr(vptr)
        md, mb = self._vec(mode, torch.int32, len(vp) - 1), self._vec(maxbits, torch.int64, len(vp) - 1)
        assert np.array_equal(k, np.sort(k)) and sorted(o.tolist()) == list(range(len(k)))
        mark, image = np.zeros(len(k), dtype=np.int32), np.full(len(k), -1, dtype=np.int64)
        for i in np.nonzero(fl)[0]:
            b = int(np.searchsorted(vp[1:], k[i] >> 32, side="right"))
            x = float(l2[o[i]])
            if not math.isfinite(x):
                continue
            if md[b] == self.REFINE_LENGTH:
                over = x > limit2
            elif md[b] == self.REFINE_LONGEST:
                over = x > 0.25 * struct.unpack("=d", struct.pack("=q", int(mb[b])))[0]
            else:
                over = False
            if over:
                mark[i], image[i] = 1, bits(x)
        return T(mark), T(image)

    def refine_budget(self, perm, rptr, budget, mark):
        self.calls.append("refine_budget")
        pm, rp, bd = self._vec(perm, torch.int64, mark.numel()), self._vec(rptr, torch.int64), self._vec(budget, torch.int64, rptr.numel() - 1)
        assert mark.dtype == torch.int32 and sorted(pm.tolist()) == list(range(len(pm)))
        m = mark.numpy()
        for b in range(len(bd)):
            seg = pm[rp[b]:rp[b + 1]]
            assert set(seg.tolist()) == set(range(rp[b], rp[b + 1]))               # the records of the mesh, reordered
            live = [p for p in seg if m[p]]
            assert list(seg[:len(live)]) == live                                  # the marked ones first
            for p in seg[min(int(bd[b]), len(seg)):]:
                m[p] = 0

    def refine_number(self, keys, order, mark, erank, vptr, mptr):
        self.calls.append("refine_number")
        k, o, mk = self._vec(keys, torch.int64), self._vec(order, torch.int64, keys.numel()), self._vec(mark, torch.int32, keys.numel())
        er, vp, mp = self._vec(erank, torch.int64, keys.numel()), self._ptr(vptr), self._vec(mptr, torch.int64, vptr.numel())
        assert np.array_equal(er, np.cumsum(mk))
        out = np.full(len(k), -1, dtype=np.int32)
        for i in np.nonzero(mk)[0]:
            b = int(np.searchsorted(vp[1:], k[i] >> 32, side="right"))
            out[o[k == k[i]]] = vp[b + 1] - vp[b] + er[i] - 1 - mp[b]
        return T(out)

    def refine_pattern(self, edge_mid, degenerate):
        self.calls.append("refine_pattern")
        dg = self._vec(degenerate, torch.int32)
        em = self._vec(edge_mid, torch.int32, 3 * len(dg)).reshape(-1, 3)
        pattern = np.where(dg != 0, 0, (em >= 0).sum(1)).astype(np.int32)
        return T(pattern + 1), T(pattern)

    def refine_emit(self, verts, parents, faces, face_map, edge_mid, crank, fptr, vptr, mptr, keys, mark, erank, n_out_rows, n_out_faces):
        self.calls.append("refine_emit")
        v, vp, fp = self._verts(verts), self._ptr(vptr), self._ptr(fptr)
        f, par = faces.numpy().astype(np.int64), parents.numpy()
        F, B = len(f), len(vp) - 1
        fm, cr, em = self._vec(face_map, torch.int64, F), self._vec(crank, torch.int64, F), self._vec(edge_mid, torch.int32, 3 * F).reshape(-1, 3)
        mp, k, mk, er = self._vec(mptr, torch.int64, B + 1), self._vec(keys, torch.int64, 3 * F), self._vec(mark, torch.int32, 3 * F), self._vec(erank, torch.int64, 3 * F)
        assert n_out_rows == len(v) + mp[-1] and n_out_faces == (cr[-1] if F else 0) and par.shape == (len(v), 2)
        out_v, out_p = np.full((n_out_rows, 3), np.nan), np.full((n_out_rows, 2), -1, dtype=np.int64)
        for b in range(B):
            out_v[vp[b] + mp[b]:vp[b + 1] + mp[b]], out_p[vp[b] + mp[b]:vp[b + 1] + mp[b]] = v[vp[b]:vp[b + 1]], par[vp[b]:vp[b + 1]]
        for i in np.nonzero(mk)[0]:
            lo, hi = int(k[i] >> 32), int(k[i] & 0xffffffff)
            b = int(np.searchsorted(vp[1:], lo, side="right"))
            with np.errstate(all="ignore"):
                out_v[vp[b + 1] + er[i] - 1], out_p[vp[b + 1] + er[i] - 1] = fo.mid(v[lo], v[hi]), (lo - vp[b], hi - vp[b])
        out_f, out_m = np.full((n_out_faces, 3), -1, dtype=np.int32), np.full(n_out_faces, -1, dtype=np.int64)
        mesh = np.searchsorted(fp[1:], np.arange(F), side="right")
        for i in range(F):
            b = mesh[i]
            t = f[i].tolist()
            new = {(min(t[c], t[(c + 1) % 3]), max(t[c], t[(c + 1) % 3])): int(em[i, c]) for c in range(3) if em[i, c] >= 0}
            pos = {x: v[vp[b] + x] for x in t}
            with np.errstate(all="ignore"):
                pos.update({m: fo.mid(pos[e[0]], pos[e[1]]) for e, m in new.items()})
                kids = fo.split_face(t, new, pos)
            at = cr[i] - len(kids)
            out_f[at:at + len(kids)], out_m[at:at + len(kids)] = kids, fm[i]
        assert (out_f >= 0).all() and (out_m >= 0).all() and (out_p >= 0).all()
        return T(out_v), T(out_p), T(out_f), T(out_m)

    def refine_interpolate(self, values, parents, row0, row1):
        self.calls.append("refine_interpolate")
        assert values.dtype in (torch.float32, torch.float64) and values.dim() == 2 and values.is_contiguous()
        p = parents.numpy()
        assert parents.dtype == torch.int64 and p.shape == (values.shape[0], 2) and 0 <= row0 <= row1 <= values.shape[0]
        assert (p[row0:row1] >= 0).all() and (p[row0:row1] < row0).all()         # the rows of a launch read rows of earlier launches only
        x = values.numpy()
        with np.errstate(all="ignore"):
            x[row0:row1] = x.dtype.type(0.5) * (x[p[row0:row1, 0]] + x[p[row0:row1, 1]])
