"""NumPy emulation of the tolerance-weld operators of morig_amd.native.NativeOps (csrc/proxweld.hip) on top of
``topology_emulate.TopologyOps``, for the CPU tests of the HOST logic of ``morig_amd.meshprep.diagnose`` / ``clean`` / ``repair`` /
``prepare_mesh`` with ``weld_tol``: the sorts and prefix sums between the kernels, the one added host read, ``max_links``, the report
columns and the error texts. It follows the kernels' contract in include/morig_hip.h on CPU tensors with its own means: the links of a
position are found by brute force over the nodes of its mesh (no grid walk), then put into the stated visiting order."""
import numpy as np
import torch

import proxweld_oracle as po
import repair_emulate as re_
import topology_emulate as te

INT64_MAX = np.iinfo(np.int64).max
CELL_BITS, CELL_TOP = 21, (1 << 21) - 2


def cell_side(eps, extent):
    h = max(eps * (1.0 + 2.0 ** -20), extent * 2.0 ** -20)
    return h if h > 0.0 else 1.0


def cell_coord(x, lo, h):
    with np.errstate(all="ignore"):
        q = (np.float64(x) - np.float64(lo)) / np.float64(h)
    if not q >= 1.0:
        return 0
    return CELL_TOP if q >= CELL_TOP else int(q)


class ProxweldMixin:
    def mesh_bbox(self, verts, vptr):
        """the header's contract: ``<`` and ``>``, so a NaN never enters; +inf / -inf for a mesh without vertices"""
        self.calls.append("mesh_bbox")
        v, vp = self._verts(verts), self._ptr(vptr)
        out = np.empty((len(vp) - 1, 6))
        for b in range(len(vp) - 1):
            rows = v[vp[b]:vp[b + 1]]
            for c in range(3):
                x = rows[:, c][~np.isnan(rows[:, c])]
                out[b, c], out[b, 3 + c] = (x.min(), x.max()) if len(x) else (np.inf, -np.inf)
        return torch.from_numpy(out)

    def proxweld_cell_keys(self, verts, nonfinite, rep, vptr, eps):
        self.calls.append("proxweld_cell_keys")
        v, vp = self._verts(verts), self._ptr(vptr)
        bad, rp, e = self._vec(nonfinite, torch.int32, len(v)), self._vec(rep, torch.int32, len(v)), self._vec(eps, torch.float64, len(vp) - 1)
        keys, frame = np.full(len(v), INT64_MAX, dtype=np.int64), np.zeros((len(vp) - 1, 4))
        for b in range(len(vp) - 1):
            rows = np.arange(vp[b], vp[b + 1])
            fin = rows[bad[rows] == 0]
            lo = v[fin].min(0) + 0.0 if len(fin) else np.zeros(3)
            with np.errstate(all="ignore"):
                extent = float((v[fin].max(0) - lo).max()) if len(fin) else 0.0
            frame[b] = [*lo, cell_side(float(e[b]), extent)]
            for r in fin[rp[fin] == fin]:
                c = [cell_coord(v[r, d], lo[d], frame[b, 3]) for d in range(3)]
                keys[r] = (c[0] << 2 * CELL_BITS) | (c[1] << CELL_BITS) | c[2]
        return torch.from_numpy(keys), torch.from_numpy(frame)

    def _sorted(self, keys, order, pos, vptr, eps2):
        vp, n = self._ptr(vptr), pos.shape[0]
        k, o, p = self._vec(keys, torch.int64, n), self._vec(order, torch.int64, n), self._verts(pos)
        e2 = self._vec(eps2, torch.float64, len(vp) - 1)
        assert sorted(o.tolist()) == list(range(n))
        for b in range(len(vp) - 1):                                             # (mesh, key, row): the positions of a mesh hold its rows
            seg = slice(vp[b], vp[b + 1])
            assert ((o[seg] >= vp[b]) & (o[seg] < vp[b + 1])).all()
            assert list(zip(k[seg].tolist(), o[seg].tolist())) == sorted(zip(k[seg].tolist(), o[seg].tolist()))
        return vp, k, o, p, e2

    def _partners(self, vp, k, o, p, e2):
        """per sorted position its linked positions with a higher row, in visiting order: cell x, then y, then position"""
        out = [[] for _ in k]
        for b in range(len(vp) - 1):
            nodes = [i for i in range(vp[b], vp[b + 1]) if k[i] != INT64_MAX]
            if not e2[b] >= po.EPS2_MIN:
                continue
            for i in nodes:
                mine = [j for j in nodes if o[j] > o[i] and po.len2(p[i], p[j]) <= e2[b]]
                out[i] = sorted(mine, key=lambda j: (int(k[j]) >> 2 * CELL_BITS, (int(k[j]) >> CELL_BITS) & ((1 << CELL_BITS) - 1), j))
        return out

    def proxweld_count_links(self, keys, order, pos, vptr, eps2):
        self.calls.append("proxweld_count_links")
        found = self._partners(*self._sorted(keys, order, pos, vptr, eps2))
        return torch.from_numpy(np.array([len(x) for x in found], dtype=np.int32))

    def proxweld_emit_links(self, keys, order, pos, vptr, eps2, count, lrank, n_links):
        self.calls.append("proxweld_emit_links")
        vp, k, o, p, e2 = self._sorted(keys, order, pos, vptr, eps2)
        found = self._partners(vp, k, o, p, e2)
        cnt, rk = self._vec(count, torch.int32, len(k)), self._vec(lrank, torch.int64, len(k))
        assert np.array_equal(cnt, [len(x) for x in found]) and np.array_equal(rk, np.cumsum(cnt)) and n_links == cnt.sum()
        links = [(int(o[i]) << 32) | (int(o[j]) << 1) | 1 for i, mine in enumerate(found) for j in mine]
        return torch.from_numpy(np.array(links, dtype=np.int64))

    def proxweld_spread(self, verts, rep, nonfinite, vptr):
        self.calls.append("proxweld_spread")
        v, vp = self._verts(verts), self._ptr(vptr)
        rp, bad = self._vec(rep, torch.int32, len(v)).astype(np.int64), self._vec(nonfinite, torch.int32, len(v))
        out = np.zeros(len(vp) - 1, dtype=np.int64)
        for b in range(len(vp) - 1):
            rows = np.arange(vp[b], vp[b + 1])
            rows = rows[(bad[rows] == 0) & (rp[rows] != rows)]
            d2 = po.len2(v[rows], v[rp[rows]])
            d2 = d2[np.isfinite(d2)]
            out[b] = d2.max().view(np.int64) if len(d2) else 0
        return torch.from_numpy(out)


class ProxweldOps(ProxweldMixin, te.TopologyOps):
    pass


class ProxweldRepairOps(ProxweldMixin, re_.RepairOps):
    pass
