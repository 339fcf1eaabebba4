"""NumPy emulation of the mesh-BVH operators of morig_amd.native.NativeOps (csrc/bvh.hip) together with the bone-ray and transfer
operators the ``accel`` routes share (tests/labels_emulate.py, tests/transfer_emulate.py), for the CPU tests of the HOST logic of
morig_amd/spatial.py: the level tables and node ranges, the stable order, the refit, the argument checks, the status handling and the
routing. Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors; the arithmetic
is that of tests/spatial_oracle.py."""
import numpy as np
import torch

import spatial_oracle as so
from labels_emulate import LabelOps
from transfer_emulate import TransferOps


class SpatialOps(LabelOps, TransferOps):
    BVH_MAX_FACES, BVH_BAD_FACE, BVH_LEVELS = 64 ** 4, 1, 4

    def mesh_bbox(self, verts, vptr):
        self.calls.append("mesh_bbox")
        vp, v = self._ptr(vptr), self._f64(verts, 3)
        out = np.empty((len(vp) - 1, 6))
        for b in range(len(vp) - 1):
            for k in range(3):
                col = v[vp[b]:vp[b + 1], k]
                col = col[~np.isnan(col)]                                               # the kernel's `<` and `>` never take a NaN
                out[b, k], out[b, 3 + k] = (col.min(), col.max()) if len(col) else (np.inf, -np.inf)
        return torch.from_numpy(out)

    def _meshes(self, verts, vptr, faces, fptr):
        vp, fp, v = self._ptr(vptr), self._ptr(fptr), self._f64(verts, 3)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert len(vp) == len(fp) and vp[-1] == len(v) and fp[-1] == len(faces)
        f = faces.numpy().astype(np.int64)
        return vp, fp, [(v[vp[b]:vp[b + 1]], f[fp[b]:fp[b + 1]]) for b in range(len(vp) - 1)]

    def bvh_build_keys(self, verts, vptr, faces, fptr, bbox):
        self.calls.append("bvh_build_keys")
        vp, fp, meshes = self._meshes(verts, vptr, faces, fptr)
        assert so.same(bbox.numpy(), self.mesh_bbox(verts, vptr).numpy()) and self.calls.pop() == "mesh_bbox"
        keys = [(b << 30) | so.morton_codes(v, so.clamped(v, f)[0]) if len(v) else np.full(len(f), b << 30, dtype=np.int64)
                for b, (v, f) in enumerate(meshes)]
        return torch.from_numpy(np.concatenate(keys).astype(np.int64) if keys else np.zeros(0, dtype=np.int64))

    def _trees(self, verts, vptr, faces, fptr, order, node_ptr):
        vp, fp, meshes = self._meshes(verts, vptr, faces, fptr)
        assert order.dtype == torch.int32 and order.dim() == 1 and order.is_contiguous() and order.numel() == fp[-1]
        assert node_ptr.dtype == torch.int32 and node_ptr.shape == (4, len(vp)) and node_ptr.is_contiguous()
        counts = np.zeros((4, len(meshes)), dtype=np.int64)
        for b, (_, f) in enumerate(meshes):
            lc = so.level_counts(len(f))
            counts[:len(lc), b] = lc
        totals = counts.sum(1)
        base = np.concatenate([[0], np.cumsum(totals)])[:-1]
        want = np.stack([base[k] + np.concatenate([[0], np.cumsum(counts[k])]) for k in range(4)])
        assert np.array_equal(node_ptr.numpy(), want), "node_ptr is not the level table of the face counts"
        trees, od = [], order.numpy().astype(np.int64)
        for b, (v, f) in enumerate(meshes):
            local = od[fp[b]:fp[b + 1]] - fp[b]
            assert np.array_equal(np.sort(local), np.arange(len(f))), "order is no permutation of the mesh's faces"
            trees.append(so.build(v, f, order=local) if len(v) else dict(verts=v, faces=f[:0], bad=len(f) > 0, order=local[:0], levels=[]))
        return vp, fp, want, totals, trees

    def bvh_boxes(self, verts, vptr, faces, fptr, order, node_ptr, level_nodes, max_faces):
        self.calls.append("bvh_boxes")
        vp, fp, table, totals, trees = self._trees(verts, vptr, faces, fptr, order, node_ptr)
        assert list(level_nodes) == list(totals) and max_faces == (np.diff(fp).max() if len(fp) > 1 else 0) <= self.BVH_MAX_FACES
        boxes = np.tile([np.inf] * 3 + [-np.inf] * 3, (int(totals.sum()), 1))
        flags = np.zeros(len(trees), dtype=np.int32)
        for b, tree in enumerate(trees):
            flags[b] = self.BVH_BAD_FACE if tree["bad"] else 0
            for k, lv in enumerate(tree["levels"]):
                boxes[table[k, b]:table[k, b + 1]] = lv
        return torch.from_numpy(boxes), torch.from_numpy(flags)

    def _checked_trees(self, verts, vptr, faces, fptr, order, boxes, node_ptr, flags):
        vp, fp, table, totals, trees = self._trees(verts, vptr, faces, fptr, order, node_ptr)
        want_boxes, want_flags = self.bvh_boxes(verts, vptr, faces, fptr, order, node_ptr, totals, np.diff(fp).max() if len(fp) > 1 else 0)
        assert self.calls.pop() == "bvh_boxes" and so.same(boxes.numpy(), want_boxes.numpy()) and so.same(flags.numpy(), want_flags.numpy())
        return trees

    def bvh_ray_cast(self, origins, dirs, ray_ptr, verts, vptr, faces, fptr, order, boxes, node_ptr, flags, orientation, want_visits=False):
        self.calls.append("bvh_ray_cast")
        trees = self._checked_trees(verts, vptr, faces, fptr, order, boxes, node_ptr, flags)
        rp, o, d = self._ptr(ray_ptr), self._f64(origins, 3), self._f64(dirs, 3)
        assert len(rp) == len(trees) + 1 and rp[-1] == len(o) == len(d) and orientation in (-1, 0, 1)
        t, face, point = np.full(len(o), np.inf), np.full(len(o), -1, dtype=np.int32), np.full((len(o), 3), np.nan)
        visits, status = np.zeros(len(o), dtype=np.int32), 0
        for b, tree in enumerate(trees):
            rs = slice(rp[b], rp[b + 1])
            c = so.cast(tree, o[rs], d[rs], orientation)
            t[rs], face[rs], point[rs], visits[rs] = c["t"], c["face"], c["point"], c["visits"]
            status |= self.RAY_BAD_FACE if c["bad"] else 0
        return (torch.from_numpy(t), torch.from_numpy(face), torch.from_numpy(point), torch.tensor([status], dtype=torch.int32),
                torch.from_numpy(visits) if want_visits else None)

    def bvh_closest(self, points, pptr, verts, vptr, faces, fptr, order, boxes, node_ptr, flags, status, want_visits=False):
        self.calls.append("bvh_closest")
        trees = self._checked_trees(verts, vptr, faces, fptr, order, boxes, node_ptr, flags)
        pp, p = self._ptr(pptr), self._f64(points, 3)
        assert len(pp) == len(trees) + 1 and pp[-1] == len(p) and status.dtype == torch.int32
        face, bary, dist = np.full(len(p), -1, dtype=np.int32), np.full((len(p), 3), np.nan), np.full(len(p), np.nan)
        visits = np.zeros(len(p), dtype=np.int32)
        for b, tree in enumerate(trees):
            ps = slice(pp[b], pp[b + 1])
            c = so.closest(tree, p[ps])
            face[ps], bary[ps], dist[ps], visits[ps] = c["face"], c["bary"], c["distance"], c["visits"]
            status[0] |= (self.TRANSFER_BAD_FACE if c["bad"] else 0) | (self.TRANSFER_NO_FACES if c["no_faces"] else 0)
        return torch.from_numpy(face), torch.from_numpy(bary), torch.from_numpy(dist), torch.from_numpy(visits) if want_visits else None

    def bvh_blocked(self, a, b, seg_ptr, skip_vertex, t_max, verts, vptr, faces, fptr, order, boxes, node_ptr, flags, want_visits=False):
        self.calls.append("bvh_blocked")
        trees = self._checked_trees(verts, vptr, faces, fptr, order, boxes, node_ptr, flags)
        sp, pa, pb = self._ptr(seg_ptr), self._f64(a, 3), self._f64(b, 3)
        assert len(sp) == len(trees) + 1 and sp[-1] == len(pa) == len(pb)
        assert skip_vertex is None or (skip_vertex.dtype == torch.int32 and skip_vertex.shape == (len(pa),))
        assert t_max is None or (t_max.dtype == torch.float64 and t_max.shape == (len(pa),))
        out, visits, status = np.zeros(len(pa), dtype=np.uint8), np.zeros(len(pa), dtype=np.int32), 0
        for m, tree in enumerate(trees):
            ss = slice(sp[m], sp[m + 1])
            c = so.blocked(tree, pa[ss], pb[ss], None if skip_vertex is None else skip_vertex.numpy()[ss], None if t_max is None else t_max.numpy()[ss])
            out[ss], visits[ss] = c["blocked"], c["visits"]
            status |= self.RAY_BAD_FACE if c["bad"] else 0
        return torch.from_numpy(out), torch.tensor([status], dtype=torch.int32), torch.from_numpy(visits) if want_visits else None
