"""NumPy emulation of the visibility operators on the mesh BVH of morig_amd.native.NativeOps (csrc/bvh.hip: bvh_view_boxes,
bvh_scan_visibility, bvh_bone_visibility) and of ``bone_visibility`` (csrc/geodesic.hip), on top of the emulated scan and mesh-BVH layers
(tests/scan_emulate.py, tests/spatial_emulate.py), for the CPU tests of the ``accel`` routes of morig_amd/scan.py and
morig_amd/geodesic.py. Installed through ``runtime._test_ops``. The arithmetic is that of tests/visibility_oracle.py."""
import numpy as np
import torch

import spatial_oracle as so
import visibility_oracle as vo
from scan_emulate import ScanOps
from spatial_emulate import SpatialOps

EMPTY = [np.inf] * 3 + [-np.inf] * 3


class VisibilityOps(ScanOps, SpatialOps):
    def _view_trees(self, verts, vptr, view_mesh, faces, fptr, order, node_ptr):
        vp, fp, vm = self._ptr(vptr), self._ptr(fptr), np.asarray(view_mesh, dtype=np.int64)
        assert order.dtype == torch.int32 and order.dim() == 1 and order.is_contiguous() and order.numel() == fp[-1] == faces.shape[0]
        assert node_ptr.dtype == torch.int32 and node_ptr.shape == (4, len(vp)) and node_ptr.is_contiguous()
        assert len(vm) == len(vp) - 1 and np.all((vm >= 0) & (vm < len(fp) - 1))
        counts = np.zeros((4, len(vm)), dtype=np.int64)
        for v, m in enumerate(vm):
            lc = so.level_counts(fp[m + 1] - fp[m])
            counts[:len(lc), v] = lc
        totals = counts.sum(1)
        base = np.concatenate([[0], np.cumsum(totals)])[:-1]
        want = np.stack([base[k] + np.concatenate([[0], np.cumsum(counts[k])]) for k in range(4)])
        assert np.array_equal(node_ptr.numpy(), want), "node_ptr is not the level table of the views' face counts"
        od, f, x = order.numpy().astype(np.int64), faces.numpy().astype(np.int64), verts.numpy()
        trees = []
        for v, m in enumerate(vm):
            local = od[fp[m]:fp[m + 1]] - fp[m]
            assert np.array_equal(np.sort(local), np.arange(len(local))), "order is no permutation of the mesh's faces"
            trees.append(vo.view_tree(x[vp[v]:vp[v + 1]], f[fp[m]:fp[m + 1]], local))
        return want, totals, trees

    def _view_boxes(self, table, totals, trees):
        boxes, flags = np.tile(EMPTY, (int(totals.sum()), 1)), np.zeros(len(trees), dtype=np.int32)
        for v, tree in enumerate(trees):
            flags[v] = self.BVH_BAD_FACE if tree["bad"] else 0
            for k, lv in enumerate(tree["levels"]):
                boxes[table[k, v]:table[k, v + 1]] = lv
        return boxes, flags

    def bvh_view_boxes(self, verts, vptr, view_mesh, faces, fptr, order, node_ptr, level_nodes, max_faces):
        self.calls.append("bvh_view_boxes")
        assert view_mesh.dtype == torch.int32 and verts.dtype == torch.float64 and verts.is_contiguous()
        table, totals, trees = self._view_trees(verts, vptr, view_mesh.numpy(), faces, fptr, order, node_ptr)
        nf = np.diff(self._ptr(fptr))[view_mesh.numpy()]
        assert list(level_nodes) == list(totals) and max_faces == (nf.max() if len(nf) else 0) <= self.BVH_MAX_FACES
        boxes, flags = self._view_boxes(table, totals, trees)
        return torch.from_numpy(boxes), torch.from_numpy(flags)

    def bvh_scan_visibility(self, verts, vptr, faces, fptr, cams, views, vis_eps, order, boxes, node_ptr, flags, want_visits=False):
        self.calls.append("bvh_scan_visibility")
        tables = self._tables(verts, vptr, faces, fptr, cams, views)
        table, totals, trees = self._view_trees(verts, vptr, views.numpy()[:, 0], faces, fptr, order, node_ptr)
        want_boxes, want_flags = self._view_boxes(table, totals, trees)
        assert so.same(boxes.numpy(), want_boxes) and so.same(flags.numpy(), want_flags)
        vis, visits, status = [], [], 0
        for tree, (_, _, cam, kind, W, H) in zip(trees, tables):
            w = vo.walk_scan(tree, cam, kind, W, H, vis_eps)
            vis.append(w["vis"]); visits.append(w["visits"])
            status |= self.SCAN_BAD_FACE if w["bad"] else 0
        cat = lambda xs, dtype: torch.from_numpy(np.concatenate(xs).astype(dtype) if xs else np.zeros(0, dtype=dtype))
        return cat(vis, np.uint8), torch.tensor([status], dtype=torch.int32), cat(visits, np.int32) if want_visits else None

    def _pairs(self, pos, vtx_ptr, bones, bone_ptr, off, n_pairs):
        vp, bp = self._ptr(vtx_ptr), self._ptr(bone_ptr)
        p, bn = self._f64(pos, 3), self._f64(bones, 6)
        assert off.dtype == torch.int64 and len(vp) == len(bp) == off.numel() and vp[-1] == len(p) and bp[-1] == len(bn)
        assert np.array_equal(off.numpy(), np.concatenate([[0], np.cumsum(np.diff(vp).astype(np.int64) * np.diff(bp))])) and n_pairs == off.numpy()[-1]
        return [(p[vp[b]:vp[b + 1]], bn[bp[b]:bp[b + 1]]) for b in range(len(vp) - 1)]

    def bone_visibility(self, pos, vtx_ptr, bones, bone_ptr, tri_pos, tp_ptr, faces, f_ptr, off, blk_ptr, n_blocks, n_pairs):
        self.calls.append("bone_visibility")
        pairs = self._pairs(pos, vtx_ptr, bones, bone_ptr, off, n_pairs)
        _, _, meshes = self._meshes(tri_pos, tp_ptr, faces, f_ptr)
        want = np.concatenate([[0], np.cumsum((np.diff(off.numpy()) + 255) // 256)])
        assert np.array_equal(self._ptr(blk_ptr), want) and n_blocks == want[-1] and len(meshes) == len(pairs)
        vis = [vo.brute_bone(p, bn, t, f)["vis"] for (p, bn), (t, f) in zip(pairs, meshes)]
        return torch.from_numpy(np.concatenate(vis))

    def bvh_bone_visibility(self, pos, vtx_ptr, bones, bone_ptr, tri_pos, tp_ptr, faces, f_ptr, off, n_pairs, order, boxes, node_ptr, flags,
                            want_visits=False):
        self.calls.append("bvh_bone_visibility")
        pairs = self._pairs(pos, vtx_ptr, bones, bone_ptr, off, n_pairs)
        trees = self._checked_trees(tri_pos, tp_ptr, faces, f_ptr, order, boxes, node_ptr, flags)
        assert len(trees) == len(pairs)
        walks = [vo.walk_bone(tree, p, bn) for (p, bn), tree in zip(pairs, trees)]
        status = self.BVH_BAD_FACE if any(w["bad"] for w in walks) else 0
        return (torch.from_numpy(np.concatenate([w["vis"] for w in walks])), torch.tensor([status], dtype=torch.int32),
                torch.from_numpy(np.concatenate([w["visits"] for w in walks])) if want_visits else None)
