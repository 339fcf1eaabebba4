"""NumPy emulation of the scan operators of morig_amd.native.NativeOps (csrc/scan.hip) and of ``fps``, for the CPU tests of the HOST logic
of morig_amd/scan.py: the view tables and ``view_mesh``, the [V, T, 3] -> per-view layout, the chunking, the ``n_pts`` errors, the
status handling, the frame column of the correspondences. Installed through ``runtime._test_ops``. It follows the kernels' contract in
include/morig_hip.h on CPU tensors; the arithmetic is that of tests/scan_oracle.py."""
import numpy as np
import torch

import point_oracle
import scan_oracle as so


class ScanOps:
    SCAN_MAX_SIDE, SCAN_ORTHOGRAPHIC, SCAN_PINHOLE, SCAN_CAM_DOUBLES, SCAN_VIEW_INTS, SCAN_BAD_FACE, SCAN_BLOCK = 1024, 0, 1, 16, 4, 1, 256

    def __init__(self):
        self.calls = []
        self.raster_views = []                                                   # the number of views of every scan_raster call

    @staticmethod
    def _ptr(p, dtype=torch.int32):
        assert p.dtype == dtype and p.dim() == 1 and p.is_contiguous()
        h = p.numpy()
        assert h[0] == 0 and np.all(np.diff(h) >= 0)
        return h

    def _tables(self, verts, vptr, faces, fptr, cams, views, kptr=None):
        vp, fp = self._ptr(vptr), self._ptr(fptr)
        nv = len(vp) - 1
        assert verts.dtype == torch.float64 and verts.dim() == 2 and verts.shape[1] == 3 and verts.is_contiguous() and verts.shape[0] == vp[-1]
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and faces.shape[0] == fp[-1]
        assert cams.dtype == torch.float64 and tuple(cams.shape) == (nv, 16) and views.dtype == torch.int32 and tuple(views.shape) == (nv, 4)
        vw = views.numpy()
        assert np.all((vw[:, 0] >= 0) & (vw[:, 0] < len(fp) - 1)) and np.all((vw[:, 3] == 0) | (vw[:, 3] == 1))
        if kptr is not None:
            kp = self._ptr(kptr, torch.int64)
            assert len(kp) == nv + 1 and np.array_equal(np.diff(kp), vw[:, 1].astype(np.int64) * vw[:, 2])
        out = []
        for v in range(nv):
            m = vw[v, 0]
            out.append((verts.numpy()[vp[v]:vp[v + 1]], faces.numpy()[fp[m]:fp[m + 1]].astype(np.int64), cams.numpy()[v], int(vw[v, 3]),
                        int(vw[v, 1]), int(vw[v, 2])))
        return out

    def scan_raster(self, verts, vptr, faces, fptr, mesh_nv, cams, views, kptr, wptr, min_side, max_side, n_pixels, n_work):
        self.calls.append("scan_raster")
        tables = self._tables(verts, vptr, faces, fptr, cams, views, kptr)
        self.raster_views.append(len(tables))
        vw, fp = views.numpy(), fptr.numpy()
        assert mesh_nv.dtype == torch.int32 and mesh_nv.numel() == len(fp) - 1
        assert min_side == vw[:, 1:3].min() and max_side == vw[:, 1:3].max() and 1 <= min_side and max_side <= self.SCAN_MAX_SIDE
        wp = self._ptr(wptr, torch.int64)
        assert np.array_equal(np.diff(wp), np.diff(fp)[vw[:, 0]]) and n_work == wp[-1] and n_pixels == kptr.numpy()[-1]
        status = 0
        for m in range(len(fp) - 1):
            f = faces.numpy()[fp[m]:fp[m + 1]]
            if f.size and (f.min() < 0 or f.max() >= mesh_nv.numpy()[m]):
                status = self.SCAN_BAD_FACE
        # the key image is not modelled: the emulated resolve renders again from the tables (the key rule lives in the oracle)
        return torch.full((int(n_pixels),), -1, dtype=torch.int64), torch.tensor([status], dtype=torch.int32)

    def scan_resolve(self, verts, vptr, faces, fptr, cams, views, kptr, keys):
        self.calls.append("scan_resolve")
        depth, face, point = [], [], []
        for v, f, cam, kind, W, H in self._tables(verts, vptr, faces, fptr, cams, views, kptr):
            f = np.clip(f, 0, max(len(v) - 1, 0))
            img = so.render(v, f if len(v) else f[:0], cam, kind, W, H)
            depth.append(img["depth"].reshape(-1))
            face.append(img["face"].reshape(-1))
            point.append(img["point"].reshape(-1, 3))
        depth, face, point = np.concatenate(depth), np.concatenate(face), np.concatenate(point)
        assert len(depth) == keys.numel()
        return (torch.from_numpy(depth), torch.from_numpy(face.astype(np.int32)), torch.from_numpy(point),
                torch.from_numpy((face >= 0).astype(np.int32)))

    def scan_compact(self, point, face, flags, rank, kptr, n_hits):
        self.calls.append("scan_compact")
        kp, fl = self._ptr(kptr, torch.int64), flags.numpy() != 0
        assert np.array_equal(rank.numpy(), np.cumsum(fl)) and n_hits == fl.sum()
        q = np.nonzero(fl)[0]
        seg = np.searchsorted(kp[1:], q, side="right")
        return (torch.from_numpy(point.numpy()[q]), torch.from_numpy((q - kp[seg]).astype(np.int32)), torch.from_numpy(face.numpy()[q]))

    def scan_visibility(self, verts, vptr, faces, fptr, cams, views, blk_ptr, n_blocks, vis_eps):
        self.calls.append("scan_visibility")
        vp = self._ptr(vptr)
        assert np.array_equal(self._ptr(blk_ptr), so_ptr((np.diff(vp) + 255) // 256)) and n_blocks == blk_ptr.numpy()[-1]
        vis = [so.visibility(v, np.clip(f, 0, max(len(v) - 1, 0)), cam, kind, W, H, vis_eps)[0]
               for v, f, cam, kind, W, H in self._tables(verts, vptr, faces, fptr, cams, views)]
        return torch.from_numpy(np.concatenate(vis) if vis else np.zeros(0, dtype=np.uint8))

    def scan_nearest(self, q, qptr, t, tptr, mask, blk_ptr, n_blocks):
        self.calls.append("scan_nearest")
        qp, tp = self._ptr(qptr), self._ptr(tptr)
        assert q.dtype == t.dtype == torch.float64 and q.shape[0] == qp[-1] and t.shape[0] == tp[-1] and len(qp) == len(tp)
        assert np.array_equal(self._ptr(blk_ptr), so_ptr((np.diff(qp) + 255) // 256)) and n_blocks == blk_ptr.numpy()[-1]
        assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == tp[-1])
        idx, d2 = np.full(qp[-1], -1, dtype=np.int32), np.full(qp[-1], np.inf)
        for b in range(len(qp) - 1):
            m = None if mask is None else mask.numpy()[tp[b]:tp[b + 1]]
            idx[qp[b]:qp[b + 1]], d2[qp[b]:qp[b + 1]] = so.nearest(q.numpy()[qp[b]:qp[b + 1]], t.numpy()[tp[b]:tp[b + 1]], m)
        return torch.from_numpy(idx), torch.from_numpy(d2)

    def fps(self, pos, ptr, out_ptr, start, n_clouds, max_cloud_points, n_samples):
        self.calls.append("fps")
        p, o = self._ptr(ptr), self._ptr(out_ptr)
        assert start is None and len(p) == len(o) == n_clouds + 1 and o[-1] == n_samples and np.diff(p).max() == max_cloud_points <= 32768
        assert np.all(np.diff(o) <= np.diff(p)) and pos.base.dtype == torch.float32 and pos.cols == 3
        return torch.from_numpy(point_oracle.fps(pos.base.numpy(), p, o).astype(np.int32))


def so_ptr(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int32)
