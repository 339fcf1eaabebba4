"""NumPy emulation of the bone-ray operators of morig_amd.native.NativeOps (csrc/labels.hip) and of ``nearest_point``, for the CPU tests of
the HOST logic of morig_amd/labels.py: the ray plan, the ragged tables, the refusals, the status handling, the per-mesh views and the file
round trips. Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors; the
arithmetic is that of tests/labels_oracle.py."""
import numpy as np
import torch

import labels_oracle as lo


class LabelOps:
    RAY_MAX_PER_JOINT, RAY_BAD_FACE, RAY_BAD_TABLE, RAY_STATS, RAY_BLOCK = 1024, 1, 2, 4, 256

    def __init__(self):
        self.calls = []

    @staticmethod
    def _ptr(p):
        assert p.dtype == torch.int32 and p.dim() == 1 and p.is_contiguous()
        h = p.numpy().astype(np.int64)
        assert h[0] == 0 and np.all(np.diff(h) >= 0)
        return h

    @staticmethod
    def _f64(t, cols=None):
        assert t.dtype == torch.float64 and t.is_contiguous() and (t.dim() == 1 if cols is None else (t.dim() == 2 and t.shape[1] == cols))
        return t.numpy()

    def ray_cast(self, origins, dirs, ray_ptr, verts, vptr, faces, fptr, orientation):
        self.calls.append("ray_cast")
        rp, vp, fp = self._ptr(ray_ptr), self._ptr(vptr), self._ptr(fptr)
        o, d, v = self._f64(origins, 3), self._f64(dirs, 3), self._f64(verts, 3)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert len(rp) == len(vp) == len(fp) and rp[-1] == len(o) == len(d) and vp[-1] == len(v) and fp[-1] == len(faces)
        assert orientation in (-1, 0, 1)
        t, face, point, status = np.full(len(o), np.inf), np.full(len(o), -1, dtype=np.int32), np.full((len(o), 3), np.nan), 0
        for b in range(len(rp) - 1):
            vb, fb = v[vp[b]:vp[b + 1]], faces.numpy()[fp[b]:fp[b + 1]].astype(np.int64)
            if rp[b + 1] == rp[b]:
                continue
            if fb.size and (fb.min() < 0 or fb.max() >= len(vb)):
                status |= self.RAY_BAD_FACE
                fb = np.clip(fb, 0, max(len(vb) - 1, 0)) if len(vb) else fb[:0]
            c = lo.cast(o[rp[b]:rp[b + 1]], d[rp[b]:rp[b + 1]], vb, fb, orientation)
            t[rp[b]:rp[b + 1]], face[rp[b]:rp[b + 1]], point[rp[b]:rp[b + 1]] = c["t"], c["face"], c["point"]
        return torch.from_numpy(t), torch.from_numpy(face), torch.from_numpy(point), torch.tensor([status], dtype=torch.int32)

    def ray_select(self, t, joint_ptr, max_rays, keep_factor, fill):
        self.calls.append("ray_select")
        jp, tt = self._ptr(joint_ptr), self._f64(t)
        counts = np.diff(jp)
        assert jp[-1] == len(tt) and max_rays == (counts.max() if len(counts) else 0) and max_rays <= self.RAY_MAX_PER_JOINT
        s = lo.select(tt, counts, keep_factor, fill)
        stats = np.stack([s["n_hit"].astype(np.float64), s["n_kept"].astype(np.float64), s["p20"], s["featuresize"]], 1).reshape(-1, 4)
        return torch.from_numpy(s["kept"]), torch.from_numpy(stats)

    def ray_attention(self, verts, vptr, blk_ptr, n_blocks, point, kept, ray_ptr, radius):
        self.calls.append("ray_attention")
        vp, rp, v, p = self._ptr(vptr), self._ptr(ray_ptr), self._f64(verts, 3), self._f64(point, 3)
        want_blk = np.concatenate([[0], np.cumsum((np.diff(vp) + 255) // 256)])
        assert np.array_equal(self._ptr(blk_ptr), want_blk) and n_blocks == want_blk[-1] and len(rp) == len(vp)
        assert kept.dtype == torch.uint8 and kept.numel() == len(p) == rp[-1] and radius >= 0.0
        out = [lo.attention(v[vp[b]:vp[b + 1]], p[rp[b]:rp[b + 1]], kept.numpy()[rp[b]:rp[b + 1]], radius)[0] for b in range(len(vp) - 1)]
        return torch.from_numpy(np.concatenate(out) if out else np.zeros(0, dtype=np.float32))

    def nearest_point(self, q, q_ptr, pts, p_ptr, squared):
        self.calls.append("nearest_point")
        qp, pp, qq, p = self._ptr(q_ptr), self._ptr(p_ptr), self._f64(q, 3), self._f64(pts, 3)
        assert squared and len(qp) == len(pp)
        out = np.zeros(len(qq), dtype=np.int32)
        for b in range(len(qp) - 1):
            dx, dy, dz = (qq[qp[b]:qp[b + 1], None, k] - p[None, pp[b]:pp[b + 1], k] for k in range(3))
            out[qp[b]:qp[b + 1]] = np.argmin((dx * dx + dy * dy) + dz * dz, 1) if pp[b + 1] > pp[b] else -1
        return torch.from_numpy(out)
