"""NumPy emulation of the simplification operators of morig_amd.native.NativeOps (csrc/simplify.hip) with ``mesh_bbox`` and
``tpl_edge_flags``, for the CPU tests of the HOST logic of ``morig_amd.meshprep.simplify``: the bisection with a resolution per mesh,
the launch groups under the 21-bit limit, the pass-through, the list shapes and the error texts. Installed through
``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors; the arithmetic of a cell is that of
tests/simplify_oracle.py (every sum sequential)."""
import numpy as np
import torch

import simplify_oracle as so

INT64_MAX = np.iinfo(np.int64).max


class SimplifyOps:
    SIMPLIFY_MAX_RES, SIMPLIFY_INDEX_BITS, SIMPLIFY_MAX_INDEX, SIMPLIFY_MESH_SHIFT = 1024, 21, 1 << 21, 30

    def __init__(self):
        self.calls = []
        self.launch_meshes = []                                                  # the number of meshes of every simplify_cell_keys call
        self.launch_res = []                                                     # and their resolutions

    @staticmethod
    def _ptr(p):
        assert p.dtype == torch.int32 and p.dim() == 1 and p.is_contiguous()
        h = p.numpy().astype(np.int64)
        assert h[0] == 0 and np.all(np.diff(h) >= 0)
        return h

    def _mesh(self, verts, vptr, faces=None, fptr=None):
        vp = self._ptr(vptr)
        assert verts.dtype == torch.float64 and verts.dim() == 2 and verts.shape[1] == 3 and verts.is_contiguous() and verts.shape[0] == vp[-1]
        if faces is None:
            return vp
        fp = self._ptr(fptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and faces.shape[0] == fp[-1]
        assert len(fp) == len(vp)
        return vp, fp

    def _frame(self, frame, res, B, min_res, max_res):
        assert frame.dtype == torch.float64 and tuple(frame.shape) == (B, 4) and res.dtype == torch.int32 and tuple(res.shape) == (B,)
        r = res.numpy()
        assert min_res == r.min() and max_res == r.max() and 1 <= min_res and max_res <= self.SIMPLIFY_MAX_RES
        return frame.numpy(), r.astype(np.int64)

    def mesh_bbox(self, verts, vptr):
        self.calls.append("mesh_bbox")
        vp = self._mesh(verts, vptr)
        v = verts.numpy()
        return torch.from_numpy(np.array([np.concatenate([v[vp[b]:vp[b + 1]].min(0), v[vp[b]:vp[b + 1]].max(0)]) for b in range(len(vp) - 1)]))

    def simplify_cell_keys(self, verts, vptr, frame, res, min_res, max_res):
        self.calls.append("simplify_cell_keys")
        vp = self._mesh(verts, vptr)
        fr, r = self._frame(frame, res, len(vp) - 1, min_res, max_res)
        assert verts.shape[0] <= self.SIMPLIFY_MAX_INDEX
        self.launch_meshes.append(len(vp) - 1)
        self.launch_res.append(r.tolist())
        keys = np.zeros(vp[-1], dtype=np.int64)
        for b in range(len(vp) - 1):
            g = (verts.numpy()[vp[b]:vp[b + 1]] - fr[b, :3]) / fr[b, 3] * r[b]
            c = np.clip(np.floor(g).astype(np.int64), 0, r[b] - 1)
            keys[vp[b]:vp[b + 1]] = (b << self.SIMPLIFY_MESH_SHIFT) | ((c[:, 0] * r[b] + c[:, 1]) * r[b] + c[:, 2])
        return torch.from_numpy(keys)

    def tpl_edge_flags(self, keys):
        self.calls.append("tpl_edge_flags")
        assert keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
        k = keys.numpy()
        assert np.all(np.diff(k) >= 0)
        first = np.ones(len(k), dtype=bool)
        first[1:] = k[1:] != k[:-1]
        return torch.from_numpy((first & (k != INT64_MAX)).astype(np.int32))

    def _cells_of(self, faces, fp, vp, cell):
        f = faces.numpy().astype(np.int64)
        off = np.repeat(vp[:-1], np.diff(fp))
        return cell.numpy().astype(np.int64)[f + off[:, None]]

    def simplify_face_keys(self, faces, fptr, vptr, cell, n_cells):
        self.calls.append("simplify_face_keys")
        vp, fp = self._ptr(vptr), self._ptr(fptr)
        assert cell.dtype == torch.int32 and cell.numel() == vp[-1] and cell.numel() <= self.SIMPLIFY_MAX_INDEX and n_cells <= self.SIMPLIFY_MAX_INDEX
        c = self._cells_of(faces, fp, vp, cell)
        assert c.size == 0 or (c.min() >= 0 and c.max() < n_cells)
        s = np.sort(c, 1)
        keys = (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2]
        keys[(s[:, 0] == s[:, 1]) | (s[:, 1] == s[:, 2])] = INT64_MAX
        return torch.from_numpy(c.reshape(-1).astype(np.int32)), torch.from_numpy(keys)

    def simplify_face_compact(self, faces, fptr, vptr, cell, cptr, order, flags, rank, n_out):
        self.calls.append("simplify_face_compact")
        vp, fp, cp = self._ptr(vptr), self._ptr(fptr), self._ptr(cptr)
        fl = flags.numpy() != 0
        assert np.array_equal(rank.numpy(), np.cumsum(fl)) and n_out == fl.sum() and order.dtype == torch.int64
        f = order.numpy()[fl]
        c = self._cells_of(faces, fp, vp, cell)[f]
        first = np.argmin(c, 1)
        rot = np.stack([c[np.arange(len(c)), (first + k) % 3] for k in range(3)], 1).reshape(-1, 3)
        mesh = np.searchsorted(fp[1:], f, side="right")
        return torch.from_numpy(rot - cp[mesh][:, None])

    def simplify_quadrics(self, verts, vptr, faces, fptr, frame, res, min_res, max_res, cell_key, mptr, members, kptr, corners):
        self.calls.append("simplify_quadrics")
        vp, fp = self._mesh(verts, vptr, faces, fptr)
        fr, r = self._frame(frame, res, len(vp) - 1, min_res, max_res)
        n = cell_key.numel()
        assert mptr.numel() == kptr.numel() == n + 1 and members.numel() == vp[-1] and corners.numel() == 3 * fp[-1]
        v, f = verts.numpy(), faces.numpy().astype(np.int64)
        key, mp, kp, mem, cor = cell_key.numpy(), mptr.numpy(), kptr.numpy(), members.numpy(), corners.numpy()
        out = np.zeros((n, 3))
        for q in range(n):
            b, ck = int(key[q] >> self.SIMPLIFY_MESH_SHIFT), int(key[q] & ((1 << self.SIMPLIFY_MESH_SHIFT) - 1))
            c = np.array([ck // (r[b] * r[b]), (ck // r[b]) % r[b], ck % r[b]])
            h = fr[b, 3] / r[b]
            ms = mem[mp[q]:mp[q + 1]]
            assert np.all(np.diff(ms) > 0) and np.all((ms >= vp[b]) & (ms < vp[b + 1]))
            cs = cor[kp[q]:kp[q + 1]]
            assert np.all(np.diff(cs) > 0)
            tris = [tuple(v[vp[b] + i].tolist() for i in f[x // 3]) for x in cs]
            out[q] = so.cell_position([v[i].tolist() for i in ms], tris, fr[b, :3] + c * h, fr[b, :3] + (c + 1) * h)
        return torch.from_numpy(out)
