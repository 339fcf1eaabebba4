"""NumPy emulation of the transfer operators of morig_amd.native.NativeOps (csrc/transfer.hip), for the CPU tests of the HOST logic of
morig_amd/transfer.py: the ragged tables, the sorted neighbour keys and their row pointer, the skin blocks of meshes with different joint
counts, the refusals, the status handling and the rigs that come back. Installed through ``runtime._test_ops``. It follows the kernels'
contract in include/morig_hip.h on CPU tensors; the arithmetic is that of tests/transfer_oracle.py, and the flood is the oracle's LOOP
run over the neighbour lists it decodes from the keys the host sorted."""
import numpy as np
import torch

import transfer_oracle as to

NO_KEY = np.iinfo(np.int64).max


class TransferOps:
    TRANSFER_BLOCK, TRANSFER_MAX_FLOOD, TRANSFER_BAD_FACE, TRANSFER_BAD_COORD, TRANSFER_NO_FACES = 256, 8192, 1, 2, 4

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

    def _blocks(self, blk_ptr, n_blocks, vp):
        want = np.concatenate([[0], np.cumsum((np.diff(vp) + 255) // 256)])
        assert np.array_equal(self._ptr(blk_ptr), want) and n_blocks == want[-1]

    def transfer_keys(self, faces, fptr, vptr, per_face, status):
        self.calls.append("transfer_keys")
        fp, vp = self._ptr(fptr), self._ptr(vptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fp[-1] == len(faces)
        assert per_face in (6, 15) and status.dtype == torch.int32 and status.numel() == len(vp) == len(fp)
        f = faces.numpy().astype(np.int64)
        keys = np.full((len(f), per_face), NO_KEY, dtype=np.int64)
        for b in range(len(vp) - 1):
            nv, fb = vp[b + 1] - vp[b], f[fp[b]:fp[b + 1]]
            for i, row in enumerate(fb):
                if row.min() < 0 or row.max() >= nv:
                    status[0] |= self.TRANSFER_BAD_FACE
                    continue
                pairs = [(row[k], row[(k + j) % 3]) for k in range(3) for j in (1, 2)]
                if per_face == 15:
                    pairs += [(row[c], fb[c][j]) if c < len(fb) and 0 <= fb[c][j] < nv else (0, 0) for c in range(3) for j in range(3)]
                keys[fp[b] + i] = [((vp[b] + v) << 32) | n if v != n else NO_KEY for v, n in pairs]
        return torch.from_numpy(keys.reshape(-1))

    def transfer_coincide(self, verts, vptr, blk_ptr, n_blocks, ori, optr, status):
        self.calls.append("transfer_coincide")
        vp, op, v, o = self._ptr(vptr), self._ptr(optr), self._f64(verts, 3), self._f64(ori, 3)
        self._blocks(blk_ptr, n_blocks, vp)
        assert len(vp) == len(op) == status.numel() and vp[-1] == len(v) and op[-1] == len(o)
        coin, near = np.full(len(v), -1, dtype=np.int32), np.full(len(v), -1, dtype=np.int32)
        for b in range(len(vp) - 1):
            vb, ob = v[vp[b]:vp[b + 1]], o[op[b]:op[b + 1]]
            if len(vb) == 0:
                continue
            if not (np.all(np.abs(vb) <= 1e7) and np.all(np.abs(ob) <= 1e7)):                           # NaN compares false
                status[0] |= self.TRANSFER_BAD_COORD
            coin[vp[b]:vp[b + 1]], near[vp[b]:vp[b + 1]] = to.coincide(vb, ob)
        return torch.from_numpy(coin), torch.from_numpy(near)

    def transfer_flood(self, verts, vptr, max_verts, rowptr, keys, coin, near, use_nearest, status):
        self.calls.append("transfer_flood")
        vp, v, rp, k = self._ptr(vptr), self._f64(verts, 3), self._ptr(rowptr), keys.numpy()
        counts = np.diff(vp)
        assert max_verts == counts.max() <= self.TRANSFER_MAX_FLOOD and len(rp) == len(v) + 1 and status.numel() == len(vp)
        assert keys.dtype == torch.int64 and np.all(np.diff(k) >= 0)                                    # sorted
        assert np.array_equal(rp, np.searchsorted(k, np.arange(len(v) + 1, dtype=np.int64) << 32))
        assert np.all(k[rp[-1]:] == NO_KEY) and np.all(k[:rp[-1]] >> 32 == np.repeat(np.arange(len(v)), np.diff(rp)))
        source, sweep = np.full(len(v), -1, dtype=np.int32), np.full(len(v), -1, dtype=np.int32)
        c, n = coin.numpy().astype(np.int64), near.numpy().astype(np.int64)
        for b in range(len(vp) - 1):
            v0, nv = vp[b], counts[b]
            vb = v[v0:v0 + nv]
            nbrs = [np.unique(k[rp[v0 + i]:rp[v0 + i + 1]] & 0xffffffff) for i in range(nv)]
            filled = c[v0:v0 + nv] >= 0
            src, sw, k_sweep = c[v0:v0 + nv].copy(), np.where(filled, 0, -1), 0
            while not filled.all():                                                                      # transfer_oracle.remesh_loop
                k_sweep += 1
                progress = False
                for i in np.argwhere(~filled).squeeze(axis=1):
                    if filled[nbrs[i]].sum() > 0:
                        best, nn = 1e8, -1
                        for u in nbrs[i]:
                            if filled[u]:
                                d = np.sqrt(to.dist2(vb[i], vb[u]))
                                if d < best:
                                    best, nn = d, u
                        src[i], filled[i], sw[i], progress = src[nn], True, k_sweep, True
                if not progress:
                    break
            if use_nearest:
                src[~filled] = n[v0:v0 + nv][~filled]
            source[v0:v0 + nv], sweep[v0:v0 + nv] = src, sw
            status[1 + b] += int((src < 0).sum())
        return torch.from_numpy(source), torch.from_numpy(sweep)

    def transfer_closest(self, dst, dptr, blk_ptr, n_blocks, verts, vptr, faces, fptr, status):
        self.calls.append("transfer_closest")
        dp, vp, fp, d, v = self._ptr(dptr), self._ptr(vptr), self._ptr(fptr), self._f64(dst, 3), self._f64(verts, 3)
        self._blocks(blk_ptr, n_blocks, dp)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert len(dp) == len(vp) == len(fp) and dp[-1] == len(d) and vp[-1] == len(v) and fp[-1] == len(faces) and status.dtype == torch.int32
        face, bary, dist = np.full(len(d), -1, dtype=np.int32), np.full((len(d), 3), np.nan), np.full(len(d), np.nan)
        for b in range(len(dp) - 1):
            vb, fb = v[vp[b]:vp[b + 1]], faces.numpy()[fp[b]:fp[b + 1]].astype(np.int64)
            if dp[b + 1] == dp[b]:
                continue
            if fb.size and (fb.min() < 0 or fb.max() >= len(vb)):
                status[0] |= self.TRANSFER_BAD_FACE
                fb = np.clip(fb, 0, max(len(vb) - 1, 0)) if len(vb) else fb[:0]
            if len(fb) == 0:
                status[0] |= self.TRANSFER_NO_FACES
            face[dp[b]:dp[b + 1]], bary[dp[b]:dp[b + 1]], dist[dp[b]:dp[b + 1]], _ = to.closest_face(d[dp[b]:dp[b + 1]], vb, fb)
        return torch.from_numpy(face), torch.from_numpy(bary), torch.from_numpy(dist)

    def transfer_rows(self, skins, skin_ptr, joints, src_vptr, vptr, blk_ptr, n_blocks, pick, out_ptr, n_out, faces=None, fptr=None, bary=None):
        self.calls.append("transfer_rows")
        sp, svp, vp, op, s = self._ptr(skin_ptr), self._ptr(src_vptr), self._ptr(vptr), self._ptr(out_ptr), self._f64(skins)
        self._blocks(blk_ptr, n_blocks, vp)
        J = joints.numpy().astype(np.int64)
        assert joints.dtype == torch.int32 and np.array_equal(np.diff(sp), np.diff(svp) * J) and np.array_equal(np.diff(op), np.diff(vp) * J)
        assert sp[-1] == len(s) and op[-1] == n_out and pick.dtype == torch.int32 and pick.numel() == vp[-1]
        out, k = np.zeros(n_out), pick.numpy().astype(np.int64)
        for b in range(len(vp) - 1):
            S = s[sp[b]:sp[b + 1]].reshape(-1, J[b])
            kb = k[vp[b]:vp[b + 1]]
            if bary is None:
                rows = to.gather_rows(S, kb)
            else:
                fb = np.clip(faces.numpy()[self._ptr(fptr)[b]:self._ptr(fptr)[b + 1]].astype(np.int64), 0, max(len(S) - 1, 0))
                rows = to.blend_rows(S, fb, kb, self._f64(bary, 3)[vp[b]:vp[b + 1]]) if len(S) else np.zeros((len(kb), J[b]))
            out[op[b]:op[b + 1]] = rows.reshape(-1)
        return torch.from_numpy(out)
