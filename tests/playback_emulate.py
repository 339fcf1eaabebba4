"""NumPy emulation of the playback operators of morig_amd.native.NativeOps (csrc/playback.hip), for the CPU tests of the HOST logic of
morig_amd/playback.py: the ragged tables, the tree-order tables, the entries taken from a rig, the slicing of the results, the status
handling. Installed through ``runtime._test_ops``. It follows the kernels' contract in include/morig_hip.h on CPU tensors; the arithmetic
is that of tests/playback_oracle.py."""
import numpy as np
import torch

import playback_oracle as po


class PlaybackOps:
    POSE_BAD_QUAT, POSE_BAD_INDEX, POSE_FRAME_TILE = 1, 2, 64

    def __init__(self):
        self.calls = []

    @staticmethod
    def _ptr(p):
        assert p.dtype == torch.int32 and p.dim() == 1 and p.is_contiguous()
        h = p.numpy()
        assert h[0] == 0 and np.all(np.diff(h) >= 0)
        return h

    def pose_validate(self, jptr, parent, order, vptr, eptr, ent_joint, status):
        self.calls.append("pose_validate")
        jp = self._ptr(jptr)
        assert parent.dtype == torch.int32 and parent.numel() == jp[-1] and status.dtype == torch.int32 and status.numel() == len(jp) - 1
        par, st = parent.numpy(), status.numpy()
        for b in range(len(jp) - 1):
            J = jp[b + 1] - jp[b]
            p = par[jp[b]:jp[b + 1]]
            bad = np.any((p < -1) | (p >= J))
            if order is not None:
                o = order.numpy()[jp[b]:jp[b + 1]]
                bad = bad or np.any((o < 0) | (o >= J))
            if eptr is not None:
                vp, ep, ej = self._ptr(vptr), eptr.numpy(), ent_joint.numpy()
                assert eptr.dtype == ent_joint.dtype == torch.int32 and eptr.numel() == vp[-1] + 1
                for v in range(vp[b], vp[b + 1]):
                    if ep[v] < 0 or ep[v + 1] < ep[v] or ep[v + 1] > len(ej):
                        bad = True
                    else:
                        j = ej[ep[v]:ep[v + 1]]
                        bad = bad or np.any((j < 0) | (j >= J))
            if bad:
                st[b] |= self.POSE_BAD_INDEX

    def pose_quats(self, quats, jptr, passes, align_signs, status, matrices=True):
        self.calls.append("pose_quats")
        jp = self._ptr(jptr)
        assert quats.dtype == torch.float64 and quats.dim() == 3 and quats.shape[2] == 4 and quats.is_contiguous() and quats.shape[0] == jp[-1]
        nj, T = quats.shape[:2]
        out, R, st = np.zeros((nj, T, 4)), np.zeros((nj, 9, T)), status.numpy()
        for b in range(len(jp) - 1):
            if st[b] & self.POSE_BAD_INDEX:
                continue
            rows = slice(jp[b], jp[b + 1])
            out[rows] = po.smooth(quats.numpy()[rows], passes, align_signs)
            if matrices:
                with np.errstate(all="ignore"):
                    n = np.sqrt(po.dot4(out[rows], out[rows]))
                ok = (n > 0.0) & np.isfinite(n)
                if not ok.all():
                    st[b] |= self.POSE_BAD_QUAT
                m = po.quat_matrices(np.where(ok[..., None], out[rows], np.array([0.0, 0.0, 0.0, 1.0])))
                R[rows] = m.reshape(-1, T, 9).transpose(0, 2, 1)
        return torch.from_numpy(out), (torch.from_numpy(R) if matrices else None)

    def pose_fk(self, R, jptr, parent, order, offsets, root_pos, pos_f32, status):
        self.calls.append("pose_fk")
        jp = self._ptr(jptr)
        nj, _, T = R.shape
        B = len(jp) - 1
        assert R.dtype == offsets.dtype == root_pos.dtype == torch.float64 and tuple(R.shape) == (jp[-1], 9, T)
        assert tuple(offsets.shape) == (nj, 3) and tuple(root_pos.shape) == (B, T, 3) and pos_f32.dtype == torch.int32 and pos_f32.numel() == B
        xf, par, ordr = np.zeros((nj, 12, T)), parent.numpy(), order.numpy()
        for b in range(B):
            if status.numpy()[b] & self.POSE_BAD_INDEX:
                continue
            j0, J = jp[b], jp[b + 1] - jp[b]
            p = par[j0:j0 + J]
            assert sorted(ordr[j0:j0 + J]) == list(range(J))
            seen = set()
            for j in ordr[j0:j0 + J]:                                          # parent first
                assert p[j] < 0 or p[j] in seen
                seen.add(j)
            root = int(np.nonzero(p < 0)[0][0])
            dt = np.float32 if pos_f32.numpy()[b] else np.float64
            rp = root_pos.numpy()[b]
            assert np.array_equal(rp.astype(dt).astype(np.float64), rp)        # already rounded to the rig's type
            rig = dict(pos=np.zeros((J, 3), dtype=dt), hierarchy=p, root_id=root, offset=offsets.numpy()[j0:j0 + J])
            G, pos = po.fk(rig, R.numpy()[j0:j0 + J].transpose(0, 2, 1).reshape(J, T, 3, 3), root_pos=rp)
            xf[j0:j0 + J, :9] = G.reshape(J, T, 9).transpose(0, 2, 1)
            xf[j0:j0 + J, 9:] = pos.astype(np.float64).transpose(0, 2, 1)
        return torch.from_numpy(xf)

    def _entries(self, vptr, eptr, b):
        vp, ep = self._ptr(vptr), eptr.numpy()
        counts = np.diff(ep[vp[b]:vp[b + 1] + 1])
        return vp[b], np.repeat(np.arange(vp[b + 1] - vp[b]), counts), slice(ep[vp[b]], ep[vp[b + 1]])

    def pose_local(self, bind, vtx, vptr, jptr, eptr, ent_joint, status):
        self.calls.append("pose_local")
        jp = self._ptr(jptr)
        assert bind.dtype == vtx.dtype == torch.float64 and tuple(bind.shape) == (jp[-1], 12) and vtx.shape[1] == 3
        local = np.zeros((ent_joint.numel(), 3))
        for b in range(len(jp) - 1):
            if status.numpy()[b] & self.POSE_BAD_INDEX:
                continue
            v0, ev, es = self._entries(vptr, eptr, b)
            bt = bind.numpy()[jp[b]:jp[b + 1]]
            rig = dict(global_transforms=bt[:, :9].reshape(-1, 3, 3), pos=bt[:, 9:])
            local[es] = po.local_vertices(rig, vtx.numpy()[v0:], ev, ent_joint.numpy()[es])
        return torch.from_numpy(local)

    def pose_skin(self, xf, jptr, vptr, eptr, ent_joint, ent_weight, local, status):
        self.calls.append("pose_skin")
        jp, vp = self._ptr(jptr), self._ptr(vptr)
        T = xf.shape[2]
        assert xf.dtype == ent_weight.dtype == local.dtype == torch.float64 and tuple(xf.shape) == (jp[-1], 12, T)
        out = np.zeros((vp[-1], T, 3))
        for b in range(len(jp) - 1):
            if status.numpy()[b] & self.POSE_BAD_INDEX:
                continue
            v0, ev, es = self._entries(vptr, eptr, b)
            x = xf.numpy()[jp[b]:jp[b + 1]].transpose(0, 2, 1)
            J = x.shape[0]
            out[v0:vp[b + 1]] = po.skin(x[:, :, :9].reshape(J, T, 3, 3), x[:, :, 9:], local.numpy()[es], ev, ent_joint.numpy()[es],
                                        ent_weight.numpy()[es], vp[b + 1] - v0)
        return torch.from_numpy(out)

    def pose_traj_errors(self, pred, gt, vis, vptr):
        self.calls.append("pose_traj_errors")
        vp = self._ptr(vptr)
        assert pred.dtype == gt.dtype == torch.float64 and vis.dtype == torch.uint8 and pred.shape == gt.shape and tuple(vis.shape) == tuple(pred.shape[:2])
        T = pred.shape[1]
        full, visible = np.zeros((len(vp) - 1, T)), np.zeros((len(vp) - 1, T))
        for b in range(len(vp) - 1):
            rows = slice(vp[b], vp[b + 1])
            full[b], visible[b] = po.trajectory_errors(pred.numpy()[rows], gt.numpy()[rows], vis.numpy()[rows])
        return torch.from_numpy(full), torch.from_numpy(visible)


# ------------------------------------------------------------------------------------------------------------------- fixture helpers
def make_rig(case, entries_device=None):
    """a formats.Rig in the state the fixture recorded (pos, offset and global_transforms as the reference's rig held them)"""
    from morig_amd.formats import Rig
    rig = Rig.from_arrays(case["pos"], case["hier"], int(case["root_id"]), skins=case["skins"])
    rig.pos, rig.offset, rig.global_transforms = case["pos"].copy(), case["offset"].copy(), case["bind_G"].copy()
    if entries_device is not None:
        rig.skin_entries_device = entries_device
    return rig


def stretch(quats, T):
    """the track repeated along t to T frames (the ragged batch of the tests needs one T for rigs recorded at different ones)"""
    q = np.asarray(quats)
    return np.ascontiguousarray(np.concatenate([q] * (T // q.shape[1] + 1), 1)[:, :T])
