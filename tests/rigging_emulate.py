"""NumPy emulation of the rig-assembly operators of morig_amd.native.NativeOps (csrc/rig_assemble.hip), for the CPU tests of the HOST
logic of morig_amd/rigging.py: the plan builder, the CSR tables and their concatenation over a batch, the slicing of the results.
Installed through ``runtime._test_ops``. It walks the tables exactly as the kernels' contract in include/morig_hip.h states."""
import numpy as np
import torch


class RigOps:
    RIG_RAW = 1

    def __init__(self):
        self.calls = []
        self.last_W = None

    @staticmethod
    def _mesh_of(vtx_ptr, v):
        m = int(np.searchsorted(vtx_ptr, v, side="right")) - 1
        return m if 0 <= m < len(vtx_ptr) - 1 and vtx_ptr[m] <= v < vtx_ptr[m + 1] else -1

    def rig_assemble(self, W, vtx_ptr, joint_ptr, seg_ptr, bone_ptr, bones, ld_out, raw=False):
        self.calls.append("rig_assemble")
        self.last_W = W
        assert W.dtype == torch.float64 and W.dim() == 2 and (W.shape[1] == 0 or W.stride(1) == 1)
        assert all(t.dtype == torch.int32 and t.dim() == 1 for t in (vtx_ptr, joint_ptr, seg_ptr, bone_ptr, bones))
        assert joint_ptr.numel() == vtx_ptr.numel() and seg_ptr.numel() == int(joint_ptr[-1]) + 1 and bone_ptr.numel() == int(seg_ptr[-1]) + 1
        assert bones.numel() == int(bone_ptr[-1]) and int(vtx_ptr[-1]) == W.shape[0]
        w, vp, jp, sp, bp, bn = (t.numpy() for t in (W, vtx_ptr, joint_ptr, seg_ptr, bone_ptr, bones))
        out = np.zeros((W.shape[0], ld_out))
        for v in range(W.shape[0]):
            m = self._mesh_of(vp, v)
            if m < 0:
                continue
            for j in range(jp[m + 1] - jp[m]):
                g = jp[m] + j
                total = None
                for s in range(sp[g], sp[g + 1]):
                    val = 0.0
                    for k in range(bp[s], bp[s + 1]):
                        assert 0 <= bn[k] < W.shape[1]
                        if raw or w[v, bn[k]] > 1e-5:
                            val = w[v, bn[k]]
                    total = val if total is None else total + val
                out[v, j] = 0.0 if total is None else total
        return torch.from_numpy(out)

    def rig_skin_counts(self, x, vtx_ptr):
        self.calls.append("rig_skin_counts")
        assert x.dtype == torch.float64 and x.is_contiguous() and vtx_ptr.dtype == torch.int32
        return torch.from_numpy((x.numpy() != 0).sum(axis=1).astype(np.int32))

    def rig_skin_fill(self, x, vtx_ptr, ent_ptr, n_entries):
        self.calls.append("rig_skin_fill")
        assert ent_ptr.dtype == torch.int32 and ent_ptr.numel() == x.shape[0] + 1 and int(ent_ptr[-1]) == n_entries
        a, vp = x.numpy(), vtx_ptr.numpy()
        ev, ej = np.nonzero(a)
        assert np.array_equal(np.bincount(ev, minlength=len(a)), np.diff(ent_ptr.numpy()))
        local = np.array([v - vp[self._mesh_of(vp, v)] if self._mesh_of(vp, v) >= 0 else -1 for v in ev], dtype=np.int32)
        return torch.from_numpy(local), torch.from_numpy(ej.astype(np.int32)), torch.from_numpy(a[ev, ej])
