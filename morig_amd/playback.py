"""Motion playback: the reference's ``smooth_quats`` (evaluate/visualize_tracking.py:43-61), the only consumer of the ``pred_quats`` that
``tracking.track`` returns -- the quaternions are smoothed over time, turned into local frames, pushed through ``Rig.FK``
(utils/rig_parser.py:63-79) for every frame, and the bind-pose vertices are skinned into a vertex trajectory.

Every list argument has one entry per mesh (numpy arrays or tensors, on any device); meshes are ragged in J and V, a batch has ONE clip
length T. The batch runs in a fixed number of launches of csrc/playback.hip and the results are device tensors. ALL arithmetic is float64
in a fixed order without floating-point atomics: two runs give the same bits and a mesh alone gives the bits it gives inside a batch.

    smooth_quats        the smoothing passes alone (optionally with this product's sign alignment)
    pose_rigs           Rig.FK on a copy of the rig, for every frame at once
    skin_trajectory     local vertices and linear-blend skinning of every frame
    replay              smooth_quats of the reference, batched: (vtx_traj, quats)
    trajectory_errors   per-frame mean vertex distances; their means over the frames are the numbers of tracking.flow_errors

The reference writes the smoothed values into the caller's array; here the inputs are never written and new tensors are returned. The
one host read of a call is the status word per mesh (``trajectory_errors`` and ``smooth_quats`` read nothing).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .ragged import as_tensor, device_of, int32_table, ptr_of
from .runtime import get_ops
from .tracking import skin_entries, tree_order


# ------------------------------------------------------------------------------------------------------------------- the ragged tables
def _quat_batch(quats: Sequence, dev, joints: Optional[Sequence[int]] = None, what: str = "playback"):
    """-> (float64 [sum J, T, 4] on dev, J per mesh, T)"""
    qs = [as_tensor(q) for q in quats]
    if any(q.dim() != 3 or q.shape[2] != 4 for q in qs):
        raise ValueError(f"{what}: quats[m] is [J, T, 4] in (x, y, z, w) order")
    T = int(qs[0].shape[1])
    if any(int(q.shape[1]) != T for q in qs):
        raise ValueError(f"{what}: a batch has one T; got {[int(q.shape[1]) for q in qs]}")
    if joints is not None and any(int(q.shape[0]) != j for q, j in zip(qs, joints)):
        raise ValueError(f"{what}: quats[m] has one row per joint of rigs[m]; got {[int(q.shape[0]) for q in qs]} for {list(joints)} joints")
    Q = torch.cat([q.to(device=dev, dtype=torch.float64) for q in qs], 0).contiguous()
    return Q, [int(q.shape[0]) for q in qs], T


class RigTables:
    """The host side of a batch of rigs as device tables (uploads only, nothing is read back): ``jptr``; per joint row the parent (local,
    -1 at the root), ``tracking.tree_order``'s level order, the offset (``rig.offset`` with the root row replaced by ``rig.pos[root]``, as
    Rig.FK overwrites it) and the bind transform the rig holds (``global_transforms`` | ``pos``); per mesh whether ``rig.pos`` is float32
    and the root position."""

    def __init__(self, rigs: Sequence, dev, what: str):
        self.joints = [len(r.names) for r in rigs]
        if any(j < 1 for j in self.joints):
            raise ValueError(f"{what}: a rig has at least one joint")
        parent, order, offsets, bind, root = [], [], [], [], []
        for m, r in enumerate(rigs):
            hier = np.asarray(r.hierarchy).astype(np.int64).reshape(-1)
            try:
                o = tree_order(hier, int(r.root_id))[0]
            except ValueError as e:
                raise ValueError(f"{what}: mesh {m}: {e}") from None
            pos = np.asarray(r.pos)
            off = np.array(r.offset, dtype=np.float64)
            off[r.root_id] = pos[r.root_id]
            parent.append(np.where(np.arange(len(hier)) == r.root_id, -1, hier))
            order.append(o)
            offsets.append(off)
            bind.append(np.concatenate([np.asarray(r.global_transforms, dtype=np.float64).reshape(-1, 9), pos.astype(np.float64)], 1))
            root.append(pos[r.root_id])
        self.pos_dtypes = [torch.float32 if np.asarray(r.pos).dtype == np.float32 else torch.float64 for r in rigs]
        self.jptr_host = ptr_of(self.joints)
        self.jptr = int32_table(self.jptr_host, dev, what)
        self.parent, self.order = int32_table(np.concatenate(parent), dev, what), int32_table(np.concatenate(order), dev, what)
        self.offsets = torch.from_numpy(np.concatenate(offsets)).to(dev)
        self.bind = torch.from_numpy(np.ascontiguousarray(np.concatenate(bind))).to(dev)
        self.pos_f32 = torch.tensor([int(d == torch.float32) for d in self.pos_dtypes], dtype=torch.int32, device=dev)
        self.root = [np.asarray(p) for p in root]

    def root_positions(self, root_pos: Optional[Sequence], T: int, dev, what: str) -> torch.Tensor:
        """-> float64 [B, T, 3]: ``rig.pos[root]`` for every frame, or ``root_pos[m]`` rounded to the rig's position type"""
        rows = []
        for m, dt in enumerate(self.pos_dtypes):
            if root_pos is None or root_pos[m] is None:
                rows.append(torch.from_numpy(self.root[m].astype(np.float64)).to(dev).reshape(1, 3).expand(T, 3))
            else:
                p = as_tensor(root_pos[m]).to(dev)
                if tuple(p.shape) != (T, 3):
                    raise ValueError(f"{what}: root_pos[{m}] is [T, 3] = [{T}, 3], got {tuple(p.shape)}")
                rows.append(p.to(dt).to(torch.float64))
        return torch.stack(rows, 0).contiguous()


class SkinTables:
    """The skin entries of a batch, vertex-major and ascending joint inside a vertex: ``eptr`` int32 [sum V + 1], ``joint`` int32 [E]
    local to the mesh, ``weight`` float64 [E]. A rig's ``skin_entries_device`` (rigging.assemble_rigs(entries=True)) is used in place;
    otherwise the entries are the non-zeros of ``rig.skins``. ``vtx``: float64 [sum V, 3]."""

    def __init__(self, rigs: Sequence, vtx: Sequence, dev, what: str):
        vs = [as_tensor(v).reshape(-1, 3) for v in vtx]
        self.sizes = [int(v.shape[0]) for v in vs]
        self.vptr_host = ptr_of(self.sizes)
        self.vptr = int32_table(self.vptr_host, dev, what)
        self.vtx = torch.cat([v.to(device=dev, dtype=torch.float64) for v in vs], 0).contiguous()
        eptr, joint, weight, e_off = [], [], [], 0
        for m, r in enumerate(rigs):
            ent = getattr(r, "skin_entries_device", None)
            if ent is not None:
                vp, _, ej, w = (torch.as_tensor(t).to(dev) for t in ent)
            else:
                if len(r.skins) != self.sizes[m]:
                    raise ValueError(f"{what}: mesh {m}: {len(r.skins)} skin rows for {self.sizes[m]} vertices")
                vp, _, ej, w = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in skin_entries(r.skins))
            if vp.numel() != self.sizes[m] + 1 or ej.numel() != w.numel():
                raise ValueError(f"{what}: mesh {m}: skin entries for {vp.numel() - 1} vertices, {self.sizes[m]} given")
            eptr.append(vp[:-1].to(torch.int64) + e_off)
            joint.append(ej.to(torch.int32))
            weight.append(w.to(torch.float64))
            e_off += int(ej.numel())                                               # a shape, not a device read
        if e_off >= 2 ** 31:
            raise ValueError(f"{what}: more than 2^31 skin entries in one call")
        eptr.append(torch.full((1,), e_off, dtype=torch.int64, device=dev))
        self.eptr = torch.cat(eptr).to(torch.int32).contiguous()
        self.joint, self.weight = torch.cat(joint).contiguous(), torch.cat(weight).contiguous()


def _raise_status(status: torch.Tensor, ops, what: str) -> None:
    host = status.cpu().numpy()                                                    # THE host read of a call
    index = np.nonzero(host & ops.POSE_BAD_INDEX)[0].tolist()
    if index:
        raise ValueError(f"{what}: meshes {index}: a joint or parent index lies outside the rig; nothing of them was computed")
    quat = np.nonzero(host & ops.POSE_BAD_QUAT)[0].tolist()
    if quat:
        raise ValueError(f"{what}: meshes {quat}: a quaternion has zero or non-finite norm (scipy's Rotation.from_quat raises there)")


def _pose(rigs, quats, root_pos, passes: int, align_signs: bool, what: str, vtx=None):
    n = len(rigs)
    if len(quats) != n or (root_pos is not None and len(root_pos) != n) or (vtx is not None and len(vtx) != n):
        raise ValueError(f"{what}: one entry per mesh in every list")
    dev = device_of(*quats, *(vtx or []))
    ops = get_ops()
    rt = RigTables(rigs, dev, what)
    Q, _, T = _quat_batch(quats, dev, rt.joints, what)
    st = SkinTables(rigs, vtx, dev, what) if vtx is not None else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if st is None:
        ops.pose_validate(rt.jptr, rt.parent, rt.order, None, None, None, status)
    else:
        ops.pose_validate(rt.jptr, rt.parent, rt.order, st.vptr, st.eptr, st.joint, status)
    qs, R = ops.pose_quats(Q, rt.jptr, passes, align_signs, status)
    xf = ops.pose_fk(R, rt.jptr, rt.parent, rt.order, rt.offsets, rt.root_positions(root_pos, T, dev, what), rt.pos_f32, status)
    traj = None
    if st is not None:
        local = ops.pose_local(rt.bind, st.vtx, st.vptr, rt.jptr, st.eptr, st.joint, status)
        traj = ops.pose_skin(xf, rt.jptr, st.vptr, st.eptr, st.joint, st.weight, local, status)
    _raise_status(status, ops, what)
    return rt, st, qs, xf, traj


# ------------------------------------------------------------------------------------------------------------------- public functions
def smooth_quats(quats: Sequence, passes: int = 2, align_signs: bool = False) -> List[torch.Tensor]:
    """The smoothing loop of the reference's ``smooth_quats`` for a list of ``[J, T, 4]`` quaternion tracks in (x, y, z, w) order, taken
    as float64. One pass is ``q[:, 1:-1] = ((q[:, 1:-1] + 0.5 * q[:, 2:]) + 0.5 * q[:, :-2]) / 2.0`` with the right side read entirely
    from the pass before; frames 0 and T - 1 never change and T < 3 is a no-op. Nothing is renormalised (neither does the reference).
    ``align_signs`` (this product's own option): before the passes, frame t of a joint is negated when its dot product with the already
    aligned frame t - 1 is < 0 (an exact 0 keeps the sign) -- q and -q are one rotation, and the reference averages them as they come.
    -> NEW float64 device tensors [J, T, 4]; the caller's arrays are not written (the reference smooths in place)."""
    if len(quats) == 0:
        return []
    if int(passes) < 0:
        raise ValueError("smooth_quats: passes >= 0")
    dev = device_of(*quats)
    Q, joints, _ = _quat_batch(quats, dev, what="smooth_quats")
    jptr = ptr_of(joints)
    status = torch.zeros(len(joints), dtype=torch.int32, device=dev)
    out, _ = get_ops().pose_quats(Q, int32_table(jptr, dev, "smooth_quats"), int(passes), bool(align_signs), status, matrices=False)
    return [out[jptr[m]:jptr[m + 1]] for m in range(len(joints))]


def pose_rigs(rigs: Sequence, quats: Sequence, root_pos: Optional[Sequence] = None) -> List[tuple]:
    """``Rig.FK`` on a copy of every rig with ``local_frames = Rotation.from_quat(quats[:, t]).as_matrix()``, for all frames at once.
    Local frames: the matrix of q / |q|. Offsets: ``rig.offset`` with the root row replaced by ``rig.pos[root]``. The root keeps
    ``rig.pos[root]`` in every frame (the reference's replay drops the solver's translation) unless ``root_pos[m]`` [T, 3] gives it per
    frame. Positions are float64 products and sums rounded to the dtype of ``rig.pos`` on store; children read the rounded value.
    -> per mesh (global_transforms [J, T, 3, 3] float64, pos [J, T, 3] in the dtype of ``rig.pos``). Raises ValueError naming the meshes
    with a quaternion of zero or non-finite norm."""
    if len(rigs) == 0:
        return []
    rt, _, _, xf, _ = _pose(rigs, quats, root_pos, 0, False, "pose_rigs")
    return _split_transforms(rt, xf)


def _split_transforms(rt: RigTables, xf: torch.Tensor) -> List[tuple]:
    out = []
    for m, dt in enumerate(rt.pos_dtypes):
        x = xf[rt.jptr_host[m]:rt.jptr_host[m + 1]].permute(0, 2, 1)               # [J, T, 12]
        out.append((x[:, :, :9].reshape(x.shape[0], x.shape[1], 3, 3), x[:, :, 9:].to(dt)))
    return out


def skin_trajectory(rigs: Sequence, vtx: Sequence, quats: Sequence, root_pos: Optional[Sequence] = None) -> List[torch.Tensor]:
    """The skinning half of the reference's ``smooth_quats``: per skin entry (v, j, w) with w != 0 the local vertex
    ``inverse(rig.global_transforms_homogeneous)[j] [v; 1]`` (the inverse of whatever the rig holds, by adjugate / determinant), then
    ``out[v, t] = sum_j w (G[j, t] local)[0:3]`` over the posed rig of ``pose_rigs``, summed in ascending joint order from zero. A vertex
    without entries gives zeros. -> float64 [V, T, 3] per mesh on the device."""
    if len(rigs) == 0:
        return []
    _, st, _, _, traj = _pose(rigs, quats, root_pos, 0, False, "skin_trajectory", vtx=vtx)
    return [traj[st.vptr_host[m]:st.vptr_host[m + 1]] for m in range(len(rigs))]


def replay(rigs: Sequence, vtx: Sequence, quats: Sequence, smooth: bool = True, passes: int = 2, align_signs: bool = False,
           root_pos: Optional[Sequence] = None) -> List[tuple]:
    """``smooth_quats(mesh, rig, quats)`` of the reference for a list of meshes: ``vtx[m]`` are ``mesh.vertices``.
    -> per mesh (vtx_traj [V, T, 3] float64, quats [J, T, 4] float64 as smoothed), device tensors. ``smooth=False`` skips the passes."""
    if len(rigs) == 0:
        return []
    if int(passes) < 0:
        raise ValueError("replay: passes >= 0")
    rt, st, qs, _, traj = _pose(rigs, quats, root_pos, int(passes) if smooth else 0, bool(align_signs), "replay", vtx=vtx)
    return [(traj[st.vptr_host[m]:st.vptr_host[m + 1]], qs[rt.jptr_host[m]:rt.jptr_host[m + 1]]) for m in range(len(rigs))]


def trajectory_errors(pred: Sequence, gt: Sequence, gt_vismask: Sequence) -> List[tuple]:
    """Per mesh and frame the mean distance between ``pred[m]`` and ``gt[m]`` (aligned, both [V, T, 3]) -> (full [T], vis [T]) float64
    on the device: ``full`` over all vertices, ``vis`` the sum of distance * (gt_vismask > 0.5) over the count of gt_vismask > 0.5 (0 / 0
    is NaN, as in numpy). The means over the frames are the two numbers of ``tracking.flow_errors`` for the same frames (the second
    when every frame sees equally many vertices). Fixed-order sums, no host read."""
    n = len(pred)
    if len(gt) != n or len(gt_vismask) != n:
        raise ValueError("trajectory_errors: one entry per mesh in every list")
    if n == 0:
        return []
    dev = device_of(*pred, *gt)
    ps, gs, ms = [as_tensor(a) for a in pred], [as_tensor(a) for a in gt], [as_tensor(a) for a in gt_vismask]
    T = int(ps[0].shape[1]) if ps[0].dim() == 3 else -1
    for m in range(n):
        if ps[m].dim() != 3 or ps[m].shape[2] != 3 or int(ps[m].shape[1]) != T or ps[m].shape != gs[m].shape or tuple(ms[m].shape) != tuple(ps[m].shape[:2]):
            raise ValueError(f"trajectory_errors: mesh {m}: pred and gt are [V, T, 3] with one T per batch, gt_vismask [V, T]")
    cat = lambda ts, dt: (ts[0].to(device=dev, dtype=dt).contiguous() if n == 1 else torch.cat([t.to(device=dev, dtype=dt) for t in ts], 0).contiguous())
    vptr = ptr_of([int(p.shape[0]) for p in ps])
    vis = cat([(m.to(dev) > 0.5) for m in ms], torch.uint8)
    full, visible = get_ops().pose_traj_errors(cat(ps, torch.float64), cat(gs, torch.float64), vis,
                                               int32_table(vptr, dev, "trajectory_errors"))
    return [(full[m], visible[m]) for m in range(n)]
