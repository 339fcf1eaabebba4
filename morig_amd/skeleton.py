"""Skeleton connection on the MI355X-native op layer (csrc/skeleton.hip): what evaluate/joint2rig.py:197-304 does between the joint
extraction and the skinning stage -- ``create_one_data``'s pair attributes, ``predict_skeleton``'s cost matrix (with
utils/mst_utils.py:269-291, ``increase_cost_for_outside_bone``) and ``primMST`` (:63-108) -- for a batch of meshes at once.

Meshes of a batch are contiguous joint ranges (``joints_batch`` is sorted, as PyG batches it); ``pairs`` index the concatenated
joints, so the reference's own forwards (``data.joints[data.pairs[:, 0].long()]``) read a batch correctly. The pairs of a mesh are in
itertools.combinations order.

Reproduced as the reference has them: an edge exists where ``cost > 0``; the first index wins among equal keys
and equal root probabilities; the diagonal is -log(1e-10); ``pair_attr[:, 1]`` is the share of bone samples INSIDE the mesh although
the reference calls it outside_proportion; the pair attributes come from the float64 joints, the outside counts of the cost matrix
from their float32 cast. The one place that is this build's own: the float32 sigmoid is the float32 nearest to the exact value.
No CPU fallback: without the library or a GPU this module raises.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .abi import CONSTANTS
from .formats import Rig
from .ragged import device_of, int32_table, ptr_of
from .runtime import get_ops
from .skinning import vox_arrays
from .synth import MeshData

MAX_JOINTS = CONSTANTS["MORIG_PRIM_MAX_JOINTS"]


def _counts_of(joints_batch, n_joints: int, n_meshes: Optional[int]) -> List[int]:
    if joints_batch is None:
        return [n_joints]
    b = torch.as_tensor(joints_batch)
    if b.numel() != n_joints:
        raise ValueError("skeleton: joints_batch must name a mesh for every joint")
    if b.numel() > 1 and bool((b[1:] < b[:-1]).any()):
        raise ValueError("skeleton: joints_batch must be sorted (meshes are contiguous joint ranges)")
    return torch.bincount(b, minlength=n_meshes or 0).tolist()


def _ptrs(counts: Sequence[int], device):
    if len(counts) == 0 or min(counts) < 1:
        raise ValueError("skeleton: every mesh needs at least one joint")
    jptr = ptr_of(counts)
    pptr = ptr_of([c * (c - 1) // 2 for c in counts])
    cptr = ptr_of([c * c for c in counts])
    if pptr[-1] >= 2 ** 31 or cptr[-1] >= 2 ** 40:
        raise ValueError("skeleton: too many joint pairs for one call")
    jp, pp = int32_table(jptr, device, "skeleton"), int32_table(pptr, device, "skeleton")
    return jptr, pptr, cptr, jp, pp, torch.from_numpy(cptr).to(device)


def _pair_geometry(j64: torch.Tensor, j32: torch.Tensor, counts, voxes):
    device = j64.device
    if len(voxes) != len(counts):
        raise ValueError("skeleton: one voxel grid per mesh")
    _, pptr, _, jp, pp, _ = _ptrs(counts, device)
    grids, tf = vox_arrays(voxes, device)
    pairs, attr, outside, status = get_ops().pair_attr(j64, j32, jp, pp, int(pptr[-1]), grids, tf)
    return pairs, attr, outside, status, pptr


def _joints64(joints_list):
    js = [torch.as_tensor(np.asarray(j.detach().cpu() if torch.is_tensor(j) else j, dtype=np.float64)).reshape(-1, 3) for j in joints_list]
    return torch.cat(js, 0), [int(j.shape[0]) for j in js]


def _pair_attributes(joints_list, voxes):
    device = device_of(joints_list[0])
    j64, counts = _joints64(joints_list)
    j64 = j64.to(device).contiguous()
    j32 = j64.float()                                                      # torch.from_numpy(joints).float() of create_one_data
    pairs, attr, outside, status, pptr = _pair_geometry(j64, j32, counts, voxes)
    if int(status.item()) != 0:
        raise RuntimeError("pair_attributes: a bone with more than 2^24 samples")
    return pairs, attr, outside, pptr, j32, counts


def pair_attributes_batched(joints_list, voxes):
    """create_one_data's pair loop (joint2rig.py:234-244) for every mesh in one launch. ``joints_list``: one float64 [J_b, 3] array per
    mesh (what create_one_data receives), ``voxes`` one binvox-like 88^3 grid per mesh. -> (pairs int64 [P, 2] rows of the concatenated
    joints, pair_attr float32 [P, 3] = distance, inside share, 1; outside_count int32 [P], the count increase_cost_for_outside_bone
    takes on the float32 joints; pair_ptr, the per-mesh prefix sums of P as a numpy array)."""
    return _pair_attributes(joints_list, voxes)[:4]


def pair_attributes(joints, vox):
    """One mesh: -> (pairs int64 [P, 2], pair_attr float32 [P, 3], outside_count int32 [P]) device tensors."""
    return _pair_attributes([joints], [vox])[:3]


def make_data(data: MeshData, joints_list, voxes) -> MeshData:
    """The fields create_one_data (joint2rig.py:232-264) adds, on a copy of ``data`` (a mesh or a collated batch with pos, the two
    edge indices and ``batch``): joints float32, pairs float32 (indices into the batch's joints), pair_attr float32, joints_batch /
    pairs_batch int64 -- and ``outside_count`` int32, which lets ``predict_skeleton`` skip the second walk over the bones."""
    pairs, attr, outside, pptr, j32, counts = _pair_attributes(joints_list, voxes)
    device = pairs.device
    out = data.to(device)
    out.joints = j32
    out.pairs = pairs.float()
    out.pair_attr = attr
    out.outside_count = outside
    mesh_ids = torch.arange(len(counts), device=device)
    out.joints_batch = torch.repeat_interleave(mesh_ids, torch.tensor(counts, device=device))
    out.pairs_batch = torch.repeat_interleave(mesh_ids, torch.tensor(np.diff(pptr), device=device))
    if not hasattr(out, "batch"):
        out.batch = torch.zeros(out.pos.shape[0], dtype=torch.long, device=device)
    return out


class _Cost:
    """cost matrices of a batch: ``flat`` float64, mesh b's [J_b, J_b] block at ``off[b]``"""

    def __init__(self, flat, off_host, off_dev, jptr_host, jptr_dev):
        self.flat, self.off_host, self.off_dev, self.jptr_host, self.jptr_dev = flat, off_host, off_dev, jptr_host, jptr_dev

    def matrices(self) -> List[torch.Tensor]:
        n = np.diff(self.jptr_host)
        return [self.flat[int(self.off_host[b]):int(self.off_host[b + 1])].view(int(n[b]), int(n[b])) for b in range(len(n))]


def _connectivity_cost(pair_logits, root_logits, joints, voxes, joints_batch, outside_count):
    j32 = torch.as_tensor(joints)
    device = device_of(j32)
    j32 = j32.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    counts = _counts_of(joints_batch, j32.shape[0], None if voxes is None else len(voxes))
    jptr, pptr, cptr, jp, pp, cp = _ptrs(counts, device)
    pl = torch.as_tensor(pair_logits).to(device=device, dtype=torch.float32)
    rl = torch.as_tensor(root_logits).to(device=device, dtype=torch.float32)
    pl = pl[:, 0] if pl.dim() == 2 and pl.shape[1] == 1 else pl.reshape(-1)
    rl = rl[:, 0] if rl.dim() == 2 and rl.shape[1] == 1 else rl.reshape(-1)
    if pl.numel() != int(pptr[-1]) or rl.numel() != j32.shape[0]:
        raise ValueError("connectivity_cost: one logit per joint pair (combinations order) and one root logit per joint")
    if outside_count is None:
        if voxes is None:
            raise ValueError("connectivity_cost: needs the voxel grids or the outside counts made from them")
        _, _, outside_count, status, _ = _pair_geometry(j32.double(), j32, counts, voxes)
        if int(status.item()) != 0:
            raise RuntimeError("connectivity_cost: a bone with more than 2^24 samples")
    oc = torch.as_tensor(outside_count).to(device=device, dtype=torch.int32).contiguous()
    flat, root = get_ops().skeleton_cost(pl, rl, j32, oc, jp, pp, cp, int(cptr[-1]), max(counts))
    return _Cost(flat, cptr, cp, jptr, jp), root


def connectivity_cost(pair_logits, root_logits, joints, voxes=None, joints_batch=None, outside_count=None):
    """predict_skeleton's cost matrix (joint2rig.py:207-218) for every mesh: ``pair_logits`` [P] or [P, 1] and ``root_logits`` [N] or
    [N, 1] float32 (PairCls / ROOTNET outputs), ``joints`` float32 [N, 3] (Data.joints), ``joints_batch`` the sorted mesh index per joint
    (None: one mesh). The outside-bone counts are taken from ``voxes`` unless ``outside_count`` (pair_attributes / make_data) is given.
    -> (list of float64 [J_b, J_b] device tensors, root ids int32 [n_meshes] device tensor)."""
    cost, root = _connectivity_cost(pair_logits, root_logits, joints, voxes, joints_batch, outside_count)
    return cost.matrices(), root


def _prim(cost: _Cost, root: torch.Tensor):
    n = np.diff(cost.jptr_host)
    parent, key, status = get_ops().prim_mst(cost.flat, cost.off_dev, cost.jptr_dev, root.to(torch.int32).contiguous(),
                                             int(cost.jptr_host[-1]), int(n.max()))
    return parent, key, status


def prim_mst(cost, root):
    """primMST (mst_utils.py:63-108). ``cost``: one float64 [J, J] matrix with an int ``root``, or a list of them with one root id per
    mesh (list / tensor). -> (parent int32, key float64) device tensors, or lists of them; parent is -1 at the root. A disconnected
    graph (a joint no ``cost > 0`` edge reaches) raises ``PrimError``, as the reference raises there."""
    single = torch.is_tensor(cost) or isinstance(cost, np.ndarray)
    mats = [cost] if single else list(cost)
    device = device_of(mats[0])
    mats = [torch.as_tensor(m).to(device=device, dtype=torch.float64) for m in mats]
    for m in mats:
        if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError("prim_mst: square cost matrices")
    counts = [int(m.shape[0]) for m in mats]
    jptr, _, cptr, jp, _, cp = _ptrs(counts, device)
    roots = torch.as_tensor([int(root)] if single else root).to(device=device, dtype=torch.int32).reshape(-1)
    if roots.numel() != len(mats):
        raise ValueError("prim_mst: one root id per cost matrix")
    flat = torch.cat([m.reshape(-1) for m in mats]).contiguous()
    parent, key, status = _prim(_Cost(flat, cptr, cp, jptr, jp), roots)
    _raise_on_status(status.tolist())
    ps = [parent[int(jptr[b]):int(jptr[b + 1])] for b in range(len(mats))]
    ks = [key[int(jptr[b]):int(jptr[b + 1])] for b in range(len(mats))]
    return (ps[0], ks[0]) if single else (ps, ks)


class PrimError(RuntimeError):
    """prim_mst / predict_skeleton could not build a tree for some mesh; ``status`` holds one code per mesh: 0 fine, 1 the cost graph
    is disconnected, 2 the root id is outside the mesh's joints, 3 more joints than MAX_JOINTS"""

    def __init__(self, status: List[int]):
        self.status = list(status)
        what = {1: "the cost graph is disconnected (no cost > 0 edge reaches some joint)", 2: "the root id is outside the mesh's joints",
                3: f"more than {MAX_JOINTS} joints"}
        bad = [(b, s) for b, s in enumerate(self.status) if s != 0]
        super().__init__("prim_mst: " + "; ".join(f"mesh {b}: {what.get(s, s)}" for b, s in bad[:4]) +
                         (f"; and {len(bad) - 4} more" if len(bad) > 4 else ""))


def _raise_on_status(status: List[int]) -> None:
    if any(s != 0 for s in status):
        raise PrimError(status)


def predict_skeleton(data: MeshData, voxes, root_net, bone_net) -> List[Rig]:
    """joint2rig.predict_skeleton for a batch: ``data`` as ``make_data`` leaves it, ``root_net`` / ``bone_net`` the ROOTNET and PairCls
    modules (called as the reference calls them: ``shuffle=False`` / ``permute_joints=False``, first output). ``voxes`` may be None
    when ``data.outside_count`` is there. -> one ``formats.Rig`` per mesh: names joint_{i}, the root, hierarchy = the MST parents,
    positions and offsets as calc_frames_and_offsets leaves them on the float32 joints."""
    with torch.no_grad():
        root_logits = root_net(data, shuffle=False)[0]
        pair_logits = bone_net(data, permute_joints=False)[0]
    cost, root = _connectivity_cost(pair_logits, root_logits, data.joints, voxes, data.joints_batch, getattr(data, "outside_count", None))
    parent, _, status = _prim(cost, root)
    _raise_on_status(status.tolist())
    parent, root = parent.cpu().numpy(), root.cpu().numpy()
    joints = torch.as_tensor(data.joints).detach().float().cpu().numpy()
    jptr = cost.jptr_host
    return [Rig.from_arrays(joints[jptr[b]:jptr[b + 1]], parent[jptr[b]:jptr[b + 1]], int(root[b])) for b in range(len(jptr) - 1)]
