"""The final rig on the MI355X-native op layer (csrc/rig_assemble.hip): the last two statements of the rigging driver,
``assemble_skel_skin`` (evaluate/joint2rig.py:147-162, over ``add_duplicate_joints`` :97-134 and ``mapping_bone_index`` :137-144) and
``remove_dup_joints`` (:363-394), as ``pred_rig_func`` calls them (:507-510). ``skinning.skin_weights(mode="joint2rig")`` ends with one
float64 [V, n_bones] matrix per mesh, indexed by BONE; ``tracking.track``, ``metrics.evaluate_rigs`` and ``Rig.save`` want a
``formats.Rig`` whose ``skins`` is [V, J], indexed by JOINT. This module goes from one to the other for a batch.

The step is not "sum the bones that start at each joint". What is replayed literally:
  * a joint with several children gets one duplicate per child, 1 % of the way to the child, named ``<parent>_dup_<k>``;
  * an old bone writes to the start joint of the NEAREST new bone in 6-D (np.linalg.norm, np.argmin: the first index wins a tie), so on
    rigs with coincident joints several bones write to one joint;
  * that write OVERWRITES: the last bone in ascending order with weight > 1e-5 wins; weights <= 1e-5 are dropped, nothing is renormalised;
  * duplicates are recognised by the substring "_dup" in a name, only a duplicate's first child is promoted, a duplicate's column is
    added to its parent's (parent first, duplicates in ascending index), and the result's joints come out breadth first;
  * positions pass through ``calc_frames_and_offsets`` once per rebuilt rig (offset + parent position, in the dtype of the joints).

Division of work: the tree bookkeeping is host work on host objects (``assembly_plan``: numpy, no device) and ends in two CSR tables
per mesh -- output joint -> segments, segment -> bones in ascending order -- concatenated over the batch; everything done with the
weights runs in two kernels. Host reads: ``assemble_rigs`` copies the dense [N, J] block to the host once per batch (``Rig.skins`` is a
numpy array, as everywhere in formats.py); with ``entries=True`` one more read of B + 1 entry offsets sizes the sparse form. There is no
CPU path: without the library or a GPU this module raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import geodesic, skinning
from .formats import Rig
from .ragged import device_of, ptr_of
from .runtime import get_ops


# ---- host plan -----------------------------------------------------------------------------------------------------------------------
def _children(hier: np.ndarray, pid: int) -> np.ndarray:
    return np.argwhere(hier == pid).squeeze(axis=1)


def add_duplicate_joints(rig) -> Rig:
    """joint2rig.py:97-134 on a ``formats.Rig``: breadth first from the root; a joint with one child hands it on; a joint with several
    children gets, per child, a duplicate ``<name>_dup_<k>`` at pos + 0.01 (child - pos) below itself and the child below the duplicate.
    Parents are looked up by name (first match), as there. -> a Rig without skins, root 0, positions rebuilt by the forward pass in the
    dtype of ``rig.pos``. Names that collide with a duplicate's raise ValueError (the reference would build a broken hierarchy)."""
    hier = np.asarray(rig.hierarchy).reshape(-1)
    pos = np.asarray(rig.pos)
    level = [int(rig.root_id)]
    pos_new, hier_new, names_new = [pos[rig.root_id]], [-1], [rig.root_name]
    while level:
        nxt = []
        for pid in level:
            ch = _children(hier, pid)
            if len(ch) > 1:
                for dup_id, cid in enumerate(ch):
                    dup = rig.names[pid] + f"_dup_{dup_id}"
                    pos_new.append(pos[pid] + 0.01 * (pos[cid] - pos[pid]))
                    names_new.append(dup)
                    hier_new.append(names_new.index(rig.names[pid]))
                    pos_new.append(pos[cid])
                    names_new.append(rig.names[cid])
                    hier_new.append(names_new.index(dup))
            elif len(ch) == 1:
                pos_new.append(pos[ch[0]])
                names_new.append(rig.names[ch[0]])
                hier_new.append(names_new.index(rig.names[pid]))
            nxt += ch.tolist()
        level = nxt
        if len(names_new) > 3 * len(hier) + 1:
            raise ValueError("add_duplicate_joints: the hierarchy is not a tree")
    return Rig.from_arrays(np.array(pos_new), np.array(hier_new), 0, names_new)


def mapping_bone_index(bones_old, bones_new) -> dict:
    """joint2rig.py:137-144: for every old bone the index of the nearest new bone, np.linalg.norm over the 6 coordinates and np.argmin
    (first index on ties) -- the very calls, so near-ties resolve the way numpy resolves them."""
    bones_old, bones_new = np.asarray(bones_old), np.asarray(bones_new)
    bone_map = {}
    for i in range(len(bones_old)):
        dist = np.linalg.norm(bones_new - bones_old[i][np.newaxis, :], axis=1)
        bone_map[i] = np.argmin(dist)
    return bone_map


def _bones(rig) -> tuple:
    """``skinning.get_bones`` (the same bones in the same order) without its cast to float64: the reference's get_bones leaves the bones
    in the dtype of ``rig.pos``, so the nearest new bone of float32 joints is found in float32 -> (bones [nb, 6], bone_names)"""
    hier, pos = np.asarray(rig.hierarchy).reshape(-1), np.asarray(rig.pos)
    bones, names, level = [], [], [int(rig.root_id)]
    while level:
        nxt = []
        for pid in level:
            ch = _children(hier, pid)
            for cid in ch:
                bones.append(np.concatenate((pos[pid], pos[cid])))
                names.append([rig.names[pid], rig.names[cid]])
                if len(_children(hier, cid)) == 0:
                    bones.append(np.concatenate((pos[cid], pos[cid])))
                    names.append([rig.names[cid], rig.names[cid] + "_leaf"])
            nxt += ch.tolist()
        level = nxt
    return np.stack(bones, axis=0), names


def _removal(rig):
    """the bookkeeping of remove_dup_joints (joint2rig.py:363-394) -> (order: the kept joints breadth first, names, hierarchy,
    segments: per kept joint the columns the reference adds up, its own first, then its "_dup" children in ascending index)"""
    hier = np.asarray(rig.hierarchy).reshape(-1)
    level = [int(rig.root_id)]
    order, segments, hier_res, names_res = [], [], [-1], [rig.root_name]
    while level:
        nxt = []
        for pid in level:
            cols = [int(pid)]
            for cid in _children(hier, pid):
                if "_dup" in rig.names[cid]:
                    below = _children(hier, cid)
                    if len(below) == 0:
                        raise ValueError(f"remove_dup_joints: joint '{rig.names[cid]}' is named like a duplicate and has no child to promote")
                    nxt.append(int(below[0]))
                    names_res.append(rig.names[below[0]])
                    cols.append(int(cid))
                else:
                    nxt.append(int(cid))
                    names_res.append(rig.names[cid])
                hier_res.append(names_res.index(rig.names[pid]))
            order.append(int(pid))
            segments.append(cols)
        level = nxt
        if len(order) > len(hier):
            raise ValueError("remove_dup_joints: the hierarchy is not a tree")
    return order, names_res, hier_res, segments


def _removed(rig) -> tuple:
    order, names, hier, segments = _removal(rig)
    return Rig.from_arrays(np.stack([np.asarray(rig.pos)[p] for p in order], axis=0), np.array(hier), 0, names), segments


@dataclass
class AssemblyPlan:
    """What ``assembly_plan`` returns. ``dup``: the rig with duplicated joints (no skins); ``new_of_bone`` int64 [n_bones]: the joint of
    ``dup`` that old bone i writes to; ``final``: the rig after duplicate removal (no skins); ``segments``: per joint of ``final`` the
    joints of ``dup`` whose columns are added into it, in the reference's addition order."""
    dup: Rig
    new_of_bone: np.ndarray
    final: Rig
    segments: List[List[int]]

    def rig(self, keep_duplicates: bool) -> Rig:
        return self.dup if keep_duplicates else self.final

    def tables(self, keep_duplicates: bool = False) -> tuple:
        """the two CSR tables of one mesh -> (seg_ptr int64 [J + 1], bone_ptr int64 [S + 1], bones int64): output joint -> segments,
        segment -> the old bones that write to it, ascending. ``keep_duplicates``: one segment per joint of ``dup``."""
        segs = [[j] for j in range(len(self.dup.names))] if keep_duplicates else self.segments
        flat = [n for cols in segs for n in cols]
        per = [np.flatnonzero(self.new_of_bone == n) for n in flat]
        seg_ptr, bone_ptr = ptr_of([len(cols) for cols in segs]), ptr_of([len(b) for b in per])
        return seg_ptr, bone_ptr, (np.concatenate(per) if per else np.zeros(0)).astype(np.int64)


def assembly_plan(rig) -> AssemblyPlan:
    """The tree bookkeeping of assemble_skel_skin and remove_dup_joints for one ``formats.Rig`` (numpy, no device). A rig of one joint
    has no bones (the reference's get_bones fails on it) and a "_dup"-named joint without a child cannot be removed (IndexError there):
    both raise ValueError."""
    if len(rig.names) < 2:
        raise ValueError("assembly_plan: a rig of one joint has no bones")
    bones_old, _ = _bones(rig)
    dup = add_duplicate_joints(rig)
    bones_new, names_new = _bones(dup)
    bone_map = mapping_bone_index(bones_old, bones_new)
    new_of_bone = np.array([dup.names.index(names_new[bone_map[i]][0]) for i in range(len(bones_old))], dtype=np.int64)
    final, segments = _removed(dup)
    return AssemblyPlan(dup, new_of_bone, final, segments)


# ---- device ----------------------------------------------------------------------------------------------------------------------------
def _weight_block(ws: List[torch.Tensor], device) -> torch.Tensor:
    """[N, max n_bones] float64 over all meshes. Views of one block with a common row stride, one mesh after the other -- what
    ``skin_weights`` returns -- are read in place through that stride; anything else is copied into a new block."""
    first, n, cols = ws[0], sum(w.shape[0] for w in ws), max(w.shape[1] for w in ws)
    ld = first.stride(0)                                           # a slice of one row still reports the stride of its block
    shared = all(w.device == device and w.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and
                 (w.shape[1] <= 1 or w.stride(1) == 1) and w.stride(0) == ld for w in ws) and ld >= cols
    if shared:
        off = first.storage_offset()
        for w in ws:
            shared = shared and w.storage_offset() == off
            off += w.shape[0] * ld
        shared = shared and first.storage_offset() + (n - 1) * ld + cols <= first.untyped_storage().nbytes() // 8
    if shared:
        return first.as_strided((n, cols), (ld, 1))
    block = torch.zeros(n, cols, dtype=torch.float64, device=device)
    r = 0
    for w in ws:
        block[r:r + w.shape[0], :w.shape[1]] = w.to(device)
        r += w.shape[0]
    return block


def _as_weights(w, n_bones: int, what: str) -> torch.Tensor:
    t = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w, dtype=np.float64))
    if t.dim() != 2 or t.shape[1] != n_bones:
        raise ValueError(f"{what}: weights must be [V, {n_bones}] (one column per bone of skinning.get_bones), got {tuple(t.shape)}")
    return t if t.dtype == torch.float64 else t.to(torch.float64)


def _run(ws: List[torch.Tensor], tables: List[tuple], n_joints: List[int], raw: bool, entries: bool, device):
    """the kernels on a batch -> (dense [N, max J] on the device, vertex ptr, per-mesh entry tuples or None)"""
    nv = [w.shape[0] for w in ws]
    vptr, jptr = ptr_of(nv), ptr_of(n_joints)
    if vptr[-1] >= 2 ** 31 or vptr[-1] * max(n_joints) >= 2 ** 38:
        raise ValueError("assemble_rigs: the batch is too large for one call")
    seg_ptr = np.concatenate([[0]] + [t[0][1:] + o for t, o in zip(tables, ptr_of([t[0][-1] for t in tables])[:-1])])
    bone_ptr = np.concatenate([[0]] + [t[1][1:] + o for t, o in zip(tables, ptr_of([t[1][-1] for t in tables])[:-1])])
    bones = np.concatenate([t[2] for t in tables])
    up = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(device)
    ops = get_ops()
    d_vptr = up(vptr)
    dense = ops.rig_assemble(_weight_block([w.to(device) for w in ws], device), d_vptr, up(jptr), up(seg_ptr), up(bone_ptr), up(bones),
                             int(max(n_joints)), raw)
    if not entries:
        return dense, vptr, None
    counts = ops.rig_skin_counts(dense, d_vptr)
    eptr = torch.zeros(dense.shape[0] + 1, dtype=torch.int64, device=device)
    eptr[1:] = torch.cumsum(counts, 0)
    cuts = eptr[torch.from_numpy(vptr).to(device)].tolist()        # THE host read of the sparse form: B + 1 entry offsets, the last the total
    if cuts[-1] >= 2 ** 31:
        raise ValueError("assemble_rigs: more than 2^31 skin entries in one call")
    eptr = eptr.to(torch.int32)
    ev, ej, ew = ops.rig_skin_fill(dense, d_vptr, eptr, int(cuts[-1]))
    per = [(eptr[vptr[b]:vptr[b + 1] + 1] - cuts[b], ev[cuts[b]:cuts[b + 1]], ej[cuts[b]:cuts[b + 1]], ew[cuts[b]:cuts[b + 1]])
           for b in range(len(ws))]
    return dense, vptr, per


def _finish(rigs: List[Rig], dense: torch.Tensor, vptr: np.ndarray, per) -> List[Rig]:
    host = dense.cpu().numpy()                                         # the one device -> host copy of the dense block
    for b, rig in enumerate(rigs):
        j = len(rig.names)
        rig.skins = np.ascontiguousarray(host[vptr[b]:vptr[b + 1], :j])
        rig.skins_device = dense[vptr[b]:vptr[b + 1], :j]
        if per is not None:
            rig.skin_entries_device = per[b]
    return rigs


def assemble_rigs(skeletons: Sequence, weights_list: Sequence, keep_duplicates: bool = False, entries: bool = False, device=None) -> List[Rig]:
    """``remove_dup_joints(assemble_skel_skin(skel, w))`` for a batch. ``skeletons``: B ``formats.Rig``; ``weights_list``: one
    [V_b, n_bones_b] matrix per mesh, columns in ``skinning.get_bones`` order -- what ``skinning.skin_weights`` returns (its views are
    read in place). -> B new ``formats.Rig`` (joints breadth first, root 0) with ``skins`` float64 [V_b, J_b] on the host (one copy of the
    dense block per batch), ``skins_device`` the same on the device and, with ``entries=True``, ``skin_entries_device`` = (vptr int32
    [V_b + 1], vertex int32, joint int32, weight float64) on the device, the form ``tracking.skin_entries`` gives.
    ``keep_duplicates``: stop after assemble_skel_skin (the rig with duplicated joints)."""
    if len(skeletons) != len(weights_list) or len(skeletons) == 0:
        raise ValueError("assemble_rigs: one weight matrix per skeleton, at least one")
    plans = [assembly_plan(s) for s in skeletons]
    ws = [_as_weights(w, len(p.new_of_bone), "assemble_rigs") for w, p in zip(weights_list, plans)]
    device = device_of(*ws, device=device)
    rigs = [p.rig(keep_duplicates) for p in plans]                    # made for this call: positions are not rebuilt a further time
    dense, vptr, per = _run(ws, [p.tables(keep_duplicates) for p in plans], [len(r.names) for r in rigs], False, entries, device)
    return _finish(rigs, dense, vptr, per)


def assemble_skel_skin(skel, attachment) -> Rig:
    """joint2rig.py:147-162 for one mesh: the rig with duplicated joints and ``skins`` [V, J_dup]."""
    return assemble_rigs([skel], [attachment], keep_duplicates=True)[0]


def remove_dup_joints(rig) -> Rig:
    """joint2rig.py:363-394 for one rig with ``skins`` [V, J]: every "_dup" child's column is added to its parent's and its first child
    promoted. Unlike the reference, which adds into ``rig_ori.skins`` in place, this does NOT mutate its argument."""
    res, segments = _removed(rig)
    skins = _as_weights(rig.skins, len(rig.names), "remove_dup_joints")
    flat = np.array([n for cols in segments for n in cols], dtype=np.int64)
    tables = (ptr_of([len(cols) for cols in segments]), np.arange(len(flat) + 1, dtype=np.int64), flat)
    dense, vptr, _ = _run([skins], [tables], [len(res.names)], True, False, device_of(skins))
    return _finish([res], dense, vptr, None)[0]


def occluders(verts: Sequence, faces: Sequence, target_faces: int = 3000) -> List[tuple]:
    """The ``tri_meshes`` of ``predict_rigs``: one (tri_pos float64 [V', 3], tri_faces int64 [F', 3]) per mesh, on the device -- the mesh
    brought down to at most ``target_faces`` faces by ``meshprep.simplify``, where calc_geodesic_matrix (joint2rig.py:319-321) calls
    open3d's simplify_quadric_decimation(3000). The rule is this product's own and does not reproduce the library's mesh; a mesh of at
    most ``target_faces`` faces is its own occluder, there as here."""
    from . import meshprep
    return [(v, f) for v, f, _, _ in meshprep.simplify(verts, faces, target_faces=target_faces)]


def draw_subsamples(n_verts: int, seed: int, n: int = 1500) -> np.ndarray:
    """The sub-sample of calc_geodesic_matrix (joint2rig.py:322): what ``np.random.choice(n_verts, min(n_verts, n), replace=False)`` draws
    right after ``np.random.seed(seed)``, from a generator of its own (the global numpy state is not touched) -> int64 [min(n_verts, n)]."""
    n_verts = int(n_verts)
    return np.random.RandomState(int(seed)).choice(n_verts, min(n_verts, int(n)), replace=False)


def predict_rigs(data, skeletons: Sequence, skin_net, surface_geodesics: Sequence, tri_meshes: Sequence,
                 subsample_ids: Optional[Sequence] = None, accel=None) -> List[Rig]:
    """The body of predict_skinning (joint2rig.py:397-464) plus remove_dup_joints (:509) for a batch. ``data``: the collated batch SkinNet
    reads (pos, batch, the edge lists, pred_flow); ``skeletons``: B ``formats.Rig``; ``skin_net``: models.skinnet_motion in eval mode;
    ``surface_geodesics``: one [V_b, V_b] matrix per mesh; ``tri_meshes``: one (tri_pos, tri_faces) occluder per mesh -- ``occluders``
    makes them where the reference simplifies with open3d; ``subsample_ids`` is one index vector per mesh (``draw_subsamples`` draws what
    the reference's np.random.choice draws), or None for the whole mesh. ``accel`` goes to ``geodesic.bone_visibility_batched``
    ("bvh": the same visibility through the occluders' mesh BVH, worth it when the occluder is the full mesh of a raw asset)."""
    if accel not in (None, "bvh"):
        raise ValueError('predict_rigs: accel is None or "bvh"')
    B = len(skeletons)
    if not (len(surface_geodesics) == len(tri_meshes) == B) or B == 0 or (subsample_ids is not None and len(subsample_ids) != B):
        raise ValueError("predict_rigs: one surface geodesic, occluder (and sub-sample) per skeleton")
    k = geodesic.NUM_NEAREST_BONE
    got = [skinning.get_bones(s) for s in skeletons]
    bones, leaf = [g[0] for g in got], [g[2] for g in got]
    nv = [int(s.shape[0]) for s in surface_geodesics]
    vptr = ptr_of(nv)
    if int(vptr[-1]) != data.pos.shape[0]:
        raise ValueError("predict_rigs: the surface geodesics do not cover the vertices of the batch")
    pos = [data.pos[vptr[b]:vptr[b + 1]].double() for b in range(B)]
    tri_pos, tri_faces = [t[0] for t in tri_meshes], [t[1] for t in tri_meshes]
    if subsample_ids is None:
        vis = geodesic.bone_visibility_batched(pos, bones, tri_pos, tri_faces, accel=accel)
        geo = geodesic.bone_geodesic_matrix_batched(pos, bones, list(surface_geodesics), vis)
    else:
        ids = [torch.as_tensor(np.asarray(i.cpu() if torch.is_tensor(i) else i)).long() for i in subsample_ids]
        vis = geodesic.bone_visibility_batched([p[i.to(p.device)] for p, i in zip(pos, ids)], bones, tri_pos, tri_faces,
                                               accel=accel)
        geo = [geodesic.bone_geodesic_matrix(p, bn, sg, v, subsample_ids=i) for p, bn, sg, v, i in zip(pos, bones, surface_geodesics, vis, ids)]
    skin_input, skin_nn, loss_mask = geodesic.skin_inputs_joint2rig_batched(geo, bones, leaf, k)
    data.skin_input = skin_input
    with torch.no_grad():
        logits = skin_net(data, data.flow if hasattr(data, "flow") else data.pred_flow)[2]
    weights = skinning.skin_weights(logits, skin_nn, loss_mask, data.tpl_edge_index, data.batch, [len(b) for b in bones], mode="joint2rig")
    return assemble_rigs(skeletons, weights)
