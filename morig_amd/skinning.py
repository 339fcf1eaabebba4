"""Skinning on either side of SkinNet on the MI355X-native op layer (csrc/skin.hip).

Input side -- what the reference computes offline in data_proc/gen_skin_data.py (``get_bones`` :14-37, the bind rows :86-118) with
data_proc/common_ops.py's ``calc_volumetric_geodesic`` (:275-328, a scipy binary-dilation BFS per bone): the volumetric geodesic
distance of every vertex to every bone, the k nearest bones per vertex with 1/D and leaf flags, the training labels, and the tensors
datasets/dataset_rig.py (:30-76, 94-101) makes of the ``_skin.txt`` file (``skin_input``, ``skin_nn``, ``loss_mask``,
``skin_nnjids``), handed to SkinNet before the file's %.6f round trip. ``write_skin_file`` writes that file byte for byte.

Output side -- the per-vertex loops after SkinNet in training/train_skin.py:232-244 (+ ``post_filter`` :40-66) and
evaluate/joint2rig.py:447-462: masked softmax, scatter into [V, n_bones], 1-ring mean, threshold relative to the row maximum,
renormalisation.

Defined where the reference is not: among bones at equal distance the smaller bone id comes first (a stable
argsort); a patched voxel with several equally near reached voxels takes the smallest of their layers; a vertex without 1-ring
neighbours keeps its own row before the threshold (the reference raises there). No CPU fallback: without the library or a GPU this
module raises.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import ragged
from .ragged import device_of, ptr_of
from .runtime import get_ops

NUM_NEAREST_BONE = 20
MAX_JOINTS = 64                      # the label kernel keeps a vertex's used joints in a 64-bit set
_MODES = {"train_skin": (0, 0.5), "joint2rig": (1, 0.35)}


def get_bones(rig):
    """gen_skin_data.py:14-37 on a ``formats.Rig`` (names, pos, hierarchy, root_id): breadth-first from the root, children in
    ascending joint index, every bone [p_pos, c_pos] named [parent, child]; a child without children adds the leaf bone
    [c_pos, c_pos] named [child, child + "_leaf"] right after. -> (bones float64 [nb, 6], bone_names, is_leaf list of bool)."""
    hier = np.asarray(rig.hierarchy)
    bones, names, leaf = [], [], []
    level = [rig.root_id]
    while level:
        nxt = []
        for pid in level:
            ch = np.argwhere(hier == pid).squeeze(axis=1)
            for cid in ch:
                bones.append(np.concatenate((rig.pos[pid], rig.pos[cid])))
                names.append([rig.names[pid], rig.names[cid]])
                leaf.append(False)
                if len(np.argwhere(hier == cid)) == 0:
                    bones.append(np.concatenate((rig.pos[cid], rig.pos[cid])))
                    names.append([rig.names[cid], rig.names[cid] + "_leaf"])
                    leaf.append(True)
            nxt += ch.tolist()
        level = nxt
    return np.stack(bones, axis=0).astype(np.float64), names, leaf


def start_joints(rig, bone_names) -> np.ndarray:
    """joint index of every bone's start joint (dataset_rig.py:94-101: ``rig.names.index(bone_names[b][0])``)"""
    return np.array([rig.names.index(n[0]) for n in bone_names], dtype=np.int32)


def vox_arrays(voxes, device):
    grids = np.stack([np.ascontiguousarray(np.asarray(v.data, dtype=np.uint8)).reshape(-1) for v in voxes], axis=0)
    for v in voxes:
        if tuple(np.asarray(v.data).shape) != (88, 88, 88) or int(v.dims[0]) != 88:
            raise ValueError("volumetric_geodesic: the reference's BFS is written for 88^3 grids only (common_ops.py:283,320)")
    tf = np.array([[float(v.translate[0]), float(v.translate[1]), float(v.translate[2]), float(v.scale), float(v.dims[0])]
                   for v in voxes], dtype=np.float64)
    return torch.from_numpy(grids).to(device), torch.from_numpy(tf).to(device)


def volumetric_geodesic_batched(pos, batch, voxes, bones_list, num_graphs: Optional[int] = None, n_slots: Optional[int] = None):
    """calc_volumetric_geodesic (common_ops.py:316-328) for every mesh of a batch in ONE launch: pos [N, 3] of the concatenated meshes,
    ``batch`` PyG's sorted mesh index per vertex, ``voxes`` one binvox-like grid per mesh (``data`` 88^3 bool, ``translate``,
    ``scale``, ``dims``), ``bones_list`` one float64 [nb_b, 6] per mesh. -> list of int32 [V_b, nb_b] views of one device buffer."""
    device = device_of(pos)
    p = (pos if torch.is_tensor(pos) else torch.as_tensor(np.asarray(pos))).to(device=device, dtype=torch.float64).contiguous()
    b = torch.as_tensor(batch).to(device)
    B = int(num_graphs) if num_graphs is not None else len(voxes)
    assert len(voxes) == B and len(bones_list) == B
    counts = torch.bincount(b, minlength=B).tolist() if b.numel() else [0] * B
    nbs = [int(np.asarray(x).shape[0]) for x in bones_list]
    if min(nbs) < 1:
        raise ValueError("volumetric_geodesic: a mesh without bones")
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] != sum(counts):
        raise ValueError("volumetric_geodesic: pos must be [N, 3] with N = len(batch)")
    vptr, bptr = ptr_of(counts), ptr_of(nbs)
    doff = ptr_of([v * n for v, n in zip(counts, nbs)])
    grids, tf = vox_arrays(voxes, device)
    bones = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 6) for x in bones_list], 0)).to(device)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(device)
    ops = get_ops()
    dist, status = ops.vol_geodesic(grids, tf, p, i32(vptr), bones.contiguous(), i32(bptr), torch.from_numpy(doff).to(device),
                                    int(doff[-1]), int(n_slots) if n_slots else ragged.n_slots(device))
    st = int(status[0].item())
    if st == 1:
        raise RuntimeError("volumetric_geodesic: a BFS layer above 65535")
    if st == 2:
        raise RuntimeError("volumetric_geodesic: a bone with more than 2^24 samples")
    return [dist[int(doff[i]):int(doff[i + 1])].view(counts[i], nbs[i]) for i in range(B)]


def volumetric_geodesic(pos, vox, bones) -> torch.Tensor:
    """calc_volumetric_geodesic(vtx, vox, bones) of one mesh -> int32 [V, nb] device tensor."""
    n = pos.shape[0]
    dev = device_of(pos)
    return volumetric_geodesic_batched(pos, torch.zeros(n, dtype=torch.long, device=dev), [vox], [bones], num_graphs=1)[0]


def skin_bind_batched(dists, bones_list, is_leaf_list, start_jid_list, skins_list=None, k: int = NUM_NEAREST_BONE) -> dict:
    """Bind rows of every mesh in one launch: ``dists`` int32 [V_b, nb_b] per mesh (volumetric_geodesic_batched), per mesh its bones,
    leaf flags, start-joint ids (``start_joints``) and optionally its rig's skins [V_b, J_b] (J_b <= 64) for the labels.
    -> dict of [N, k] device tensors, meshes concatenated: bind_ids (-1 past the bone count), bind_invd (float64), labels (or None),
    skin_input [N, 8k] float32, skin_nn, loss_mask, skin_nnjids (int64)."""
    device = dists[0].device
    counts = [int(d.shape[0]) for d in dists]
    nbs = [int(d.shape[1]) for d in dists]
    if min(nbs) < 1:
        raise ValueError("skin_bind: a mesh without bones")
    vptr, bptr = ptr_of(counts), ptr_of(nbs)
    doff = ptr_of([v * n for v, n in zip(counts, nbs)])
    flat = torch.cat([d.reshape(-1) for d in dists]).to(torch.int32).contiguous()
    bones = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 6) for x in bones_list], 0)).to(device)
    leaf = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.uint8).reshape(-1) for x in is_leaf_list])).to(device)
    sj = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in start_jid_list])).to(device)
    skins = None
    if skins_list is not None:
        J = max(int(np.asarray(s).shape[1]) for s in skins_list)
        if J > MAX_JOINTS:
            raise ValueError(f"skin labels: at most {MAX_JOINTS} joints per rig, got {J}")
        sk = np.zeros((sum(counts), J), dtype=np.float64)
        for i, s in enumerate(skins_list):
            s = np.asarray(s, dtype=np.float64)
            assert s.shape[0] == counts[i]
            sk[vptr[i]:vptr[i + 1], :s.shape[1]] = s
        skins = torch.from_numpy(sk).to(device)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(device)
    return get_ops().skin_bind(flat, torch.from_numpy(doff).to(device), i32(vptr), i32(bptr), sum(counts), bones.contiguous(), leaf,
                               sj, skins, int(k))


def skin_bind(dist, bones, is_leaf, k: int = NUM_NEAREST_BONE, rig=None, bone_names=None) -> dict:
    """gen_skin_data.py:86-118 for one mesh: ``dist`` int32 [V, nb] device tensor. With a rig (and its ``bone_names`` from get_bones,
    recomputed when omitted) the start-joint ids come from its names and, when it carries skins, the labels are made too."""
    if rig is not None and bone_names is None:
        bone_names = get_bones(rig)[1]
    sj = start_joints(rig, bone_names) if rig is not None else np.zeros(len(is_leaf), dtype=np.int32)
    skins = None
    if rig is not None and len(getattr(rig, "skins", [])) > 0:
        skins = [np.asarray(rig.skins)]
    return skin_bind_batched([dist], [bones], [is_leaf], [sj], skins, k)


def skin_inputs(dist, bones, is_leaf, rig, k: int = NUM_NEAREST_BONE, bone_names=None):
    """-> (skin_input float32 [V, 8k], skin_nn, loss_mask, skin_nnjids int64 [V, k]): what ``formats.load_rig_sample`` sets on a
    MeshData for SkinMotion, without the %.6f file round trip."""
    o = skin_bind(dist, bones, is_leaf, k, rig=rig, bone_names=bone_names)
    return o["skin_input"], o["skin_nn"], o["loss_mask"], o["skin_nnjids"]


def bind_rows(bind: dict, is_leaf_list) -> np.ndarray:
    """[N, 3k] float64 rows (bone id, 1/D, leaf) per slot, the reference's ``input_samples`` without the leading vertex id; an invalid
    slot is (-1, 0, 0). ``is_leaf_list``: per mesh, or one mesh's flags."""
    ids = bind["bind_ids"].cpu().numpy().astype(np.int64)
    invd = bind["bind_invd"].cpu().numpy()
    if len(is_leaf_list) and not isinstance(is_leaf_list[0], (bool, np.bool_, int, np.integer)):
        raise ValueError("bind_rows: pass one mesh's leaf flags")
    leaf = np.asarray(is_leaf_list, dtype=np.int64)
    out = np.zeros((ids.shape[0], 3 * ids.shape[1]), dtype=np.float64)
    valid = ids >= 0
    out[:, 0::3] = ids
    out[:, 1::3] = np.where(valid, invd, 0.0)
    out[:, 2::3] = np.where(valid, leaf[np.where(valid, ids, 0)], 0)
    return out


def write_skin_file(filename: str, bones, bone_names, bind, labels) -> None:
    """The ``{id}_skin.txt`` of gen_skin_data.py:120-135, byte for byte: ``bind`` [V, 3k] rows (bind_rows), ``labels`` [V, k]."""
    bones = np.asarray(bones, dtype=np.float64)
    bind = np.asarray(bind, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.float64)
    parts = []
    for i in range(len(bones)):
        parts.append("bones {:s} {:s} {:.6f} {:.6f} {:.6f} {:.6f} {:.6f} {:.6f}\n".format(
            bone_names[i][0], bone_names[i][1], *[float(x) for x in bones[i, :6]]))
    for v in range(bind.shape[0]):
        row = ["bind {:d} ".format(v)]
        for j in range(0, bind.shape[1], 3):
            row.append("{:d} {:.6f} {:d} ".format(int(bind[v, j]), float(bind[v, j + 1]), int(bind[v, j + 2])))
        parts.append("".join(row) + "\n")
    for v in range(labels.shape[0]):
        parts.append("influence " + "".join("{:.3f} ".format(float(x)) for x in labels[v]) + "\n")
    with open(filename, "w") as f:
        f.write("".join(parts))


def one_ring_csr(tpl_edge_index: torch.Tensor, n: int):
    """unique 1-ring neighbours of every vertex from the tpl edges in both directions, self excluded -> (rowptr int32 [n + 1],
    cols int32), rows in ascending neighbour order (post_filter's set of adjacent vertices, train_skin.py:45-55)."""
    e = tpl_edge_index.to(torch.int64)
    if e.numel() and (int(e.min()) < 0 or int(e.max()) >= n):
        raise ValueError("one_ring_csr: an edge names a vertex out of range")
    src = torch.cat([e[0], e[1]])
    dst = torch.cat([e[1], e[0]])
    keep = src != dst
    key = torch.unique(src[keep] * n + dst[keep])
    s, d = key // n, key % n
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=e.device)
    rowptr[1:] = torch.cumsum(torch.bincount(s, minlength=n), 0)
    return rowptr.to(torch.int32), d.to(torch.int32).contiguous()


def skin_weights(skin_cls_pred, skin_nn, loss_mask, tpl_edge_index, batch, n_bones, mode: str = "train_skin",
                 ratio: Optional[float] = None) -> List[torch.Tensor]:
    """SkinNet logits [N, k] -> final weights, one float64 [V_b, n_bones[b]] device tensor per mesh. mode "train_skin"
    (train_skin.py:232-244): softmax, then x loss_mask, ratio 0.5; mode "joint2rig" (joint2rig.py:447-462): logits x loss_mask, then
    softmax, ratio 0.35. Then scatter at skin_nn (mask-1 slots), post_filter (1-ring mean; a vertex without neighbours keeps its row),
    entries < ratio * row max -> 0, division by row sum + 1e-10."""
    if mode not in _MODES:
        raise ValueError(f"skin_weights: mode must be one of {sorted(_MODES)}")
    m, r0 = _MODES[mode]
    ratio = r0 if ratio is None else float(ratio)
    x = skin_cls_pred.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    k = x.shape[1]
    nn = skin_nn[:, :k].to(torch.int64).contiguous()
    msk = loss_mask[:, :k].to(torch.int64).contiguous()
    b = torch.as_tensor(batch).to(x.device).to(torch.int64).contiguous()
    nbs = [int(v) for v in n_bones]
    nb_d = torch.tensor(nbs, dtype=torch.int32, device=x.device)
    n = x.shape[0]
    if b.numel() and (int(b.min()) < 0 or int(b.max()) >= len(nbs)):
        raise ValueError("skin_weights: `batch` names a mesh without an entry in n_bones")
    ops = get_ops()
    P = ops.skin_scatter(x, nn, msk, b, nb_d, m, max(nbs))
    rowptr, cols = one_ring_csr(torch.as_tensor(tpl_edge_index).to(x.device), n)
    W = ops.skin_filter(P, rowptr, cols, b, nb_d, ratio)
    counts = torch.bincount(b, minlength=len(nbs)).tolist()
    out, off = [], 0
    for c, nb in zip(counts, nbs):
        out.append(W[off:off + c, :nb])
        off += c
    return out
