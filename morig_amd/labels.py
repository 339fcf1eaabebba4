"""Bone rays: the two per-model inputs of the rig-training and rig-evaluation loop that the reference only LOADS -- the per-vertex attention
ground truth ``{id}_attn.txt`` (datasets/dataset_rig.py:84 -> ``data.mask``, the target of masknet_motion's loss, training/train_rig.py:157)
and ``joint_featuresize/{id}.txt``, one length per ground-truth joint (evaluate/eval_rigging.py:100-120) -- computed on the device
(csrc/labels.hip, csrc/boneray_core.h, csrc/raytri_core.h). Both files come from RigNet's offline preprocessing,
which is not part of the reference. THE RULE BELOW IS THIS PRODUCT'S OWN: it is modelled on that preprocessing, no parity with it exists
or is claimed, and nobody has measured what its choices (``n_rays``, ``keep_factor``, ``radius``) do to a trained network's accuracy.

    bone_rays          host plan: the rays that leave every joint perpendicular to its bones
    cast_rays          the nearest hit of arbitrary rays on the meshes of a ragged batch
    select_hits        per joint: the 20th percentile of the hit distances, the kept hits, the feature size
    attention          per vertex: 1 where a kept hit lies within ``radius``
    bone_ray_labels    the four above in one call: attn float32 [V], featuresize float64 [J] and the details, per mesh
    rig_targets        nearest_jid, offsets and gt_skin of dataset_rig.py:90-93
    write_attn, write_featuresize, read_featuresize      the two files

The rule, all float64 in the written order. (1) Axes of joint j: one per child c with |pos[c] - pos[j]| > 1e-8, (pos[c] - pos[j]) / norm,
children ascending; without any, and with a parent farther than 1e-8, the single axis unit(pos[j] - pos[parent]); otherwise none. Frame of an
axis a: e = the coordinate axis of the smallest |a_k| (lowest k among equals), u = unit(a x e), w = a x u. Directions
d_i = c_i u + s_i w, (c_i, s_i) = (cos, sin)(2 pi i / n_rays) from numpy, i < n_rays; the origin is pos[j]. d is a unit vector up to rounding
only, so t is the distance up to rounding. Rays are ordered by (mesh, joint, child, i). (2) Every ray takes its nearest hit at t > 0 over all
faces of its mesh (raytri_core.h: division-free, touching counts), ties on t to the lowest face; ``orientation`` +1 keeps only hits with
d . n > 0 for n = (B - A) x (C - A), -1 the opposite, and a nearest hit of the wrong orientation makes the ray a MISS (it does not continue).
A miss has t = +inf, face = -1 and a NaN point. (3) Per joint, with s the hit t sorted ascending and n their number: h = 0.2 (n - 1),
lo = floor(h), p20 = s[lo] + (h - lo) (s[min(lo + 1, n - 1)] - s[lo]); a hit is kept when t <= keep_factor p20; featuresize = the kept t
added in ascending ray order over their count, ``fill`` when nothing is kept (NaN: ``d < fs`` is then never true in the metrics).
(4) attn[v] = 1.0 iff a kept hit of the vertex's mesh has (dx^2 + dy^2) + dz^2 <= radius^2.

Host reads: ONE status word per call of ``cast_rays`` / ``bone_ray_labels``; none in ``select_hits`` / ``attention`` / ``rig_targets``.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from .formats import NUM_MAX_JOINT
from .meshbatch import MeshBatch, bad_face
from .ragged import as_tensor, check_ptr, device_of, int32_table, ptr_of
from .runtime import get_ops

MAX_RAYS_PER_AXIS = 64
MAX_RAYS_PER_JOINT = 1024        # MORIG_RAY_MAX_PER_JOINT of include/morig_hip.h
MIN_BONE = 1e-8


class RayTable(NamedTuple):
    """``bone_rays``' plan, numpy: origins, dirs float64 [R, 3]; ray_ptr int64 [B + 1] the rays of every mesh; joint_ptr int64 [J + 1] the
    rays of every joint, the joints of all meshes concatenated in ``rig.pos`` order; ray_joint int64 [R] the joint of a ray within its mesh"""
    origins: np.ndarray
    dirs: np.ndarray
    ray_ptr: np.ndarray
    joint_ptr: np.ndarray
    ray_joint: np.ndarray


def _norm(v: np.ndarray) -> np.ndarray:
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def _cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _rig_arrays(rig, what: str):
    pos = np.asarray(rig.pos, dtype=np.float64).reshape(-1, 3)
    hier = np.asarray(rig.hierarchy, dtype=np.int64).reshape(-1)
    if len(hier) != len(pos) or np.any(hier >= len(pos)):
        raise ValueError(f"{what}: a rig's hierarchy names a joint outside it")
    return pos, hier


def _axes(pos: np.ndarray, hier: np.ndarray):
    """-> (joint int64 [A], axis float64 [A, 3]) ordered by (joint, child)"""
    J = len(pos)
    child = np.nonzero(hier >= 0)[0]
    parent = hier[child]
    vec = pos[child] - pos[parent]
    length = _norm(vec)
    with np.errstate(all="ignore"):
        far = length > MIN_BONE
    child, parent, vec, length = child[far], parent[far], vec[far], length[far]
    has_child = np.zeros(J, dtype=bool)
    has_child[parent] = True
    unit = vec / length[:, None]
    leaf = ~has_child[child]                                                            # no usable child, but this usable parent: one axis
    joint = np.concatenate([parent, child[leaf]])
    key = np.concatenate([child, np.zeros(int(leaf.sum()), dtype=np.int64)])
    axis = np.concatenate([unit, unit[leaf]], 0)
    order = np.lexsort((key, joint))
    return joint[order], axis[order]


def bone_rays(rigs: Sequence, n_rays: int = 14) -> RayTable:
    """The ray table of a batch of rigs (``pos`` [J, 3], ``hierarchy`` with -1 at the root), rule (1) of the module docstring: a host plan
    in numpy float64, like ``rigging.assembly_plan``, one pass of array statements over the joints of all rigs together. ``n_rays``: rays
    per axis, 1 .. 64; a joint with more than 1 024 rays is refused."""
    n_rays = int(n_rays)
    if not 1 <= n_rays <= MAX_RAYS_PER_AXIS:
        raise ValueError(f"bone_rays: n_rays {n_rays}: supported are 1 .. {MAX_RAYS_PER_AXIS}")
    arrays = [_rig_arrays(rig, "bone_rays") for rig in rigs]
    jptr = ptr_of([len(p) for p, _ in arrays])
    if jptr[-1] == 0:
        return RayTable(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(len(arrays) + 1, dtype=np.int64), np.zeros(1, dtype=np.int64),
                        np.zeros(0, dtype=np.int64))
    pos = np.concatenate([p for p, _ in arrays], 0)
    hier = np.concatenate([np.where(h >= 0, h + jptr[m], -1) for m, (_, h) in enumerate(arrays)])       # parents as rows of pos
    joint, a = _axes(pos, hier)
    counts = np.bincount(joint, minlength=len(pos)).astype(np.int64) * n_rays
    if counts.max() > MAX_RAYS_PER_JOINT:
        j = int(counts.argmax())
        m = int(np.searchsorted(jptr, j, side="right")) - 1
        raise ValueError(f"bone_rays: joint {j - int(jptr[m])} of rig {m} has {int(counts[j])} rays: at most {MAX_RAYS_PER_JOINT} per joint")
    ang = (2.0 * np.pi * np.arange(n_rays, dtype=np.float64)) / n_rays
    cs, sn = np.cos(ang), np.sin(ang)
    e = np.zeros_like(a)
    e[np.arange(len(a)), np.argmin(np.abs(a), 1) if len(a) else []] = 1.0
    u = _cross(a, e)
    u = u / _norm(u)[:, None]
    w = _cross(a, u)
    d = cs[None, :, None] * u[:, None, :] + sn[None, :, None] * w[:, None, :]           # [A, n_rays, 3]
    mesh = np.searchsorted(jptr, joint, side="right") - 1                               # joints ascend: the axes are grouped by mesh
    per_mesh = np.bincount(mesh, minlength=len(arrays)).astype(np.int64) * n_rays
    return RayTable(np.repeat(pos[joint], n_rays, 0), d.reshape(-1, 3), ptr_of(per_mesh), ptr_of(counts), np.repeat(joint - jptr[mesh], n_rays))


# ------------------------------------------------------------------------------------------------------------------------- device stages
def _rays(what: str, origins, dirs, ray_ptr, n_meshes: int, device):
    o, d = as_tensor(origins), as_tensor(dirs)
    if o.dim() != 2 or o.shape[1] != 3 or tuple(d.shape) != tuple(o.shape):
        raise ValueError(f"{what}: origins and dirs are [R, 3]")
    rp = check_ptr(np.asarray(ray_ptr.cpu() if isinstance(ray_ptr, torch.Tensor) else ray_ptr), int(o.shape[0]), f"{what}: ray_ptr")
    if len(rp) != n_meshes + 1:
        raise ValueError(f"{what}: ray_ptr has one segment per mesh")
    return (o.to(device=device, dtype=torch.float64).contiguous(), d.to(device=device, dtype=torch.float64).contiguous(), rp,
            int32_table(rp, device, what))


def _orientation(what: str, orientation) -> int:
    if orientation not in (-1, 0, 1):
        raise ValueError(f"{what}: orientation is -1, 0 or +1")
    return int(orientation)


def _raise_on(what: str, status: int, ops) -> None:
    if status & ops.RAY_BAD_FACE:
        raise bad_face(what)
    if status != 0:
        raise RuntimeError(f"{what}: status {status}")


def _split(t: torch.Tensor, ptr: np.ndarray) -> List[torch.Tensor]:
    return [t[ptr[b]:ptr[b + 1]] for b in range(len(ptr) - 1)]


def _accel(what: str, accel) -> bool:
    if accel not in (None, "bvh"):
        raise ValueError(f'{what}: accel is None or "bvh"')
    return accel == "bvh"


def _cast(ops, what: str, mesh: MeshBatch, o, d, rp_dev, orientation: int, accel: bool):
    """-> (t, face, point, status): ``morig_ray_cast``, or with ``accel`` the same results through a tree built here (spatial.py)"""
    if not accel:
        return ops.ray_cast(o, d, rp_dev, mesh.verts, mesh.vptr, mesh.faces, mesh.fptr, orientation)
    from . import spatial                                                                               # spatial imports this module
    return spatial._ray_cast(ops, spatial.MeshBVH(mesh, what), o, d, rp_dev, orientation, False)[:4]


def cast_rays(origins, dirs, ray_ptr, verts: Sequence, faces: Sequence, orientation: int = 0, accel=None):
    """The nearest hit of ARBITRARY rays, rule (2): ``origins``, ``dirs`` [R, 3] with mesh b owning the rows
    [ray_ptr[b], ray_ptr[b + 1]); ``verts[b]`` [V, 3], ``faces[b]`` integer [F, 3]. -> (t, face, point), each a list with one device
    tensor per mesh: t float64 [R_b] (+inf: a miss), face int32 (-1), point float64 [R_b, 3] = o + t d coordinate-wise (NaN). ``dirs``
    need not be unit vectors: t is the ray parameter. One wave per ray over all faces of its mesh; ``accel="bvh"`` builds the mesh
    BVH of ``spatial`` first and walks it instead, for the same results (worth it for large meshes; to cast
    several times against one mesh, build once and call ``spatial.cast_rays``). A face index outside its mesh is a ValueError (checked
    on the device, the call's one host read)."""
    orientation, accel = _orientation("cast_rays", orientation), _accel("cast_rays", accel)
    mesh = MeshBatch("cast_rays", verts, faces, like=(origins, dirs))
    o, d, rp, rp_dev = _rays("cast_rays", origins, dirs, ray_ptr, mesh.n, mesh.device)
    if mesh.n == 0:
        return [], [], []
    ops = get_ops()
    t, face, point, status = _cast(ops, "cast_rays", mesh, o, d, rp_dev, orientation, accel)
    _raise_on("cast_rays", int(status.cpu()[0]), ops)                                                   # the status read
    return _split(t, rp), _split(face, rp), _split(point, rp)


def _select(ops, what: str, t: torch.Tensor, joint_ptr, keep_factor: float, fill: float):
    jp = check_ptr(np.asarray(joint_ptr.cpu() if isinstance(joint_ptr, torch.Tensor) else joint_ptr), int(t.numel()), f"{what}: joint_ptr")
    most = int(np.diff(jp).max())
    if most > MAX_RAYS_PER_JOINT:
        raise ValueError(f"{what}: a joint with {most} rays: at most {MAX_RAYS_PER_JOINT} per joint")
    kept, stats = ops.ray_select(t, int32_table(jp, t.device, what), most, float(keep_factor), float(fill))
    return kept, stats, jp


def select_hits(t, joint_ptr, keep_factor: float = 2.0, fill: float = float("nan")) -> dict:
    """Rule (3) for hit distances ``t`` float64 [R] (+inf: a miss) with joint j owning [joint_ptr[j], joint_ptr[j + 1]), at most 1 024
    each. -> dict on the device: kept uint8 [R], n_hit, n_kept int32 [J], p20 float64 [J] (NaN without a hit), featuresize float64 [J]
    (``fill`` where nothing is kept). One wave per joint; no host read."""
    tt = as_tensor(t)
    tt = tt.to(device=device_of(tt), dtype=torch.float64).reshape(-1).contiguous()
    kept, stats, _ = _select(get_ops(), "select_hits", tt, joint_ptr, keep_factor, fill)
    return _stats_dict(kept, stats)


def _stats_dict(kept, stats) -> dict:
    return dict(kept=kept, n_hit=stats[:, 0].to(torch.int32), n_kept=stats[:, 1].to(torch.int32), p20=stats[:, 2].contiguous(),
                featuresize=stats[:, 3].contiguous())


def _radius(what: str, radius: float) -> float:
    radius = float(radius)
    if not (radius >= 0.0 and math.isfinite(radius)):
        raise ValueError(f"{what}: radius is finite and at least 0")
    return radius


def attention(verts: Sequence, point, kept, ray_ptr, radius: float = 0.02) -> List[torch.Tensor]:
    """Rule (4): ``verts[b]`` [V, 3]; ``point`` float64 [R, 3] and ``kept`` uint8 [R] with mesh b owning [ray_ptr[b], ray_ptr[b + 1]).
    -> per mesh attn float32 [V] on the device: 1.0 where a kept point lies within ``radius`` (closed), else 0.0. No host read."""
    radius = _radius("attention", radius)
    mesh = MeshBatch("attention", verts, like=(point, kept))
    p, k = as_tensor(point), as_tensor(kept)
    if p.dim() != 2 or p.shape[1] != 3 or k.numel() != p.shape[0]:
        raise ValueError("attention: point is [R, 3] with one kept flag per row")
    rp = check_ptr(np.asarray(ray_ptr.cpu() if isinstance(ray_ptr, torch.Tensor) else ray_ptr), int(p.shape[0]), "attention: ray_ptr")
    if len(rp) != mesh.n + 1:
        raise ValueError("attention: ray_ptr has one segment per mesh")
    if mesh.n == 0:
        return []
    dev, ops = mesh.device, get_ops()
    blk, n_blk = mesh.blocks(ops.RAY_BLOCK)
    attn = ops.ray_attention(mesh.verts, mesh.vptr, blk, n_blk, p.to(device=dev, dtype=torch.float64).contiguous(),
                                   (k.reshape(-1) != 0).to(device=dev, dtype=torch.uint8).contiguous(), int32_table(rp, dev, "attention"), radius)
    return mesh.split_v(attn)


def bone_ray_labels(verts: Sequence, faces: Sequence, rigs: Sequence, n_rays: int = 14, keep_factor: float = 2.0, radius: float = 0.02,
                    orientation: int = 0, fill: float = float("nan"), accel=None) -> List[tuple]:
    """The attention label and the joint feature sizes of every mesh, rules (1)-(4) of the module docstring. ``verts[b]`` [V, 3],
    ``faces[b]`` integer [F, 3], ``rigs[b]`` a ``formats.Rig`` (or anything with ``pos`` and ``hierarchy``) in the mesh's coordinates.
    -> per mesh (attn float32 [V], what ``load_rig_sample`` puts into ``data.mask``; featuresize float64 [J] in ``rig.pos`` order, what
    ``metrics.evaluate_rigs`` takes; details: dict of t float64 [R], face int32 [R], point float64 [R, 3], kept uint8 [R], ray_joint
    int64 [R], n_hit, n_kept int32 [J], p20 float64 [J]), all on the device. The defaults are this product's own choices; their effect on
    a trained network's accuracy is unmeasured. ``accel="bvh"`` casts through the mesh BVH of ``spatial`` (the same labels). Host reads:
    one status word."""
    orientation, accel = _orientation("bone_ray_labels", orientation), _accel("bone_ray_labels", accel)
    radius = _radius("bone_ray_labels", radius)
    rigs = list(rigs)
    mesh = MeshBatch("bone_ray_labels", verts, faces)
    if len(rigs) != mesh.n:
        raise ValueError("bone_ray_labels: one rig per mesh")
    table = bone_rays(rigs, n_rays)
    if mesh.n == 0:
        return []
    dev, ops = mesh.device, get_ops()
    o, d, rp, rp_dev = _rays("bone_ray_labels", table.origins, table.dirs, table.ray_ptr, mesh.n, dev)
    t, face, point, status = _cast(ops, "bone_ray_labels", mesh, o, d, rp_dev, orientation, accel)
    kept, stats, jp = _select(ops, "bone_ray_labels", t, table.joint_ptr, keep_factor, fill)
    blk, n_blk = mesh.blocks(ops.RAY_BLOCK)
    attn = ops.ray_attention(mesh.verts, mesh.vptr, blk, n_blk, point, kept, rp_dev, radius)
    _raise_on("bone_ray_labels", int(status.cpu()[0]), ops)                                              # the status read
    st = _stats_dict(kept, stats)
    jptr = ptr_of([len(np.asarray(r.pos).reshape(-1, 3)) for r in rigs])
    ray_joint = torch.from_numpy(table.ray_joint).to(dev)
    out = []
    for b, a in enumerate(mesh.split_v(attn)):
        rs, js = slice(rp[b], rp[b + 1]), slice(jptr[b], jptr[b + 1])
        out.append((a, st["featuresize"][js], dict(t=t[rs], face=face[rs], point=point[rs], kept=kept[rs], ray_joint=ray_joint[rs],
                                                   n_hit=st["n_hit"][js], n_kept=st["n_kept"][js], p20=st["p20"][js])))
    return out


def rig_targets(first_frame_vertices: Sequence, rigs: Sequence) -> List[tuple]:
    """The joint targets ``load_rig_sample`` derives (datasets/dataset_rig.py:90-93) for a batch: per mesh (nearest_jid int64 [V]: the
    joint with the smallest squared distance (dx^2 + dy^2) + dz^2 in float64, the first index among equals (morig_nearest_point);
    offsets float32 [V, 3] = joints[nearest_jid] - vertex, subtracted in float64 and rounded on return, as ``data.offsets`` is;
    gt_skin float32 [V, 48]: ``rig.skins`` padded with zero columns), on the device. No host read."""
    rigs = list(rigs)
    mesh = MeshBatch("rig_targets", first_frame_vertices)
    if len(rigs) != mesh.n:
        raise ValueError("rig_targets: one rig per mesh")
    if mesh.n == 0:
        return []
    dev = mesh.device
    pos = [np.asarray(r.pos, dtype=np.float64).reshape(-1, 3) for r in rigs]
    if any(len(p) < 1 for p in pos):
        raise ValueError("rig_targets: a rig without joints")
    jptr = ptr_of([len(p) for p in pos])
    joints = torch.from_numpy(np.concatenate(pos, 0)).to(dev)
    near = get_ops().nearest_point(mesh.verts, mesh.vptr, joints, int32_table(jptr, dev, "rig_targets"), True).long()
    base = torch.repeat_interleave(torch.from_numpy(jptr[:-1]).to(dev), torch.from_numpy(mesh.nv).to(dev), output_size=int(mesh.vptr_host[-1]))
    offsets = (joints[near + base] - mesh.verts).float()
    out = []
    for b, rig in enumerate(rigs):
        vs = slice(mesh.vptr_host[b], mesh.vptr_host[b + 1])
        skins = np.asarray(rig.skins, dtype=np.float64) if len(rig.skins) else np.zeros((int(mesh.nv[b]), 0))
        if skins.shape[0] != mesh.nv[b] or skins.shape[1] > NUM_MAX_JOINT:
            raise ValueError(f"rig_targets: rig {b}: skins are [V, J] with J <= {NUM_MAX_JOINT}")
        gt_skin = np.zeros((skins.shape[0], NUM_MAX_JOINT))
        gt_skin[:, :skins.shape[1]] = skins
        out.append((near[vs], offsets[vs], torch.from_numpy(gt_skin).float().to(dev)))
    return out


# ------------------------------------------------------------------------------------------------------------------------- files
def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_attn(filename: str, attn) -> None:
    """``{id}_attn.txt``: one ``%d`` per line, what ``np.loadtxt`` in ``formats.load_rig_sample`` reads back into ``data.mask``"""
    a = _host(attn).reshape(-1)
    with open(filename, "w") as f:
        f.write("".join("%d\n" % int(x) for x in a))


def write_featuresize(filename: str, rig, featuresize) -> None:
    """``joint_featuresize/{id}.txt``: ``"{name} {repr(float)}"`` per joint in ``rig.pos`` order, the lines
    evaluate/eval_rigging.py:21-28 (load_featuresize) parses; ``repr`` round-trips the float64 (and ``nan``)"""
    fs = _host(featuresize).astype(np.float64).reshape(-1)
    if len(fs) != len(rig.names):
        raise ValueError("write_featuresize: one value per joint of the rig")
    with open(filename, "w") as f:
        f.write("".join("{} {}\n".format(name, repr(float(x))) for name, x in zip(rig.names, fs)))


def read_featuresize(filename: str, rig) -> np.ndarray:
    """-> float64 [J] in ``rig.pos`` order (eval_rigging.py:101-105: a dict by joint name, then ``[fs_dict[n] for n in names]``)"""
    table = {}
    with open(filename, "r") as f:
        for line in f.readlines():
            w = line.strip().split()
            if w:
                table[w[0]] = float(w[1])
    missing = [n for n in rig.names if n not in table]
    if missing:
        raise ValueError(f"read_featuresize: {filename} has no line for joint {missing[0]!r}")
    return np.array([table[n] for n in rig.names], dtype=np.float64)
