"""Surface geodesics and vertex-to-bone distances on the MI355X-native op layer (csrc/geodesic.hip): the inference-side skinning
inputs, which the reference computes on the CPU.

Stage 1 -- data_proc/common_ops.py:175-211 ``calc_surface_geodesic``: a 5-NN graph over the surface samples filtered by their normals,
all-pairs shortest paths, the ``8 + euclid`` patch of unreachable pairs, the nearest sample of every vertex. The Poisson-disk sampling
and the normal estimation (open3d there) stay with the caller: the inputs are ``verts``, ``pts``, ``normals``.
Stage 2 -- evaluate/joint2rig.py:41-68 ``pts2line``, :307-360 ``calc_geodesic_matrix`` and the bind loop of ``predict_skinning``
(:413-442): the vertex-to-bone matrix and SkinNet's ``skin_input`` / ``skin_nn`` / ``loss_mask`` at inference time; the output plugs
into ``SkinMotion`` and ``skinning.skin_weights(mode="joint2rig")``.
Stage 3 -- evaluate/joint2rig.py:71-94 ``calc_pts2bone_visible_mat``: visibility of every vertex from every bone by ray casting
against an occluder mesh (trimesh there; a brute-force float64 Moeller-Trumbore here).

Everything is float64 and batched over the meshes of a batch (ragged sizes); the single-mesh functions are thin wrappers. Inputs may be
numpy arrays or tensors on any device; results are device tensors. No CPU fallback: without the library or a GPU this module raises
(arguments are validated first, so a bad call raises ``ValueError`` anywhere).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import ragged, spatial
from .labels import _accel
from .meshbatch import MeshBatch
from .ragged import cat_to, check_ptr, device_of, int32_table, ptr_of
from .runtime import get_ops

MAX_SAMPLES = 65535                  # include/morig_hip.h: a mesh's sample count
MIN_SAMPLES = 6                      # 5 neighbours besides the sample itself
LDS_DOUBLES = 16384                  # the shortest-path kernel's LDS budget: nsrc * S distances
NUM_NEAREST_BONE = 5                 # predict_skinning, joint2rig.py:408
_VIS_BLOCK = 256                     # (vertex, bone) pairs per workgroup of the visibility kernel: VIS_THREADS of csrc/geodesic.hip


def _as64(x, what: str, cols: int = 3) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{what}: expected [n, {cols}], got {tuple(t.shape)}")
    return t.to(torch.float64)


def _counts_of(ptr, n: int, what: str) -> List[int]:
    if ptr is None:
        return [n]
    p = np.asarray(ptr.cpu() if torch.is_tensor(ptr) else ptr, dtype=np.int64).reshape(-1)      # device tensors and any shape are taken
    return np.diff(check_ptr(p, n, f"{what}: ptr")).tolist()


# ---------------------------------------------------------------------------------------------------------------- stage 1
def surface_geodesic_samples(pts, normals, ptr=None, n_slots: Optional[int] = None, lds: Optional[bool] = None, return_stats: bool = False):
    """The sample-to-sample matrix of calc_surface_geodesic (``dist`` after the patch, common_ops.py:184-203): ``pts`` / ``normals``
    float64 [S, 3] -> float64 [S, S]. With ``ptr`` (prefix sums of the meshes' sample counts over the concatenated rows) every mesh of
    a batch runs in one launch -> a list of [S_b, S_b] views of one device buffer; that buffer holds sum S_b^2 doubles (128 MB per mesh
    at S = 4000), so a large batch is better run in chunks (``surface_geodesic_batched`` does). ``lds=False`` keeps the distance
    vectors in global memory (forced when a mesh has more than 16384 samples). ``return_stats``: also a dict (max_sweeps, total_sweeps
    over the jobs, jobs, nsrc sources per job, entries = directed adjacency entries of all meshes)."""
    p, nrm = _as64(pts, "surface_geodesic_samples: pts"), _as64(normals, "surface_geodesic_samples: normals")
    if p.shape != nrm.shape:
        raise ValueError("surface_geodesic_samples: pts and normals differ in shape")
    counts = _counts_of(ptr, p.shape[0], "surface_geodesic_samples")
    if min(counts) < MIN_SAMPLES:
        raise ValueError(f"surface_geodesic_samples: a mesh needs at least {MIN_SAMPLES} samples (5 neighbours each)")
    if max(counts) > MAX_SAMPLES:
        raise ValueError(f"surface_geodesic_samples: at most {MAX_SAMPLES} samples per mesh")
    smax = max(counts)
    if lds is None:
        lds = smax <= LDS_DOUBLES
    if lds and smax > LDS_DOUBLES:
        raise ValueError(f"surface_geodesic_samples: lds=True holds at most {LDS_DOUBLES} samples per mesh")
    nsrc = 4 if not lds else max(n for n in (1, 2, 4) if n * smax <= LDS_DOUBLES)
    device = device_of(pts, normals)
    jobs = [(c + nsrc - 1) // nsrc for c in counts]
    s_ptr, job_ptr, out_off = ptr_of(counts), ptr_of(jobs), ptr_of([c * c for c in counts])
    what = "surface_geodesic_samples"
    out, status = get_ops().surface_geodesic(p.to(device).contiguous(), nrm.to(device).contiguous(), int32_table(s_ptr, device, what),
                                             int32_table(job_ptr, device, what), torch.from_numpy(out_off).to(device), int(out_off[-1]), smax,
                                             int(job_ptr[-1]), nsrc, bool(lds), int(n_slots) if n_slots else ragged.n_slots(device))
    st = status.tolist()
    if st[0] == 1:
        raise RuntimeError("surface_geodesic_samples: a source did not settle within S sweeps")
    if st[0] != 0:
        raise RuntimeError(f"surface_geodesic_samples: status {st[0]}")
    mats = [out[int(out_off[i]):int(out_off[i + 1])].view(c, c) for i, c in enumerate(counts)]
    res = mats if ptr is not None else mats[0]
    return (res, dict(max_sweeps=st[2], total_sweeps=st[3], jobs=int(job_ptr[-1]), nsrc=nsrc, entries=st[4])) if return_stats else res


def nearest_sample(verts, pts, v_ptr=None, p_ptr=None, squared: bool = False) -> torch.Tensor:
    """np.argmin over the samples of the float64 distance (common_ops.py:206-207): the first minimum -> int32 [V], indices within the
    mesh's own samples. ``squared``: compare squared distances (joint2rig.py:356-357)."""
    v, p = _as64(verts, "nearest_sample: verts"), _as64(pts, "nearest_sample: pts")
    vc, pc = _counts_of(v_ptr, v.shape[0], "nearest_sample"), _counts_of(p_ptr, p.shape[0], "nearest_sample")
    if len(vc) != len(pc):
        raise ValueError("nearest_sample: v_ptr and p_ptr name different numbers of meshes")
    if any(a > 0 and b == 0 for a, b in zip(vc, pc)):
        raise ValueError("nearest_sample: a mesh without samples")
    device = device_of(verts, pts)
    return get_ops().nearest_point(v.to(device).contiguous(), int32_table(ptr_of(vc), device, "nearest_sample"), p.to(device).contiguous(),
                                   int32_table(ptr_of(pc), device, "nearest_sample"), squared)


def surface_geodesic(verts, pts, normals) -> torch.Tensor:
    """calc_surface_geodesic's return value for one mesh: ``dist[nn][:, nn]`` -> float64 [V, V]."""
    return surface_geodesic_batched([verts], [pts], [normals])[0]


def surface_geodesic_batched(verts_list, pts_list, normals_list, chunk: int = 8) -> List[torch.Tensor]:
    """calc_surface_geodesic for every mesh -> list of float64 [V_b, V_b]. The S x S matrices are made ``chunk`` meshes at a time and
    dropped once their V x V gather is taken."""
    if not (len(verts_list) == len(pts_list) == len(normals_list)):
        raise ValueError("surface_geodesic: one verts / pts / normals per mesh")
    vs = [_as64(v, "surface_geodesic: verts") for v in verts_list]
    ps = [_as64(p, "surface_geodesic: pts") for p in pts_list]
    ns = [_as64(n, "surface_geodesic: normals") for n in normals_list]
    for p, n in zip(ps, ns):
        if p.shape != n.shape:
            raise ValueError("surface_geodesic: pts and normals differ in shape")
        if not MIN_SAMPLES <= p.shape[0] <= MAX_SAMPLES:
            raise ValueError(f"surface_geodesic: {MIN_SAMPLES} .. {MAX_SAMPLES} samples per mesh")
    device = device_of(*verts_list, *pts_list)
    out = []
    for c0 in range(0, len(vs), max(int(chunk), 1)):
        sl = slice(c0, c0 + max(int(chunk), 1))
        P = cat_to(ps[sl], device)
        p_ptr = ptr_of([p.shape[0] for p in ps[sl]])
        mats = surface_geodesic_samples(P, cat_to(ns[sl], device), ptr=p_ptr)
        nn = nearest_sample(cat_to(vs[sl], device), P, ptr_of([v.shape[0] for v in vs[sl]]), p_ptr).long()
        o = 0
        for m, v in zip(mats, vs[sl]):
            i = nn[o:o + v.shape[0]]
            out.append(m[i][:, i])
            o += v.shape[0]
    return out


# ---------------------------------------------------------------------------------------------------------------- stages 2 and 3
def _bones_of(bones, what: str) -> torch.Tensor:
    b = _as64(bones, what + ": bones", 6)
    if b.shape[0] < 1:
        raise ValueError(f"{what}: a mesh without bones")
    return b


class _Pairs:
    """(vertex, bone) pairs of a batch: pair (v, c) of mesh b is element off[b] + v * nb_b + c"""

    def __init__(self, pos_list, bones_list, what: str):
        if len(pos_list) != len(bones_list) or not len(pos_list):
            raise ValueError(f"{what}: one pos / bones per mesh")
        self.what = what
        self.pos =[_as64(p, what + ": pos") for p in pos_list]
        self.bones = [_bones_of(b, what) for b in bones_list]
        self.nv = [p.shape[0] for p in self.pos]
        self.nb = [b.shape[0] for b in self.bones]
        self.off = ptr_of([v * n for v, n in zip(self.nv, self.nb)])
        self.n = int(self.off[-1])

    def to(self, device):
        self.device = device
        self.d_pos, self.d_bones = cat_to(self.pos, device), cat_to(self.bones, device)
        self.vtx_ptr, self.bone_ptr = int32_table(ptr_of(self.nv), device, self.what), int32_table(ptr_of(self.nb), device, self.what)
        self.d_off = torch.from_numpy(self.off).to(device)
        return self

    def split(self, flat: torch.Tensor, tail=()) -> List[torch.Tensor]:
        return [flat[int(self.off[i]):int(self.off[i + 1])].view(self.nv[i], self.nb[i], *tail) for i in range(len(self.nv))]


def bone_point_distance_batched(pos_list, bones_list):
    """pts2line for every mesh -> (origins list of [V_b, nb_b, 3], dist list of [V_b, nb_b])"""
    pr = _Pairs(pos_list, bones_list, "bone_point_distance")
    pr.to(device_of(*pos_list))
    origins, dist = get_ops().bone_point_distance(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, pr.d_off, pr.n)
    return pr.split(origins, (3,)), pr.split(dist)


def bone_point_distance(pos, bones):
    """pts2line (joint2rig.py:41-68) incl. its zero-length-bone branch: the nearest point of every bone to every vertex and the distance
    -> (origins float64 [V, nb, 3], dist float64 [V, nb]). (The reference lays the pairs out bone-major; this is its transpose, the
    layout calc_geodesic_matrix works in.)"""
    o, d = bone_point_distance_batched([pos], [bones])
    return o[0], d[0]


def _faces_of(faces, n_pts: int) -> torch.Tensor:
    f = faces if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces))
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"bone_visibility: tri_faces must be [F, 3], got {tuple(f.shape)}")
    if f.is_floating_point():
        raise ValueError("bone_visibility: tri_faces must be integers")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= n_pts):
        raise ValueError("bone_visibility: a face names a vertex out of range")
    return f.to(torch.int32)


def bone_visibility_batched(pos_list, bones_list, tri_pos_list, tri_faces_list, accel=None) -> List[torch.Tensor]:
    """calc_pts2bone_visible_mat for every mesh -> list of bool [V_b, nb_b]. ``accel="bvh"`` builds the occluders' mesh BVH
    (``spatial.MeshBVH``) and walks it, one wave per (vertex, bone), for the same mask (worth it for occluders of
    many thousand faces, not for the 3 000-face ones)."""
    bvh = _accel("bone_visibility", accel)
    pr = _Pairs(pos_list, bones_list, "bone_visibility")
    if not (len(tri_pos_list) == len(tri_faces_list) == len(pr.nv)):
        raise ValueError("bone_visibility: one occluder per mesh")
    tps = [_as64(t, "bone_visibility: tri_pos") for t in tri_pos_list]
    fs = [_faces_of(f, t.shape[0]) for f, t in zip(tri_faces_list, tps)]
    device = device_of(*pos_list)
    pr.to(device)
    if bvh:                                                                              # indices were checked above: the status word is not read
        tree = spatial.MeshBVH(MeshBatch(pr.what, tps, fs, like=(pr.d_pos,)), pr.what)
        m = tree.mesh
        vis = get_ops().bvh_bone_visibility(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, m.verts, m.vptr, m.faces, m.fptr, pr.d_off, pr.n,
                                            tree.order, tree.boxes, tree.node_ptr, tree.flags)[0]
        return [v.bool() for v in pr.split(vis)]
    blk_ptr, n_blocks = ragged.blocks([v * n for v, n in zip(pr.nv, pr.nb)], _VIS_BLOCK, device, pr.what)
    tptr, fptr = ptr_of([t.shape[0] for t in tps]), ptr_of([f.shape[0] for f in fs])
    vis = get_ops().bone_visibility(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, cat_to(tps, device), int32_table(tptr, device, pr.what),
                                    cat_to(fs, device), int32_table(fptr, device, pr.what), pr.d_off, blk_ptr, n_blocks, pr.n)
    return [v.bool() for v in pr.split(vis)]


def bone_visibility(pos, bones, tri_pos, tri_faces, accel=None) -> torch.Tensor:
    """calc_pts2bone_visible_mat (joint2rig.py:71-94): for every (vertex, bone) a ray from the bone's nearest point towards the vertex,
    direction (vertex - origin) + 1e-15, against the triangles (tri_pos [T, 3], tri_faces [F, 3]); min_hit = the nearest hit's distance
    from the origin over all hits at positive ray parameter, or the ray's length without a hit; visible iff |min_hit - length| < 1e-4
    -> bool [V, nb]. ``accel`` as in ``bone_visibility_batched``."""
    return bone_visibility_batched([pos], [bones], [tri_pos], [tri_faces], accel=accel)[0]


def _matrix(x, shape, what: str, dtype) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected {tuple(shape)}, got {tuple(t.shape)}")
    return t.to(dtype)


def bone_geodesic_matrix_batched(pos_list, bones_list, sg_list, visible_list, dist_list=None, return_aux: bool = False):
    """calc_geodesic_matrix (without sub-sampling) for every mesh -> list of float64 [V_b, nb_b]; ``return_aux``: also a dict of lists
    (visible_after bool [V, nb], nn int32 [V, nb], percentile float64 [nb])."""
    pr = _Pairs(pos_list, bones_list, "bone_geodesic_matrix")
    B = len(pr.nv)
    if not (len(sg_list) == len(visible_list) == B) or (dist_list is not None and len(dist_list) != B):
        raise ValueError("bone_geodesic_matrix: one surface_geodesic / visible / dist per mesh")
    sgs = [_matrix(s, (v, v), "bone_geodesic_matrix: surface_geodesic", torch.float64) for s, v in zip(sg_list, pr.nv)]
    vis = [_matrix(x, (v, n), "bone_geodesic_matrix: visible", torch.uint8) for x, v, n in zip(visible_list, pr.nv, pr.nb)]
    if dist_list is not None:
        dists = [_matrix(d, (v, n), "bone_geodesic_matrix: dist", torch.float64) for d, v, n in zip(dist_list, pr.nv, pr.nb)]
    device = device_of(*pos_list, *sg_list)
    pr.to(device)
    ops = get_ops()
    if dist_list is None:
        dist = ops.bone_point_distance(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, pr.d_off, pr.n)[1]
    else:
        dist = torch.cat([d.to(device).reshape(-1) for d in dists]).contiguous()
    sg_off = ptr_of([v * v for v in pr.nv])
    sg = sgs[0].to(device).contiguous().view(-1) if B == 1 else torch.cat([s.to(device).reshape(-1) for s in sgs])
    o = ops.bone_geodesic(dist, torch.cat([x.to(device).reshape(-1) for x in vis]).contiguous(), sg, torch.from_numpy(sg_off).to(device),
                          pr.vtx_ptr, pr.bone_ptr, pr.d_off, sum(pr.nb))
    res = pr.split(o["out"])
    if not return_aux:
        return res
    bp = ptr_of(pr.nb)
    return res, dict(visible_after=[x.bool() for x in pr.split(o["vis_after"])], nn=pr.split(o["nn"]),
                     percentile=[o["pct"][int(bp[i]):int(bp[i + 1])] for i in range(B)])


def bone_geodesic_matrix(pos, bones, surface_geodesic, visible, dist=None, subsample_ids=None, return_aux: bool = False):
    """calc_geodesic_matrix (joint2rig.py:307-360) given the visibility: per bone the 15th percentile (numpy's linear interpolation) of
    ``dist`` over the visible vertices, visibility cleared where dist > 1.3 x percentile; a visible pair takes dist, a bone without
    visible vertices takes dist for its whole column; an invisible vertex takes min over the visible of surface_geodesic[r, .] + the
    value at the first arg-min, or 8 + dist where that minimum is infinite -> float64 [V, nb]. ``dist``: pts2line's (computed when
    omitted). ``subsample_ids``: the reference's sub-sampled form -- ``visible`` (and ``dist``) are then [len(ids), nb], given for
    pos[ids]; the matrix is computed on pos[ids] with surface_geodesic[ids][:, ids] and every vertex takes the row of its nearest
    sub-sample by squared distance (first minimum)."""
    if subsample_ids is None:
        r = bone_geodesic_matrix_batched([pos], [bones], [surface_geodesic], [visible], None if dist is None else [dist], return_aux)
        return (r[0][0], {k: v[0] for k, v in r[1].items()}) if return_aux else r[0]
    p = _as64(pos, "bone_geodesic_matrix: pos")
    ids = subsample_ids if torch.is_tensor(subsample_ids) else torch.as_tensor(np.asarray(subsample_ids))
    if ids.dim() != 1 or ids.is_floating_point() or ids.numel() == 0:
        raise ValueError("bone_geodesic_matrix: subsample_ids must be a non-empty integer vector")
    if int(ids.min()) < 0 or int(ids.max()) >= p.shape[0]:
        raise ValueError("bone_geodesic_matrix: a subsample id out of range")
    sg = _matrix(surface_geodesic, (p.shape[0], p.shape[0]), "bone_geodesic_matrix: surface_geodesic", torch.float64)
    device = device_of(pos, surface_geodesic)
    ids = ids.to(device).long()
    p, sg = p.to(device), sg.to(device)
    sub = p[ids].contiguous()
    r = bone_geodesic_matrix_batched([sub], [bones], [sg[ids][:, ids].contiguous()], [visible], None if dist is None else [dist], return_aux)
    nn = nearest_sample(p, sub, squared=True).long()
    if return_aux:
        aux = {k: v[0] for k, v in r[1].items()}
        aux["nn_subsample"] = nn
        return r[0][0][nn], aux
    return r[0][nn]


def skin_inputs_joint2rig_batched(geo_list, bones_list, is_leaf_list, k: int = NUM_NEAREST_BONE):
    """predict_skinning's bind loop for every mesh in one launch -> (skin_input float32 [N, 8k], skin_nn, loss_mask int64 [N, k]),
    meshes concatenated."""
    if not (len(geo_list) == len(bones_list) == len(is_leaf_list)) or not len(geo_list):
        raise ValueError("skin_inputs_joint2rig: one geo_dist / bones / is_leaf per mesh")
    if int(k) < 1:
        raise ValueError("skin_inputs_joint2rig: k < 1")
    bones = [_bones_of(b, "skin_inputs_joint2rig") for b in bones_list]
    geos, leafs = [], []
    for g, b, lf in zip(geo_list, bones, is_leaf_list):
        t = g if torch.is_tensor(g) else torch.as_tensor(np.asarray(g))
        if t.dim() != 2 or t.shape[1] != b.shape[0]:
            raise ValueError(f"skin_inputs_joint2rig: geo_dist must be [V, {b.shape[0]}], got {tuple(t.shape)}")
        lf = np.asarray(lf.cpu() if torch.is_tensor(lf) else lf).astype(np.uint8).reshape(-1)
        if lf.shape[0] != b.shape[0]:
            raise ValueError("skin_inputs_joint2rig: one leaf flag per bone")
        geos.append(t.to(torch.float64))
        leafs.append(lf)
    device = device_of(*geo_list)
    nv, nb = [g.shape[0] for g in geos], [b.shape[0] for b in bones]
    off = ptr_of([v * n for v, n in zip(nv, nb)])
    what = "skin_inputs_joint2rig"
    return get_ops().skin_bind_geo(torch.cat([g.to(device).reshape(-1) for g in geos]).contiguous(), torch.from_numpy(off).to(device),
                                   int32_table(ptr_of(nv), device, what), int32_table(ptr_of(nb), device, what), sum(nv), cat_to(bones, device),
                                   torch.from_numpy(np.concatenate(leafs)).to(device), int(k))


def skin_inputs_joint2rig(geo_dist, bones, is_leaf, k: int = NUM_NEAREST_BONE):
    """predict_skinning's loop (joint2rig.py:413-442) -> (skin_input float32 [V, 8k], skin_nn int64 [V, k], loss_mask int64 [V, k]):
    per slot the bone (6), 1 / (D + 1e-10), the leaf flag; equal distances by ascending bone id; a slot past the
    bone count repeats the nearest bone with skin_nn = 0 and loss_mask = 0."""
    return skin_inputs_joint2rig_batched([geo_dist], [bones], [is_leaf], k)
