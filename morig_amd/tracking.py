"""Rig tracking: evaluate/eval_tracking.py:56-170 (``ik_drag``, ``tracking_one``) on utils/deform_ik.py (``Deform_IK.run``).

``ik_solve``   a batch of inverse-kinematics problems in ONE launch of csrc/track.hip (morig_ik_solve): every Adam iteration runs inside
               the kernel, one workgroup per problem. There is no other path: without the library or a GPU it raises.
``ik_drag``    the two solves of the reference around it, batched over meshes: local vertices, the rig update in the reference's number
               formats, the correspondence selection from the features (morig_cosine_nn + morig_corr_select; no
               V x P matrix) or from an explicit ``corrmat``, the final skinning, quaternions.
``track``      ``tracking_one``: DeformNet, then ``ik_drag`` from the frame-0 vertices, frame after frame.
``flow_errors`` the two metrics of eval_tracking.py:230-231.

The per-joint host work (4 x 4 inverses, the rig's forward kinematics) is NumPy float64 as in the reference: a rig has tens of joints.
"""
from __future__ import annotations

import copy
from typing import List, Optional, Sequence

import numpy as np
import torch

from .formats import Rig, _with_self_loops
from .native import Mat, NativeOps
from .ragged import ptr_of
from .runtime import get_ops
from .synth import MeshData

VISMASK_THRD = 0.3                      # ik_drag's Deform_IK(vismask_thrd=0.3)
STAGE1 = dict(iter_time=200, lr=5e-2, w_invis=0.0)          # Deform_IK.run's defaults with ik_drag's iter_time (:72)
STAGE2 = dict(iter_time=400, lr=1e-3, w_invis=0.0)          # :125
SIM_THD, DIST_THD = 0.5, 1e-2           # :93, :107
BETA1, BETA2 = 0.9, 0.999


# ------------------------------------------------------------------------------------------------------------------- the solver
def tree_order(parent, root: int):
    """-> (order, level_ptr, child_lo, child_hi) int32: the joints breadth first from the root, a joint's children ascending and contiguous
    in ``order`` at [child_lo, child_hi), level_ptr the offsets of the tree levels in ``order``"""
    parent = np.asarray(parent).astype(np.int64).reshape(-1)
    n = len(parent)
    if not 0 <= root < n or parent[root] >= 0:
        raise ValueError("tree_order: root outside the joints or with a parent")
    kids = [[] for _ in range(n)]
    for j, p in enumerate(parent):
        if j != root:
            if not 0 <= p < n:
                raise ValueError("tree_order: parent index out of range")
            kids[p].append(j)
    order, level_ptr, level = [root], [0, 1], [root]
    lo, hi = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    while level:
        nxt = []
        for p in level:
            lo[p] = len(order) + len(nxt)
            nxt += kids[p]
            hi[p] = len(order) + len(nxt)
        order += nxt
        if nxt:
            level_ptr.append(len(order))
        level = nxt
    if len(order) != n:
        raise ValueError("tree_order: hierarchy is not a tree rooted at root")
    return np.array(order, dtype=np.int32), np.array(level_ptr, dtype=np.int32), lo, hi


def bias_tables(max_iter: int):
    """Adam's bias corrections as torch computes them from Python floats: 1 - beta1^t and (1 - beta2^t)^0.5 for t = 1 .. max_iter"""
    b1 = np.array([1 - BETA1 ** t for t in range(1, max_iter + 1)], dtype=np.float64)
    b2 = np.array([(1 - BETA2 ** t) ** 0.5 for t in range(1, max_iter + 1)], dtype=np.float64)
    return b1, b2


def make_problem(locals_in, offsets, parent, root, vptr, ent_j, ent_w, ent_x, constraints, vismask, iter_time=100, lr=5e-2, w_invis=0.0,
                 thrd=0.35) -> dict:
    """One solve: the arguments of Deform_IK.run with the skin as its non-zero entries (vptr [V + 1] offsets; per entry the joint, the
    weight and the vertex in that joint's frame, ascending joint inside a vertex). Defaults are Deform_IK's."""
    p = dict(locals_in=np.ascontiguousarray(locals_in, dtype=np.float32).reshape(-1, 3, 3),
             offsets=np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1, 3), parent=np.asarray(parent, dtype=np.int32).reshape(-1),
             root=int(root), vptr=np.asarray(vptr, dtype=np.int32).reshape(-1), ent_j=np.asarray(ent_j, dtype=np.int32).reshape(-1),
             ent_w=np.asarray(ent_w, dtype=np.float32).reshape(-1), ent_x=np.asarray(ent_x, dtype=np.float32).reshape(-1, 3),
             constraints=np.asarray(constraints, dtype=np.float32).reshape(-1, 3), vismask=np.asarray(vismask, dtype=np.float32).reshape(-1),
             iter_time=int(iter_time), lr=float(lr), w_invis=float(w_invis), thrd=float(thrd))
    J, V, E = len(p["parent"]), len(p["vismask"]), len(p["ent_j"])
    if J < 1 or V < 1 or p["iter_time"] < 1:
        raise ValueError("ik problem: at least one joint, one vertex and one iteration")
    if len(p["locals_in"]) != J or len(p["offsets"]) != J or len(p["vptr"]) != V + 1 or len(p["constraints"]) != V:
        raise ValueError("ik problem: array sizes disagree")
    if len(p["ent_w"]) != E or len(p["ent_x"]) != E or p["vptr"][0] != 0 or p["vptr"][-1] != E or np.any(np.diff(p["vptr"]) < 0):
        raise ValueError("ik problem: vptr does not describe the entries")
    if E and (p["ent_j"].min() < 0 or p["ent_j"].max() >= J):
        raise ValueError("ik problem: skin entry names a joint outside the rig")
    return p


def pack_problems(problems: Sequence[dict], device) -> tuple:
    """the members of morig_ik_args as device tensors -> (tensors, n_problems, max_joints, max_vertices, max_iter, joint_ptr, vert_ptr)"""
    cat = {k: [] for k in ("locals_in", "offsets", "parent", "order", "level_ptr", "child_lo", "child_hi", "vptr", "vent_j", "vent_xw", "jptr",
                           "jent_v", "jent_xw", "constraints", "vismask")}
    joint_ptr, vert_ptr, level_off, e_off = [0], [0], [0], 0
    for p in problems:
        J, V, E = len(p["parent"]), len(p["vismask"]), len(p["ent_j"])
        order, level_ptr, lo, hi = tree_order(p["parent"], p["root"])
        ev = np.repeat(np.arange(V, dtype=np.int32), np.diff(p["vptr"]))
        by_joint = np.lexsort((ev, p["ent_j"]))                                # joint-major copy, ascending vertex inside a joint
        xw = np.concatenate([p["ent_x"], p["ent_w"][:, None]], 1).astype(np.float32)
        for k, v in (("locals_in", p["locals_in"].reshape(-1)), ("offsets", p["offsets"].reshape(-1)), ("parent", p["parent"]), ("order", order),
                     ("level_ptr", level_ptr), ("child_lo", lo), ("child_hi", hi), ("vptr", p["vptr"][:-1] + e_off), ("vent_j", p["ent_j"]),
                     ("vent_xw", xw.reshape(-1)), ("jptr", ptr_of(np.bincount(p["ent_j"], minlength=J))[:-1] + e_off),
                     ("jent_v", ev[by_joint]), ("jent_xw", xw[by_joint].reshape(-1)), ("constraints", p["constraints"].reshape(-1)),
                     ("vismask", p["vismask"])):
            cat[k].append(v)
        e_off += E
        joint_ptr.append(joint_ptr[-1] + J)
        vert_ptr.append(vert_ptr[-1] + V)
        level_off.append(level_off[-1] + len(level_ptr))
    if e_off >= 2 ** 31:
        raise ValueError("ik batch: more than 2^31 skin entries")
    cat["vptr"].append([e_off])
    cat["jptr"].append([e_off])
    max_iter = max(p["iter_time"] for p in problems)
    b1, b2 = bias_tables(max_iter)
    host = {k: np.concatenate([np.asarray(x) for x in v]) for k, v in cat.items()}
    host.update(joint_ptr=joint_ptr, vert_ptr=vert_ptr, level_off=level_off, root=[p["root"] for p in problems],
                iter_time=[p["iter_time"] for p in problems], lr=[p["lr"] for p in problems], w_invis=[p["w_invis"] for p in problems],
                thrd=[p["thrd"] for p in problems], bias1=b1, bias2_sqrt=b2)
    dtype = {**{k: np.int32 for k in NativeOps.IK_FIELDS_I32}, **{k: np.float32 for k in NativeOps.IK_FIELDS_F32},
             **{k: np.float64 for k in NativeOps.IK_FIELDS_F64}}
    t = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=dtype[k]))).to(device) for k, v in host.items()}
    if e_off == 0:                                                             # all-zero skins: the kernel still wants valid pointers
        for k, n, dt in (("vent_j", 1, torch.int32), ("jent_v", 1, torch.int32), ("vent_xw", 4, torch.float32), ("jent_xw", 4, torch.float32)):
            t[k] = torch.zeros(n, dtype=dt, device=device)[:0]
    max_j = max(len(p["parent"]) for p in problems)
    max_v = max(len(p["vismask"]) for p in problems)
    return t, len(problems), max_j, max_v, max_iter, joint_ptr, vert_ptr


def ik_solve(problems: Sequence[dict], with_grad: bool = False, device="cuda") -> List[dict]:
    """Deform_IK.run for every problem (``make_problem``) in one launch -> per problem dict(angles [J,3], trans [3] after the last step;
    locals, globals [J,3,3], jpos [J,3] of the last iteration's forward[; loss, grad_angles, grad_trans of the last iteration]), float32
    NumPy arrays. A launch whose largest problem does not fit in LDS raises (MorigNativeError: unsupported)."""
    ops = get_ops()
    t, n, max_j, max_v, max_iter, joint_ptr, vert_ptr = pack_problems(problems, device)
    out = ops.ik_solve(t, n, max_j, max_v, max_iter, with_grad=with_grad)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    if np.any(host["status"] != 0):
        raise ValueError(f"ik_solve: the kernel refused problems {np.nonzero(host['status'])[0].tolist()} (status {host['status'].tolist()})")
    res = []
    for b in range(n):
        j0, j1 = joint_ptr[b], joint_ptr[b + 1]
        r = dict(angles=host["angles"][j0:j1], trans=host["trans"][b], locals=host["locals"][j0:j1], globals=host["globals"][j0:j1],
                 jpos=host["jpos"][j0:j1])
        if with_grad:
            r.update(loss=host["loss"][b], grad_angles=host["grad_angles"][j0:j1], grad_trans=host["grad_trans"][b])
        res.append(r)
    return res


# ------------------------------------------------------------------------------------------------------------------- rig pieces
def skin_entries(skins):
    """the non-zero entries of a dense V x J weight matrix, vertex-major, ascending joint -> (vptr int32 [V + 1], vertex, joint, weight)"""
    skins = np.asarray(skins)
    ev, ej = np.nonzero(skins)
    vptr = ptr_of(np.bincount(ev, minlength=len(skins))).astype(np.int32)
    return vptr, ev, ej, skins[ev, ej]


def local_vertices(globals_h, vtx, ev, ej):
    """inverse(globals_h)[joint] [v; 1] in float64 for the given (vertex, joint) entries -> ([E, 4] float64, the inverses)"""
    inv = np.linalg.inv(np.asarray(globals_h, dtype=np.float64))
    v1 = np.concatenate([np.asarray(vtx, dtype=np.float64), np.ones((len(vtx), 1))], 1)
    return np.einsum("eab,eb->ea", inv[ej], v1[ev]), inv


def skin_vertices(globals_h, local4, ev, ej, w, n_vtx):
    """linear-blend skinning in float64: sum over a vertex's entries of w (globals_h[joint] local)"""
    contrib = np.einsum("eab,eb->ea", np.asarray(globals_h, dtype=np.float64)[ej], local4)[:, :3] * np.asarray(w, dtype=np.float64)[:, None]
    out = np.zeros((n_vtx, 3))
    np.add.at(out, ev, contrib)
    return out


def update_rig(rig: Rig, jpos, locals_) -> Rig:
    """the reference's rig update after a solve (:75-78): a copy whose pos and local_frames are the solver's float32 results, then fk()"""
    out = copy.deepcopy(rig)
    out.pos = np.asarray(jpos, dtype=np.float32)
    out.local_frames = np.asarray(locals_, dtype=np.float32)
    out.fk()
    return out


def quat_from_matrix(m) -> np.ndarray:
    """[n, 3, 3] -> [n, 4] unit quaternions (x, y, z, w) in float64 by the rule scipy documents for Rotation.from_matrix(m).as_quat(): the
    nearest orthogonal matrix first (U V^T of the SVD), then the largest of (m00, m11, m22, trace) picks the branch of Markley's formula."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 3, 3)
    q = np.zeros((len(m), 4))
    for n, a in enumerate(m):
        u, _, vt = np.linalg.svd(a)
        a = u @ vt
        dec = np.array([a[0, 0], a[1, 1], a[2, 2], a[0, 0] + a[1, 1] + a[2, 2]])
        i = int(np.argmax(dec))
        if i != 3:
            j, k = (i + 1) % 3, (i + 2) % 3
            q[n, i] = 1 - dec[3] + 2 * a[i, i]
            q[n, j] = a[j, i] + a[i, j]
            q[n, k] = a[k, i] + a[i, k]
            q[n, 3] = a[k, j] - a[j, k]
        else:
            q[n] = [a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1], 1 + dec[3]]
        q[n] /= np.linalg.norm(q[n])
    return q


# ------------------------------------------------------------------------------------------------------------------- selection
def winners_from_corrmat(corrmat):
    """the reference's loop (:84-91) on an explicit V x P matrix: per point the vertex with the largest row maximum among the rows whose
    arg-max is the point, the first vertex on ties, maximum > 0 -> (winner int64 [P], -1 where none; its similarity [P])"""
    corrmat = np.asarray(corrmat)
    best_of_row, nn = corrmat.max(axis=1), corrmat.argmax(axis=1)
    n_pts = corrmat.shape[1]
    winner, best = np.full(n_pts, -1, dtype=np.int64), np.zeros(n_pts, dtype=np.float64)
    order = np.lexsort((np.arange(len(nn)), -best_of_row.astype(np.float64)))   # descending similarity, ascending vertex
    order = order[best_of_row[order] > 0]
    pts, first = np.unique(nn[order], return_index=True)                         # the first hit of a point in that order wins it
    winner[pts], best[pts] = order[first], best_of_row[order[first]]
    return winner, best


def winners_from_features(vtx_features: Sequence, pts_features: Sequence, device="cuda"):
    """the same per mesh from unit feature rows, on the device and without the V x P matrix: morig_cosine_nn (similarity GEMM fused with the
    row arg-max and maximum) over the whole batch, then morig_corr_select -> list of (winner, similarity) per mesh"""
    ops = get_ops()
    vf = torch.cat([torch.as_tensor(f, dtype=torch.float32) for f in vtx_features], 0).to(device).contiguous()
    pf = torch.cat([torch.as_tensor(f, dtype=torch.float32) for f in pts_features], 0).to(device).contiguous()
    vc, pc = [len(f) for f in vtx_features], [len(f) for f in pts_features]
    ptr_v = torch.tensor(ptr_of(vc), dtype=torch.int32, device=device)
    ptr_p = torch.tensor(ptr_of(pc), dtype=torch.int32, device=device)
    nn, sim = ops.cosine_nn(Mat.of(vf), ptr_v, Mat.of(pf), ptr_p, len(vc), max(vc))
    winner, wsim = ops.corr_select(nn, sim, int(sum(pc)))
    winner, wsim = winner.cpu().numpy().astype(np.int64), wsim.cpu().numpy().astype(np.float64)
    out, v0, p0 = [], 0, 0
    for nv, npt in zip(vc, pc):
        w = winner[p0:p0 + npt]
        out.append((np.where(w >= 0, w - v0, -1), wsim[p0:p0 + npt]))
        v0, p0 = v0 + nv, p0 + npt
    return out


def keep_pairs(winner, best, posed, pts):
    """similarity > 0.5, then squared distance < 1e-2 between the stage-1 posed vertex and the point (float64), ascending point order
    -> (pairs after the first filter, pairs after both) as [n, 2] (vertex, point)"""
    p1 = np.nonzero(best > SIM_THD)[0]
    pairs1 = np.stack([winner[p1], p1], 1).astype(np.int64)
    d2 = ((np.asarray(posed, dtype=np.float64)[pairs1[:, 0]] - np.asarray(pts)[pairs1[:, 1]]) ** 2).sum(-1)
    return pairs1, pairs1[d2 < DIST_THD]


# ------------------------------------------------------------------------------------------------------------------- ik_drag
def ik_drag(vtx_src: Sequence, vtx_dst: Sequence, pts_dst: Sequence, rig: Sequence[Rig], vtx_feature: Optional[Sequence] = None,
            pts_feature: Optional[Sequence] = None, vismask: Optional[Sequence] = None, corrmat: Optional[Sequence] = None, device="cuda",
            details: Optional[list] = None):
    """ik_drag (eval_tracking.py:56-154) for a list of meshes: every argument is a list with one entry per mesh (vtx_src / vtx_dst [V, 3],
    pts_dst [P, 3], a formats.Rig with skins, unit features [V, 64] / [P, 64] or an explicit ``corrmat`` [V, P], vismask [V]). Both solves
    are one launch each over all meshes. Without features and corrmat only the first solve runs, as in the reference; a mesh that keeps no
    correspondence also returns its first solve.
    -> (posed vertices [V, 3] float64, updated rigs, quaternions [J, 4] (x, y, z, w)) per mesh. ``details``: a list that receives per mesh
    dict(stage1_vtx, pairs_similarity, pairs, rig1, solve1, solve2)."""
    n = len(vtx_src)
    if vismask is None:
        raise ValueError("ik_drag: vismask is required")
    ents, locs, invs, probs = [], [], [], []
    for m in range(n):
        vptr, ev, ej, w = skin_entries(rig[m].skins)
        loc, _ = local_vertices(rig[m].global_transforms_homogeneous, vtx_src[m], ev, ej)
        ents.append((vptr, ev, ej, w))
        locs.append(loc)
        probs.append(make_problem(rig[m].local_frames, rig[m].offset, rig[m].hierarchy, rig[m].root_id, vptr, ej, w, loc[:, :3], vtx_dst[m],
                                  vismask[m], thrd=VISMASK_THRD, **STAGE1))
    sol1 = ik_solve(probs, device=device)
    rig1 = [update_rig(rig[m], sol1[m]["jpos"], sol1[m]["locals"]) for m in range(n)]
    posed1 = [skin_vertices(rig1[m].global_transforms_homogeneous, locs[m], ents[m][1], ents[m][2], ents[m][3], len(vtx_src[m])) for m in range(n)]
    if corrmat is None and vtx_feature is None:
        if details is not None:
            details.extend(dict(stage1_vtx=posed1[m], rig1=rig1[m], solve1=sol1[m]) for m in range(n))
        return posed1, rig1, [quat_from_matrix(r.local_frames) for r in rig1]
    if corrmat is not None:
        won = [winners_from_corrmat(c) for c in corrmat]
    else:
        won = winners_from_features(vtx_feature, pts_feature, device=device)
    probs2, pairs_all, locs_all, solved = [], [], [], []
    for m in range(n):
        pairs1, pairs = keep_pairs(won[m][0], won[m][1], posed1[m], pts_dst[m])
        pairs_all.append((pairs1, pairs))
        vptr, ev, ej, w = ents[m]
        loc_all, _ = local_vertices(rig1[m].global_transforms_homogeneous, posed1[m], ev, ej)     # every vertex, for the final skinning (:134)
        locs_all.append(loc_all)
        if len(pairs) == 0:                  # nothing to fit (the reference takes the mean of an empty loss there): the first solve stands
            continue
        rows = pairs[:, 0]
        sub_vptr = ptr_of((vptr[1:] - vptr[:-1])[rows]).astype(np.int32)
        take = np.repeat(vptr[rows] - sub_vptr[:-1], np.diff(sub_vptr)) + np.arange(sub_vptr[-1])       # the entries of the kept vertices
        probs2.append(make_problem(rig1[m].local_frames, rig1[m].offset, rig1[m].hierarchy, rig1[m].root_id, sub_vptr, ej[take],
                                   np.asarray(w)[take], loc_all[take, :3], np.asarray(pts_dst[m])[pairs[:, 1]],
                                   np.asarray(vismask[m])[rows], thrd=VISMASK_THRD, **STAGE2))
        solved.append(m)
    done = ik_solve(probs2, device=device) if probs2 else []
    sol2 = [None] * n
    for m, r in zip(solved, done):
        sol2[m] = r
    rig2 = [rig1[m] if sol2[m] is None else update_rig(rig1[m], sol2[m]["jpos"], sol2[m]["locals"]) for m in range(n)]
    posed2 = [posed1[m] if sol2[m] is None else
              skin_vertices(rig2[m].global_transforms_homogeneous, locs_all[m], ents[m][1], ents[m][2], ents[m][3], len(vtx_src[m]))
              for m in range(n)]
    if details is not None:
        details.extend(dict(stage1_vtx=posed1[m], pairs_similarity=pairs_all[m][0], pairs=pairs_all[m][1], rig1=rig1[m], solve1=sol1[m],
                            solve2=sol2[m]) for m in range(n))
    return posed2, rig2, [quat_from_matrix(r.local_frames) for r in rig2]


# ------------------------------------------------------------------------------------------------------------------- the frame loop
def deform_batch(vtx: Sequence, pts: Sequence, tpl_e: Sequence, geo_e: Sequence, device="cuda") -> MeshData:
    """run_deform_net_inference's Data (:33-44) for a list of meshes: float32 vertices and points, both edge lists with one self loop per
    vertex appended, PyG batch vectors"""
    d = MeshData()
    off, vs, ps, te, ge, vb, pb = 0, [], [], [], [], [], []
    for b in range(len(vtx)):
        v = torch.as_tensor(np.asarray(vtx[b])).float()
        p = torch.as_tensor(np.asarray(pts[b])).float()
        te.append(_with_self_loops(torch.as_tensor(np.asarray(tpl_e[b])).long(), len(v)) + off)
        ge.append(_with_self_loops(torch.as_tensor(np.asarray(geo_e[b])).long(), len(v)) + off)
        vs.append(v)
        ps.append(p)
        vb.append(torch.full((len(v),), b, dtype=torch.long))
        pb.append(torch.full((len(p),), b, dtype=torch.long))
        off += len(v)
    d.vtx, d.pts = torch.cat(vs, 0), torch.cat(ps, 0)
    d.pos = d.vtx
    d.tpl_edge_index, d.geo_edge_index = torch.cat(te, 1), torch.cat(ge, 1)
    d.vtx_batch, d.pts_batch = torch.cat(vb, 0), torch.cat(pb, 0)
    d.batch = d.vtx_batch
    d.num_graphs = len(vtx)
    return d.to(device)


def deform_inference(deformnet, vtx: Sequence, pts: Sequence, tpl_e: Sequence, geo_e: Sequence, device="cuda"):
    """run_deform_net_inference (:32-53) without the V x P matrix -> per mesh (vert_shift float64-promoted as the reference's
    ``vtx_in + pred_flow``, pred_vismask [V], vtx_feature, pts_feature)"""
    with torch.no_grad():
        flow, vf, pf, vis, _ = deformnet(deform_batch(vtx, pts, tpl_e, geo_e, device))
    flow, vf, pf, vis = flow.cpu().numpy(), vf.cpu().numpy(), pf.cpu().numpy(), vis.cpu().numpy()
    out, v0, p0 = [], 0, 0
    for b in range(len(vtx)):
        nv, npt = len(vtx[b]), len(pts[b])
        out.append((np.asarray(vtx[b]) + flow[v0:v0 + nv], vis[v0:v0 + nv, 0], vf[v0:v0 + nv], pf[p0:p0 + npt]))
        v0, p0 = v0 + nv, p0 + npt
    return out


def track(vtx0: Sequence, rigs: Sequence[Rig], pts_traj: Sequence, tpl_e: Sequence, geo_e: Sequence, deformnet, device="cuda"):
    """tracking_one (:157-170) for a list of meshes with sequences of one length: pts_traj[m] is [P, T, 3]. Frame t = 1 .. T - 1: DeformNet
    on the previous posed vertices and the frame's points, then ik_drag from the frame-0 vertices.
    -> per mesh (pred_vtx_traj [V, T - 1, 3], pred_vismask [V, T - 1], pred_quats [J, T - 1, 4])"""
    n = len(vtx0)
    T = int(np.asarray(pts_traj[0]).shape[1])
    if any(np.asarray(p).shape[1] != T for p in pts_traj):
        raise ValueError("track: the sequences of a batch have one length")
    prev = [np.asarray(v) for v in vtx0]
    traj, masks, quats = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    for t in range(1, T):
        pts = [np.asarray(p)[:, t, :] for p in pts_traj]
        inf = deform_inference(deformnet, prev, pts, tpl_e, geo_e, device)
        posed, _, q = ik_drag([np.asarray(v) for v in vtx0], [i[0] for i in inf], pts, rigs, [i[2] for i in inf], [i[3] for i in inf],
                              [i[1] for i in inf], device=device)
        prev = posed
        for m in range(n):
            traj[m].append(posed[m])
            masks[m].append(inf[m][1])
            quats[m].append(q[m])
    return [(np.stack(traj[m], 1), np.stack(masks[m], 1), np.stack(quats[m], 1)) for m in range(n)]


def track_piecewise(vtx0: Sequence, segs: Sequence, pts_traj: Sequence, tpl_e: Sequence, geo_e: Sequence, deformnet, vismask_threshold=0.3,
                    rng=None, device="cuda"):
    """The frame loop of ``track`` for meshes WITHOUT a rig: per frame t = 1 .. T - 1 DeformNet on the previous result and the frame's
    points gives the target and the visibility mask, then ``piecewise.piecewise_ransac`` moves every segment (``segs[m]``: integer labels
    [V], from ``piecewise.kernel_kmeans`` or ``piecewise.segments_from_skins``) of the PREVIOUS frame's result rigidly onto the target.
    The reference has the method (utils/piecewise_ransac.py) but no driver for it: this loop is this project's choice and mirrors
    ``tracking_one`` (eval_tracking.py:157-170). ``rng``: the ``np.random.RandomState`` of the sample draws (None: numpy's global one).
    -> per mesh (pred_vtx_traj [V, T - 1, 3] float64, pred_vismask [V, T - 1]), shaped like ``track``'s first two results;
    ``flow_errors`` applies unchanged."""
    from . import piecewise
    n = len(vtx0)
    T = int(np.asarray(pts_traj[0]).shape[1])
    if any(np.asarray(p).shape[1] != T for p in pts_traj):
        raise ValueError("track_piecewise: the sequences of a batch have one length")
    prev = [np.asarray(v) for v in vtx0]
    traj, masks = [[] for _ in range(n)], [[] for _ in range(n)]
    for t in range(1, T):
        pts = [np.asarray(p)[:, t, :] for p in pts_traj]
        inf = deform_inference(deformnet, prev, pts, tpl_e, geo_e, device)
        moved = piecewise.piecewise_ransac(prev, [i[0] for i in inf], [i[1] for i in inf], segs, vismask_threshold=vismask_threshold, rng=rng)
        prev = [v.cpu().numpy() for v in moved]
        for m in range(n):
            traj[m].append(prev[m])
            masks[m].append(inf[m][1])
    return [(np.stack(traj[m], 1), np.stack(masks[m], 1)) for m in range(n)]


def flow_errors(pred, gt, gt_vismask):
    """eval_tracking.py:230-231: pred [V, T - 1, 3] against gt [V, T, 3] (frame 0 dropped) -> (full_flow_error, vis_flow_error): the mean
    vertex distance, and the same over the entries with gt_vismask > 0.5"""
    gt, vis = np.asarray(gt)[:, 1:, :], np.asarray(gt_vismask)[:, 1:] > 0.5
    d = np.sqrt(np.sum((np.asarray(pred) - gt) ** 2, axis=2))
    return d.mean(), (d * vis).sum() / vis.sum()
