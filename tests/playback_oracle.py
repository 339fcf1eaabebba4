"""NumPy restatement of motion playback (csrc/playback.hip, csrc/pose_core.h) in the kernels' stated order of operations: every product
and sum below is written in the order the kernels execute it, on float64 arrays, so that the device results can be compared bit for bit.
Imports nothing of morig_amd. A rig is a dict(pos [J, 3] (its dtype matters), hierarchy [J] (parent, -1 at the root), root_id, offset
[J, 3] float64, global_transforms [J, 3, 3], skins [V, J]); see ``load_cases`` for the fixtures of tests/golden/playback_cases.npz."""
import json
import os

import numpy as np

FRAME_TILE = 64                                   # MORIG_POSE_FRAME_TILE
ERR_LANES = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "playback_cases.npz")


def bound(depth, scale):
    """first-order rounding bound of a chain of `depth` 3 x 3 products against another summation order (the issue's bound)"""
    return (8 * depth + 32) * 2.0 ** -53 * max(1.0, scale)


# ------------------------------------------------------------------------------------------------------------------- quaternions
def dot4(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def align_signs(q):
    q = np.array(q, dtype=np.float64)
    for t in range(1, q.shape[1]):
        flip = dot4(q[:, t], q[:, t - 1]) < 0.0
        q[flip, t] = -q[flip, t]
    return q


def smooth(quats, passes=2, align=False):
    """-> a new [J, T, 4] float64 array"""
    q = np.array(quats, dtype=np.float64)
    if align:
        q = align_signs(q)
    if q.shape[1] >= 3:
        for _ in range(passes):
            q[:, 1:-1] = ((q[:, 1:-1] + 0.5 * q[:, 2:]) + 0.5 * q[:, :-2]) / 2.0
    return q


def quat_matrices(q):
    """[..., 4] -> [..., 3, 3]: the matrix of q / |q|; ValueError on a zero or non-finite norm, as scipy raises"""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt(dot4(q, q))
    if not np.all((n > 0.0) & np.isfinite(n)):
        raise ValueError("quat_matrices: a quaternion has zero or non-finite norm")
    x, y, z, w = (q[..., c] / n for c in range(4))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = ((x2 - y2) - z2) + w2
    R[..., 0, 1] = 2.0 * (xy - zw)
    R[..., 0, 2] = 2.0 * (xz + yw)
    R[..., 1, 0] = 2.0 * (xy + zw)
    R[..., 1, 1] = ((y2 - x2) - z2) + w2
    R[..., 1, 2] = 2.0 * (yz - xw)
    R[..., 2, 0] = 2.0 * (xz - yw)
    R[..., 2, 1] = 2.0 * (yz + xw)
    R[..., 2, 2] = ((-x2 - y2) + z2) + w2
    return R


# ------------------------------------------------------------------------------------------------------------------- forward kinematics
def level_order(hierarchy, root):
    """(joints parent first, depth of the tree in edges)"""
    hier = np.asarray(hierarchy).astype(np.int64)
    order, level, depth = [int(root)], [int(root)], 0
    while level:
        level = [j for j in range(len(hier)) if j != root and hier[j] in level]
        order += level
        depth += bool(level)
    assert len(order) == len(hier)
    return order, depth


def mat_apply(M, t, v):
    """M [..., 3, 3], t [..., 3], v [..., 3] -> ((m0 v0 + m1 v1) + m2 v2) + t per row"""
    return ((M[..., :, 0] * v[..., None, 0] + M[..., :, 1] * v[..., None, 1]) + M[..., :, 2] * v[..., None, 2]) + t


def fk(rig, R, root_pos=None, unrounded=None):
    """R [J, T, 3, 3] -> (G [J, T, 3, 3] float64, pos [J, T, 3] in the dtype of rig['pos']); ``unrounded``: a list that receives the
    float64 value of every child position before it is rounded on store"""
    pos0 = np.asarray(rig["pos"])
    dt = np.float32 if pos0.dtype == np.float32 else np.float64
    J, T = R.shape[:2]
    root = int(rig["root_id"])
    offset = np.array(rig["offset"], dtype=np.float64)
    offset[root] = pos0[root]
    G, pos = np.zeros((J, T, 3, 3)), np.zeros((J, T, 3), dtype=dt)
    G[root] = R[root]
    pos[root] = pos0[root] if root_pos is None else np.asarray(root_pos).astype(dt)
    order, _ = level_order(rig["hierarchy"], root)
    for j in order[1:]:
        p = int(rig["hierarchy"][j])
        for b in range(3):
            G[j, :, :, b] = (G[p, :, :, 0] * R[j, :, None, 0, b] + G[p, :, :, 1] * R[j, :, None, 1, b]) + G[p, :, :, 2] * R[j, :, None, 2, b]
        exact = mat_apply(G[p], pos[p].astype(np.float64), np.broadcast_to(offset[j], (T, 3)))
        if unrounded is not None:
            unrounded.append(exact)
        pos[j] = exact.astype(dt)
    return G, pos


# ------------------------------------------------------------------------------------------------------------------- skinning
def inverse_transforms(A, p):
    """A [J, 3, 3], p [J, 3] -> (A^-1 by adjugate / determinant, -(A^-1 p))"""
    A = np.asarray(A, dtype=np.float64)
    a = A.reshape(-1, 9).T
    c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c0 + a[1] * c1) + a[2] * c2
    inv = np.stack([c0 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                    c1 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                    c2 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det], 1).reshape(-1, 3, 3)
    p = np.asarray(p, dtype=np.float64)
    t = -((inv[:, :, 0] * p[:, None, 0] + inv[:, :, 1] * p[:, None, 1]) + inv[:, :, 2] * p[:, None, 2])
    return inv, t


def entries(skins):
    """the non-zeros of a dense [V, J] matrix, vertex-major, ascending joint -> (vertex, joint, weight)"""
    skins = np.asarray(skins, dtype=np.float64)
    ev, ej = np.nonzero(skins)
    return ev, ej, skins[ev, ej]


def local_vertices(rig, vtx, ev, ej):
    inv, t = inverse_transforms(rig["global_transforms"], np.asarray(rig["pos"]).astype(np.float64))
    return mat_apply(inv[ej], t[ej], np.asarray(vtx, dtype=np.float64)[ev])


def skin(G, pos, local, ev, ej, w, n_vtx):
    """-> [V, T, 3]: per vertex its entries in stored order, acc = acc + w (G local + pos) from zero"""
    T = G.shape[1]
    out = np.zeros((n_vtx, T, 3))
    pos = pos.astype(np.float64)
    for e in range(len(ev)):
        if w[e] == 0.0:
            continue
        term = mat_apply(G[ej[e]], pos[ej[e]], np.broadcast_to(local[e], (T, 3)))
        out[ev[e]] = out[ev[e]] + w[e] * term
    return out


def replay(rig, vtx, quats, smooth_passes=2, align=False, root_pos=None, ent=None):
    """-> dict(quats, R, G, pos, local, traj)"""
    q = smooth(quats, smooth_passes, align)
    R = quat_matrices(q)
    G, pos = fk(rig, R, root_pos)
    ev, ej, w = entries(rig["skins"]) if ent is None else ent
    local = local_vertices(rig, vtx, ev, ej)
    return dict(quats=q, R=R, G=G, pos=pos, local=local, traj=skin(G, pos, local, ev, ej, w, len(vtx)))


# ------------------------------------------------------------------------------------------------------------------- errors
def trajectory_errors(pred, gt, vismask):
    """-> (full [T], vis [T]) in the kernel's order: vertex lane l of 16 adds l, l + 16, ... ascending, then the lanes ascending"""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    seen = (np.asarray(vismask) > 0.5)
    dx, dy, dz = (pred[..., c] - gt[..., c] for c in range(3))
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    V, T = d.shape
    S, SV = np.zeros(T), np.zeros(T)
    for lane in range(ERR_LANES):
        s, sv = np.zeros(T), np.zeros(T)
        for v in range(lane, V, ERR_LANES):
            s = s + d[v]
            sv = sv + d[v] * seen[v].astype(np.float64)
        S, SV = S + s, SV + sv
    with np.errstate(all="ignore"):
        return S / np.float64(V), SV / seen.sum(0).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- fixtures
def load_cases(path=GOLDEN):
    """-> (meta, list of dict): per case name, J, V, T, depth, rig (see the module text), vtx, quats (the input), and the reference's
    recorded ref_quats, ref_traj, ref_G, ref_pos [; aligned_in, ref_quats_aligned, ref_traj_aligned on the sign-flip case]"""
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    cases = []
    for i, m in enumerate(meta["cases"]):
        c = dict(m)
        for k in z.files:
            if k.startswith(f"c{i}_"):
                c[k[len(f"c{i}_"):]] = z[k]
        c["rig"] = dict(pos=c["pos"], hierarchy=c["hier"], root_id=int(m["root_id"]), offset=c["offset"], global_transforms=c["bind_G"],
                        skins=c["skins"])
        cases.append(c)
    return meta, cases


def midpoint_margin(values64):
    """the smallest distance of float64 values to a float32 rounding midpoint, relative to |value| (inf for a zero)"""
    v = np.asarray(values64, dtype=np.float64).reshape(-1)
    f = v.astype(np.float32)
    with np.errstate(all="ignore"):
        up, down = np.nextafter(f, np.float32(np.inf)).astype(np.float64), np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
        f = f.astype(np.float64)
        gap = np.minimum(np.abs(v - (f + up) / 2.0), np.abs(v - (f + down) / 2.0)) / np.abs(v)
    return float(np.min(np.where(v == 0.0, np.inf, gap))) if v.size else float("inf")
