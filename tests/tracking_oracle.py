"""NumPy float64 restatement of the tracking stage (morig_amd/tracking.py, csrc/track.hip), written from the definitions in DESIGN.md
section 13: Euler rotations, forward kinematics, sparse linear-blend skinning, the masked mean-square loss, its ANALYTIC gradient
(no autograd anywhere), torch's Adam with L2 weight decay, the correspondence selection and the matrix -> quaternion rule.

A problem is a dict:
  locals_in [J,3,3]  offsets [J,3]  parent [J] (-1 at the root)  root (int)
  vptr [V+1], ent_j [E], ent_w [E], ent_x [E,3]   the non-zero skin entries of every vertex, ascending joint, with the vertex position
                                                   in that joint's frame
  constraints [V,3]  vismask [V]
"""
import numpy as np

BETA1, BETA2, EPS, WEIGHT_DECAY = 0.9, 0.999, 1e-8, 1e-4
INIT = 0.01


# ------------------------------------------------------------------------------------------------------------------- the tree
def bfs(parent, root):
    """-> (order, level_ptr, child_lo, child_hi): joints breadth first from the root, the children of a joint ascending and contiguous;
    level_ptr the offsets of the levels in ``order``; child_lo/hi [J] the range of a joint's children in ``order``"""
    parent = np.asarray(parent).astype(np.int64)
    J = len(parent)
    order, level_ptr = [int(root)], [0, 1]
    lo, hi = np.zeros(J, dtype=np.int32), np.zeros(J, dtype=np.int32)
    level = [int(root)]
    while level:
        nxt = []
        for p in level:
            ch = [int(c) for c in np.nonzero(parent == p)[0]]
            lo[p], hi[p] = len(order) + len(nxt), len(order) + len(nxt) + len(ch)
            nxt += ch
        order += nxt
        if nxt:
            level_ptr.append(len(order))
        level = nxt
    assert len(order) == J and len(set(order)) == J, "parent is not a tree rooted at root"
    return np.array(order, dtype=np.int32), np.array(level_ptr, dtype=np.int32), lo, hi


# ------------------------------------------------------------------------------------------------------------------- rotations
def axis_rotations(a, dtype=np.float64):
    """a [J,3] -> (Rx, Ry, Rz, dRx, dRy, dRz), each [J,3,3]"""
    a = np.asarray(a, dtype=dtype)
    c, s = np.cos(a), np.sin(a)
    J = len(a)
    z, o = np.zeros(J, dtype=dtype), np.ones(J, dtype=dtype)
    m = lambda rows: np.stack([np.stack(r, -1) for r in rows], -2)
    Rx = m([[o, z, z], [z, c[:, 0], -s[:, 0]], [z, s[:, 0], c[:, 0]]])
    Ry = m([[c[:, 1], z, s[:, 1]], [z, o, z], [-s[:, 1], z, c[:, 1]]])
    Rz = m([[c[:, 2], -s[:, 2], z], [s[:, 2], c[:, 2], z], [z, z, o]])
    dRx = m([[z, z, z], [z, -s[:, 0], -c[:, 0]], [z, c[:, 0], -s[:, 0]]])
    dRy = m([[-s[:, 1], z, c[:, 1]], [z, z, z], [-c[:, 1], z, -s[:, 1]]])
    dRz = m([[-s[:, 2], -c[:, 2], z], [c[:, 2], -s[:, 2], z], [z, z, z]])
    return Rx, Ry, Rz, dRx, dRy, dRz


def euler_matrix(a, dtype=np.float64):
    Rx, Ry, Rz = axis_rotations(a, dtype)[:3]
    return Rx @ (Ry @ Rz)


# ------------------------------------------------------------------------------------------------------------------- forward
def forward(angles, trans, prob, tree=None, dtype=np.float64):
    """-> (locals, globals, jpos)"""
    order = (tree or bfs(prob["parent"], prob["root"]))[0]
    L0, off, parent = np.asarray(prob["locals_in"], dtype), np.asarray(prob["offsets"], dtype), prob["parent"]
    L = euler_matrix(angles, dtype) @ L0
    G, P = np.zeros_like(L), np.zeros_like(off)
    root = int(prob["root"])
    G[root], P[root] = L[root], off[root] + np.asarray(trans, dtype)
    for c in order[1:]:
        p = int(parent[c])
        G[c] = G[p] @ L[c]
        P[c] = G[p] @ off[c] + P[p]
    return L, G, P


def entry_vertex(prob):
    vptr = np.asarray(prob["vptr"])
    return np.repeat(np.arange(len(vptr) - 1), np.diff(vptr))


def skin(G, P, prob, dtype=np.float64):
    ej, ew, ex = prob["ent_j"], np.asarray(prob["ent_w"], dtype), np.asarray(prob["ent_x"], dtype)
    V = len(prob["vptr"]) - 1
    contrib = ew[:, None] * (np.einsum("eab,eb->ea", G[ej], ex) + P[ej])
    out = np.zeros((V, 3), dtype=dtype)
    np.add.at(out, entry_vertex(prob), contrib)
    return out


def mask_of(vismask, thrd, w_invis, dtype=np.float64):
    """quirk (ii): (vismask > thrd) as 1.0, zeros replaced by w_invis"""
    m = (np.asarray(vismask) > thrd).astype(dtype)
    m[m == 0] = w_invis
    return m


def loss_and_gradient(angles, trans, prob, mask, tree=None, dtype=np.float64):
    """mean over V*3 of (out - c)^2 * mask and its analytic gradient -> (loss, g_angles [J,3], g_trans [3], (L, G, P)). With
    ``dtype=np.float32`` the same analytic route with every array, product and sum in float32 (the arithmetic of the reference's torch)"""
    tree = tree or bfs(prob["parent"], prob["root"])
    order, _, lo, hi = tree
    L0, off, parent = np.asarray(prob["locals_in"], dtype), np.asarray(prob["offsets"], dtype), prob["parent"]
    L, G, P = forward(angles, trans, prob, tree, dtype)
    out = skin(G, P, prob, dtype)
    V = len(out)
    d = out - np.asarray(prob["constraints"], dtype)
    loss = float((d * d * mask[:, None]).sum(dtype=dtype) / dtype(3 * V))
    r = dtype(2.0) * mask[:, None] * d / dtype(3 * V)                        # dLoss / d out_v
    ej, ew, ex, ev = prob["ent_j"], np.asarray(prob["ent_w"], dtype), np.asarray(prob["ent_x"], dtype), entry_vertex(prob)
    J = len(L0)
    gG, gP = np.zeros((J, 3, 3), dtype=dtype), np.zeros((J, 3), dtype=dtype)
    wr = ew[:, None] * r[ev]
    np.add.at(gG, ej, wr[:, :, None] * ex[:, None, :])                       # sum_v w r x^T
    np.add.at(gP, ej, wr)
    for p in order[::-1]:                                                    # child first: a joint is final before its parent reads it
        for c in order[lo[p]:hi[p]]:
            gP[p] += gP[c]
            gG[p] += np.outer(gP[c], off[c]) + gG[c] @ L[c].T
    gL = np.zeros_like(gG)
    for j in range(J):
        gL[j] = gG[j] if parent[j] < 0 else G[int(parent[j])].T @ gG[j]
    gR = gL @ np.transpose(L0, (0, 2, 1))
    Rx, Ry, Rz, dRx, dRy, dRz = axis_rotations(angles, dtype)
    g = np.stack([(gR * (dRx @ (Ry @ Rz))).sum((1, 2)), (gR * (Rx @ (dRy @ Rz))).sum((1, 2)), (gR * (Rx @ (Ry @ dRz))).sum((1, 2))], -1)
    assert g.dtype == dtype and gP.dtype == dtype and L.dtype == dtype and out.dtype == dtype
    return loss, g, gP[int(prob["root"])].copy(), (L, G, P)


# ------------------------------------------------------------------------------------------------------------------- Adam
class Adam:
    """torch.optim.Adam on one parameter array: L2 weight decay added to the gradient, bias corrections as torch applies them (Python
    floats); with ``dtype=np.float32`` the moments and every product are float32"""

    def __init__(self, shape, lr, weight_decay=WEIGHT_DECAY, dtype=np.float64):
        self.m, self.v, self.t, self.lr, self.wd, self.dtype = np.zeros(shape, dtype), np.zeros(shape, dtype), 0, float(lr), weight_decay, dtype

    def step(self, p, g):
        f = self.dtype
        self.t += 1
        g = g + f(self.wd) * p
        self.m = self.m + (g - self.m) * f(1 - BETA1)
        self.v = self.v * f(BETA2) + f(1 - BETA2) * g * g
        bc1, bc2 = 1 - BETA1 ** self.t, 1 - BETA2 ** self.t
        denom = np.sqrt(self.v) / f(np.sqrt(bc2)) + f(EPS)
        out = p - f(self.lr / bc1) * self.m / denom
        assert out.dtype == f and self.m.dtype == f and self.v.dtype == f
        return out


def solve(prob, iter_time, lr, w_invis=0.0, thrd=0.3, dtype=np.float64):
    """the whole solve -> dict(angles, trans: after the last step; locals, globals, jpos, loss, g_angles, g_trans: of the LAST forward,
    i.e. at the parameters before the last step (quirk i)). ``dtype=np.float32``: the float32 twin -- the same analytic route with every
    array, every product and the Adam state in float32, as the reference's torch computes; not the kernel (whose backward is float64)"""
    tree = bfs(prob["parent"], prob["root"])
    J = len(prob["parent"])
    a, t = np.full((J, 3), INIT, dtype=dtype), np.full(3, INIT, dtype=dtype)
    oa, ot = Adam((J, 3), lr * np.pi, dtype=dtype), Adam(3, lr, dtype=dtype)
    mask = mask_of(prob["vismask"], thrd, w_invis, dtype)
    for _ in range(int(iter_time)):
        loss, ga, gt, (L, G, P) = loss_and_gradient(a, t, prob, mask, tree, dtype)
        a, t = oa.step(a, ga), ot.step(t, gt)
    return dict(angles=a, trans=t, locals=L, globals=G, jpos=P, loss=loss, g_angles=ga, g_trans=gt)


def solve_f32(prob, iter_time, lr, w_invis=0.0, thrd=0.3):
    return solve(prob, iter_time, lr, w_invis, thrd, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------- selection
def select_pairs(max_sim, nn, n_points):
    """per point the vertex with the largest similarity among those whose arg-max is the point: first vertex on ties, similarity > 0.
    -> (winner [P] int64, -1 where none; winner_sim [P]; runner_up_margin [P])"""
    winner, best = np.full(n_points, -1, dtype=np.int64), np.zeros(n_points)
    margin = np.full(n_points, np.inf)
    for v in range(len(nn)):
        p = int(nn[v])
        if max_sim[v] > best[p]:
            if winner[p] >= 0:
                margin[p] = max_sim[v] - best[p]
            winner[p], best[p] = v, max_sim[v]
        elif winner[p] >= 0:
            margin[p] = min(margin[p], best[p] - max_sim[v])
    return winner, best, margin


def keep_pairs(winner, best, posed, pts, sim_thd=0.5, dist_thd=1e-2):
    """-> (pairs after the similarity filter [n,2], pairs after the distance filter [m,2], squared distances of the former), both in
    ascending point order, columns (vertex, point)"""
    p1 = np.nonzero(best > sim_thd)[0]
    pairs1 = np.stack([winner[p1], p1], 1).astype(np.int64)
    d2 = ((np.asarray(posed, np.float64)[pairs1[:, 0]] - np.asarray(pts, np.float64)[pairs1[:, 1]]) ** 2).sum(-1)
    return pairs1, pairs1[d2 < dist_thd], d2


# ------------------------------------------------------------------------------------------------------------------- quaternions
def quat_from_matrix(m):
    """[n,3,3] -> ([n,4] (x, y, z, w) unit quaternions, margin [n]), as scipy.spatial.transform.Rotation.from_matrix documents it: the
    matrix is first replaced by the nearest orthogonal one (orthogonal Procrustes: U V^T of its SVD; float32 frames are not orthogonal
    to float64 precision), then the largest of (m00, m11, m22, trace) picks the branch of Markley's formula; margin = the lead of that
    entry over the next"""
    m = np.asarray(m, dtype=np.float64)
    q, margin = np.zeros((len(m), 4)), np.zeros(len(m))
    for n, a in enumerate(m):
        u, _, vt = np.linalg.svd(a)
        a = u @ vt
        dec = np.array([a[0, 0], a[1, 1], a[2, 2], a[0, 0] + a[1, 1] + a[2, 2]])
        ch = int(np.argmax(dec))
        s = np.sort(dec)
        margin[n] = s[-1] - s[-2]
        if ch != 3:
            i = ch
            j, k = (i + 1) % 3, (i + 2) % 3
            q[n, i] = 1 - dec[3] + 2 * a[i, i]
            q[n, j] = a[j, i] + a[i, j]
            q[n, k] = a[k, i] + a[i, k]
            q[n, 3] = a[k, j] - a[j, k]
        else:
            q[n] = [a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1], 1 + dec[3]]
        q[n] /= np.linalg.norm(q[n])
    return q, margin


def quat_distance(a, b):
    """max over quaternions of the distance up to one sign each"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1)).max())


# ------------------------------------------------------------------------------------------------------------------- rig pieces
def local_entries(globals_h, vtx, skins):
    """the sparse skin of a dense weight matrix and the vertices in the joints' frames: inverse(globals_h) [v; 1] in float64, the
    entries with non-zero weight only -> (vptr, ent_j, ent_w float32, ent_x float32)"""
    skins = np.asarray(skins)
    ev, ej = np.nonzero(skins)                                               # row-major: vertex ascending, then joint ascending
    inv = np.linalg.inv(np.asarray(globals_h, np.float64))
    v1 = np.concatenate([np.asarray(vtx, np.float64), np.ones((len(vtx), 1))], 1)
    x = np.einsum("eab,eb->ea", inv[ej], v1[ev])[:, :3]
    vptr = np.concatenate([[0], np.cumsum(np.bincount(ev, minlength=len(skins)))]).astype(np.int32)
    return vptr, ej.astype(np.int32), skins[ev, ej].astype(np.float32), x.astype(np.float32)
