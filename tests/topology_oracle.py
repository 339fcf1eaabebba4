"""NumPy / pure-Python oracle of ``morig_amd.meshprep.diagnose`` / ``clean``, written independently of the kernels'
method: ``np.unique`` for the weld, dicts for faces and edges, union-find for the components. Two things are restated literally because
the rule fixes them: the component ROUND (``cc_rounds``: its labels must equal the union-find's, its round count is part of the result)
and the order of the area sum (``lane_sum``). Also the mesh generators of the topology tests."""
import math

import numpy as np

FIELDS = ("input_verts", "input_faces", "nonfinite_verts", "duplicate_verts", "degenerate_faces", "duplicate_faces", "faces",
          "zero_area_faces", "verts", "unreferenced_verts", "edges", "boundary_edges", "nonmanifold_edges", "orientation_conflicts",
          "components", "euler")


# ------------------------------------------------------------------------------------------------------------------------- the rule
def weld_rep(v, weld=True):
    """the representative (lowest index of its class) of every vertex"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    rep = np.arange(len(v))
    if weld and len(v):
        fin = np.nonzero(np.isfinite(v).all(1))[0]
        if len(fin):
            _, first, inv = np.unique(v[fin] + 0.0, axis=0, return_index=True, return_inverse=True)   # -0.0 + 0.0 = +0.0
            rep[fin] = fin[first[np.asarray(inv).reshape(-1)]]
    return rep


def normal(v, a, b, c):
    with np.errstate(all="ignore"):
        e1, e2 = v[b] - v[a], v[c] - v[a]
        return (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])


def face_area(v, t):
    n = normal(v, *t)
    return 0.5 * math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])


def lane_sum(terms):
    """the stated order: lane l of 64 adds the terms l, l + 64, ... one after the other, then lane l takes lane l + h, h = 32 .. 1"""
    s = [0.0] * 64
    for i, a in enumerate(terms):
        s[i % 64] = s[i % 64] + a
    h = 32
    while h:
        for l in range(h):
            s[l] = s[l] + s[l + h]
        h //= 2
    return s[0]


def union_find_labels(n, pairs):
    """label = the lowest vertex of the component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def cc_rounds(n, pairs):
    """The component round, restated: gp = cur[cur]; m[v] = min(gp[v], gp[n] over the neighbours n); next[v] = min(cur[v], m[v]); then
    next[cur[v]] = min(next[cur[v]], m[v]); repeated until a round changes nothing -> (labels, rounds with the last one)."""
    cur = np.arange(n, dtype=np.int64)
    p = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    rounds = 0
    while True:
        gp = cur[cur]
        m = gp.copy()
        np.minimum.at(m, p[:, 0], gp[p[:, 1]])
        np.minimum.at(m, p[:, 1], gp[p[:, 0]])
        nxt = np.minimum(cur, m)
        np.minimum.at(nxt, cur, m)
        rounds += 1
        if np.array_equal(nxt, cur):
            return cur, rounds
        cur = nxt
        assert rounds <= n + 2


def diagnose(v, f, weld=True):
    """-> dict: the report fields, ``watertight``, ``rounds`` and the intermediate results the tests compare (rep, surv, labels, the
    component table, the boundary edge list)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    rep = weld_rep(v, weld)
    surv, seen, kept = np.full(F, -1, dtype=np.int64), {}, []
    for i in range(F):
        t = tuple(int(rep[x]) for x in f[i])
        if len(set(t)) < 3:
            continue
        key = frozenset(t)
        if key not in seen:
            seen[key] = i
            kept.append((i, t))
        surv[i] = seen[key]
    edges = {}
    for i, t in kept:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            n, fw = edges.get((min(a, b), max(a, b)), (0, 0))
            edges[(min(a, b), max(a, b))] = (n + 1, fw + (1 if a < b else 0))
    referenced = sorted({x for _, t in kept for x in t})
    labels = union_find_labels(V, edges.keys())
    labels2, rounds = cc_rounds(V, edges.keys())
    roots = sorted({int(labels[x]) for x in referenced})
    number = {r: c for c, r in enumerate(roots)}
    comp = dict(root=np.array(roots, dtype=np.int64), verts=np.zeros(len(roots), dtype=np.int64), faces=np.zeros(len(roots), dtype=np.int64),
                boundary_edges=np.zeros(len(roots), dtype=np.int64), area=np.zeros(len(roots)))
    for x in referenced:
        comp["verts"][number[int(labels[x])]] += 1
    terms = [[] for _ in roots]
    for i, t in kept:
        c = number[int(labels[t[0]])]
        comp["faces"][c] += 1
        terms[c].append(face_area(v, t))
    for c in range(len(roots)):
        comp["area"][c] = lane_sum(terms[c])
    boundary = sorted(e for e, (n, _) in edges.items() if n == 1)
    for e in boundary:
        comp["boundary_edges"][number[int(labels[e[0]])]] += 1
    classes = len(set(rep.tolist()))
    r = dict(input_verts=V, input_faces=F, nonfinite_verts=int((~np.isfinite(v).all(1)).sum()), duplicate_verts=V - classes,
             degenerate_faces=int((surv < 0).sum()), duplicate_faces=int(((surv >= 0) & (surv != np.arange(F))).sum()), faces=len(kept),
             zero_area_faces=sum(1 for _, t in kept if all(x == 0.0 for x in normal(v, *t))), verts=len(referenced),
             unreferenced_verts=classes - len(referenced), edges=len(edges), boundary_edges=len(boundary),
             nonmanifold_edges=sum(1 for n, _ in edges.values() if n >= 3),
             orientation_conflicts=sum(1 for n, fw in edges.values() if n == 2 and fw != 1), components=len(roots))
    r["euler"] = r["verts"] - r["edges"] + r["faces"]
    r["watertight"] = bool(r["faces"] > 0 and not r["boundary_edges"] and not r["nonmanifold_edges"] and not r["orientation_conflicts"])
    r.update(rounds=rounds, rep=rep, surv=surv, kept=kept, labels=labels, labels_by_rounds=labels2, component_table=comp,
             boundary_edge_list=np.array(boundary, dtype=np.int64).reshape(-1, 2), edge_table=edges)
    return r


def clean(v, f, weld=True, keep="all", drop_unreferenced=True):
    """-> (verts, faces, vertex_map, face_map)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    d = diagnose(v, f, weld)
    comp, labels, rep, surv = d["component_table"], d["labels"], d["rep"], d["surv"]
    if keep == "all":
        stay = set(comp["root"].tolist())
    elif keep == "largest":
        stay = {int(comp["root"][int(np.argmax(comp["faces"]))])} if len(comp["root"]) else set()      # the first maximum: lowest label
    else:
        stay = {int(r) for r, n in zip(comp["root"], comp["faces"]) if n >= keep}
    faces_out = [(i, t) for i, t in d["kept"] if int(labels[t[0]]) in stay]
    if drop_unreferenced:
        vs = sorted({x for _, t in faces_out for x in t})
    else:
        vs = sorted(set(rep.tolist()))
    new = {x: k for k, x in enumerate(vs)}
    vmap = np.array([new.get(int(rep[x]), -1) for x in range(len(v))], dtype=np.int64)
    where = {i: k for k, (i, _) in enumerate(faces_out)}
    fmap = np.array([where.get(int(s), -1) if s >= 0 else -1 for s in surv], dtype=np.int64)
    out_f = np.array([[new[x] for x in t] for _, t in faces_out], dtype=np.int64).reshape(-1, 3)
    return v[vs].reshape(-1, 3), out_f, vmap, fmap


# ------------------------------------------------------------------------------------------------------------------------- generators
def torus(n, m=None, perm=None):
    m = m or n
    idx = lambda i, j: (i % n) * m + (j % m)
    v = np.array([[(2 + math.cos(2 * math.pi * j / m)) * math.cos(2 * math.pi * i / n), (2 + math.cos(2 * math.pi * j / m)) * math.sin(2 * math.pi * i / n),
                   math.sin(2 * math.pi * j / m)] for i in range(n) for j in range(m)])
    f = np.array([t for i in range(n) for j in range(m) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))])
    return renumber(v, f, perm)


def renumber(v, f, perm):
    """vertex p of the mesh becomes vertex perm[p]"""
    if perm is None:
        return v, f
    perm = np.asarray(perm, dtype=np.int64)
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[f]


_CUBE_QUADS = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))      # outward, corner = 4 x + 2 y + z
_CUBE_CORNERS = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])


def cube():
    f = [t for q in _CUBE_QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return _CUBE_CORNERS.copy(), np.array(f, dtype=np.int64)


def split_cube():
    """every side with four vertices of its own, as an OBJ with UV seams has them: 24 vertices, 12 faces"""
    v, f = [], []
    for q in _CUBE_QUADS:
        k = len(v)
        v += [_CUBE_CORNERS[c] for c in q]
        f += [(k, k + 1, k + 2), (k, k + 2, k + 3)]
    return np.array(v), np.array(f, dtype=np.int64)


def mobius(n=12):
    v = []
    for i in range(n):
        a = 2 * math.pi * i / n
        for s in (-0.5, 0.5):
            r = 2 + s * math.cos(a / 2)
            v.append([r * math.cos(a), r * math.sin(a), s * math.sin(a / 2)])
    f = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < n else (1, 0)                              # the twist
        f += [(a, c, b), (b, c, d)]
    return np.array(v), np.array(f, dtype=np.int64)


def shared_edge_tetrahedra():
    """two closed tetrahedra with the edge (0, 1) in common: that edge has four faces"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0.3], [0.5, 0.4, 1], [0.5, -1, -0.3], [0.5, -0.4, -1]], dtype=np.float64)
    tet = lambda a, b, c, d: [(a, b, c), (a, d, b), (b, d, c), (a, c, d)]
    return v, np.array(tet(0, 1, 2, 3) + tet(0, 1, 4, 5), dtype=np.int64)


def numbering(n, kind, seed=0):
    if kind == "ascending":
        return np.arange(n)
    if kind == "descending":
        return np.arange(n)[::-1].copy()
    if kind == "zigzag":
        return np.array([p // 2 if p % 2 == 0 else n - 1 - p // 2 for p in range(n)])
    return np.random.default_rng(seed).permutation(n)


def strip(n_verts, kind="ascending", seed=0):
    """a triangle strip of ``n_verts`` vertices (n_verts - 2 faces, consistently oriented), its vertices numbered by ``kind``"""
    v = np.array([[p // 2, p % 2, 0.0] for p in range(n_verts)], dtype=np.float64)
    f = np.array([(p, p + 1, p + 2) if p % 2 == 0 else (p + 1, p, p + 2) for p in range(n_verts - 2)], dtype=np.int64).reshape(-1, 3)
    return renumber(v, f, numbering(n_verts, kind, seed))


def fan(k, flip=()):
    """k faces on the edge (0, 1); the faces in ``flip`` traverse it high -> low"""
    v = [[0.0, 0, 0], [1.0, 0, 0]] + [[0.5, math.cos(2 * math.pi * i / (k + 1)) + 1.5, math.sin(2 * math.pi * i / (k + 1))] for i in range(k)]
    f = [(1, 0, 2 + i) if i in flip else (0, 1, 2 + i) for i in range(k)]
    return np.array(v), np.array(f, dtype=np.int64)
