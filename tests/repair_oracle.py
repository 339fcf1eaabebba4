"""NumPy / pure-Python oracle of ``morig_amd.meshprep.repair``, written independently of the kernels' method: a
dict of edges, a breadth-first search with parity from the lowest face of every component, a dict walk along the boundary half-edges.
Three things come from tests/topology_oracle.py because the rule fixes them: the cleaning pass (``clean``), the component ROUND on the
double cover (``cc_rounds``: its labels must say what the search says -- asserted here on every call --, its round count is part of the
report) and the order of the sums (``lane_sum``). The pointer doubling is NOT restated: loops come from walking ``nxt``."""
import numpy as np

import topology_oracle as to

FIELDS = ("orientation_components", "nonorientable_components", "closed_components", "flipped_faces", "inverted_components",
          "boundary_loops", "tangled_boundary_edges", "filled_loops", "added_verts", "added_faces")


def term(v, t):
    """t(f) in the written order, as Python floats"""
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ([float(x) for x in v[i]] for i in t)
    return (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)


def edge_table(faces):
    """(lo, hi) -> [(face, dir), ...] in ascending face"""
    edges = {}
    for i, t in enumerate(faces):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            a, b = int(a), int(b)
            edges.setdefault((min(a, b), max(a, b)), []).append((i, 1 if a < b else 0))
    return edges


def orientation(v, faces):
    """-> dict(comp, parity, nonorientable roots, open faces, flip, counts, rounds)"""
    F = len(faces)
    edges = edge_table(faces)
    links = [(r[0][0], r[1][0], int(r[0][1] == r[1][1])) for r in edges.values() if len(r) == 2]
    open_faces = {i for r in edges.values() if len(r) != 2 for i, _ in r}
    adj = [[] for _ in range(F)]
    for f, g, p in links:
        adj[f].append((g, p))
        adj[g].append((f, p))
    comp, par, twisted = [-1] * F, [0] * F, set()
    for r in range(F):
        if comp[r] >= 0:
            continue
        comp[r], queue = r, [r]
        while queue:
            f = queue.pop(0)
            for g, p in adj[f]:
                if comp[g] < 0:
                    comp[g], par[g] = r, par[f] ^ p
                    queue.append(g)
                elif par[g] != par[f] ^ p:
                    twisted.add(r)
    # the double cover under the restated component round: the same components, the same parity, the same verdict
    lab, rounds = to.cc_rounds(2 * F, [(2 * f + s, 2 * g + (s ^ p)) for f, g, p in links for s in (0, 1)])
    for f in range(F):
        assert lab[2 * f] >> 1 == comp[f] and (lab[2 * f] == lab[2 * f + 1]) == (comp[f] in twisted), f
        assert comp[f] in twisted or (lab[2 * f] & 1 == par[f] and lab[2 * f + 1] == 2 * comp[f] + (1 ^ par[f])), f
    flip = np.zeros(F, dtype=bool)
    count = dict(orientation_components=0, nonorientable_components=0, closed_components=0, inverted_components=0)
    volume = {}
    for r in sorted(set(comp)):
        members = [f for f in range(F) if comp[f] == r]
        count["orientation_components"] += 1
        if r in twisted:
            count["nonorientable_components"] += 1
            continue
        closed = not any(f in open_faces for f in members)
        n1 = sum(par[f] for f in members)
        with np.errstate(all="ignore"):
            s = to.lane_sum([-term(v, faces[f]) if par[f] else term(v, faces[f]) for f in members])
        volume[r] = s
        by_volume = closed and (s > 0 or s < 0)
        cls = (1 if s > 0 else 0) if by_volume else (1 if n1 <= len(members) - n1 else 0)
        turned = [f for f in members if par[f] == cls]
        flip[turned] = True
        count["closed_components"] += int(closed)
        count["inverted_components"] += int(by_volume and len(turned) == len(members))
    return dict(comp=comp, parity=par, twisted=twisted, open_faces=open_faces, flip=flip, count=count, rounds=rounds, volume=volume, edges=edges)


def boundary(faces, flip, edges):
    """-> (half-edges [(from, to)], simple loops {label: [vertices in walk order]}, tangled half-edge count)"""
    half = []
    for (lo, hi), r in edges.items():
        if len(r) == 1:
            f, d = r[0]
            half.append((lo, hi) if bool(d) != bool(flip[f]) else (hi, lo))
    out, indeg = {}, {}
    for a, b in half:
        out.setdefault(a, []).append(b)
        indeg[b] = indeg.get(b, 0) + 1
    regular = lambda x: len(out.get(x, ())) == 1 and indeg.get(x, 0) == 1
    loops, seen = {}, set()
    for start in sorted(out):
        if start in seen or not regular(start):
            continue
        path, cur = [start], out[start][0]
        while cur != start and regular(cur) and len(path) <= len(half):
            path.append(cur)
            cur = out[cur][0]
        if cur == start:                                                         # every vertex on the way was regular
            loops[min(path)] = path
            seen.update(path)
    tangled = sum(1 for a, _ in half if a not in seen)
    return half, loops, tangled


def repair(v, f, weld=True, keep="all", orient=True, fill_holes=None):
    """-> dict(verts, faces, vertex_map, face_map, flipped, report, loops, centroids)"""
    cv, cf, vmap, fmap = to.clean(v, f, weld, keep)
    F = len(cf)
    report = {k: 0 for k in FIELDS}
    if orient:
        o = orientation(cv, cf)
        flip, edges = o["flip"], o["edges"]
        report.update(o["count"], flipped_faces=int(flip.sum()), orient_rounds=o["rounds"])
    else:
        flip, edges = np.zeros(F, dtype=bool), edge_table(cf)
        report["orient_rounds"] = 0
    faces = cf.copy()
    faces[flip] = faces[flip][:, [0, 2, 1]]
    half, loops, tangled = boundary(faces, flip, edges)
    report.update(boundary_loops=len(loops), tangled_boundary_edges=tangled)
    chosen = [] if fill_holes is None else [l for l in sorted(loops) if fill_holes == "all" or len(loops[l]) <= fill_holes]
    number = {x: k for k, l in enumerate(chosen) for x in loops[l]}
    with np.errstate(all="ignore"):
        centroids = np.array([[to.lane_sum([float(cv[x, d]) for x in sorted(loops[l])]) / len(loops[l]) for d in range(3)] for l in chosen]).reshape(-1, 3)
    new = [(b, a, len(cv) + number[a]) for a, b in sorted(half) if a in number]
    report.update(filled_loops=len(chosen), added_verts=len(chosen), added_faces=len(new))
    report["input"] = to.diagnose(v, f, weld)
    return dict(verts=np.concatenate([cv, centroids]), faces=np.concatenate([faces, np.array(new, dtype=np.int64).reshape(-1, 3)]), vertex_map=vmap,
                face_map=fmap, flipped=np.concatenate([flip, np.zeros(len(new), dtype=bool)]), report=report, loops=loops, centroids=centroids)


# ------------------------------------------------------------------------------------------------------------------------- generators
def cube():
    """the unit cube with every normal (B - A) x (C - A) pointing outward (topology_oracle.cube winds the other way)"""
    v, f = to.cube()
    return v, f[:, [0, 2, 1]].copy()


def flip_faces(f, which):
    f = np.array(f, dtype=np.int64)
    which = np.asarray(list(which), dtype=np.int64)
    f[which] = f[which][:, [0, 2, 1]]
    return f


def drop_faces(f, which):
    keep = np.ones(len(f), dtype=bool)
    keep[list(which)] = False
    return np.asarray(f)[keep]


def torus_disc(n, m, length):
    """a torus (n x m quads) with a disc cut out whose rim has ``length`` edges: 3: one triangle; 4: one quad; an even length 2 k + 2:
    k quads in a row; an odd length 2 k + 1: k - 1 quads in a row and one triangle of the next quad"""
    v, f = to.torus(n, m)
    if length == 3:
        return v, drop_faces(f, [0])
    quads, odd = (length - 2) // 2 if length % 2 == 0 else (length - 3) // 2, length % 2
    assert quads + odd <= n - 2
    gone = [2 * (i * m) + k for i in range(quads) for k in (0, 1)] + ([2 * (quads * m) + 1] if odd else [])
    return v, drop_faces(f, gone)


def bowtie():
    """a 3 x 3 grid of quads without two quads that touch at one vertex: that vertex has two boundary half-edges out and two in"""
    idx = lambda i, j: 4 * i + j
    v = np.array([[i, j, 0.0] for i in range(4) for j in range(4)], dtype=np.float64)
    f = [t for i in range(3) for j in range(3) if (i, j) not in ((0, 0), (1, 1))
         for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v, np.array(f, dtype=np.int64)


def cube_two_holes_touching():
    """a cube without one triangle of each of two neighbouring sides, chosen so that the two holes share exactly one vertex"""
    v, f = cube()
    sets = [set(t.tolist()) for t in f]
    for i in range(len(f)):
        for j in range(i + 1, len(f)):
            if len(sets[i] & sets[j]) == 1:
                return v, drop_faces(f, [i, j])
    raise AssertionError("no such pair")
