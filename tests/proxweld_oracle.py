"""NumPy / pure-Python oracle of the tolerance weld of ``morig_amd.meshprep.diagnose`` / ``clean``, written
independently of the kernels' method: brute force over all pairs of nodes, ``topology_oracle.union_find_labels`` for the classes, then
``topology_oracle.diagnose`` / ``clean`` on the vertices replaced by their representatives' coordinates. There is no grid here. Also the
mesh generators of the tolerance tests."""
import math

import numpy as np

import topology_oracle as to

WELD_FIELDS = ("near_verts", "weld_links", "weld_tol", "weld_spread")
EPS2_MIN = 2.0 ** -1022


# ------------------------------------------------------------------------------------------------------------------------- the rule
def len2(p, q):
    """(d0 d0 + d1 d1) + d2 d2, d = p - q, every operation rounded on its own"""
    with np.errstate(all="ignore"):
        d = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def links_of(v, nodes, eps):
    """every pair (u, w), u < w, of ``nodes`` (ascending rows) within the tolerance, in ascending order; a squared tolerance that is
    no normal double (0 or subnormal: below 2^-1022) links nothing"""
    eps2 = np.float64(eps) * np.float64(eps)
    out = []
    if eps2 >= EPS2_MIN:
        for k, u in enumerate(nodes):
            later = nodes[k + 1:]
            if len(later):
                out += [(int(u), int(w)) for w in later[len2(v[later], v[u]) <= eps2]]
    return out


def weld(v, eps):
    """-> dict(rep0: the exact representatives, rep: the final ones, links, near_verts, weld_links, weld_tol, weld_spread)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    rep0 = to.weld_rep(v)
    fin = np.isfinite(v).all(1)
    nodes = np.nonzero((rep0 == np.arange(len(v))) & fin)[0]
    links = links_of(v, nodes, eps)
    rep = to.union_find_labels(len(v), links)[rep0] if len(v) else rep0
    moved = fin & (rep != np.arange(len(v)))
    spread2 = float(len2(v[moved], v[rep[moved]]).max()) if moved.any() else 0.0
    return dict(rep0=rep0, rep=rep, links=links, near_verts=len(set(rep0.tolist())) - len(set(rep.tolist())), weld_links=len(links),
                weld_tol=float(eps), weld_spread=math.sqrt(spread2))


def moved(v, eps):
    """(the vertices replaced by their representatives' coordinates, the weld)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    w = weld(v, eps)
    out = v[w["rep"]]
    assert np.array_equal(to.weld_rep(out), w["rep"])                            # the exact weld of the moved mesh IS the tolerance weld
    return out, w


def diagnose(v, f, eps):
    out, w = moved(v, eps)
    r = to.diagnose(out, f)
    r.update({k: w[k] for k in WELD_FIELDS})
    return r


def clean(v, f, eps, keep="all", drop_unreferenced=True):
    return to.clean(moved(v, eps)[0], f, True, keep, drop_unreferenced)


def diagonal(v):
    """of the bounding box over the finite vertices; 0 where there is none"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    fin = v[np.isfinite(v).all(1)]
    if not len(fin):
        return 0.0
    e = fin.max(0) - fin.min(0)
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


# ------------------------------------------------------------------------------------------------------------------------- generators
def jitter(v, amplitude, seed=0):
    """every coordinate moved by at most ``amplitude``"""
    return v + np.random.default_rng(seed).uniform(-amplitude, amplitude, v.shape)


def seam_split(v, f, patch):
    """every patch of faces (``patch``: its number per face) with vertices of its own, as an OBJ with UV seams has them"""
    out_v, out_f, own = [], np.empty_like(f), {}
    for i, t in enumerate(f):
        for c, x in enumerate(t):
            k = (int(patch[i]), int(x))
            if k not in own:
                own[k] = len(out_v)
                out_v.append(v[x])
            out_f[i, c] = own[k]
    return np.array(out_v, dtype=np.float64).reshape(-1, 3), out_f


def seam_cube(amplitude=1e-9, seed=0):
    """the seam-split cube of the topology suite, jittered: 24 vertices in 8 clusters of 3"""
    v, f = to.split_cube()
    return jitter(v, amplitude, seed), f


def seam_torus(n, m, strips=4, amplitude=1e-9, seed=0):
    """a torus of n x m vertices cut into ``strips`` bands with vertices of their own along the cuts, jittered"""
    v, f = to.torus(n, m)
    patch = (np.arange(len(f)) // (2 * m)) * strips // n                          # the faces come ring by ring, 2 m to a ring
    sv, sf = seam_split(v, f, patch)
    return jitter(sv, amplitude, seed), sf


def chain(n, spacing, axis=0):
    """n points on a line, ``spacing`` apart, and no face"""
    v = np.zeros((n, 3))
    v[:, axis] = np.arange(n) * spacing
    return v, np.zeros((0, 3), dtype=np.int64)


def clusters(n_clusters, size, radius, seed=0):
    """``size`` points within ``radius`` of each of ``n_clusters`` far-apart centres, in shuffled order"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (n_clusters, 3)) * 50.0
    v = np.repeat(centres, size, 0) + rng.uniform(-radius, radius, (n_clusters * size, 3)) / math.sqrt(3.0)
    return v[rng.permutation(len(v))], np.zeros((0, 3), dtype=np.int64)


def subnormal_square(eps):
    """Three points on a line for a tolerance whose square is subnormal: the second just below the end of the first cell, the third
    eps (1 + 1e-4) on, two cells from the first. With squares rounded to multiples of 2^-1074 the comparison would accept the pair
    (1, 2) across a cell that the walk does not visit; the rule links nothing there."""
    h = eps * (1.0 + 2.0 ** -20)
    return np.array([[0.0, 0, 0], [0.99995 * h, 0, 0], [0.99995 * h + eps * (1.0 + 1e-4), 0, 0]])


DIRECTIONS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def border_pairs(eps, h, frac, extent):
    """A grid of cell side ``h`` anchored by the corners (0, 0, 0) and (extent, extent, extent), and for each of the 26 directions three
    pairs, four cells from the next: a point at ``frac`` of its cell on every axis (0: on the low border, so a step down leaves the
    cell; near 1: a step up does) and a partner along the direction at the length eps / |direction|, one ulp below and one ulp above --
    which of them link is what the brute force says. Also a partner half a tolerance below the top corner. -> vertices"""
    out = [np.zeros(3), np.full(3, float(extent)), np.array([extent - 0.5 * eps, extent, extent])]
    k = 0
    for d in DIRECTIONS:
        n = math.sqrt(sum(x * x for x in d))
        for step in (0, -1, 1):
            k += 1
            base = np.array([(4 * k + frac) * h, (4 + frac) * h, (4 + frac) * h])
            length = eps / n
            if step:
                length = np.nextafter(length, math.inf * step)
            out += [base, base + np.array(d, dtype=np.float64) * length]
    return np.array(out, dtype=np.float64)
