"""Differential tests of csrc/geodesic.hip and csrc/skin.hip on GENERATED inputs: every case compares the device with the plain float64
oracle of tests/skin_oracle.py (pinned to the reference-made fixtures by tests/test_skin_oracle.py) on the same input, at the sizes the
kernels branch on: every instantiation of the shortest-path kernel and its global-memory path, ragged batches of stages 2 and 3 with
non-zero offsets, both branches of the percentile kernel, occluders around the triangle tile size, voxel rows on the word boundaries
and the grid border, ragged bind rows and weights.

Criteria are the project's own (tests/test_geodesic.py states why): bitwise for stage 1 and stage 2, exact for indices, booleans and
integer distances, 1e-6 for the final weights. Inputs are held to conditions instead of tolerances: a generator draws again until the
ORACLE alone confirms the margins the fixtures are held to (the 7 nearest distances of a sample differ by >= 1e-9, no |cos + 0.5| <
1e-6); a ray whose outcome rests on the order of float64 operations (skin_oracle.bone_visibility: ``unsure``) is left out of the
comparison, at most 0.1 % of a case's rays, asserted on the oracle's record before the device is consulted."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import skin_oracle as so  # noqa: E402
from morig_amd import geodesic, skinning, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = 20


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def npy(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- generators
def torus_params(seed):
    rng = np.random.default_rng([0x4D6F5269, seed])                                   # the first two draws of synth.make_mesh
    return 0.35 * (1.0 + 0.1 * rng.uniform(-1, 1)), 0.12 * (1.0 + 0.1 * rng.uniform(-1, 1))


def torus_samples(R, r, n, rng):
    """random points on the torus of synth.make_mesh with their analytic normals"""
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    pts = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v) + r, (R + r * np.cos(v)) * np.sin(u)], 1)
    nrm = np.stack([np.cos(v) * np.cos(u), np.sin(v), np.cos(v) * np.sin(u)], 1)
    return pts, nrm


def facing_sheets(n, rng):
    """two flat layers 0.008 apart with opposite, jittered normals, at the density of 600 points per unit square"""
    side = np.sqrt(n / 600.0)
    xz = rng.uniform(0, side, size=(n, 2))
    sgn = np.where(np.arange(n) < n // 2, 1.0, -1.0)
    pts = np.stack([xz[:, 0], 0.004 * sgn, xz[:, 1]], 1)
    nrm = np.stack([np.zeros(n), sgn, np.zeros(n)], 1) + rng.normal(0.0, 0.15, size=(n, 3))
    return pts, nrm


@functools.lru_cache(maxsize=None)
def sample_set(S):
    """(pts, normals, the oracle's graph). S < 600: random points with random normals (five neighbours connect everything) and at least
    one filtered arc. Otherwise a torus plus, far away, a pair of facing sheets: at least two components (the 8 + euclid patch) and
    filtered arcs. Both are asserted on the oracle's graph, with the fixtures' margins; a seed that misses them is drawn again."""
    for seed in range(SEEDS):
        rng = np.random.default_rng([0x5347, S, seed])
        if S < 600:
            pts, nrm = rng.normal(0.0, 1.0, size=(S, 3)), rng.normal(0.0, 1.0, size=(S, 3))
        else:
            n_sheet = S // 3
            pa, na = torus_samples(*torus_params(5), S - n_sheet, rng)
            pb, nb = facing_sheets(n_sheet, rng)
            pts, nrm = np.concatenate([pa, pb + np.array([3.0, 0.2, -0.4])]), np.concatenate([na, nb])
        g = so.SampleGraph(pts, nrm)
        gap, cmargin, removed = g.margins()
        ncomp = len(np.unique(g.components()))
        ok = gap >= 1e-9 and cmargin >= 1e-6 and removed >= 1 and (S < 600 or ncomp >= 2)
        print(f"sample_set S={S} seed {seed}: nn gap {gap:.2e} cos margin {cmargin:.2e} filtered {removed} components {ncomp} {'ok' if ok else 'rejected'}")
        if ok:
            return pts, nrm, g
    raise RuntimeError(f"sample_set({S}): no seed holds the margins")


def torus_faces(n_side):
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    a, b, c, d = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    return np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0).astype(np.int32)


def mesh_verts(seed, n_side):
    return synth.make_mesh(seed, n_side=n_side, with_skin=False, geo="none").pos.numpy().astype(np.float64)


def circle(R, r, deg, inward=0.0, up=0.0):
    a = np.deg2rad(deg)
    return np.array([(R - inward) * np.cos(a), r + up, (R - inward) * np.sin(a)])


def cube(c, h):
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)]) + c
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v, f


def random_bones(R, r, n, rng, boxed=None):
    """bones between jittered points of the tube's centre circle; every fifth of zero length; with 15 or more, bone 7 repeats bone 2
    (equal distances: the ascending-bone-id rule) and bone 4 is the zero-length bone ``boxed``"""
    bones = np.zeros((n, 6))
    for i in range(n):
        a = circle(R, r, rng.uniform(0, 360)) + rng.normal(0.0, 0.02, 3)
        b = circle(R, r, rng.uniform(0, 360)) + rng.normal(0.0, 0.02, 3)
        bones[i] = np.concatenate([a, a if i % 5 == 4 else b])
    if n >= 15:
        bones[7] = bones[2]
        if boxed is not None:
            bones[4] = np.concatenate([boxed, boxed])
    return bones


def seeded_surface(V, rng):
    """a symmetric matrix with zero diagonal, infinite between the lower and the upper half of the vertices, and with DUPLICATED
    rows / columns (equal minima: the first arg-min in vertex order must win)"""
    a = rng.uniform(0.05, 2.0, size=(V, V))
    sg = (a + a.T) * 0.5
    for j in range(1, V, 5):                                                           # every fifth vertex repeats its predecessor
        sg[j, :] = sg[j - 1, :]
        sg[:, j] = sg[:, j - 1]
    grp = np.arange(V) < V // 2
    sg[grp[:, None] != grp[None, :]] = np.inf
    sg[np.arange(V), np.arange(V)] = 0.0
    return sg


# ---------------------------------------------------------------------------------------------------------------- a. shortest paths
NSRC = {6: 4, 7: 4, 1023: 4, 1025: 4, 4096: 4, 4097: 2, 8192: 2, 8193: 1, 16385: 4}      # what geodesic.py:97 implies for the size


def chosen_sources(S):
    """0, 1, the four sources of the last full job at 4 per job, the last two, and 8 seeded others"""
    q = (S // 4 - 1) * 4
    extra = np.random.default_rng([0x537263, S]).integers(0, S, 8).tolist()
    return np.unique(np.array([0, 1, q, q + 1, q + 2, q + 3, S - 2, S - 1] + extra, dtype=np.int64))


@pytest.mark.parametrize("S", sorted(NSRC))
def test_shortest_paths_every_instantiation(S):
    pts, nrm, g = sample_set(S)
    src = chosen_sources(S)
    want = so.surface_geodesic_rows(pts, nrm, src, graph=g)
    if S >= 600:
        assert (want >= 8.0).any() and np.isfinite(want).all()                         # unreachable pairs: the patch branch is taken
    assert (~g.keep).any()                                                             # the normal filter removed arcs
    d, st = geodesic.surface_geodesic_samples(pts, nrm, return_stats=True)
    print(f"S={S}: nsrc {st['nsrc']} jobs {st['jobs']} sweeps max {st['max_sweeps']} mean {st['total_sweeps'] / st['jobs']:.1f} entries {st['entries']}")
    # which instantiation ran: the sources per job, and (above 16384 samples) the global-memory path, the only one the library accepts
    # 4 sources per job for at that size
    assert st["nsrc"] == NSRC[S] and st["jobs"] == (S + NSRC[S] - 1) // NSRC[S]
    assert (S > geodesic.LDS_DOUBLES) == (S == 16385)
    if S in (6, 7, 1023, 1025, 4097, 16385):
        assert st["jobs"] * st["nsrc"] > S                                             # a partial last job
    assert 1 <= st["max_sweeps"] <= S
    assert st["entries"] == g.n_entries                                                # the undirected CSR holds the oracle's arcs
    assert d.shape == (S, S) and d.dtype == torch.float64
    got = d[torch.from_numpy(src).to(d.device)]
    assert same_bits(got, want)
    assert bool((torch.diagonal(d) == 0).all())
    d3 = geodesic.surface_geodesic_samples(pts, nrm, n_slots=3)
    assert torch.equal(d, d3)
    del d, d3, got
    torch.cuda.empty_cache()


def test_shortest_paths_ragged_batch_is_nsrc_independent():
    sizes = (6, 601, 4097, 1023)
    sets = [sample_set(S) for S in sizes]
    pts, nrm = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    mats, st = geodesic.surface_geodesic_samples(pts, nrm, ptr=ptr, return_stats=True)
    assert st["nsrc"] == 2 and st["jobs"] == sum((S + 1) // 2 for S in sizes)           # the largest mesh decides for all four
    assert st["entries"] == sum(s[2].n_entries for s in sets)
    for S, (p, n, g), m in zip(sizes, sets, mats):
        one, st1 = geodesic.surface_geodesic_samples(p, n, return_stats=True)
        assert st1["nsrc"] == (2 if S == 4097 else 4)
        assert torch.equal(m, one)
        src = chosen_sources(S)[::3]
        assert same_bits(m[torch.from_numpy(src).to(m.device)], so.surface_geodesic_rows(p, n, src, graph=g))


# ---------------------------------------------------------------------------------------------------------------- b. nearest sample
def test_nearest_sample_ragged_exact_hits_and_duplicates():
    rng = np.random.default_rng(0x4E4E)
    v_counts, p_counts = [1, 300, 128, 77], [6, 50, 130, 9]
    assert v_counts[0] == 1 and any(v % 128 for v in v_counts[1:])
    verts, pts, firsts = [], [], []
    for V, P in zip(v_counts, p_counts):
        p = rng.normal(0.0, 1.0, size=(P, 3))
        p[P - 1] = p[2]                                                                # duplicated samples: the smaller index must win
        p[4] = p[1]
        v = rng.normal(0.0, 1.0, size=(V, 3))
        on = [P - 1, 2, 4, 1, 0, 3][:V]                                                # vertices exactly ON samples, duplicated ones too
        v[:len(on)] = p[on]
        verts.append(v)
        pts.append(p)
        firsts.append(np.array([{P - 1: 2, 4: 1}.get(i, i) for i in on]))
    vp, pp = np.concatenate([[0], np.cumsum(v_counts)]), np.concatenate([[0], np.cumsum(p_counts)])
    for squared in (False, True):
        got = npy(geodesic.nearest_sample(np.concatenate(verts), np.concatenate(pts), vp, pp, squared=squared))
        assert got.dtype == np.int32
        for i, (v, p) in enumerate(zip(verts, pts)):
            ids, best = so.nearest_sample(v, p, squared=squared)
            assert np.array_equal(got[vp[i]:vp[i + 1]], ids)
            assert np.array_equal(ids[:len(firsts[i])], firsts[i]) and (best[:len(firsts[i])] == 0).all()
            assert np.array_equal(npy(geodesic.nearest_sample(v, p, squared=squared)), ids)


# ---------------------------------------------------------------------------------------------------------------- c. stages 2 and 3
STAGE23 = [  # V, bones, occluder faces, torus (seed, n_side)
    (1, 1, 0, (5, 24)),
    (255, 2, 1, (5, 24)),
    (257, 15, 255, (6, 31)),
    (576, 33, 257, (5, 24)),
    (961, 7, 1922, (6, 31)),
]
ORDERS = [(0, 1, 2, 3, 4), (4, 2, 0, 3, 1)]


def _device_surface(pos, seed):
    """the device's surface_geodesic of a whole torus mesh, rows checked against the oracle"""
    for s in range(SEEDS):
        rng = np.random.default_rng([0x5347, seed, s])
        pts, nrm = torus_samples(*torus_params(seed), 640, rng)
        g = so.SampleGraph(pts, nrm)
        gap, cmargin, _ = g.margins()
        if gap >= 1e-9 and cmargin >= 1e-6:
            break
    else:
        raise RuntimeError("no sample set holds the margins")
    sg = geodesic.surface_geodesic(pos, pts, nrm)
    nn, _ = so.nearest_sample(pos, pts)
    assert np.array_equal(npy(geodesic.nearest_sample(pos, pts)), nn)
    rows = np.array([0, 1, len(pos) // 2, len(pos) - 1])
    want = so.surface_geodesic_rows(pts, nrm, nn[rows], graph=g)[:, nn]
    assert same_bits(sg[torch.from_numpy(rows).to(sg.device)], want)
    return sg.cpu().numpy()


@pytest.fixture(scope="module")
def stage23():
    """the five meshes with the oracle's results; asserts what the batch is built to reach"""
    meshes = []
    for i, (V, nb, nf, (seed, n_side)) in enumerate(STAGE23):
        rng = np.random.default_rng([0x533233, i])
        R, r = torus_params(seed)
        full = mesh_verts(seed, n_side)
        pos = full[:V].copy()
        faces = torus_faces(n_side)
        box = circle(R, r, 144.0)
        if nf in (255, 257):                                                           # a subset of the torus' faces plus the cube
            cv, cf = cube(box, 0.02)
            keep = np.sort(rng.permutation(len(faces))[:nf - len(cf)])
            tri_pos, tri_faces = np.concatenate([full, cv]), np.concatenate([faces[keep], cf + len(full)]).astype(np.int32)
        else:
            tri_pos, tri_faces = full, faces[:nf]
        assert len(tri_faces) == nf
        bones = random_bones(R, r, nb, rng, boxed=box)
        leaf = (np.arange(nb) % 3 == 1).astype(np.uint8)
        m = types.SimpleNamespace(V=V, nb=nb, pos=pos, bones=bones, leaf=leaf, tri_pos=tri_pos, tri_faces=tri_faces)
        m.sg = _device_surface(pos, seed) if V == n_side * n_side else seeded_surface(V, rng)
        m.origins, m.dist = so.pts2line(pos, bones)
        m.vis, m.unsure, _ = so.bone_visibility(pos, bones, tri_pos, tri_faces)
        share = m.unsure.mean()
        print(f"mesh {i}: V={V} bones={nb} faces={nf}: {int(m.vis.sum())} of {m.vis.size} rays visible, {int(m.unsure.sum())} left out ({100 * share:.4f} %)")
        assert share <= 1e-3                                                           # on the oracle's record, before the device is consulted
        m.out, m.vis_after, m.nn, m.pct, _, m.n_inf = so.restate(m.dist, m.vis, m.sg)
        m.ties = equal_minima(m)
        meshes.append(m)
    assert (np.sum((meshes[3].bones[:, 3:] - meshes[3].bones[:, :3]) ** 2, axis=1) < 1e-8).any()       # zero-length bones
    assert meshes[0].vis.all()                                                                        # no faces: everything visible
    assert any((~m.vis).all(0).any() for m in meshes) and any(np.isnan(m.pct).any() for m in meshes)  # an all-invisible column
    assert sum(m.n_inf for m in meshes) > 0                                                           # the 8 + dist branch
    assert sum(m.ties for m in meshes) > 0                                                            # equal minima: first arg-min
    assert any((m.vis & ~m.vis_after).any() for m in meshes)                                          # the 1.3 rule cleared something
    assert min(m.V * m.nb for m in meshes) < 256 < max(m.V * m.nb for m in meshes)                    # a pair count below one block
    return meshes


def equal_minima(m):
    """the number of (invisible vertex, bone) pairs whose finite minimum over the visible vertices is attained more than once"""
    n = 0
    for c in range(m.nb):
        ids, inv = np.flatnonzero(m.vis_after[:, c]), np.flatnonzero(~m.vis_after[:, c])
        if len(ids) and len(inv):
            sub = m.sg[np.ix_(inv, ids)]
            best = sub.min(1, keepdims=True)
            n += int((((sub == best).sum(1) > 1) & np.isfinite(best[:, 0])).sum())
    return n


def _cols(ms, name):
    return [getattr(m, name) for m in ms]


@pytest.mark.parametrize("order", ORDERS)
def test_stage23_batched_equals_oracle_and_single_mesh_calls(stage23, order):
    ms = [stage23[i] for i in order]
    assert ms[0].V * ms[0].nb > 0 and len(ms) == 5                                     # every later mesh sits at a non-zero offset
    pos, bones = _cols(ms, "pos"), _cols(ms, "bones")
    origins, dist = geodesic.bone_point_distance_batched(pos, bones)
    vis = geodesic.bone_visibility_batched(pos, bones, _cols(ms, "tri_pos"), _cols(ms, "tri_faces"))
    out_a, aux_a = geodesic.bone_geodesic_matrix_batched(pos, bones, _cols(ms, "sg"), _cols(ms, "vis"), _cols(ms, "dist"), return_aux=True)
    out_b, aux_b = geodesic.bone_geodesic_matrix_batched(pos, bones, _cols(ms, "sg"), _cols(ms, "vis"), None, return_aux=True)
    for i, m in enumerate(ms):
        o1, d1 = geodesic.bone_point_distance(m.pos, m.bones)
        assert same_bits(origins[i], m.origins) and same_bits(dist[i], m.dist)
        assert torch.equal(origins[i], o1) and torch.equal(dist[i], d1)
        v1 = geodesic.bone_visibility(m.pos, m.bones, m.tri_pos, m.tri_faces)
        assert vis[i].dtype == torch.bool and torch.equal(vis[i], v1)
        assert np.array_equal(npy(vis[i])[~m.unsure], m.vis[~m.unsure])
        s1, x1 = geodesic.bone_geodesic_matrix(m.pos, m.bones, m.sg, m.vis, m.dist, return_aux=True)
        for out, aux in ((out_a, aux_a), (out_b, aux_b)):
            assert same_bits(out[i], m.out) and torch.equal(out[i], s1)
            assert np.array_equal(npy(aux["visible_after"][i]), m.vis_after) and torch.equal(aux["visible_after"][i], x1["visible_after"])
            assert np.array_equal(npy(aux["nn"][i]), m.nn) and torch.equal(aux["nn"][i], x1["nn"])
            p = npy(aux["percentile"][i])
            assert np.array_equal(np.isnan(p), np.isnan(m.pct)) and same_bits(np.nan_to_num(p) + 0.0, np.nan_to_num(m.pct) + 0.0)
            assert np.array_equal(np.isnan(p), np.isnan(npy(x1["percentile"])))


def test_visibility_pair_counts_at_the_segment_edges_equal_the_meshes_alone_and_the_oracle():
    counts = [0, 1, 256, 0, 257, 255, 0]                       # (vertex, bone) pairs per mesh, one bone each: empty meshes in front, between, behind
    rng = np.random.default_rng(0x626c6b)
    (R, r), full, faces = torus_params(5), mesh_verts(5, 24), torus_faces(24)[::9]
    pos = [full[rng.permutation(len(full))[:n]] for n in counts]
    bones = [random_bones(R, r, 1, rng) for _ in counts]
    vis = geodesic.bone_visibility_batched(pos, bones, [full] * len(counts), [faces] * len(counts))
    seen = 0
    for p, b, got in zip(pos, bones, vis):
        want, unsure, _ = so.bone_visibility(p, b, full, faces)
        alone = geodesic.bone_visibility(p, b, full, faces)
        assert got.dtype == torch.bool and tuple(got.shape) == (len(p), 1) and torch.equal(got, alone)
        assert unsure.sum() <= 1e-3 * unsure.size and np.array_equal(npy(got)[~unsure], want[~unsure])
        seen += int(want.sum())
    assert 0 < seen < sum(counts)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", [1, 5, 20])
def test_joint2rig_bind_batched_equals_oracle_and_single_mesh_calls(stage23, order, k):
    ms = [stage23[i] for i in order]
    nbs = [m.nb for m in ms]
    if k > 1:
        assert min(nbs) < k < max(nbs)                                                 # k above some bone counts of the batch, below others
    assert any(np.array_equal(m.out[:, 7], m.out[:, 2]) for m in ms if m.nb >= 15)     # equal distances: ascending bone id
    si, nn, mask = geodesic.skin_inputs_joint2rig_batched(_cols(ms, "out"), _cols(ms, "bones"), _cols(ms, "leaf"), k)
    assert si.dtype == torch.float32 and nn.dtype == mask.dtype == torch.int64 and si.shape == (sum(m.V for m in ms), 8 * k)
    o = 0
    for m in ms:
        w_si, w_nn, w_mask = so.bind_joint2rig(m.out, m.bones, m.leaf, k)
        sl = slice(o, o + m.V)
        assert np.array_equal(npy(nn[sl]), w_nn) and np.array_equal(npy(mask[sl]), w_mask)
        assert np.array_equal(npy(si[sl]).view(np.int32), w_si.view(np.int32))
        s1, n1, m1 = geodesic.skin_inputs_joint2rig(m.out, m.bones, m.leaf, k)
        assert torch.equal(si[sl], s1) and torch.equal(nn[sl], n1) and torch.equal(mask[sl], m1)
        o += m.V


# ---------------------------------------------------------------------------------------------------------------- d. percentile
VISIBLE_COUNTS = (0, 1, 2, 3, 5, 7, 8, 12, 21, 41, 101)


def percentile_column(V, n, rng, ties):
    """(dist [V], visible [V]) with n visible vertices; ``ties``: the two order statistics of the 15th percentile each sit in a group of
    exactly equal distances (where n allows it)"""
    dist = rng.uniform(0.05, 1.0, V)
    vis = np.zeros(V, dtype=bool)
    ids = rng.permutation(V)[:n]
    vis[ids] = True
    if ties and n >= 2:
        lo = int(np.floor((n - 1) * 0.15))
        hi = min(lo + 1, n - 1)
        x = np.sort(dist[ids])
        x[max(lo - 1, 0):lo + 1] = x[lo]
        x[hi:min(hi + 2, n)] = x[hi]
        dist[ids] = x[rng.permutation(n)]
    return dist, vis


def check_geodesic_matrix(pos_list, bones_list, sg_list, vis_list, dist_list, sg_host):
    out, aux = geodesic.bone_geodesic_matrix_batched(pos_list, bones_list, sg_list, vis_list, dist_list, return_aux=True)
    for i in range(len(pos_list)):
        w_out, w_after, w_nn, w_pct, _, _ = so.restate(dist_list[i], vis_list[i], sg_host[i])
        p = npy(aux["percentile"][i])
        assert np.array_equal(np.isnan(p), np.isnan(w_pct)) and same_bits(np.nan_to_num(p) + 0.0, np.nan_to_num(w_pct) + 0.0)
        assert np.array_equal(npy(aux["visible_after"][i]), w_after)
        assert np.array_equal(npy(aux["nn"][i]), w_nn)
        assert same_bits(out[i], w_out)
    return aux


def test_percentile_chosen_visible_counts_and_ties():
    rng = np.random.default_rng(0x506374)
    V, nb = 300, len(VISIBLE_COUNTS)
    frac = [((n - 1) * 0.15) % 1.0 for n in VISIBLE_COUNTS if n]
    assert any(f == 0.0 for f in frac) and any(0 < f < 0.5 for f in frac) and any(f >= 0.5 for f in frac)
    assert (21 - 1) * 0.15 == 3.0 and (41 - 1) * 0.15 == 6.0                           # an exact integer virtual index
    pos, bones = rng.normal(size=(V, 3)), rng.normal(size=(nb, 6))
    sg = seeded_surface(V, rng)
    dists, viss = [], []
    for ties in (True, False):
        cols = [percentile_column(V, n, rng, ties) for n in VISIBLE_COUNTS]
        dists.append(np.stack([c[0] for c in cols], 1))
        viss.append(np.stack([c[1] for c in cols], 1))
    straddle = 0
    for c, n in enumerate(VISIBLE_COUNTS):
        x = np.sort(dists[0][viss[0][:, c], c])
        lo = int(np.floor((n - 1) * 0.15))
        if lo >= 1 and lo + 2 < n:
            straddle += int(x[lo - 1] == x[lo] and x[lo + 1] == x[lo + 2] and (x[lo] < x[lo + 1]))
    assert straddle >= 4                                                               # equal groups on both order statistics
    aux = check_geodesic_matrix([pos, pos], [bones, bones], [sg, sg], viss, dists, [sg, sg])
    assert np.isnan(npy(aux["percentile"][0])[0]) and not np.isnan(npy(aux["percentile"][0])[1:]).any()   # n = 0 -> NaN


def test_percentile_staged_and_unstaged_branch():
    """V = 8192 stages the column in LDS, V = 8193 reads global memory (PCT_CAP of csrc/geodesic.hip); one batch, so the second mesh's
    surface matrix sits at an offset of 8192^2"""
    rng = np.random.default_rng(0x38313932)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(8192)
    pos, bones, sgs, host, dists, viss = [], [], [], [], [], []
    for V in (8192, 8193):
        a = torch.rand(V, V, generator=gen, device=DEV, dtype=torch.float64)
        sg = a + a.T + 0.01
        for i, j in [(5, 3), (4000, 17), (8000, 8100)]:                                # duplicated rows / columns: equal minima
            sg[j, :] = sg[i, :]
            sg[:, j] = sg[:, i]
        half = torch.arange(V, device=DEV) < V // 3
        sg[half[:, None] != half[None, :]] = float("inf")
        sg.fill_diagonal_(0.0)
        cols = [percentile_column(V, 3000, rng, False), percentile_column(V, 2001, rng, True), percentile_column(V, 8, rng, True)]
        d = np.stack([c[0] for c in cols], 1)
        d[:, 1] = np.round(d[:, 1] * 16.0) / 16.0                                      # heavy ties: the u < v rule of the rank count
        pos.append(rng.normal(size=(V, 3)))
        bones.append(rng.normal(size=(3, 6)))
        sgs.append(sg)
        host.append(sg.cpu().numpy())                                                  # copied once, for the oracle
        dists.append(d)
        viss.append(np.stack([c[1] for c in cols], 1))
        del a
    assert pos[0].shape[0] == 8192 and pos[1].shape[0] > 8192                          # the staged and the unstaged branch
    check_geodesic_matrix(pos, bones, sgs, viss, dists, host)
    check_geodesic_matrix(pos[1:], bones[1:], sgs[1:], viss[1:], dists[1:], host[1:])
    del sgs, host
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- e. volumetric geodesic
def _vox(mask):
    return types.SimpleNamespace(data=mask, translate=[0.0, 0.0, 0.0], scale=1.0, dims=[88, 88, 88])


def _world(*voxels):
    return np.array(voxels, dtype=np.float64) / 88.0


def _bone(a, b):
    return np.concatenate([_world(a)[0], _world(b)[0]])


def half_way_points():
    """coordinates whose voxel coordinate is EXACTLY i + 0.5 in float64: np.round / rint go to the even neighbour"""
    found = {}
    for i in (20, 21, 42, 43, 85, 86):
        p = (i + 0.5) / 88.0
        for _ in range(8):
            if (p - 0.0) / 1.0 * 88.0 == i + 0.5:
                found[i] = p
                break
            p = np.nextafter(p, 1.0 if (p - 0.0) / 1.0 * 88.0 < i + 0.5 else 0.0)
    return found


def volumetric_cases():
    """(name, mask, bones, vertices): grids built to sit on the word boundaries (z = 31 / 32, 63 / 64) and the grid border"""
    rng = np.random.default_rng(0x566F78)
    cases = []
    line = np.zeros((88, 88, 88), dtype=bool)
    line[40, 41, :] = True
    on = _world(*[(40, 41, z) for z in range(88)]) + rng.uniform(-0.3, 0.3, size=(88, 3)) / 88.0
    halves = half_way_points()
    assert any(i % 2 == 0 for i in halves) and any(i % 2 == 1 for i in halves)
    hw = np.array([[40.0 / 88.0, 41.0 / 88.0, p] for p in halves.values()])
    off = _world((0, 0, 0), (87, 87, 87), (40, 42, 50), (39, 41, 31))                  # unoccupied voxels: read 0
    cases.append(("line z", line, np.stack([_bone((40, 41, 0), (40, 41, 0)), _bone((40, 41, 30), (40, 41, 60)),
                                            _bone((10, 10, 10), (10, 10, 20)), _bone((40, 41, -20), (40, 41, -5)),
                                            _bone((40, 41, 87), (40, 41, 87))]), np.concatenate([on, hw, off])))
    lx = np.zeros_like(line)
    lx[:, 0, 87] = True
    cases.append(("line x", lx, np.stack([_bone((0, 0, 87), (0, 0, 87)), _bone((60, 3, 80), (70, 3, 80)), _bone((87, 0, 87), (50, 0, 87))]),
                  np.concatenate([_world(*[(x, 0, 87) for x in range(88)]), _world((0, 1, 87), (87, 0, 86))])))
    ly = np.zeros_like(line)
    ly[87, :, 0] = True
    cases.append(("line y", ly, np.stack([_bone((87, 87, 0), (87, 87, 0)), _bone((87, 95, 0), (87, 120, 0)), _bone((87, 20, 0), (87, 40, 0))]),
                  np.concatenate([_world(*[(87, y, 0) for y in range(88)]), _world((86, 5, 0), (87, 5, 1))])))
    slab = np.zeros_like(line)
    slab[:, 42:45, :] = True
    slab[20:22, :, :] = True
    vv = np.argwhere(slab)[rng.permutation(int(slab.sum()))[:200]]
    border = [(0, 43, 0), (87, 44, 87), (20, 0, 5), (21, 87, 80), (0, 42, 87), (87, 43, 31), (87, 43, 32), (5, 44, 63), (5, 44, 64), (1, 1, 1)]
    cases.append(("slab", slab, np.stack([_bone((10, 43, 10), (70, 43, 75)), _bone((-30, 43, 40), (-10, 43, 40)), _bone((21, 80, 80), (21, 80, 80)),
                                          _bone((60, 10, 60), (60, 30, 60))]),
                  np.concatenate([_world(*vv.tolist()) + rng.uniform(-0.3, 0.3, size=(200, 3)) / 88.0, _world(*border)])))
    two = np.zeros_like(line)
    two[10:20, 10:20, 10:20] = True
    two[50:58, 50:60, 28:36] = True                                                    # across z = 31 / 32
    three = two.copy()
    three[70:80, 20:30, 60:70] = True                                                  # across z = 63 / 64
    for name, grid in (("two islands", two), ("three islands", three)):
        vv = np.argwhere(grid)[rng.permutation(int(grid.sum()))[:150]]
        cases.append((name, grid, np.stack([_bone((12, 12, 12), (17, 16, 15)), _bone((40, 40, 40), (40, 40, 40)), _bone((52, 55, 30), (56, 55, 34))]),
                      np.concatenate([_world(*vv.tolist()), _world((30, 30, 30), (0, 87, 0))])))
    horse = np.zeros_like(line)                                                        # a horseshoe around one isolated voxel
    horse[10:13, 10:31, 10:13] = True
    horse[18:21, 10:31, 10:13] = True
    horse[10:21, 10:13, 10:13] = True
    horse[15, 25, 11] = True                                                           # 3 voxels from either arm: near and far from the bone
    vv = np.argwhere(horse)
    cases.append(("horseshoe", horse, np.stack([_bone((11, 28, 11), (11, 28, 11)), _bone((19, 29, 11), (19, 20, 11))]), _world(*vv.tolist())))
    return cases


def test_volumetric_geodesic_word_boundaries_border_and_patches():
    cases = volumetric_cases()
    want, patches, ties = [], {}, {}
    for name, mask, bones, verts in cases:
        w, infos = so.volumetric_geodesic(verts, mask, bones, [0.0, 0.0, 0.0], 1.0, 88, return_info=True)
        want.append(w)
        patches[name] = [i["patches"] for i in infos]
        ties[name] = [i["layer_ties"] for i in infos]
        print(f"{name}: {len(bones)} bones, {len(verts)} vertices, patches per bone {patches[name]}, largest layer {int(w.max())}")
    assert np.array_equal(want[0][:88, 0], np.arange(88)) and np.array_equal(want[0][:88, 4], np.arange(87, -1, -1))   # carries both ways
    assert want[0][:88, 3].tolist() == want[0][:88, 0].tolist()                        # seeds clipped to the border voxel
    assert (want[0][-4:] == 0).all()                                                   # unoccupied voxels read 0
    assert patches["line z"][2] >= 1 and patches["slab"][1] == 0                       # a bone wholly outside; one whose clipped seeds are inside
    assert max(patches["two islands"]) >= 1 and max(patches["three islands"]) >= 2     # a second patch, after the one-call lag
    assert patches["three islands"][1] >= 3                                            # a bone outside all three islands
    assert min(ties["horseshoe"]) >= 1                                                 # equally near reached voxels of different layers
    n_jobs = sum(len(c[2]) for c in cases)
    assert n_jobs > 3                                                                  # more jobs than slots in the second run
    pos = torch.from_numpy(np.concatenate([c[3] for c in cases])).to(DEV)
    batch = torch.cat([torch.full((len(c[3]),), i, dtype=torch.long) for i, c in enumerate(cases)]).to(DEV)
    voxes, bones = [_vox(c[1]) for c in cases], [c[2] for c in cases]
    for n_slots in (3, None):
        got = skinning.volumetric_geodesic_batched(pos, batch, voxes, bones, n_slots=n_slots)
        for (name, _, _, _), g, w in zip(cases, got, want):
            assert g.dtype == torch.int32 and np.array_equal(npy(g).astype(np.int64), w), name
    one = skinning.volumetric_geodesic(torch.from_numpy(cases[5][3]).to(DEV), voxes[5], bones[5])
    assert np.array_equal(npy(one).astype(np.int64), want[5])


# ---------------------------------------------------------------------------------------------------------------- f. bind rows, weights
def test_skin_bind_batched_ragged_equals_oracle_bitwise():
    rng = np.random.default_rng(0x42696E)
    k = 20
    counts, nbs, joints = [130, 77, 200], [3, 20, 41], [2, 37, 64]
    assert min(nbs) < k < max(nbs) and k in nbs
    dists, bones, leafs, sjs, skins = [], [], [], [], []
    for V, nb, J in zip(counts, nbs, joints):
        dists.append(rng.integers(0, 7, size=(V, nb)).astype(np.int32))                # ties and zeros
        bones.append(rng.normal(size=(nb, 6)))
        leafs.append(rng.integers(0, 2, nb).astype(np.uint8))
        sj = rng.integers(0, J, nb).astype(np.int32)
        sj[-1] = J - 1
        sjs.append(sj)
        s = rng.uniform(0, 1, size=(V, J)) * (rng.uniform(0, 1, size=(V, J)) < 0.6)
        skins.append(s)
    assert sjs[2].max() == 63 and (skins[2][:, 63] > 0).any()                          # joint 63: the top bit of the used-joint set
    o = skinning.skin_bind_batched([torch.from_numpy(d).to(DEV) for d in dists], bones, leafs, sjs, skins, k)
    off = 0
    for i, V in enumerate(counts):
        sl = slice(off, off + V)
        ids, invd = so.stable_rows(dists[i], leafs[i], k)
        assert (np.diff(np.take_along_axis(dists[i], ids[:, :min(k, nbs[i])], 1), axis=1) == 0).any()
        assert np.array_equal(npy(o["bind_ids"][sl]).astype(np.int64), ids)
        assert same_bits(o["bind_invd"][sl], invd)
        lab = so.labels_of(ids, skins[i], sjs[i])
        assert (lab > 0).any() and same_bits(o["labels"][sl], lab)
        si, nn, mask, jids = so.bind_tensors(ids, invd, bones[i], leafs[i], sjs[i])
        assert np.array_equal(npy(o["skin_input"][sl]).view(np.int32), si.view(np.int32))
        assert np.array_equal(npy(o["skin_nn"][sl]), nn) and np.array_equal(npy(o["loss_mask"][sl]), mask)
        assert np.array_equal(npy(o["skin_nnjids"][sl]), jids)
        one = skinning.skin_bind_batched([torch.from_numpy(dists[i]).to(DEV)], [bones[i]], [leafs[i]], [sjs[i]], [skins[i]], k)
        for key in ("bind_ids", "bind_invd", "labels", "skin_input", "skin_nn", "loss_mask", "skin_nnjids"):
            assert torch.equal(o[key][sl], one[key])
        off += V


@pytest.mark.parametrize("mode,ratio", [("train_skin", None), ("joint2rig", None), ("train_skin", 0.2), ("joint2rig", 0.6)])
def test_skin_weights_ragged_batch_equals_oracle(mode, ratio):
    rng = np.random.default_rng(0x577473)
    k = 20
    sides, nbs = [9, 8, 11], [3, 17, 41]
    logits, nns, masks, edges, batch = [], [], [], [], []
    off = 0
    lonely = 30
    for i, (n_side, nb) in enumerate(zip(sides, nbs)):
        V = n_side * n_side
        m = min(k, nb)
        nn = np.zeros((V, k), dtype=np.int64)
        mask = np.zeros((V, k), dtype=np.int64)
        for v in range(V):
            nn[v, :m] = rng.permutation(nb)[:m]
        mask[:, :m] = 1
        mask[rng.uniform(size=(V, k)) < 0.1] = 0
        if i == 0:
            nn[5, 1], mask[5, 1] = 10, 1                                               # a bone id past this mesh's count: dropped
            nn[6, 4], mask[6, 4] = 2, 1                                                # a masked-in slot past the bone count
        e = np.array([(a, b) for a, b in synth.make_mesh(3, n_side=n_side, with_skin=False, geo="none").tpl_edge_index.numpy().T.tolist()
                      if i != 1 or lonely not in (a, b)], dtype=np.int64).T           # the middle mesh: a vertex without neighbours
        e = np.concatenate([e, e[:, :40], np.stack([np.arange(10), np.arange(10)])], 1)  # duplicated edges and self edges
        logits.append(rng.normal(0.0, 2.0, size=(V, k)).astype(np.float32))
        nns.append(nn)
        masks.append(mask)
        edges.append(e)
        batch.append(np.full(V, i, dtype=np.int64))
        off += V
    assert not len(so.one_ring(edges[1], sides[1] ** 2)[lonely]) and all(len(r) for r in so.one_ring(edges[0], sides[0] ** 2))
    offs = np.concatenate([[0], np.cumsum([s * s for s in sides])])
    tpl = np.concatenate([e + offs[i] for i, e in enumerate(edges)], 1)
    ws = skinning.skin_weights(torch.from_numpy(np.concatenate(logits)).to(DEV), torch.from_numpy(np.concatenate(nns)).to(DEV),
                               torch.from_numpy(np.concatenate(masks)).to(DEV), torch.from_numpy(tpl).to(DEV),
                               torch.from_numpy(np.concatenate(batch)).to(DEV), nbs, mode=mode, ratio=ratio)
    assert len(ws) == 3
    for i, w in enumerate(ws):
        want = so.skin_weights(logits[i], nns[i], masks[i], edges[i], nbs[i], mode=mode, ratio=ratio)
        assert w.dtype == torch.float64 and tuple(w.shape) == (sides[i] ** 2, nbs[i])   # no column at or past the mesh's bone count
        got = npy(w)
        print(f"{mode} ratio {ratio} mesh {i}: max abs diff {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= 1e-6
        sums = got.sum(1)                                                              # s / (s + 1e-10) with s the kept mass of the row: 1 or 0
        assert np.all((np.abs(sums - 1.0) <= 1e-6) | (sums == 0.0))
    # the padded columns of the shared buffer stay zero for the meshes with fewer bones
    base = ws[0]._base if ws[0]._base is not None else ws[0]
    assert base.shape[1] == max(nbs) and bool((base[:sides[0] ** 2, nbs[0]:] == 0).all())
