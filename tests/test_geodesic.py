"""Surface geodesics and vertex-to-bone distances on the device (morig_amd/geodesic.py, csrc/geodesic.hip) against fixtures made by
the reference's own functions (tools/make_geodesic_golden.py): calc_surface_geodesic / get_geo_edges, pts2line, calc_geodesic_matrix
and the bind loop of predict_skinning; the visibility against the generator's float64 ray caster (the hit rule of DESIGN.md
section 11) and two analytic scenes.

Where the criteria come from: shortest paths are bitwise (a label-correcting fixed point equals Dijkstra's left-to-right float64 sums;
the full matrices are compared by sha256, a stored subset of rows element by element); indices are exact (np.argmin's first minimum);
stage 2 is a few float64 operations at magnitude <= 10, good to ~1e-14: 1e-12 leaves 100x and is eight orders below the float32 1/D
that SkinNet reads -- and since the kernels keep numpy's operation order with contraction off, the results were measured to be
bitwise equal, which is what is asserted; the network comparison keeps the suite's 1e-4."""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from morig_amd import geodesic, graph_build, skinning  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
STAGE1 = ("geo_connected", "geo_islands", "geo_sheets", "geo_4000")
NEW_SYMBOLS = ("morig_surface_geodesic_workspace", "morig_surface_geodesic", "morig_nearest_point", "morig_bone_point_distance",
               "morig_bone_visibility", "morig_bone_geodesic", "morig_skin_bind_geo")
DEV = "cuda:0"


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = {k: z[k] for k in z.files if k != "meta"}
    c["meta"] = json.loads(bytes(z["meta"]).decode())
    return c


def sha(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else t
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------- host / CPU
def test_new_symbols_declared_and_exported():
    from morig_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "morig_hip.h")).read(), flags=re.S)
    lib = native.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in native.EXPORTS
        assert hasattr(lib, s)
    assert native.ABI_VERSION == 3 and lib.morig_abi_version() == 3


def test_argument_validation_raises_value_error():
    p = np.random.default_rng(0).normal(size=(5, 3))
    with pytest.raises(ValueError):
        geodesic.surface_geodesic_samples(p, p)                                        # S < 6
    p8 = np.random.default_rng(0).normal(size=(8, 3))
    with pytest.raises(ValueError):
        geodesic.surface_geodesic_samples(p8, p8[:7])                                  # pts / normals differ
    with pytest.raises(ValueError):
        geodesic.surface_geodesic_samples(p8, p8, ptr=[0, 3, 8])                       # a mesh of 3 samples
    with pytest.raises(ValueError):
        geodesic.surface_geodesic_samples(p8, p8, ptr=[0, 9])                          # ptr past the rows
    with pytest.raises(ValueError):
        geodesic.surface_geodesic_samples(np.zeros((8, 2)), np.zeros((8, 2)))
    with pytest.raises(ValueError):
        geodesic.surface_geodesic_samples(np.zeros((65536, 3)), np.zeros((65536, 3)))  # ids are refused, not truncated
    with pytest.raises(ValueError):
        geodesic.surface_geodesic(p8, p, p)
    bones = np.zeros((2, 6))
    with pytest.raises(ValueError):
        geodesic.bone_point_distance(p8, np.zeros((2, 5)))
    with pytest.raises(ValueError):
        geodesic.bone_point_distance(p8, np.zeros((0, 6)))
    with pytest.raises(ValueError):
        geodesic.bone_visibility(p8, bones, p8, np.array([[0, 1, 8]]))                 # a face id out of range
    with pytest.raises(ValueError):
        geodesic.bone_visibility(p8, bones, p8, np.array([[0, 1]]))
    sg, vis = np.zeros((8, 8)), np.ones((8, 2), dtype=bool)
    with pytest.raises(ValueError):
        geodesic.bone_geodesic_matrix(p8, bones, np.zeros((8, 7)), vis)
    with pytest.raises(ValueError):
        geodesic.bone_geodesic_matrix(p8, bones, sg, np.ones((8, 3), dtype=bool))
    with pytest.raises(ValueError):
        geodesic.bone_geodesic_matrix(p8, bones, sg, vis, dist=np.zeros((7, 2)))
    with pytest.raises(ValueError):
        geodesic.bone_geodesic_matrix(p8, bones, sg, vis[:2], subsample_ids=np.array([0, 8]))   # an id out of range
    with pytest.raises(ValueError):
        geodesic.skin_inputs_joint2rig(np.zeros((8, 3)), bones, [False, True])
    with pytest.raises(ValueError):
        geodesic.skin_inputs_joint2rig(np.zeros((8, 2)), bones, [False])


@pytest.mark.parametrize("name", STAGE1)
def test_stage1_fixtures_satisfy_their_margins(name):
    c = load_case(name)
    m, pts, nrm = c["meta"], c["pts"], c["normals"]
    assert pts.shape == nrm.shape == (m["S"], 3) and c["verts"].shape == (m["V"], 3)
    d = np.sqrt(np.sum((pts[np.newaxis, ...] - pts[:, np.newaxis, :]) ** 2, axis=2))
    order = np.argsort(d, axis=1)[:, :7]
    near = np.take_along_axis(d, order, 1)
    assert np.diff(near, axis=1).min() >= 1e-9 and np.isclose(np.diff(near, axis=1).min(), m["nn_gap"], rtol=1e-6, atol=0)
    nn = order[:, 1:6]
    cos = np.einsum("pkc,pc->pk", nrm[nn], nrm) / (np.linalg.norm(nrm[nn], axis=2) * np.linalg.norm(nrm, axis=1)[:, None] + 1e-10)
    assert np.abs(cos + 0.5).min() >= 1e-6 and int((cos <= -0.5).sum()) == m["arcs_removed"]
    assert c["rows"].shape == (len(c["row_ids"]), m["S"]) and c["vrows"].shape == (len(c["vrow_ids"]), m["V"])
    assert (c["rows"][np.arange(len(c["row_ids"])), c["row_ids"]] == 0).all()
    assert c["nn"].shape == (m["V"],) and 0 <= c["nn"].min() and c["nn"].max() < m["S"]
    assert len(m["sha_samples"]) == len(m["sha_verts"]) == 64
    if name == "geo_islands":
        assert m["patched_entries"] > 0 and (c["rows"] >= 8.0).any()
    if name == "geo_sheets":
        assert m["arcs_removed"] > 0
    if name == "geo_4000":
        assert m["ref_seconds"] > 0


def test_bone_fixtures_satisfy_their_margins():
    c = load_case("bone_geo_torus")
    m = c["meta"]
    V, nb = m["V"], m["n_bones"]
    assert c["visible"].shape == c["dist"].shape == c["geo_dist"].shape == (V, nb)
    assert m["rule_margin"] >= 5e-5 and m["min_ray"] >= 1e-9 and m["bary_margin"] >= 1e-6 and m["percentile_margin"] >= 1e-9
    assert (~c["visible"]).all(0).any()                                                # an all-invisible column
    assert (np.sum((c["bones"][:, 3:] - c["bones"][:, :3]) ** 2, axis=1) < 1e-8).any()  # a zero-length bone
    for b in range(nb):
        ids = np.flatnonzero(c["visible"][:, b])
        if len(ids):
            p = np.percentile(c["dist"][ids, b], 15)
            assert p == c["percentile"][b] and np.abs(c["dist"][:, b] - 1.3 * p).min() >= 1e-9
    assert int(c["tri_faces"].max()) < len(c["tri_pos"]) and c["sub_ids"].max() < V
    assert (c["loss_mask3"][:, 3:] == 0).all() and (c["loss_mask"] == 1).all()
    ci = load_case("bone_geo_inf")
    assert ci["meta"]["n_inf"] > 0 and ci["meta"]["sha_surface"] == m["sha_surface"]


# ---------------------------------------------------------------- device: stage 1
@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGE1)
def test_surface_geodesic_samples_bitwise(name):
    c = load_case(name)
    d, stats = geodesic.surface_geodesic_samples(c["pts"], c["normals"], return_stats=True)
    print(f"{name}: sweeps max {stats['max_sweeps']} mean {stats['total_sweeps'] / stats['jobs']:.1f} entries {stats['entries']}")
    assert d.dtype == torch.float64 and d.shape == (c["meta"]["S"],) * 2
    got = d[torch.from_numpy(c["row_ids"]).long().to(d.device)].cpu().numpy()
    assert np.array_equal(bits(got), bits(c["rows"]))
    assert sha(d) == c["meta"]["sha_samples"]


@pytest.mark.gpu
def test_surface_geodesic_samples_global_memory_path_bitwise():
    c = load_case("geo_islands")
    d = geodesic.surface_geodesic_samples(c["pts"], c["normals"], lds=False, n_slots=7)
    assert sha(d) == c["meta"]["sha_samples"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGE1)
def test_nearest_sample_and_surface_geodesic(name):
    c = load_case(name)
    nn = geodesic.nearest_sample(c["verts"], c["pts"])
    assert nn.dtype == torch.int32 and np.array_equal(nn.cpu().numpy(), c["nn"])
    sg = geodesic.surface_geodesic(c["verts"], c["pts"], c["normals"])
    assert sg.shape == (c["meta"]["V"],) * 2
    got = sg[torch.from_numpy(c["vrow_ids"]).long().to(sg.device)].cpu().numpy()
    assert np.array_equal(bits(got), bits(c["vrows"]))
    assert sha(sg) == c["meta"]["sha_verts"]


@pytest.mark.gpu
def test_get_geo_edges_from_samples_against_the_reference():
    from test_geo_graph import _check_over, _rows
    c = load_case("geo_connected")
    m = c["meta"]
    V, mx = m["V"], m["max_nn"]
    inside = np.unpackbits(c["inside_bits"])[:V * V].reshape(V, V).astype(bool)
    ei, members = graph_build.get_geo_edges_from_samples(c["verts"], c["pts"], c["normals"], m["radius"], mx, seed=3, return_members=True)
    assert np.array_equal(members.cpu().numpy(), c["counts"])
    e = _rows(ei)
    _check_over(e, c["counts"], mx, inside, V)
    ref = c["edges"].astype(np.int64)
    assert e.shape == ref.shape
    within = c["counts"] <= mx                                                         # rows within the cap: identical to the reference's
    assert np.array_equal(e[within[e[:, 0]]], ref[within[ref[:, 0]]])
    e2 = _rows(graph_build.get_geo_edges_from_samples(c["verts"], c["pts"], c["normals"], m["radius"], mx, seed=3, self_loops=True))
    assert np.array_equal(e2[:-V], e) and np.array_equal(e2[-V:], np.stack([np.arange(V)] * 2, 1))


@pytest.mark.gpu
def test_surface_geodesic_batched_ragged_and_deterministic():
    cs = [load_case(n) for n in ("geo_sheets", "geo_islands", "geo_connected", "geo_sheets")]
    pts = np.concatenate([c["pts"] for c in cs])
    nrm = np.concatenate([c["normals"] for c in cs])
    ptr = np.concatenate([[0], np.cumsum([len(c["pts"]) for c in cs])])
    runs = [geodesic.surface_geodesic_samples(pts, nrm, ptr=ptr, n_slots=s) for s in (None, 3, None, 3)]
    for i, c in enumerate(cs):
        one = geodesic.surface_geodesic_samples(c["pts"], c["normals"])
        assert sha(one) == c["meta"]["sha_samples"]
        for r in runs:
            assert torch.equal(r[i], one)
    vs = geodesic.surface_geodesic_batched([c["verts"] for c in cs], [c["pts"] for c in cs], [c["normals"] for c in cs], chunk=3)
    for v, c in zip(vs, cs):
        assert sha(v) == c["meta"]["sha_verts"]


# ---------------------------------------------------------------- device: stages 2 and 3
def _surface(c):
    sg = geodesic.surface_geodesic(c["pos"], c["pts"], c["normals"])
    assert sha(sg) == c["meta"]["sha_surface"]                                         # the reference's matrix, bit for bit
    return sg


def _assert_close(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    diff = np.abs(got - want).max()
    print(f"{what}: max abs diff {diff:.3e}, bitwise {np.array_equal(bits(got), bits(want))}")
    assert diff <= 1e-12, what
    assert np.array_equal(bits(got), bits(want)), what                                 # measured: bitwise holds, so it is asserted


@pytest.mark.gpu
def test_bone_point_distance():
    c = load_case("bone_geo_torus")
    origins, dist = geodesic.bone_point_distance(c["pos"], c["bones"])
    assert origins.shape == c["origins"].shape and dist.shape == c["dist"].shape
    _assert_close(origins, c["origins"], "pts2line origins")
    _assert_close(dist, c["dist"], "pts2line dist")


@pytest.mark.gpu
def test_bone_geodesic_matrix_given_the_visibility():
    c = load_case("bone_geo_torus")
    sg = _surface(c)
    out, aux = geodesic.bone_geodesic_matrix(c["pos"], c["bones"], sg, c["visible"], c["dist"], return_aux=True)
    assert np.array_equal(aux["visible_after"].cpu().numpy(), c["visible_after"])
    assert np.array_equal(aux["nn"].cpu().numpy(), c["nn"])
    pct = aux["percentile"].cpu().numpy()
    assert np.array_equal(np.isnan(pct), np.isnan(c["percentile"]))
    _assert_close(np.nan_to_num(pct) + 0.0, np.nan_to_num(c["percentile"]) + 0.0, "percentile")
    _assert_close(out, c["geo_dist"], "geo_dist")
    # dist computed on the device (pts2line) instead of handed in
    _assert_close(geodesic.bone_geodesic_matrix(c["pos"], c["bones"], sg, c["visible"]), c["geo_dist"], "geo_dist, own dist")


@pytest.mark.gpu
def test_bone_geodesic_matrix_subsampled():
    c = load_case("bone_geo_torus")
    sg = _surface(c)
    out, aux = geodesic.bone_geodesic_matrix(c["pos"], c["bones"], sg, c["sub_visible"], c["sub_dist"], subsample_ids=c["sub_ids"],
                                             return_aux=True)
    assert np.array_equal(aux["nn_subsample"].cpu().numpy(), c["nn_sub"])
    _assert_close(out, c["geo_dist_sub"], "geo_dist, sub-sampled")


@pytest.mark.gpu
def test_bone_geodesic_matrix_infinite_surface_entries():
    c, ci = load_case("bone_geo_torus"), load_case("bone_geo_inf")
    sg = _surface(c)
    g = torch.from_numpy(ci["group"]).to(sg.device)
    sg_inf = torch.where(g[:, None] != g[None, :], torch.full_like(sg, float("inf")), sg)
    out, aux = geodesic.bone_geodesic_matrix(c["pos"], c["bones"], sg_inf, c["visible"], c["dist"], return_aux=True)
    assert np.array_equal(aux["visible_after"].cpu().numpy(), ci["visible_after"])
    assert np.array_equal(aux["nn"].cpu().numpy(), ci["nn"])
    _assert_close(out, ci["geo_dist"], "geo_dist, infinite entries")


@pytest.mark.gpu
def test_bone_visibility_equals_fixture():
    c = load_case("bone_geo_torus")
    vis = geodesic.bone_visibility(c["pos"], c["bones"], c["tri_pos"], c["tri_faces"])
    assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), c["visible"])
    sub = geodesic.bone_visibility(c["pos"][c["sub_ids"]], c["bones"], c["tri_pos"], c["tri_faces"])
    assert np.array_equal(sub.cpu().numpy(), c["sub_visible"])


def _icosphere(levels=2):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.stack(v), np.array(f, dtype=np.int32)


@pytest.mark.gpu
def test_bone_visibility_analytic():
    """a convex mesh sees every vertex from an interior bone; from a bone outside, behind a second sphere, no vertex of the far sphere
    is visible (every ray crosses the near sphere, whose radius 0.5 leaves the grazing rays 0.1 short of its silhouette)"""
    v, f = _icosphere(2)
    v = v * 0.5
    inside = np.array([[-0.1, 0.02, 0.03, 0.12, -0.04, 0.05]])
    vis = geodesic.bone_visibility(v, inside, v, f)
    assert vis.shape == (len(v), 1) and bool(vis.all())
    far = v * 0.3 + np.array([3.0, 0.0, 0.0])
    both_v = np.concatenate([v, far])
    both_f = np.concatenate([f, f + len(v)])
    outside = np.array([[-2.0, 0.01, 0.02, -1.8, -0.02, 0.01]])
    vis = geodesic.bone_visibility(both_v, outside, both_v, both_f).cpu().numpy()[:, 0]
    assert not vis[len(v):].any()
    assert vis[:len(v)].any() and not vis[:len(v)].all()                               # the near sphere: its front yes, its back no


def _tie_aware_equal(nn, mask, ref_nn, ref_mask, geo, k):
    """the reference's argsort is not stable: per vertex the distance sequence is equal, tie groups hold the same ids (a group cut at
    slot k: a subset of the tied bones), and among equal distances ours ascend by bone id"""
    assert np.array_equal(mask, ref_mask)
    nb = geo.shape[1]
    m = min(k, nb)
    for v in range(len(nn)):
        dv = geo[v, nn[v, :m]]
        assert np.array_equal(dv, geo[v, ref_nn[v, :m]]) and (np.diff(dv) >= 0).all()
        for d in np.unique(dv):
            ours, theirs = nn[v, :m][dv == d], ref_nn[v, :m][dv == d]
            assert (np.diff(ours) > 0).all()
            tied = set(np.flatnonzero(geo[v] == d).tolist())
            if len(tied) == len(ours):
                assert set(ours.tolist()) == set(theirs.tolist()) == tied
            else:
                assert set(ours.tolist()) <= tied and set(theirs.tolist()) <= tied
        assert (nn[v, m:] == 0).all() and (ref_nn[v, m:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("suffix,n_bones", [("", None), ("3", 3)])
def test_skin_inputs_joint2rig_equals_reference_loop(suffix, n_bones):
    c = load_case("bone_geo_torus")
    k = c["meta"]["k"]
    nb = n_bones or c["meta"]["n_bones"]
    geo = c["geo_dist"][:, :nb].copy()
    si, nn, mask = geodesic.skin_inputs_joint2rig(geo, c["bones"][:nb], c["is_leaf"][:nb], k)
    assert si.dtype == torch.float32 and si.shape == (len(geo), 8 * k) and nn.dtype == mask.dtype == torch.int64
    nn, mask = nn.cpu().numpy(), mask.cpu().numpy()
    ref_nn, ref_mask = c["skin_nn" + suffix], c["loss_mask" + suffix]
    _tie_aware_equal(nn, mask, ref_nn, ref_mask, geo, k)
    got, want = si.cpu().numpy().reshape(len(geo), k, 8), c["skin_input" + suffix].reshape(len(geo), k, 8)
    for v in range(len(geo)):
        for s in range(k):
            # the reference's slot with the same bone (another slot of the same tie group where its unstable sort ordered a tie otherwise);
            # a slot past the bone count repeats the nearest bone
            bone = nn[v, s] if mask[v, s] else nn[v, 0]
            t = int(np.flatnonzero(ref_nn[v, :min(k, nb)] == bone)[0])
            assert np.array_equal(got[v, s].view(np.int32), want[v, t].view(np.int32)), (v, s)


@pytest.mark.gpu
def test_end_to_end_skinning_inputs_feed_skinnet():
    from helpers import rel_excess
    from morig_amd import models, synth
    c = load_case("bone_geo_torus")
    m = c["meta"]
    k, V, nb = m["k"], m["V"], m["n_bones"]
    mesh = synth.make_mesh(m["seed"], n_side=m["n_side"], with_skin=False)
    assert np.array_equal(mesh.pos.numpy().astype(np.float64), c["pos"])
    kw = dict(nearest_bone=k, use_Dg=True, use_Lf=True, num_keyframes=5, use_motion=True, motion_dim=32, aggr_method="attn")
    net = synth.load_recipe(models.skinnet_motion(**kw).eval(), 204).to(DEV)

    def chain():
        sg = geodesic.surface_geodesic(c["pos"], c["pts"], c["normals"])
        vis = geodesic.bone_visibility(c["pos"], c["bones"], c["tri_pos"], c["tri_faces"])
        geo = geodesic.bone_geodesic_matrix(c["pos"], c["bones"], sg, vis)
        return geodesic.skin_inputs_joint2rig(geo, c["bones"], c["is_leaf"], k)

    def weights(skin_input, nn, mask):
        mesh.skin_input = skin_input.cpu()
        b = synth.collate([mesh]).to(DEV)
        with torch.no_grad():
            logits = net(b, b.pred_flow)[2]
        w = skinning.skin_weights(logits, nn.to(DEV), mask.to(DEV), b.tpl_edge_index, torch.zeros(V, dtype=torch.long, device=DEV), [nb],
                                  mode="joint2rig")[0]
        return logits, w

    si, nn, mask = chain()
    logits, w = weights(si, nn, mask)
    si2, nn2, mask2 = chain()
    assert torch.equal(si, si2) and torch.equal(nn, nn2) and torch.equal(mask, mask2)
    logits2, w2 = weights(si2, nn2, mask2)
    assert torch.equal(w, w2)                                                          # deterministic
    assert bool(torch.isfinite(w).all()) and w.shape == (V, nb)
    sums = w.sum(1).cpu().numpy()
    assert np.all((np.abs(sums - 1.0) <= 1e-9) | (sums == 0.0))
    # the same chain fed with the reference-made skin_input (its slots reordered to ours inside tie groups: SkinNet sees slot order)
    ref = torch.from_numpy(c["skin_input"]).float().view(V, k, 8)
    ref_nn = c["skin_nn"]
    ours_nn = nn.cpu().numpy()
    perm = np.stack([[int(np.flatnonzero(ref_nn[v] == ours_nn[v, s])[0]) for s in range(k)] for v in range(V)])
    ref_in = torch.gather(ref, 1, torch.from_numpy(perm)[:, :, None].expand(-1, -1, 8)).reshape(V, 8 * k)
    logits_ref, w_ref = weights(ref_in, nn, mask)
    assert rel_excess(logits, logits_ref, 1e-4) <= 0
    assert float((w - w_ref).abs().max()) <= 1e-4
