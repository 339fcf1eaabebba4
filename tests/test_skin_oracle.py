"""tests/skin_oracle.py against the fixtures the reference's own functions made (tools/make_geodesic_golden.py,
tools/make_skin_golden.py): the oracle is only worth something if it IS the reference. No GPU, no native library.

Criteria are the ones the device tests are held to: shortest paths, pts2line, the percentile and the vertex-to-bone matrix bit for
bit; indices, booleans and integer distances exact; the bind rows tie-aware where the reference's unstable argsort ordered equal
distances its own way; the final weights within 1e-6."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import skin_oracle as so  # noqa: E402
from test_geodesic import STAGE1, _tie_aware_equal, bits, load_case  # noqa: E402
from test_skinning_prep import CASES, load_case as load_skin_case  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------- stage 1
@pytest.mark.parametrize("name", STAGE1)
def test_surface_geodesic_rows_equal_fixture_bitwise(name):
    c = load_case(name)
    m = c["meta"]
    g = so.SampleGraph(c["pts"], c["normals"])
    gap, cmargin, removed = g.margins()
    assert np.isclose(gap, m["nn_gap"], rtol=1e-6, atol=0) and np.isclose(cmargin, m["cos_margin"], rtol=1e-6, atol=0)
    assert removed == m["arcs_removed"]
    rows = so.surface_geodesic_rows(c["pts"], c["normals"], c["row_ids"], graph=g)
    assert np.array_equal(bits(rows), bits(c["rows"]))
    assert int((rows >= 8.0).sum()) > 0 or m["patched_entries"] == 0
    nn, _ = so.nearest_sample(c["verts"], c["pts"])
    assert np.array_equal(nn, c["nn"])
    # the vertex matrix is a gather of the sample matrix at the nearest samples
    vr = so.surface_geodesic_rows(c["pts"], c["normals"], nn[c["vrow_ids"][:6]], graph=g)[:, nn]
    assert np.array_equal(bits(vr), bits(c["vrows"][:6]))


def test_components_and_filtered_arcs_are_read_off_the_graph():
    c = load_case("geo_islands")
    lab = so.SampleGraph(c["pts"], c["normals"]).components()
    assert len(np.unique(lab)) == 2 and (lab[:300] == lab[0]).all() and (lab[300:] == lab[300]).all()
    s = load_case("geo_sheets")
    g = so.SampleGraph(s["pts"], s["normals"])
    assert int((~g.keep).sum()) == s["meta"]["arcs_removed"] > 0 and g.n_entries % 2 == 0


def test_knn_in_row_blocks_is_independent_of_the_block_size():
    c = load_case("geo_connected")
    a, b = so.SampleGraph(c["pts"], c["normals"], block=64), so.SampleGraph(c["pts"], c["normals"], block=600)
    assert np.array_equal(a.nbr, b.nbr) and np.array_equal(bits(a.w.astype(np.float64)), bits(b.w.astype(np.float64)))
    assert np.array_equal(a.keep, b.keep)


# ---------------------------------------------------------------------------------------------------------------- stages 2 and 3
def _surface(c):
    g = so.SampleGraph(c["pts"], c["normals"])
    nn, _ = so.nearest_sample(c["pos"], c["pts"])
    used = np.unique(nn)
    rows = so.surface_geodesic_rows(c["pts"], c["normals"], used, graph=g)
    sg = rows[np.searchsorted(used, nn)][:, nn]
    assert sha(sg) == c["meta"]["sha_surface"]                                        # the reference's matrix, bit for bit
    return sg


@pytest.fixture(scope="module")
def torus():
    c = load_case("bone_geo_torus")
    c["sg"] = _surface(c)
    return c


def test_pts2line_equals_fixture_bitwise(torus):
    origins, dist = so.pts2line(torus["pos"], torus["bones"])
    assert np.array_equal(bits(origins), bits(torus["origins"]))
    assert np.array_equal(bits(dist), bits(torus["dist"]))
    _, sub = so.pts2line(torus["pos"][torus["sub_ids"]], torus["bones"])
    assert np.array_equal(bits(sub), bits(torus["sub_dist"]))


def test_visibility_equals_fixture(torus):
    c = torus
    vis, unsure, _ = so.bone_visibility(c["pos"], c["bones"], c["tri_pos"], c["tri_faces"])
    assert np.array_equal(vis, c["visible"]) and not unsure.any()                      # the generator held the fixture to these margins
    sub, unsure, _ = so.bone_visibility(c["pos"][c["sub_ids"]], c["bones"], c["tri_pos"], c["tri_faces"])
    assert np.array_equal(sub, c["sub_visible"]) and not unsure.any()
    everything, unsure, _ = so.bone_visibility(c["pos"], c["bones"], c["tri_pos"], np.zeros((0, 3), dtype=np.int32))
    assert everything.all() and not unsure.any()                                       # no occluder: min_hit is the ray's length


def test_geodesic_matrix_equals_fixture_bitwise(torus):
    c = torus
    out, vis_after, nn, pct, margin, n_inf = so.restate(c["dist"], c["visible"], c["sg"])
    assert np.array_equal(vis_after, c["visible_after"]) and np.array_equal(nn, c["nn"]) and n_inf == 0
    assert np.array_equal(np.isnan(pct), np.isnan(c["percentile"])) and np.isnan(pct).any()
    assert np.array_equal(bits(np.nan_to_num(pct) + 0.0), bits(np.nan_to_num(c["percentile"]) + 0.0))
    assert np.array_equal(bits(out), bits(c["geo_dist"]))
    assert np.isclose(margin, c["meta"]["percentile_margin"], rtol=1e-6) or margin >= c["meta"]["percentile_margin"]
    sub, nn_sub = so.geodesic_matrix_subsampled(c["pos"], c["sub_ids"], c["sub_dist"], c["sub_visible"], c["sg"])
    assert np.array_equal(nn_sub, c["nn_sub"]) and np.array_equal(bits(sub), bits(c["geo_dist_sub"]))


def test_geodesic_matrix_infinite_entries_equal_fixture_bitwise(torus):
    c, ci = torus, load_case("bone_geo_inf")
    g = ci["group"]
    sg_inf = np.where(g[:, None] != g[None, :], np.inf, c["sg"])
    out, vis_after, nn, _, _, n_inf = so.restate(c["dist"], c["visible"], sg_inf)
    assert n_inf == ci["meta"]["n_inf"] > 0
    assert np.array_equal(vis_after, ci["visible_after"]) and np.array_equal(nn, ci["nn"])
    assert np.array_equal(bits(out), bits(ci["geo_dist"]))


@pytest.mark.parametrize("suffix,n_bones", [("", None), ("3", 3)])
def test_bind_joint2rig_equals_reference_loop(torus, suffix, n_bones):
    c = torus
    k = c["meta"]["k"]
    nb = n_bones or c["meta"]["n_bones"]
    geo = c["geo_dist"][:, :nb].copy()
    si, nn, mask = so.bind_joint2rig(geo, c["bones"][:nb], c["is_leaf"][:nb], k)
    ref_nn, ref_mask = c["skin_nn" + suffix], c["loss_mask" + suffix]
    _tie_aware_equal(nn, mask, ref_nn, ref_mask, geo, k)
    got, want = si.reshape(len(geo), k, 8), c["skin_input" + suffix].reshape(len(geo), k, 8)
    for v in range(len(geo)):
        for s in range(k):
            bone = nn[v, s] if mask[v, s] else nn[v, 0]
            t = int(np.flatnonzero(ref_nn[v, :min(k, nb)] == bone)[0])
            assert np.array_equal(got[v, s].view(np.int32), want[v, t].view(np.int32)), (v, s)


# ---------------------------------------------------------------------------------------------------------------- skinning
@pytest.mark.parametrize("name", CASES)
def test_volumetric_geodesic_equals_fixture(name, tmp_path):
    c = load_skin_case(name, tmp_path)
    m = c["meta"]
    got, infos = so.volumetric_geodesic(c["pos"], c["vox"].data, c["bones"], m["translate"], m["scale"], m["dims"][0], return_info=True)
    assert np.array_equal(got, c["dist"].astype(np.int64))                            # every bone, integer for integer
    patches = sum(i["patches"] for i in infos)
    print(f"{name}: {patches} patches, {sum(i['patched'] for i in infos)} voxels patched, {max(i['steps'] for i in infos)} steps at most")
    assert patches == m["n_patches"]
    if name == "skin_islands":
        assert patches > 0 and max(i["patches"] for i in infos) >= 2                   # a second patch after the one-call lag


def test_patch_over_boundaries_equals_patch_over_all_voxels():
    """the closest pair of two voxel sets has both ends on their 6-boundaries: the boundary lists lose nothing"""
    rng = np.random.default_rng(11)
    for _ in range(4):
        a = np.zeros((88, 88, 88), dtype=bool)
        b = np.zeros_like(a)
        lo = rng.integers(0, 30, 3)
        a[lo[0]:lo[0] + 6, lo[1]:lo[1] + 5, lo[2]:lo[2] + 7] = True
        hi = rng.integers(45, 80, 3)
        b[hi[0]:hi[0] + 5, hi[1]:hi[1] + 8, hi[2]:hi[2] + 4] = True
        full = np.sum((np.argwhere(a)[:, None, :] - np.argwhere(b)[None, :, :]) ** 2, axis=2).min()
        bnd = np.sum((so.boundary6(a)[:, None, :] - so.boundary6(b)[None, :, :]) ** 2, axis=2).min()
        assert full == bnd and len(so.boundary6(a)) < int(a.sum())
    edge = np.zeros((88, 88, 88), dtype=bool)
    edge[0:3, 85:88, 0:88] = True                                                      # outside the grid counts as outside the set
    assert len(so.boundary6(edge)) == int(edge.sum()) - 86                             # only the middle line (1, 86, 1 .. 86) is interior


@pytest.mark.parametrize("name", CASES)
def test_bind_rows_labels_and_tensors_equal_fixture(name, tmp_path):
    from morig_amd import formats, skinning
    c = load_skin_case(name, tmp_path)
    k = c["meta"]["k"]
    bones, names, leaf = skinning.get_bones(c["rig"])
    dist = c["dist"]
    V, nb = dist.shape
    m = min(k, nb)
    ids, invd = so.stable_rows(dist, leaf, k)
    ref = c["bind_rows"][:, 1:]
    ref_ids, ref_invd = ref[:, 0::3].astype(np.int64), ref[:, 1::3]
    assert np.array_equal(bits(invd), bits(ref_invd))                                  # 1/D does not depend on how ties are ordered
    assert np.array_equal(ids[:, m:], ref_ids[:, m:]) and (ids[:, m:] == -1).all()
    same = (ids == ref_ids).all(1)
    print(f"{name}: {int(same.sum())} of {V} rows order their ties as the reference's argsort did")
    for v in np.flatnonzero(~same):                                                    # equal id sets per tie group, a cut group a subset
        dv = dist[v, ids[v, :m]]
        assert np.array_equal(dv, dist[v, ref_ids[v, :m]])
        for d in np.unique(dv):
            ours, theirs, tied = set(ids[v, :m][dv == d]), set(ref_ids[v, :m][dv == d]), set(np.flatnonzero(dist[v] == d))
            assert (ours == theirs) if len(tied) == len(ours) else (ours <= tied and theirs <= tied)
    assert same.any()
    sj = skinning.start_joints(c["rig"], names)
    lab = so.labels_of(ids, np.asarray(c["rig"].skins), sj)
    assert np.array_equal(lab, so.labels(ids, c["rig"], names))
    assert np.array_equal(lab[same], c["labels"][same])                                # exact where the slot order is the reference's
    assert np.array_equal(so.labels_of(ref_ids, np.asarray(c["rig"].skins), sj), c["labels"])   # and for the reference's own order
    lf = np.asarray(leaf, dtype=np.int64)
    assert np.array_equal(ref[:, 2::3][same], np.where(ids >= 0, lf[np.maximum(ids, 0)], 0)[same])
    # the dataset tensors against load_skin of the reference's own file, per bone id, within the file's %.6f and float32
    si, snn, mask, jids = so.bind_tensors(ids, invd, bones, leaf, sj)
    ref_input, ref_nn, _, ref_mask, _ = formats.load_skin(c["skin_file"], k)
    assert np.array_equal(mask, ref_mask) and np.array_equal(snn[same], ref_nn[same])
    assert np.array_equal(jids, sj[snn].astype(np.int64))
    g3, r3 = si.astype(np.float64).reshape(V, k, 8), ref_input.reshape(V, k, 8)
    for v in range(V):
        for s in range(m):
            t = int(np.nonzero(ids[v] == ref_nn[v, s])[0][0])
            assert np.all(np.abs(g3[v, t] - r3[v, s]) <= 5e-7 + np.abs(r3[v, s]) * 2.0 ** -23)
        assert np.array_equal(g3[v, m:], np.repeat(g3[v, :1], k - m, 0))


@pytest.mark.parametrize("mode,key", [("train_skin", "weights_train_skin"), ("joint2rig", "weights_joint2rig")])
def test_skin_weights_equal_fixture(mode, key, tmp_path):
    from morig_amd import formats
    c = load_skin_case("skin_connected", tmp_path)
    _, nn, _, mask, _ = formats.load_skin(c["skin_file"], c["meta"]["k"])
    w = so.skin_weights(c["logits"], nn, mask, c["tpl_edge_index"], len(c["meta"]["bone_names"]), mode=mode)
    assert w.shape == c[key].shape and np.abs(w - c[key]).max() <= 1e-6
    sums = w.sum(1)
    assert np.all((np.abs(sums - 1.0) <= 1e-9) | (sums == 0.0))
