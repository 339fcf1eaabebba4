"""GPU: morig_amd/labels.py (csrc/labels.hip) against tests/labels_oracle.py -- on-grid scenes where every product of the ray test is exact
(bit for bit, nothing excused: this is where touching, ties, orientation and the miss rule are tested), the smallest shapes at which the
kernels branch, generated scenes (a ray, a kept flag or a label is excused only where the oracle's own margin is under 1e-9, for the
radius 1e-12, and tests/test_labels_oracle.py shows on the CPU that this is under a thousandth), determinism, and the results going
through the stages that consume them."""
import numpy as np
import pytest
import torch

import labels_oracle as lo
from morig_amd import labels, metrics, models, synth
from morig_amd.formats import Rig

pytestmark = pytest.mark.gpu


def host(t):
    return t.cpu().numpy()


def same_bits(got, want):
    """equal shapes, types and bits; every NaN counts as the same NaN"""
    got, want = host(got) if isinstance(got, torch.Tensor) else np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()
    return got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------------------- on grid
@pytest.mark.parametrize("orientation", [0, 1, -1])
def test_on_grid_rays_equal_the_oracle_bit_for_bit(orientation):
    v, f, o, d, names = lo.on_grid_scene()
    nothing = np.zeros((0, 3), dtype=np.int64)
    # the scene, a mesh without faces and a mesh without rays in one batch
    t, face, point = labels.cast_rays(np.concatenate([o, o]), np.concatenate([d, d]), [0, len(o), 2 * len(o), 2 * len(o)], [v, v[:4], v],
                                      [f, nothing, f], orientation=orientation)
    want = lo.cast(o, d, v, f, orientation)
    assert t[0].is_cuda and same_bits(t[0], want["t"]) and same_bits(face[0], want["face"]) and same_bits(point[0], want["point"])
    assert bool(torch.isinf(t[1]).all()) and bool((face[1] == -1).all()) and bool(torch.isnan(point[1]).all()) and t[2].numel() == 0
    at = {n: i for i, n in enumerate(names)}
    got = host(face[0])
    if orientation == 0:
        assert got[at["shared_edge"]] == got[at["corner"]] == 0 and got[at["twins"]] == 8 and got[at["zero_area"]] == 5 and got[at["nan_vertex"]] == 7
        assert got[at["coplanar"]] == got[at["behind"]] == got[at["on_the_face"]] == -1
    if orientation == -1:
        assert got[at["two_plates"]] == -1 and got[at["inside"]] == -1 and got[at["from_above"]] == 0      # the ray does not continue


@pytest.mark.parametrize("n_faces", [0, 1, 63, 64, 65, 129])
def test_face_counts_around_the_wave_width(n_faces):
    v, f = lo.grid_triangles(n_faces, 1)
    o, d = lo.grid_rays(37, n_faces)
    v2, f2 = lo.grid_triangles(65, 2)
    t, face, point = labels.cast_rays(np.concatenate([o, o]), np.concatenate([d, d]), [0, 37, 74], [v, v2], [f, f2])
    hits = 0
    for b, (vb, fb) in enumerate(((v, f), (v2, f2))):
        want = lo.cast(o, d, vb, fb)
        assert same_bits(t[b], want["t"]) and same_bits(face[b], want["face"]) and same_bits(point[b], want["point"]), b
        hits += int((want["face"] >= 0).sum())
    assert hits > 5


def test_a_face_outside_its_mesh_is_reported_not_read():
    v, f = lo.grid_triangles(5, 3)
    o, d = lo.grid_rays(9, 3)
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError, match="outside its mesh"):
        labels.cast_rays(o, d, [0, 9], [v], [bad])
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="outside its mesh"):
        labels.bone_ray_labels([v], [bad], [lo.PlainRig([[1, 1, 1], [2, 2, 2]], [-1, 0])])


# ------------------------------------------------------------------------------------------------------------------------- the branches
def test_rays_per_joint_where_the_select_kernel_branches():
    counts = [0, 1, 2, 5, 6, 14, 64, 65, 1024, 0, 63, 128, 3]
    sets = [lo.hit_set(n, 7) for n in counts] + [np.full(6, np.inf), np.full(14, 0.25), np.array([0.5, np.inf, 0.5, 0.5, np.inf, 0.25])]
    t, ptr = np.concatenate(sets), np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    for keep_factor, fill in ((2.0, float("nan")), (0.5, -1.0), (1.0, 0.0)):
        got = labels.select_hits(torch.from_numpy(t).cuda(), ptr, keep_factor=keep_factor, fill=fill)
        want = lo.select(t, np.diff(ptr), keep_factor, fill)
        for k in ("kept", "n_hit", "n_kept", "p20", "featuresize"):
            assert got[k].is_cuda and same_bits(got[k], want[k]), (k, keep_factor)
        assert (want["n_kept"] < want["n_hit"]).any() and (want["n_hit"] == 0).any()
    with pytest.raises(ValueError, match="1025 rays"):
        labels.select_hits(torch.ones(1025, dtype=torch.float64).cuda(), [0, 1025])


@pytest.mark.parametrize("n_verts", [1, 255, 256, 257])
def test_vertex_counts_and_kept_counts_around_the_tile(n_verts):
    rng = np.random.default_rng(n_verts)
    radius = 0.15
    verts = [rng.uniform(0, 1, (n_verts, 3)), rng.uniform(0, 1, (300, 3)), np.zeros((0, 3)), rng.uniform(0, 1, (40, 3))]
    n_rays = [300, 256, 5, 0]                                                           # kept: 201 (no multiple of the tile), 0, some, no rays
    ptr = np.concatenate([[0], np.cumsum(n_rays)])
    point = rng.uniform(0, 1, (ptr[-1], 3))
    kept = np.zeros(ptr[-1], dtype=np.uint8)
    kept[:300][rng.permutation(300)[:201]] = 1
    kept[556:561] = [1, 0, 1, 0, 0]
    point[kept == 0] = np.nan                                                           # what is not kept is never looked at
    point[299] = verts[0][0] + [0.0, 0.0, radius / 2]
    kept[299] = 1                                                                       # vertex 0 of mesh 0 is labelled by the last ray of the second tile
    got = labels.attention(verts, point, kept, ptr, radius=radius)
    excused = 0
    for b in range(4):
        want, margin = lo.attention(verts[b], point[ptr[b]:ptr[b + 1]], kept[ptr[b]:ptr[b + 1]], radius)
        firm = margin >= lo.RADIUS_MARGIN
        excused += int((~firm).sum())
        assert got[b].dtype == torch.float32 and tuple(got[b].shape) == (len(verts[b]),) and np.array_equal(host(got[b])[firm], want[firm]), b
    assert excused == 0 and host(got[0])[0] == 1.0 and not host(got[1]).any() and not host(got[3]).any()


def test_vertex_counts_at_the_segment_edges_equal_the_meshes_alone_and_the_oracle():
    counts = [0, 1, 256, 0, 257, 255, 0]                       # empty meshes in front, between and behind; a full workgroup, one row more, one less
    rng, radius = np.random.default_rng(7), 0.15
    verts = [rng.uniform(0, 1, (n, 3)) for n in counts]
    ptr = np.arange(len(counts) + 1) * 6
    point, kept = rng.uniform(0, 1, (ptr[-1], 3)), (rng.uniform(size=ptr[-1]) < 0.7).astype(np.uint8)
    got = labels.attention(verts, point, kept, ptr, radius=radius)
    for b, n in enumerate(counts):
        rows = slice(ptr[b], ptr[b + 1])
        want, margin = lo.attention(verts[b], point[rows], kept[rows], radius)
        firm = margin >= lo.RADIUS_MARGIN
        alone, = labels.attention(verts[b:b + 1], point[rows], kept[rows], [0, 6], radius=radius)
        assert tuple(got[b].shape) == (n,) and same_bits(got[b], host(alone)) and np.array_equal(host(got[b])[firm], want[firm]) and firm.all(), b
    assert 0 < sum(float(g.sum()) for g in got) < sum(counts)


# ------------------------------------------------------------------------------------------------------------------------- generated
def firm_compare(got, want, what):
    """discrete results equal wherever the oracle's margins allow; continuous ones within 1e-12 where the discrete ones agree"""
    attn, fs, det = got
    ray_firm = want["ray_margin"] >= lo.MARGIN
    joint_firm = np.array([ray_firm[want["ray_joint"] == j].all() for j in range(len(want["n_hit"]))])
    keep_firm = ray_firm & (want["keep_margin"] >= lo.MARGIN) & joint_firm[want["ray_joint"]]
    vert_firm = (want["radius_margin"] >= lo.RADIUS_MARGIN) & keep_firm.all()
    R, V = len(ray_firm), len(vert_firm)
    assert (~keep_firm).sum() <= 0.001 * R and (~vert_firm).sum() <= 0.001 * V, what
    face, t, point = host(det["face"]), host(det["t"]), host(det["point"])
    assert np.array_equal(face[ray_firm], want["face"][ray_firm]), what
    assert np.array_equal(host(det["kept"])[keep_firm], want["kept"][keep_firm]), what
    assert np.array_equal(host(attn)[vert_firm], want["attn"][vert_firm]) and attn.dtype == torch.float32, what
    agree = (face == want["face"]) & (face >= 0)
    dt, dp = np.abs(t[agree] - want["t"][agree]).max(initial=0.0), np.abs(point[agree] - want["point"][agree]).max(initial=0.0)
    assert np.all(np.isinf(t[face < 0])) and np.all(np.isnan(point[face < 0])), what
    assert np.array_equal(host(det["n_hit"])[joint_firm], want["n_hit"][joint_firm]) and np.array_equal(host(det["ray_joint"]), want["ray_joint"]), what
    settled = joint_firm & np.array([keep_firm[want["ray_joint"] == j].all() for j in range(len(joint_firm))])
    assert np.array_equal(host(det["n_kept"])[settled], want["n_kept"][settled]), what
    def gap(a, b):                                                                      # a joint without a hit has NaN on both sides
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        return np.abs(a[~np.isnan(b)] - b[~np.isnan(b)]).max(initial=0.0)

    dq, df = gap(host(det["p20"])[settled], want["p20"][settled]), gap(host(fs)[settled], want["featuresize"][settled])
    bit_equal = all(same_bits(a, want[k]) for a, k in ((det["t"], "t"), (det["point"], "point"), (det["p20"], "p20"), (fs, "featuresize")))
    print(f"{what}: {R} rays, {int((~keep_firm).sum())} left out; {V} vertices, {int((~vert_firm).sum())} left out; max |t diff| {dt:.3g}, "
          f"|point diff| {dp:.3g}, |p20 diff| {dq:.3g}, |featuresize diff| {df:.3g}; labelled {int(host(attn).sum())}; bit-equal {bit_equal}")
    assert dt <= 1e-12 and dp <= 1e-12 and dq <= 1e-12 and df <= 1e-12, what


def generated_batch():
    scenes = [lo.generated_scene(n) for n in lo.GENERATED_SIDES]
    # (a formats.Rig rebuilds its positions parent-first, which moves them by a rounding: the oracle's reference is of the plain arrays)
    return [s[0] for s in scenes], [s[1] for s in scenes], [lo.PlainRig(s[2], s[3]) for s in scenes]


def test_generated_torus_batch_equals_the_oracle_where_it_is_firm():
    verts, faces, rigs = generated_batch()
    out = labels.bone_ray_labels(verts, faces, rigs)
    for n, got in zip(lo.GENERATED_SIDES, out):
        firm_compare(got, lo.generated_reference(n), f"torus {n}")
        assert np.all(np.abs(host(got[1]) - 0.12) < 0.012)


def test_a_batch_mixing_the_edge_shapes():
    v16, f16, pos, hier = lo.generated_scene(16)
    bv, bf = lo.box_mesh(0.5, 0.2, 0.125)
    nv, nf = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    star = lo.PlainRig(np.concatenate([[[0.01, 0.02, 0.005]], np.random.default_rng(0).uniform(-0.3, 0.3, (16, 3))]), [-1] + [0] * 16)
    meshes = [(v16, f16, lo.PlainRig(pos, hier)), (nv, nf, lo.PlainRig([[0, 0, 0], [0, 1, 0]], [-1, 0])), (bv, bf, lo.PlainRig([[0, 0, 0]], [-1])),
              (bv, bf, star), (v16, nf, lo.PlainRig(pos, hier))]
    for n_rays in (14, 64, 5):                                                          # 64 x 16 children: 1 024 rays at one joint
        out = labels.bone_ray_labels([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes], n_rays=n_rays, radius=0.03)
        for i, ((v, f, rig), got) in enumerate(zip(meshes, out)):
            want = lo.labels(v, f, rig.pos, rig.hierarchy, n_rays=n_rays, radius=0.03)
            if i == 3:                                                                  # a box is all edges and diagonals: only what is firm, no share promised
                firm = want["ray_margin"] >= lo.MARGIN
                face, t = host(got[2]["face"]), host(got[2]["t"])
                agree = (face == want["face"]) & (face >= 0)
                assert np.array_equal(face[firm], want["face"][firm]) and firm.sum() > 0.5 * len(firm)
                assert np.abs(t[agree] - want["t"][agree]).max(initial=0.0) <= 1e-12 and host(got[2]["n_hit"])[0] == 16 * n_rays
            else:
                firm_compare(got, want, f"mixed batch, mesh {i}, {n_rays} rays")


# ------------------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_and_a_mesh_alone_give_the_same_bits():
    verts, faces, rigs = generated_batch()
    first = labels.bone_ray_labels(verts, faces, rigs, orientation=-1)
    second = labels.bone_ray_labels(verts, faces, rigs, orientation=-1)
    alone = labels.bone_ray_labels(verts[1:2], faces[1:2], rigs[1:2], orientation=-1)[0]

    def equal(a, b):
        return same_bits(a[0], host(b[0])) and same_bits(a[1], host(b[1])) and all(same_bits(a[2][k], host(b[2][k])) for k in a[2])

    assert all(equal(a, b) for a, b in zip(first, second)) and equal(alone, first[1])
    assert int(host(first[1][2]["n_hit"]).sum()) == 168                                 # the torus' normals point into the tube


# ------------------------------------------------------------------------------------------------------------------------- downstream
def test_labels_feed_the_mask_training_step_and_the_metrics():
    n_side = 9
    batch = synth.make_batch([21, 22], n_side=n_side)
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    i10, i01, i11 = np.roll(idx, -1, 0), np.roll(idx, -1, 1), np.roll(np.roll(idx, -1, 0), -1, 1)
    faces = np.concatenate([np.stack([idx, i10, i11], -1).reshape(-1, 3), np.stack([idx, i11, i01], -1).reshape(-1, 3)], 0)
    verts = [batch.pos[batch.batch == b].double() for b in range(2)]
    rigs = []
    for v in verts:
        pos, hier = lo.torus_chain(8, seed=3)
        pos[:, 1] += float(v[:, 1].mean())                                              # synth lifts the torus onto y >= 0
        rigs.append(Rig.from_arrays(pos, hier, 0))
    out = labels.bone_ray_labels([v.cuda() for v in verts], [faces, faces], rigs, radius=0.08)
    mask = torch.cat([o[0] for o in out])
    assert mask.is_cuda and mask.dtype == torch.float32 and 0.0 < float(mask.mean()) < 1.0
    model = models.masknet_motion(num_keyframes=5, chn_output=1, aggr_method="attn").train().cuda()
    data = batch.to("cuda")
    data.mask = mask
    with torch.enable_grad():
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
        _, _, mask_pred = model(data, data.pred_flow)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(mask_pred, data.mask.float().unsqueeze(1), reduction="mean")   # train_rig.py:157
        loss.backward()
        opt.step()
    assert np.isfinite(float(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    fs = [o[1] for o in out]
    assert all(bool((f > 0.05).all()) and bool((f < 0.2).all()) for f in fs)
    pred = np.concatenate([rigs[0].pos + 0.01, rigs[1].pos + 0.5])
    res = metrics.evaluate_rigs(torch.from_numpy(pred).cuda(), [0, 8, 16], rigs, fs)
    assert res["hits"].tolist() == [8, 0] and res["recall"].tolist() == [1.0, 0.0]
