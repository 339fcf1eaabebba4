"""Skinning on the device (morig_amd/skinning.py, csrc/skin.hip) against fixtures made by the reference's own functions
(tools/make_skin_golden.py): volumetric geodesic distances, bind rows and labels, the dataset tensors SkinNet reads, the _skin.txt
writer, and the post-processing of SkinNet's logits in both callers' orders."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from morig_amd import formats, skinning  # noqa: E402
from skin_oracle import labels as _labels, stable_rows as _stable_rows  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("skin_connected", "skin_islands", "skin_outside", "skin_fewbones")
NEW_SYMBOLS = ("morig_vol_geodesic_workspace", "morig_vol_geodesic", "morig_skin_bind", "morig_skin_scatter", "morig_skin_filter")
DEV = "cuda:0"


def load_case(name, tmp_path):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    c = {k: z[k] for k in z.files if k != "meta"}
    c["meta"] = meta
    grid = np.unpackbits(c["vox_bits"])[:88 ** 3].reshape(88, 88, 88).astype(bool)
    c["vox"] = types.SimpleNamespace(data=grid, translate=meta["translate"], scale=meta["scale"], dims=meta["dims"])
    rig_file = os.path.join(str(tmp_path), name + "_rig.txt")
    with open(rig_file, "wb") as f:
        f.write(c["rig_txt"].tobytes())
    c["rig"] = formats.Rig(rig_file)
    skin_file = os.path.join(str(tmp_path), name + "_skin.txt")
    with open(skin_file, "wb") as f:
        f.write(c["skin_txt"].tobytes())
    c["skin_file"] = skin_file
    return c


# ---------------------------------------------------------------- host / CPU
@pytest.mark.parametrize("name", CASES)
def test_get_bones_matches_reference(name, tmp_path):
    c = load_case(name, tmp_path)
    bones, names, leaf = skinning.get_bones(c["rig"])
    assert names == c["meta"]["bone_names"]
    assert np.array_equal(np.asarray(leaf, dtype=np.uint8), c["is_leaf"])
    assert np.array_equal(bones, c["bones"])


@pytest.mark.parametrize("name", CASES)
def test_write_skin_file_reproduces_reference_bytes(name, tmp_path):
    c = load_case(name, tmp_path)
    out = os.path.join(str(tmp_path), "ours_skin.txt")
    skinning.write_skin_file(out, c["bones"], c["meta"]["bone_names"], c["bind_rows"][:, 1:], c["labels"])
    with open(out, "rb") as f:
        assert f.read() == c["skin_txt"].tobytes()
    for a, b in zip(formats.load_skin(out), formats.load_skin(c["skin_file"])):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b)
        else:
            assert a == b


def test_new_symbols_declared_and_exported():
    from morig_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "morig_hip.h")).read(), flags=re.S)
    lib = native.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in native.EXPORTS
        assert hasattr(lib, s)


def test_skin_weights_rejects_unknown_mode():
    with pytest.raises(ValueError):
        skinning.skin_weights(torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.long), torch.ones(1, 2, dtype=torch.long),
                              torch.zeros(2, 0, dtype=torch.long), torch.zeros(1, dtype=torch.long), [2], mode="eval")


# ---------------------------------------------------------------- device
def _dist(c):
    bones, _, _ = skinning.get_bones(c["rig"])
    pos = torch.from_numpy(c["pos"]).to(DEV)
    return skinning.volumetric_geodesic(pos, c["vox"], bones)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_volumetric_geodesic_equals_reference(name, tmp_path):
    c = load_case(name, tmp_path)
    d = _dist(c)
    assert d.dtype == torch.int32 and d.shape == c["dist"].shape
    assert np.array_equal(d.cpu().numpy(), c["dist"])


@pytest.mark.gpu
def test_volumetric_geodesic_batched_ragged_and_deterministic(tmp_path):
    cs = [load_case(n, tmp_path) for n in ("skin_fewbones", "skin_islands", "skin_connected", "skin_outside")]
    pos = torch.from_numpy(np.concatenate([c["pos"] for c in cs], 0)).to(DEV)
    batch = torch.cat([torch.full((len(c["pos"]),), i, dtype=torch.long) for i, c in enumerate(cs)]).to(DEV)
    bones = [skinning.get_bones(c["rig"])[0] for c in cs]
    a = skinning.volumetric_geodesic_batched(pos, batch, [c["vox"] for c in cs], bones)
    b = skinning.volumetric_geodesic_batched(pos, batch, [c["vox"] for c in cs], bones, n_slots=3)
    for i, c in enumerate(cs):
        one = _dist(c)
        assert torch.equal(a[i], one) and torch.equal(b[i], one)
        assert np.array_equal(a[i].cpu().numpy(), c["dist"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_bind_rows_and_labels(name, tmp_path):
    c = load_case(name, tmp_path)
    k = c["meta"]["k"]
    bones, names, leaf = skinning.get_bones(c["rig"])
    dist_ref = c["dist"]
    o = skinning.skin_bind(torch.from_numpy(dist_ref).to(DEV), bones, leaf, k, rig=c["rig"])
    ids = o["bind_ids"].cpu().numpy().astype(np.int64)
    invd = o["bind_invd"].cpu().numpy()
    want_ids, want_invd = _stable_rows(dist_ref, leaf, k)
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(invd.view(np.int64), want_invd.view(np.int64))           # bit-exact fp64
    assert np.array_equal(o["labels"].cpu().numpy(), _labels(want_ids, c["rig"], names))
    rows = skinning.bind_rows(o, leaf)
    lf = np.asarray(leaf, dtype=np.int64)
    assert np.array_equal(rows[:, 2::3], np.where(want_ids >= 0, lf[np.maximum(want_ids, 0)], 0))
    # against the reference's own rows (its argsort is not stable): equal D sequences, equal id sets per tie group, the group cut at
    # slot k a subset
    ref = c["bind_rows"][:, 1:]
    ref_ids = ref[:, 0::3].astype(np.int64)
    nb = dist_ref.shape[1]
    for v in range(len(ids)):
        m = min(k, nb)
        dv = dist_ref[v, ids[v, :m]]
        assert np.array_equal(dv, dist_ref[v, ref_ids[v, :m]])
        for d in np.unique(dv):
            ours, theirs = set(ids[v, :m][dv == d]), set(ref_ids[v, :m][dv == d])
            if (dist_ref[v] == d).sum() == len(ours):
                assert ours == theirs
            else:
                assert ours <= set(np.nonzero(dist_ref[v] == d)[0]) and theirs <= set(np.nonzero(dist_ref[v] == d)[0])
        assert np.all(ref_ids[v, m:] == -1) and np.all(ids[v, m:] == -1)
    # the dataset tensors against formats.load_skin of the same rows through the file (%.6f) -- written by write_skin_file, whose
    # bytes equal the reference's writer (test above) -- within that rounding and float32's; the reference's own file orders tie groups
    # its own way, so it is compared per bone id
    ours_file = os.path.join(str(tmp_path), "ours_skin.txt")
    skinning.write_skin_file(ours_file, bones, names, rows, o["labels"].cpu().numpy())
    skin_input, skin_nn, _, loss_mask, _ = formats.load_skin(ours_file, k)
    got = o["skin_input"].cpu().numpy().astype(np.float64)
    tol = 5e-7 + np.abs(skin_input) * 2.0 ** -23
    assert np.all(np.abs(got - skin_input) <= tol)
    assert np.array_equal(o["skin_nn"].cpu().numpy(), skin_nn)
    ref_input, ref_nn, _, ref_mask, _ = formats.load_skin(c["skin_file"], k)
    assert np.array_equal(ref_mask, loss_mask)
    g3 = got.reshape(len(ids), k, 8)
    r3 = ref_input.reshape(len(ids), k, 8)
    for v in range(len(ids)):
        for s in range(min(k, nb)):
            t = int(np.nonzero(ids[v] == ref_nn[v, s])[0][0])
            assert np.all(np.abs(g3[v, t] - r3[v, s]) <= 5e-7 + np.abs(r3[v, s]) * 2.0 ** -23)
    assert np.array_equal(o["loss_mask"].cpu().numpy(), loss_mask)
    nnj = o["skin_nnjids"].cpu().numpy()
    nn = o["skin_nn"].cpu().numpy()
    assert np.array_equal(nnj, np.array([[c["rig"].names.index(names[b][0]) for b in row] for row in nn]))


@pytest.mark.gpu
def test_skinnet_on_device_inputs_equals_file_inputs(tmp_path):
    from helpers import rel_excess
    from morig_amd import models, synth
    c = load_case("skin_connected", tmp_path)
    k = c["meta"]["k"]
    bones, names, leaf = skinning.get_bones(c["rig"])
    d = _dist(c)
    o = skinning.skin_bind(d, bones, leaf, k, rig=c["rig"])
    si = o["skin_input"]
    # the same rows through the _skin.txt round trip (the reference's own file orders equal-distance bones its own way, so the slot
    # order -- which SkinNet sees -- is taken from the rows made here)
    path = os.path.join(str(tmp_path), "dev_skin.txt")
    skinning.write_skin_file(path, bones, names, skinning.bind_rows(o, leaf), o["labels"].cpu().numpy())
    file_input = torch.from_numpy(formats.load_skin(path, k)[0]).float()
    mesh = synth.make_mesh(5, n_side=24, with_skin=False)
    kw = dict(nearest_bone=k, use_Dg=True, use_Lf=True, num_keyframes=5, use_motion=True, motion_dim=32, aggr_method="attn")
    m = synth.load_recipe(models.skinnet_motion(**kw).eval(), 204).to(DEV)
    outs = []
    for s_in in (si, file_input):
        mesh.skin_input = s_in.cpu()
        b = synth.collate([mesh]).to(DEV)
        outs.append(m(b, b.pred_flow)[2])
    assert rel_excess(outs[0], outs[1], 1e-4) <= 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode,key", [("train_skin", "weights_train_skin"), ("joint2rig", "weights_joint2rig")])
def test_skin_weights_equal_reference(mode, key, tmp_path):
    c = load_case("skin_connected", tmp_path)
    _, nn, _, mask, _ = formats.load_skin(c["skin_file"], c["meta"]["k"])
    V = len(c["pos"])
    nb = len(c["meta"]["bone_names"])
    w = skinning.skin_weights(torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(nn).to(DEV), torch.from_numpy(mask).to(DEV),
                              torch.from_numpy(c["tpl_edge_index"]).to(DEV), torch.zeros(V, dtype=torch.long, device=DEV), [nb], mode=mode)
    assert len(w) == 1 and w[0].shape == (V, nb) and w[0].dtype == torch.float64
    assert np.abs(w[0].cpu().numpy() - c[key]).max() <= 1e-6


@pytest.mark.gpu
def test_skin_weights_batched_and_isolated_vertex(tmp_path):
    """two meshes in one batch (the second a copy with one extra vertex that has no edges): the first mesh's weights are unchanged,
    the isolated vertex keeps its own unfiltered row before the threshold (documented in skinning.py)"""
    c = load_case("skin_connected", tmp_path)
    _, nn, _, mask, _ = formats.load_skin(c["skin_file"], c["meta"]["k"])
    V = len(c["pos"])
    nb = len(c["meta"]["bone_names"])
    rng = np.random.default_rng(3)
    extra_logits = rng.normal(0.0, 2.0, size=(1, nn.shape[1])).astype(np.float32)
    logits = np.concatenate([c["logits"], c["logits"], extra_logits], 0)
    nn2 = np.concatenate([nn, nn, nn[:1]], 0)
    mask2 = np.concatenate([mask, mask, mask[:1]], 0)
    tpl = c["tpl_edge_index"]
    tpl2 = np.concatenate([tpl, tpl + V], 1)
    batch = np.concatenate([np.zeros(V), np.ones(V + 1)]).astype(np.int64)
    ws = skinning.skin_weights(torch.from_numpy(logits).to(DEV), torch.from_numpy(nn2).to(DEV), torch.from_numpy(mask2).to(DEV),
                               torch.from_numpy(tpl2).to(DEV), torch.from_numpy(batch).to(DEV), [nb, nb], mode="train_skin")
    assert np.abs(ws[0].cpu().numpy() - c["weights_train_skin"]).max() <= 1e-6
    assert np.abs(ws[1][:V].cpu().numpy() - c["weights_train_skin"]).max() <= 1e-6
    p = torch.softmax(torch.from_numpy(extra_logits), dim=1).numpy()[0] * mask[0]
    row = np.zeros(nb)
    for s in range(nn.shape[1]):
        if mask[0, s] == 1:
            row[nn[0, s]] = p[s]
    row[row < row.max() * 0.5] = 0.0
    row = row / (row.sum() + 1e-10)
    assert np.abs(ws[1][V].cpu().numpy() - row).max() <= 1e-6
