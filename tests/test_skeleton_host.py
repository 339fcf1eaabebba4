"""CPU: the host logic of the two skeleton networks (morig_amd/models/rootnet.py, bonenet.py) -- packing, the per-mesh row bias,
the order of the random draws, batching -- on the torch emulation of the op layer (tests/emulate.py), against the reference's logits
in tests/golden/skel_nets.npz. This does NOT exercise the HIP kernels (tests/test_gpu_skeleton.py does, on an MI355X)."""
import numpy as np
import pytest
import torch

import morig_amd.runtime as runtime
from emulate import EmuOps
from helpers import rel_excess
from morig_amd import synth
from morig_amd.models import bonenet, rootnet
from test_skeleton_oracle import NET_CASES, case, load

MODELS = {"rootnet": rootnet.ROOTNET, "bonenet": bonenet.PairCls}


@pytest.fixture(autouse=True, params=["fp32-activations", "split-activations"])
def emulated_ops(request):
    ops = EmuOps()
    ops.emulate_split = request.param == "split-activations"
    runtime._test_ops = ops
    yield
    runtime._test_ops = None


def net_batch(meta, arrs, name, device="cpu"):
    """the batch a case of skel_nets was made from: the synthetic meshes regenerated, the stored joints and pair attributes, pairs in
    combinations order over the concatenated joints"""
    c = case(arrs, name)
    spec, counts = meta["cases"][name]["spec"], meta["cases"][name]["n_joints"]
    data = synth.collate([synth.make_mesh(seed, n_side=n_side, with_skin=False) for seed, n_side, _ in spec])
    jp = np.concatenate([[0], np.cumsum(counts)])
    pairs = np.concatenate([np.stack(np.triu_indices(n, k=1), 1) + jp[b] for b, n in enumerate(counts)], 0)
    data.joints = torch.from_numpy(c["joints"]).float()
    data.pairs = torch.from_numpy(pairs).float()
    data.pair_attr = torch.from_numpy(c["pair_attr"])
    data.joints_batch = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    data.pairs_batch = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor([n * (n - 1) // 2 for n in counts]))
    return data.to(device), c


def net_models(meta, device="cpu"):
    return {net: synth.load_recipe(MODELS[net]().eval(), meta["nets"][net]["recipe_seed"], mild=True).to(device) for net in MODELS}


def net_tolerance(c, net):
    """criterion 4: 1e-4 of max(1, output scale), or the reference's own float32-against-float64 deviation where that is larger"""
    own = float(np.abs(c[f"{net}_f32"].astype(np.float64) - c[f"{net}_f64"]).max())
    return max(1e-4, own / max(1.0, float(np.abs(c[f"{net}_f32"]).max())))


def run_both(models, meta, data, seed_key="torch_seed", random=False):
    """ROOTNET then PairCls after one torch.manual_seed: predict_skeleton's order, the order the fixture's draws were made in"""
    torch.manual_seed(meta[seed_key])
    return {net: models[net](data, **{meta["nets"][net]["flag"]: random}) for net in ("rootnet", "bonenet")}


@pytest.mark.parametrize("name", NET_CASES)
def test_logits_equal_reference_on_the_emulated_op_layer(name):
    meta, arrs = load("skel_nets")
    data, c = net_batch(meta, arrs, name)
    outs = run_both(net_models(meta), meta, data)
    counts = meta["cases"][name]["n_joints"]
    torch.manual_seed(meta["torch_seed"])                       # the recorded draws are what this seed gives, in this order
    assert [int(torch.randint(n, (1,))) for _ in range(4) for n in counts] == c["fps_starts"].tolist()
    for net in MODELS:
        logits, labels = outs[net]
        ref = torch.from_numpy(c[f"{net}_f32"])
        assert logits.shape == ref.shape and rel_excess(logits, ref, net_tolerance(c, net), strict=False) <= 0, net
    assert torch.equal(outs["bonenet"][1], data.pair_attr[:, -1:]) and outs["rootnet"][1].sum() == len(counts)


def test_random_branches_draw_as_the_reference_does():
    meta, arrs = load("skel_nets")
    data, c = net_batch(meta, arrs, "single")
    outs = run_both(net_models(meta), meta, data, "random_torch_seed", True)
    for net in MODELS:
        logits, labels = outs[net]
        assert rel_excess(logits, torch.from_numpy(c[f"{net}_random_f32"]), net_tolerance(c, net), strict=False) <= 0, net
        assert torch.equal(labels.cpu(), torch.from_numpy(c[f"{net}_random_labels"])), net


def test_shape_encoder_rows_of_a_batch_equal_the_mesh_alone():
    """meshes of a batch do not see each other: the shape encoder (no random draws) gives a mesh the same vector alone and batched"""
    meta, arrs = load("skel_nets")
    data, _ = net_batch(meta, arrs, "ragged")
    enc = net_models(meta)["bonenet"].shape_encoder
    whole = enc(data)
    one = synth.collate([synth.make_mesh(meta["cases"]["ragged"]["spec"][1][0], n_side=meta["cases"]["ragged"]["spec"][1][1], with_skin=False)])
    assert torch.allclose(enc(one)[0], whole[1], rtol=0, atol=2e-5)


@pytest.mark.parametrize("net", sorted(MODELS))
def test_train_mode_is_refused(net):
    meta, arrs = load("skel_nets")
    data, _ = net_batch(meta, arrs, "single")
    with pytest.raises(NotImplementedError, match="train-mode"):
        MODELS[net]().train()(data)


def test_pooled_layers_reach_the_library_with_128_rows():
    """the pooled GEMM launch always runs the 128-column tile and reads weights, bias and affine up to the next multiple of 128 rows:
    bonenet's 64-wide mlp_glb output is handed over with zero rows appended (a 64-row image is read past its end on the device)"""
    from morig_amd import native
    narrow = bonenet.ShapeEncoder()._pack()[-1]
    assert narrow.N == 64 and narrow.W.shape[0] == 64
    wide = native.padded_for_pool(narrow)
    assert wide is native.padded_for_pool(narrow) and wide.N == 64 and wide.K == narrow.K and wide.W.shape == (128, narrow.W.shape[1])
    for name, fill in (("W", 0.0), ("bias", 0.0), ("scale", 1.0), ("shift", 0.0), ("Wsplit", 0.0)):
        a, b = getattr(narrow, name), getattr(wide, name)
        assert b.shape[0] == 128 and torch.equal(b[:64], a) and bool((b[64:] == fill).all()), name
    full = rootnet.ShapeEncoder()._pack()[-1]
    assert native.padded_for_pool(full) is full
