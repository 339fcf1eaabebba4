"""tests/skin_loss_oracle.py (float64, closed-form gradients) against a literal statement of the log-ratio formula, against the
reference's recorded float32 results (tests/golden/loss_logratio_*.npz, loss_skin_ce.npz; tools/make_skin_loss_golden.py) within the
deviations the generator stored, and the conditions the fixtures were generated under; the C ABI of the new entry points."""
import itertools
import os

import numpy as np
import pytest
import torch

import skin_loss_oracle as so
from conftest import GOLDEN
from test_loss_oracle import ids, load, rel_max

N_SAMPLE, MIN_DIST, FACTOR = 50, 1e-3, 10.0
LR_CASES = ("all50", "ragged", "d4", "coincident")
LR = {c: load(f"loss_logratio_{c}") for c in LR_CASES}
CE_META, CE = load("loss_skin_ce")


def literal_log_ratio(f, g):
    """the loss of one mesh exactly as the formula reads: every pair against every pair, transposed minus plain, the later pairs weighted"""
    S = f.shape[0]
    pairs = torch.tensor(list(itertools.combinations(range(S), 2)))
    n = len(pairs)
    dist = ((f[pairs[:, 0], None, :] - f[None, pairs[:, 1], :]) ** 2).sum(-1)
    gdist = ((g[pairs[:, 0], None, :] - g[None, pairs[:, 1], :]) ** 2).sum(-1)
    ld, lg = torch.log(dist + 1e-6), torch.log(gdist + 1e-6)
    sq = ((ld.T - ld) - (lg.T - lg)) ** 2
    idx = torch.arange(n)
    wgt = (idx[:, None] < idx[None, :]).to(f.dtype)
    return (sq * wgt / wgt.sum()).sum()


def test_closed_form_gradients_equal_autograd_of_the_literal_statement():
    g = torch.Generator().manual_seed(3)
    for S, D, W in ((3, 4, 4), (7, 8, 4), (12, 4, 8)):
        f = torch.randn(S, D, dtype=torch.float64, generator=g)
        skin = torch.rand(S, W, dtype=torch.float64, generator=g)
        skin[1] = skin[0]                                  # identical skin rows: log(eps) on both sides of the diagonal terms
        with torch.enable_grad():
            leaf = f.clone().requires_grad_(True)
            want = literal_log_ratio(leaf, skin)
            want.backward()
        loss, grad = so.logratio_mesh(f, skin)
        assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
        assert (grad - leaf.grad).abs().max() <= 1e-12 * leaf.grad.abs().max()
        assert abs(float(so.logratio_mesh_loss(f, skin)) - float(want)) <= 1e-12 * abs(float(want))


def test_the_owner_enumeration_of_the_backward_equals_the_scatter():
    """what each entry of the table gathers in the backward kernel, against autograd of the pair sum"""
    g = torch.Generator().manual_seed(4)
    for S in (3, 4, 9):
        L = torch.randn(S, S, dtype=torch.float64, generator=g)
        a, b = so.pair_ids(S)
        n = a.numel()
        with torch.enable_grad():
            leaf = L.clone().requires_grad_(True)
            R = leaf[a[None, :], b[:, None]] - leaf[a[:, None], b[None, :]]
            (0.5 * (R * R)[torch.triu(torch.ones(n, n, dtype=torch.bool), 1)].sum()).backward()
        assert (so.logratio_dL_by_owner(L) - leaf.grad).abs().max() <= 1e-12 * leaf.grad.abs().max()


def test_ce_closed_form_gradient_equals_autograd():
    x = torch.from_numpy(CE["x"]).double()
    label, mask = torch.from_numpy(CE["label"]), ids(CE["mask"])
    with torch.enable_grad():
        leaf = x.clone().requires_grad_(True)
        so.skin_ce_loss(leaf, label, mask, CE_META["K"]).backward()
    assert (so.skin_ce(x, label, mask, CE_META["K"])[1] - leaf.grad).abs().max() <= 1e-13
    g = torch.Generator().manual_seed(5)
    t, w, up = (torch.rand(x.shape, dtype=torch.float64, generator=g) for _ in range(3))
    for reduction, u in (("none", up), ("mean", 1.7), ("sum", 0.3)):
        with torch.enable_grad():
            leaf = x.clone().requires_grad_(True)
            value = so.ce_probs(leaf, t, w, reduction)[0]
            (value * u).sum().backward()
        assert (so.ce_probs(x, t, w, reduction, u)[1] - leaf.grad).abs().max() <= 1e-12


@pytest.mark.parametrize("case", LR_CASES)
def test_log_ratio_oracle_against_the_reference(case):
    meta, z = LR[case]
    loss, grad = so.logratio(torch.from_numpy(z["feat"]).double(), torch.from_numpy(z["gt"]).double(), ids(z["batch"]), ids(z["samples"]),
                             len(meta["sizes"]))
    dev = meta["deviations"]
    assert abs(float(z["loss"]) - float(loss)) / abs(float(loss)) <= dev["dev_loss"] * FACTOR
    assert rel_max(z["grad"].astype(np.float64), grad.numpy()) <= dev["dev_grad"] * FACTOR
    assert dev["dev_loss"] < 1e-6 and dev["dev_grad"] < 1e-5           # the reference itself is a float32 computation, no worse


def test_skin_ce_oracle_against_the_reference():
    loss, grad = so.skin_ce(torch.from_numpy(CE["x"]).double(), torch.from_numpy(CE["label"]).double(), ids(CE["mask"]), CE_META["K"])
    dev = CE_META["deviations"]
    assert abs(float(CE["loss"]) - float(loss)) / abs(float(loss)) <= dev["dev_loss"] * FACTOR
    assert rel_max(CE["grad"].astype(np.float64), grad.numpy()) <= dev["dev_grad"] * FACTOR


@pytest.mark.parametrize("case", LR_CASES)
def test_log_ratio_fixture_conditions(case):
    meta, z = LR[case]
    batch, samples = z["batch"].astype(np.int64), z["samples"].astype(np.int64)
    assert samples.shape == (len(meta["sizes"]), N_SAMPLE) and meta["n_sample"] == N_SAMPLE
    for b, size in enumerate(meta["sizes"]):
        rows = np.nonzero(batch == b)[0]
        assert len(rows) == size >= N_SAMPLE and len(set(samples[b].tolist())) == N_SAMPLE and samples[b].max() < size
        d = so.sq_dist(torch.from_numpy(z["feat"][rows[samples[b]]]).double()).numpy()
        d[np.diag_indices(N_SAMPLE)] = np.inf
        close = sorted(map(tuple, np.argwhere(d < MIN_DIST).tolist()))
        if case == "coincident":
            c = meta["coincident"]
            i, j = (int(np.nonzero(samples[b] == r)[0][0]) for r in c["feature_rows"])
            assert close == sorted([(i, j), (j, i)]) and d[i, j] == 0.0
            assert np.array_equal(z["gt"][c["skin_rows"][0]], z["gt"][c["skin_rows"][1]])
            assert np.isfinite(z["grad"]).all() and np.isfinite(z["loss"])
        else:
            assert close == []
    if case == "all50":
        assert meta["sizes"] == [50] and sorted(samples[0].tolist()) == list(range(50))
    if case == "ragged":
        assert meta["sizes"] == [50, 67, 130] and (meta["D"], meta["W"]) == (32, 48) and meta["keyframe_view"]["T"] == 5
    if case == "d4":
        assert (meta["D"], meta["W"]) == (4, 4)


def test_skin_ce_fixture_conditions():
    K = CE_META["K"]
    label, mask = CE["label"], CE["mask"].astype(np.float32)
    orders = so.vert_mask_orders(label, mask, K)
    assert orders.shape[:2] == (105, 105)
    assert (orders == orders[0, 0]).all(), "a fixture row whose vert_mask depends on the order of the sums"
    vm = so.vert_mask_sequential(label, mask, K)
    assert np.array_equal(vm, CE["vert_mask"]) and np.array_equal(vm, orders[0, 0])
    nz = ((label[:, :K] * mask[:, :K]) != 0).sum(1)
    assert set(nz.tolist()) == set(range(K + 1))
    assert (vm & (nz > 0)).any() and (~vm & (nz > 0)).any() and not vm[nz == 0].any()
    assert (mask[:, :K] == 0).any() and CE_META["redrawn"] > 0
    # the known-answer rows are order-DEPENDENT, a dozen, both answers among them, and the stored answer is the sequential rule's
    kl, km = CE["known_label"], CE["known_mask"].astype(np.float32)
    ko = so.vert_mask_orders(kl, km, K)
    assert len(kl) == 12 and not (ko == ko[0, 0]).all(axis=(0, 1)).any()
    assert np.array_equal(so.vert_mask_sequential(kl, km, K), CE["known_vert_mask"])
    assert CE["known_vert_mask"].any() and not CE["known_vert_mask"].all()


def test_fixture_files_stay_small():
    limit = os.path.getsize(os.path.join(GOLDEN, "loss_multipos.npz"))
    for f in os.listdir(GOLDEN):
        if f.startswith("loss_logratio") or f.startswith("loss_skin_ce"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= min(limit, 1 << 20), f


def test_entry_points_are_exported():
    import ctypes as C
    from morig_amd import native
    names = ("morig_logratio_forward", "morig_logratio_backward", "morig_skin_ce_forward", "morig_skin_ce_backward", "morig_ce_probs_forward",
             "morig_ce_probs_backward")
    lib = native.load_library()
    for n in names:
        assert n in native.EXPORTS and hasattr(lib, n)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "morig_hip.h")).read()
    assert f"#define MORIG_LOGRATIO_STRUCT_BYTES {C.sizeof(native.LogRatioArgs)}u" in hdr
    assert lib.morig_abi_version() == 3
    a = native._args(native.LogRatioArgs)
    a.struct_size = 8                                                     # shorter than the struct: refused before anything is read
    assert lib.morig_logratio_forward(C.byref(a), None) == -1
    assert lib.morig_skin_ce_forward(None, 0, None, 0, None, 0, 0, 5, None, None, None, None, None) == -1
    kinds = [lib.morig_prof_name(k).decode() for k in range(64) if lib.morig_prof_name(k)]
    assert {"loss_logratio", "loss_skin_ce"} <= set(kinds)
