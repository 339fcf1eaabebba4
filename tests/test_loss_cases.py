"""tests/loss_cases.py without a device: every generator terminates within its attempts and the ORACLE ALONE confirms the conditions of
every case; the family-maximum float32-oracle deviations (the tolerance inputs of tests/test_loss_differential.py) are computed and
printed; and every case runs through morig_amd.losses on the emulated op layer (tests/skin_loss_emulate.py through
``runtime._test_ops``) and through the very comparison functions the device file uses -- index plumbing, views and comparison code are
proven here before a device sees them."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_oracle as lo
import skin_loss_emulate
import skin_loss_oracle as so
from morig_amd import losses, runtime
from test_gpu_losses import FACTOR, ULP
from test_loss_oracle import CHAMFER_MARGIN
from test_skin_loss_oracle import MIN_DIST


@pytest.fixture()
def ops(monkeypatch):
    o = skin_loss_emulate.SkinLossOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


@pytest.fixture(autouse=True)
def _grad_on():
    """conftest.py runs every test under torch.no_grad(); these need the graph"""
    # the emulated ops are the oracles: the comparison code asserts that a second run gives the same bits, as the device does by construction
    with lc.fixed_order(), torch.enable_grad():
        yield
    losses.check_inputs()


@pytest.mark.parametrize("family,name", lc.ALL)
def test_every_case_is_generated_and_runs_on_the_emulated_ops(ops, family, name):
    c = lc.case(family, name)
    assert 1 <= c["attempts"] <= lc.ATTEMPTS
    lc.check(family, name, "cpu")
    assert ops.calls


def test_tolerance_inputs():
    print("\n" + lc.table())
    for family in lc.FAMILIES:
        for q, d in lc.deviations(family).items():
            assert np.isfinite(d) and d >= 0, (family, q, d)
            assert lc.bounds(family)[q] == max(FACTOR * d, ULP)
    upstreams = lambda family: sorted(lc.case(family, n)["c"] for n in lc.FAMILIES[family][0] if "c" in lc.case(family, n))
    for family in ("infonce", "multipos", "chamfer", "logratio", "frames", "skin_ce"):     # about half of the cases with c = 2.5
        u = upstreams(family)
        assert set(u) == {1.0, 2.5} and abs(u.count(2.5) - u.count(1.0)) <= 1, (family, u)
    for family in lc.FAMILIES:                                                              # one case read through a strided view
        assert any(lc.case(family, n)["view"] for n in lc.FAMILIES[family][0]), family


# ------------------------------------------------------------------------------------------------------------------- infoNCE
def test_infonce_conditions():
    keys = {0: set(), 1: set()}
    rows = {0: set(), 1: set()}
    for name in lc.NCE_CASES:
        c = lc.case("infonce", name)
        assert np.isfinite(c["want"][0]) and c["want"][0] != 0
        norms = c["vtx"].double().norm(dim=1)
        assert float((norms - 1).abs().max()) < 1e-6 and c["vtx"].shape[1] == 64
        skipped = [b for b, p in enumerate(c["pairs"]) if p[2] == 0 and p[3] > 0]
        live_before = [b for b, p in enumerate(c["pairs"]) if p[2] > 0]
        for d, (corr, cb, side) in enumerate(((c["corr_v2p"], c["cb_v2p"], 1), (c["corr_p2v"], c["cb_p2v"], 0))):
            for b, p in enumerate(c["pairs"]):
                r, nk = p[2 + d], p[side]
                if r == 0 or b in skipped:
                    continue
                keys[d].add(nk); rows[d].add(r)
                labels = set(corr[cb == b][:, 1].tolist())
                assert set(lc.nce_forced_labels(nk)[:r]) <= labels and max(labels) < nk
                if r >= 4:                                                                  # both lane halves of the last tile, 0 and nk - 1
                    base = 32 * ((nk - 1) // 32)
                    last = [k - base for k in labels if k >= base]
                    assert {0, nk - 1} <= labels and any(o % 8 < 4 for o in last) and (nk - base <= 4 or any(o % 8 >= 4 for o in last))
        if name.startswith("edges"):
            assert skipped == [lc.NCE_SKIPPED] and min(live_before) < lc.NCE_SKIPPED < max(live_before)
            assert c["pairs"][lc.NCE_NO_P2V][3] == 0 and c["pairs"][lc.NCE_NO_P2V][2] > 0
            shared = [b for b, p in enumerate(c["pairs"]) if p[4]]
            assert shared and all(len(set(c["corr_v2p"][c["cb_v2p"] == b][:, 0].tolist())) == 1 for b in shared)
            assert int(c["vtx_batch"][0]) == 0 and len(c["pairs"]) == 10                    # ragged: every later pair at a non-zero offset
    assert keys[0] == set(lc.NCE_KEYS) == keys[1] and rows[0] | rows[1] == set(lc.NCE_ROWS)
    assert {1, 4} <= keys[0] and {1, 4} <= keys[1]                                          # the upper lane half of the only tile is empty
    assert {t for _, t, _, _ in lc.NCE_CASES.values()} == {0.07, 0.01}


# ------------------------------------------------------------------------------------------------------------------- multi-positive
def test_multipos_conditions():
    seen = dict(S=set(), D=set(), P=set(), N=set(), B=set())
    for name in lc.MP_CASES:
        c = lc.case("multipos", name)
        S, D, P, N = c["S"], c["feat"].shape[1], c["pos_ids"].shape[2], c["neg_ids"].shape[2]
        for k, v in zip("SDPNB", (S, D, P, N, c["B"])):
            seen[k].add(v)
        assert lc.mp_products(c) <= lc.MP_PRODUCT_LIMIT and np.isfinite(c["want"][0]) and c["want"][0] != 0
        for b, n in enumerate(c["sizes"]):
            ids = c["sample_ids"][b]
            assert len(torch.unique(ids)) == S and 0 <= int(ids.min()) and int(ids.max()) < n
            assert S < 3 or bool((ids[1:] < ids[:-1]).any())                               # not monotone
        if N >= 2:
            assert lc.mp_shared_and_repeated(c)
        assert S > 1
    assert seen == dict(S={2, 3, 63, 64, 65, 129, 257}, D={4, 8, 60, 64, 124, 128}, P={1, 2, 63, 64}, N={1, 63, 64, 65, 255, 256}, B={1, 3})
    assert any(len(set(lc.case("multipos", n)["sizes"])) == 3 for n in lc.MP_CASES)        # ragged meshes, non-zero offsets


def test_multipos_without_a_negative_is_exactly_zero(ops):
    c = lc.mp_no_negative_case()
    loss, grad = lc.mp_run(c, "cpu")
    assert loss == 0 and (grad == 0).all()


# ------------------------------------------------------------------------------------------------------------------- chamfer
def test_chamfer_conditions():
    meshes = set()
    for name in lc.CH_CASES:
        c = lc.case("chamfer", name)
        meshes |= set(c["meshes"])
        for b in range(c["B"]):
            p, q = c["p"][c["batch"] == b], c["q"][c["q_batch"] == b]
            assert lo.chamfer_margin(p.double(), q.double()) >= CHAMFER_MARGIN
            if b in lc.CH_LARGE.get(name, ()):
                carried = lc.ch_slots_carry(p, q)
                print(f"\nchamfer {name} mesh {b}: joints of slots 1, 2, 3 that are nearest to vertices of two vertex blocks: {carried}")
                assert min(carried) >= 1
    assert meshes == {(1, 1), (1, 2), (2, 1), (255, 255), (256, 256), (257, 257), (513, 1024), (1025, 1023), (1, 1024)}
    assert any(c["B"] == 4 and len(set(c["meshes"])) == 4 for c in (lc.case("chamfer", n) for n in lc.CH_CASES))
    c = lc.case("chamfer", "coincide_view")
    v, j = lc.CH_COINCIDE
    assert j >= 256 and torch.equal(c["p"][v], c["q"][j])
    d = (c["p"][:, None, :].double() - c["q"][None, :, :].double()).pow(2).sum(-1).sqrt()
    assert int(d[v].argmin()) == j and int(d[:, j].argmin()) == v and float(d[v, j]) == 0


def test_chamfer_tie_is_judged_by_first_occurrence():
    c = lc.case("chamfer", "tie")
    lo_j, hi_j = lc.CH_TIE
    p, q = c["p"].numpy().astype(np.float64), c["q"].numpy().astype(np.float64)
    assert lo_j < 256 <= hi_j and np.array_equal(q[lo_j], q[hi_j])
    d = np.sqrt(((p[:, None, :] - q[None, :, :]) ** 2).sum(-1))
    a1 = d.argmin(axis=1)
    assert (a1 == lo_j).any() and not (a1 == hi_j).any() and np.array_equal(d[:, lo_j], d[:, hi_j])
    # away from the tie the numpy statement IS the torch oracle
    rest = np.delete(np.arange(len(q)), hi_j)
    z = lambda n: torch.zeros(n, dtype=torch.long)
    want = lo.chamfer(torch.from_numpy(p), z(len(p)), torch.from_numpy(q[rest]), z(len(rest)), 1)
    got = lc.chamfer_first_occurrence(p, q[rest])
    assert abs(got[0] - float(want[0])) <= 1e-14 and np.abs(got[1] - want[1].numpy()).max() <= 1e-15 and np.abs(got[2] - want[2].numpy()).max() <= 1e-15


def test_chamfer_swap_through_the_reference_signature(ops):
    c = lc.case("chamfer", "ragged_b")
    loss, gp, gq = lc.ch_swapped_run(c, "cpu")
    s, sq = c["batch"] == 2, c["q_batch"] == 2
    z = lambda n: torch.zeros(n, dtype=torch.long)
    want = [t.numpy() for t in lo.chamfer(c["p"][s].double(), z(int(s.sum())), c["q"][sq].double(), z(int(sq.sum())), 1)]
    lc.ch_compare("swapped (1023 | 1025)", c, (loss, gp, gq), lc.bounds("chamfer"), want=want)


# ------------------------------------------------------------------------------------------------------------------- log-ratio
def test_log_ratio_conditions():
    seen = dict(S=set(), DW=set(), B=set())
    for family, names in (("logratio", lc.LR_CASES), ("frames", lc.FRAME_CASES)):
        for name in names:
            c = lc.case(family, name)
            sets = [c["feat"]] if family == "logratio" else [c["motion_all"][:, t] for t in range(c["T"])] + [c["motion_aggr"]]
            samples = c["samples"].reshape(len(sets), c["B"], c["S"])
            for k, f in enumerate(sets):
                assert lc.lr_min_dist(f, c["batch"], samples[k], c["B"]) >= MIN_DIST
            assert lc.lr_min_dist(c["gt"], c["batch"], samples, c["B"]) >= MIN_DIST
            assert all(c["S"] <= n <= c["S"] + 70 for n in c["sizes"])
            if family == "logratio":
                seen["S"].add(c["S"]); seen["DW"].add((c["feat"].shape[1], c["gt"].shape[1])); seen["B"].add(c["B"])
    assert seen == dict(S={3, 4, 16, 17, 23, 24, 50, 63, 64}, DW={(4, 4), (4, 128), (128, 4), (124, 60), (128, 128), (32, 48)}, B={1, 2, 4})
    assert any(c["S"] in c["sizes"] and c["B"] > 1 for c in (lc.case("logratio", n) for n in lc.LR_CASES))   # every row of a mesh sampled
    assert {c["T"] for c in (lc.case("frames", n) for n in lc.FRAME_CASES)} == {1, 3}
    pairs = lambda S: S * (S - 1) // 2
    assert pairs(23) == 253 <= 256 < pairs(24) == 276 and 16 * 16 == 256 < 17 * 17        # one / two rounds; S * S at and over 256


# ------------------------------------------------------------------------------------------------------------------- the two cross-entropies
def test_skin_ce_conditions():
    Ks, rows = set(), set()
    for name in lc.CE_CASES:
        c = lc.case("skin_ce", name)
        K, n = c["K"], len(c["x"])
        Ks.add(K); rows.add(n)
        assert c["label"].shape == c["mask"].shape == (n, K + 2) and c["x"].shape == (n, K)
        label, mask = c["label"].numpy()[:, :K], c["mask"].numpy()[:, :K]
        nz = label[label != 0]
        assert nz.min() >= lc.CE_MIN_LABEL and nz.max() <= 1.0
        vm = so.vert_mask_sequential(c["label"].numpy(), c["mask"].numpy().astype(np.float32), K)
        assert np.array_equal(vm, c["vert_mask"]) and vm.any()
        if n > 1:
            assert set((label != 0).sum(1).tolist()) == set(range(K + 1)) and (mask.sum(1) == 0).any()
            nonempty = (label * mask != 0).any(axis=1)
            assert K < 2 or (vm[nonempty].any() and (~vm[nonempty]).any())
    assert Ks == set(range(1, 9)) and rows == {1, 255, 256, 257, 513}


def test_skin_ce_all_masked_is_nan(ops):
    c = lc.case("skin_ce", "k5_n513")
    assert torch.isnan(losses.skin_ce_loss(c["x"], c["label"], torch.zeros_like(c["mask"]), nearest_bone=c["K"]))


def test_ce_probs_conditions():
    combos = {(K, n) for K, n, _, _ in lc.CEP_CASES.values()}
    assert combos == {(K, n) for K in (1, 2, 127, 128) for n in (1, 256, 257)}
    assert {kind for _, _, kind, _ in lc.CEP_CASES.values()} == set(lc.CEP_WEIGHTS)
    assert [r for r, _ in lc.CEP_REDUCTIONS] == ["none", "mean", "sum"]
    for name in lc.CEP_CASES:
        c = lc.case("ce_probs", name)
        K, n, kind, _ = lc.CEP_CASES[name]
        assert (c["weight"] is None) == (kind == "none")
        assert n > 1 or K == 1 or float(torch.softmax(c["x"].double(), dim=1).max()) <= lc.CEP_MAX_PROB
        assert c["weight"] is None or tuple(c["weight"].shape) == dict(K=(K,), N1=(n, 1), NK=(n, K))[kind]
