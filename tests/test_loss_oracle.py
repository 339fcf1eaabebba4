"""tests/loss_oracle.py (float64, closed-form gradients) against the reference's recorded float32 results (tests/golden/loss_*.npz,
tools/make_loss_golden.py), within the deviations the generator stored; the conditions the fixtures were generated under; the C ABI of
the new entry points."""
import json
import os

import numpy as np
import pytest
import torch

import loss_oracle as lo
from conftest import GOLDEN

CHAMFER_MARGIN, SIM_MARGIN, N_SAMPLE = 1e-5, 1e-4, 512
SLACK = 1.0 + 1e-6                                   # the stored deviations were measured with these very functions


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


def ids(a):
    return torch.from_numpy(a.astype(np.int64))


NCE_META, NCE_IN = load("loss_nce_inputs")
MP_META, MP = load("loss_multipos")
CH_META, CH = load("loss_chamfer")


def nce_tensors(scale=1.0, dtype=torch.float64):
    t = {k: ids(v) for k, v in NCE_IN.items() if v.dtype == np.uint16}
    vtx = (torch.from_numpy(NCE_IN["vtx"]) * np.float32(scale)).to(dtype)
    pts = (torch.from_numpy(NCE_IN["pts"]) * np.float32(scale)).to(dtype)
    return vtx, pts, t


def nce_args(vtx, pts, t):
    return (vtx, pts, t["corr_v2p"], t["corr_p2v"], t["vtx_batch"], t["pts_batch"], t["corr_v2p_batch"], t["corr_p2v_batch"])


def rel_max(a, b):
    scale = np.abs(b).max()
    return np.abs(a - b).max() / scale if scale > 0 else np.abs(a).max()


@pytest.mark.parametrize("case", list(NCE_META["cases"]))
def test_infonce_oracle_against_the_reference(case):
    meta, ref = load(f"loss_nce_{case}")
    vtx, pts, t = nce_tensors(meta["scale"])
    loss, gv, gp = lo.infonce(*nce_args(vtx, pts, t), meta["tau"], len(NCE_META["pairs"]))
    dev = meta["deviations"]
    assert abs(float(ref["loss"]) - float(loss)) / abs(float(loss)) <= dev["dev_loss"] * SLACK
    assert rel_max(ref["grad_vtx"].astype(np.float64), gv.numpy()) <= dev["dev_grad_vtx"] * SLACK
    assert rel_max(ref["grad_pts"].astype(np.float64), gp.numpy()) <= dev["dev_grad_pts"] * SLACK


def test_closed_form_gradients_equal_autograd():
    """the oracle's gradients are written out by hand: float64 autograd of its own forward formulas agrees to rounding"""
    with torch.enable_grad():
        vtx, pts, t = nce_tensors()
        vtx.requires_grad_(True); pts.requires_grad_(True)
        lo.infonce_loss(*nce_args(vtx, pts, t), 0.07, 5).backward()
        _, gv, gp = lo.infonce(*nce_args(vtx.detach(), pts.detach(), t), 0.07, 5)
        assert (vtx.grad - gv).abs().max() <= 1e-13 and (pts.grad - gp).abs().max() <= 1e-13
        f = torch.from_numpy(MP["feat"]).double().requires_grad_(True)
        a = (ids(MP["batch"]), ids(MP["sample_ids"]), ids(MP["pos_ids"]), ids(MP["neg_ids"]), 2)
        lo.multipos_loss(f, *a).backward()
        assert (f.grad - lo.multipos(f.detach(), *a)[1]).abs().max() <= 1e-13
        p = torch.from_numpy(CH["n65_m33_p"]).double().requires_grad_(True)
        q = torch.from_numpy(CH["n65_m33_q"]).double().requires_grad_(True)
        zb = lambda x: torch.zeros(len(x), dtype=torch.long)
        lo.chamfer_loss(p, zb(p), q, zb(q), 1).backward()
        _, gp_, gq_ = lo.chamfer(p.detach(), zb(p), q.detach(), zb(q), 1)
        assert (p.grad - gp_).abs().max() <= 1e-13 and (q.grad - gq_).abs().max() <= 1e-13


def test_infonce_quirks_of_the_reference():
    """pair 1 has no v2p rows: its 17 p2v rows add nothing and its features get no gradient; pair 2 has no p2v rows: its v2p term counts"""
    vtx, pts, t = nce_tensors()
    loss, gv, gp = lo.infonce(*nce_args(vtx, pts, t), 0.07, 5)
    assert (gv[t["vtx_batch"] == 1] == 0).all() and (gp[t["pts_batch"] == 1] == 0).all()
    assert gv[t["vtx_batch"] == 2].abs().max() > 0
    assert (gv[t["vtx_batch"] == 3] == 0).all() and (gp[t["pts_batch"] == 3] == 0).all()          # the (1, 1, 1, 1) pair
    keep = t["corr_p2v_batch"] != 1
    t2 = dict(t, corr_p2v=t["corr_p2v"][keep], corr_p2v_batch=t["corr_p2v_batch"][keep])
    assert float(lo.infonce(*nce_args(vtx, pts, t2), 0.07, 5)[0]) == float(loss)
    pairs = NCE_META["pairs"]
    assert len(torch.unique(t["corr_v2p"][t["corr_v2p_batch"] == 4][:, 0])) < pairs[4][2]           # duplicate anchors
    assert len(torch.unique(t["corr_v2p"][t["corr_v2p_batch"] == 4][:, 1])) < pairs[4][2]           # duplicate labels


def test_multipos_oracle_against_the_reference():
    f = torch.from_numpy(MP["feat"]).double()
    loss, g = lo.multipos(f, ids(MP["batch"]), ids(MP["sample_ids"]), ids(MP["pos_ids"]), ids(MP["neg_ids"]), 2)
    dev = MP_META["deviations"]
    assert abs(float(MP["loss"]) - float(loss)) / abs(float(loss)) <= dev["dev_loss"] * SLACK
    assert rel_max(MP["grad"].astype(np.float64), g.numpy()) <= dev["dev_grad"] * SLACK
    sampled = np.zeros(len(f), dtype=bool)
    for b in range(2):
        sampled[np.nonzero(MP["batch"] == b)[0][MP["sample_ids"][b]]] = True
    assert (~sampled).sum() == 700 - 512 and (MP["grad"][~sampled] == 0).all() and (g.numpy()[~sampled] == 0).all()


def test_multipos_fixture_conditions():
    for k in ("sample_ids", "pos_ids", "neg_ids", "batch"):
        assert MP[k].dtype == np.uint16
    for b in range(2):
        sel = MP["batch"] == b
        assert sel.sum() >= N_SAMPLE
        sid = MP["sample_ids"][b]
        assert len(np.unique(sid)) == N_SAMPLE and sid.max() < sel.sum()
        sim = lo.gt_similarity(torch.from_numpy(MP["skin"][sel][sid]).double()).numpy()
        assert np.abs(sim - 0.9).min() >= SIM_MARGIN
        assert ((sim <= 0.9).sum(1) > 0).all()
        rows = np.arange(N_SAMPLE)[:, None]
        assert (sim[rows, MP["pos_ids"][b]] > 0.9).all() and (sim[rows, MP["neg_ids"][b]] <= 0.9).all()
    own = int(np.nonzero(MP["sample_ids"][0] == MP_META["lone_vertex"])[0][0])
    assert (MP["pos_ids"][0, own] == own).all()                          # the vertex nobody shares a skin row with: its positives are itself


@pytest.mark.parametrize("name", CH_META["batch"] + ["coincide"])
def test_chamfer_oracle_against_the_reference(name):
    p, q = torch.from_numpy(CH[f"{name}_p"]).double(), torch.from_numpy(CH[f"{name}_q"]).double()
    assert lo.chamfer_margin(p, q) >= CHAMFER_MARGIN
    zb = lambda x: torch.zeros(len(x), dtype=torch.long)
    loss, gp, gq = lo.chamfer(p, zb(p), q, zb(q), 1)
    dev = CH_META["deviations"][name]
    assert abs(float(CH[f"{name}_loss"]) - float(loss)) / abs(float(loss)) <= dev["dev_loss"] * SLACK
    assert rel_max(CH[f"{name}_grad_p"].astype(np.float64), gp.numpy()) <= dev["dev_grad_p"] * SLACK
    assert rel_max(CH[f"{name}_grad_q"].astype(np.float64), gq.numpy()) <= dev["dev_grad_q"] * SLACK


def test_coincident_joint_has_finite_results_and_no_gradient_through_the_zero_distance():
    c = CH_META["coincide"]
    p, q = CH["coincide_p"], CH["coincide_q"]
    assert (p[c["vertex"]] == q[c["joint"]]).all()
    assert np.isfinite(CH["coincide_grad_p"]).all() and np.isfinite(CH["coincide_grad_q"]).all() and np.isfinite(CH["coincide_loss"])
    assert (CH["coincide_grad_p"][c["vertex"]] == 0).all()                # both of its terms run through the zero distance
    zb = lambda x: torch.zeros(len(x), dtype=torch.long)
    _, gp, gq = lo.chamfer(torch.from_numpy(p).double(), zb(p), torch.from_numpy(q).double(), zb(q), 1)
    assert (gp[c["vertex"]] == 0).all() and torch.isfinite(gp).all() and torch.isfinite(gq).all()


def test_fixture_files_stay_small():
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("loss_"))
    for f in os.listdir(GOLDEN):
        if f.startswith("loss_"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= min(largest, 1 << 20), f


def test_entry_points_are_exported():
    from morig_amd import native
    names = ("morig_loss_segment_ptr", "morig_infonce_forward", "morig_infonce_backward", "morig_multipos_forward", "morig_multipos_backward",
             "morig_chamfer_forward", "morig_chamfer_backward")
    lib = native.load_library()
    for n in names:
        assert n in native.EXPORTS and hasattr(lib, n)
    import ctypes as C
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "morig_hip.h")).read()
    assert f"#define MORIG_NCE_STRUCT_BYTES {C.sizeof(native.NceArgs)}u" in hdr
    a = native._args(native.NceArgs)
    a.struct_size = 8                                                     # shorter than the struct: refused before anything is read
    assert lib.morig_infonce_forward(C.byref(a), None) == -1
    kinds = [lib.morig_prof_name(k).decode() for k in range(64) if lib.morig_prof_name(k)]
    assert {"loss_infonce_fwd", "loss_infonce_bwd", "loss_multipos", "loss_chamfer"} <= set(kinds)
