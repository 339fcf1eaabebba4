"""morig_amd/losses.py on an emulated op layer (tests/loss_emulate.py through ``runtime._test_ops``): autograd wiring, the two
empty-direction quirks of infoNCE, num_graphs handling, what is refused, and the properties of the batched sampler."""
import numpy as np
import pytest
import torch

import loss_emulate
import loss_oracle as lo
from morig_amd import losses, runtime
from test_loss_oracle import CH, CH_META, MP, ids, nce_args, nce_tensors


@pytest.fixture()
def ops(monkeypatch):
    o = loss_emulate.LossOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


def nce_f32():
    vtx, pts, t = nce_tensors(dtype=torch.float32)
    return vtx, pts, t


def test_infonce_autograd_wiring(ops):
    vtx, pts, t = nce_f32()
    with torch.enable_grad():
        vtx.requires_grad_(True); pts.requires_grad_(True)
        loss = losses.infoNCE(*nce_args(vtx, pts, t), 0.07, num_graphs=5)
        (3.0 * loss).backward()
    want, gv, gp = lo.infonce(*nce_args(vtx.detach().double(), pts.detach().double(), t), 0.07, 5)
    assert loss.shape == () and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert (vtx.grad.double() - 3.0 * gv).abs().max() <= 1e-5 * gv.abs().max() * 3
    assert (pts.grad.double() - 3.0 * gp).abs().max() <= 1e-5 * gp.abs().max() * 3
    assert ops.calls == ["infonce_forward", "infonce_backward"]


def test_infonce_empty_directions(ops):
    """no v2p rows: the pair's p2v rows are skipped too; no p2v rows: the v2p term alone"""
    vtx, pts, t = nce_f32()
    full = float(losses.infoNCE(*nce_args(vtx, pts, t), 0.07, num_graphs=5))
    keep = t["corr_p2v_batch"] != 1
    t2 = dict(t, corr_p2v=t["corr_p2v"][keep], corr_p2v_batch=t["corr_p2v_batch"][keep])
    assert float(losses.infoNCE(*nce_args(vtx, pts, t2), 0.07, num_graphs=5)) == full
    cv, cp = t["corr_v2p"][t["corr_v2p_batch"] == 2], t["corr_p2v"][t["corr_p2v_batch"] == 2]
    sel_v, sel_p = t["vtx_batch"] == 2, t["pts_batch"] == 2
    zeros = lambda n: torch.zeros(n, dtype=torch.long)
    alone = losses.infoNCE(vtx[sel_v], pts[sel_p], cv, cp, zeros(int(sel_v.sum())), zeros(int(sel_p.sum())), zeros(len(cv)), zeros(len(cp)), 0.07,
                           num_graphs=1)
    only2 = dict(corr_v2p=cv, corr_p2v=cp)
    c = only2["corr_v2p"]
    logits = vtx[sel_v][c[:, 0]].double() @ pts[sel_p].double().T / 0.07
    want = (torch.logsumexp(logits, 1) - logits[torch.arange(len(c)), c[:, 1]]).mean()
    assert only2["corr_p2v"].shape[0] == 0 and abs(float(alone) - float(want)) <= 1e-5 * float(want)


def test_num_graphs(ops):
    vtx, pts, t = nce_f32()
    a = float(losses.infoNCE(*nce_args(vtx, pts, t), 0.07))                        # read from the batch vector
    b = float(losses.infoNCE(*nce_args(vtx, pts, t), 0.07, num_graphs=5))
    c = float(losses.infoNCE(*nce_args(vtx, pts, t), 0.07, num_graphs=10))       # five empty pairs more: the divisor doubles
    assert a == b and abs(c - b / 2) <= 1e-6 * b
    with pytest.raises(losses.LossInputError, match="outside"):
        losses.infoNCE(*nce_args(vtx, pts, t), 0.07, num_graphs=4)
    p, q = torch.from_numpy(CH["n65_m33_p"]), torch.from_numpy(CH["n65_m33_q"])
    zb = lambda x: torch.zeros(len(x), dtype=torch.long)
    one = float(losses.chamfer_batched(p, zb(p), q, zb(q)))
    assert one == float(losses.chamfer_batched(p, zb(p), q, zb(q), num_graphs=1))
    assert abs(one - float(CH["n65_m33_loss"])) <= 1e-6


def test_refusals(ops):
    vtx, pts, t = nce_f32()
    with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*width 64"):
        losses.infoNCE(vtx[:, :32], pts[:, :32], *nce_args(vtx, pts, t)[2:], 0.07, num_graphs=5)
    bad = dict(t, vtx_batch=t["vtx_batch"].flip(0))
    with pytest.raises(losses.LossInputError, match="not sorted"):
        losses.infoNCE(*nce_args(vtx, pts, bad), 0.07, num_graphs=5)
    corr = t["corr_v2p"].clone()
    corr[3, 1] = 200                                                          # pair 0 has 200 points: labels 0..199
    with pytest.raises(losses.LossInputError, match="index"):
        losses.infoNCE(*nce_args(vtx, pts, dict(t, corr_v2p=corr)), 0.07, num_graphs=5)
    corr[3, 1] = -1
    with pytest.raises(losses.LossInputError, match="index"):
        losses.infoNCE(*nce_args(vtx, pts, dict(t, corr_v2p=corr)), 0.07, num_graphs=5)
    f = torch.from_numpy(MP["feat"])
    samples = (ids(MP["sample_ids"]), ids(MP["pos_ids"]), ids(MP["neg_ids"]))
    with pytest.raises(losses.LossInputError, match="multiple of 4 up to 128"):
        losses.multi_pos_infoNCE(f[:, :30], None, ids(MP["batch"]), samples=samples, num_graphs=2)
    with pytest.raises(losses.LossInputError, match="multiple of 4 up to 128"):
        losses.multi_pos_infoNCE(torch.zeros(len(f), 132), None, ids(MP["batch"]), samples=samples, num_graphs=2)
    sid = samples[0].clone()
    sid[0, 0] = 600                                                           # mesh 0 has 512 vertices
    with pytest.raises(losses.LossInputError, match="index"):
        losses.multi_pos_infoNCE(f, None, ids(MP["batch"]), samples=(sid,) + samples[1:], num_graphs=2)
    with pytest.raises(losses.LossInputError, match="dimension 3"):
        losses.chamfer_distance_with_average(torch.zeros(1, 5, 2), torch.zeros(1, 4, 2))
    with pytest.raises(losses.LossInputError, match="at most 1024"):
        losses.chamfer_distance_with_average(torch.zeros(1, 1025, 3), torch.zeros(1, 1025, 3))
    p, q = torch.rand(10, 3), torch.rand(1030, 3)
    with pytest.raises(losses.LossInputError, match="1024 joints"):
        losses.chamfer_batched(p, torch.zeros(10, dtype=torch.long), q, torch.zeros(1030, dtype=torch.long), num_graphs=1)
    assert float(losses.chamfer_distance_with_average(p[None], q[None])) > 0      # symmetric: the small set goes to LDS


def test_multipos_autograd_wiring_and_strided_view(ops):
    f = torch.from_numpy(MP["feat"])
    samples = (ids(MP["sample_ids"]), ids(MP["pos_ids"]), ids(MP["neg_ids"]))
    want, g = lo.multipos(f.double(), ids(MP["batch"]), *samples, 2)
    with torch.enable_grad():
        stack = torch.randn(len(f), 3, 32)
        stack[:, 1, :] = f
        stack.requires_grad_(True)
        loss = losses.multi_pos_infoNCE(stack[:, 1, :], None, ids(MP["batch"]), samples=samples, num_graphs=2)
        loss.backward()
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert (stack.grad[:, 1, :].double() - g).abs().max() <= 1e-5 * g.abs().max()
    assert (stack.grad[:, 0, :] == 0).all() and (stack.grad[:, 2, :] == 0).all()
    sampled = np.zeros(len(f), dtype=bool)
    for b in range(2):
        sampled[np.nonzero(MP["batch"] == b)[0][MP["sample_ids"][b]]] = True
    assert (stack.grad[~torch.from_numpy(sampled)] == 0).all()


def test_chamfer_autograd_wiring(ops):
    names = CH_META["batch"]
    p = torch.cat([torch.from_numpy(CH[f"{n}_p"]) for n in names])
    q = torch.cat([torch.from_numpy(CH[f"{n}_q"]) for n in names])
    pb = torch.cat([torch.full((len(CH[f"{n}_p"]),), i) for i, n in enumerate(names)])
    qb = torch.cat([torch.full((len(CH[f"{n}_q"]),), i) for i, n in enumerate(names)])
    with torch.enable_grad():
        p.requires_grad_(True); q.requires_grad_(True)
        loss = losses.chamfer_batched(p, pb, q, qb, num_graphs=len(names))
        loss.backward()
    want = np.mean([float(CH[f"{n}_loss"]) for n in names])
    assert abs(float(loss) - want) <= 1e-6
    gp = np.concatenate([CH[f"{n}_grad_p"] for n in names]) / len(names)
    assert np.abs(p.grad.numpy() - gp).max() <= 1e-6 * np.abs(gp).max() * 10


def test_sampler_properties(ops):
    g = torch.Generator().manual_seed(3)
    skin, batch = torch.from_numpy(MP["skin"]), ids(MP["batch"])
    sid, pos, neg = losses.draw_multi_pos_samples(skin, batch, generator=g, num_graphs=2)
    assert sid.shape == (2, 512) and pos.shape == (2, 512, 10) and neg.shape == (2, 512, 200)
    for b, n in enumerate((512, 700)):
        assert sid[b].min() >= 0 and sid[b].max() < n and len(torch.unique(sid[b])) == 512
        sim = lo.gt_similarity(skin[batch == b][sid[b]].double())
        rows = torch.arange(512)[:, None]
        assert pos[b].min() >= 0 and pos[b].max() < 512 and neg[b].min() >= 0 and neg[b].max() < 512
        assert (sim[rows, pos[b]] > 0.9).all() and (sim[rows, neg[b]] <= 0.9).all()
    assert len(torch.unique(sid[1])) == 512 and not torch.equal(sid[1], torch.arange(512))      # a draw, not the first 512
    sid2, _, _ = losses.draw_multi_pos_samples(skin, batch, generator=torch.Generator().manual_seed(3), num_graphs=2)
    assert torch.equal(sid, sid2)
    with pytest.raises(losses.LossInputError, match="fewer than 512"):
        losses.draw_multi_pos_samples(skin[1:], batch[1:], num_graphs=2)          # mesh 0 is left with 511 vertices
    same = torch.zeros(600, 6)
    same[:, 0] = 1.0
    with pytest.raises(losses.LossInputError, match="no negative"):
        losses.draw_multi_pos_samples(same, torch.zeros(600, dtype=torch.long), num_graphs=1)
    loss = losses.multi_pos_infoNCE(torch.from_numpy(MP["feat"]), skin, batch, num_graphs=2)     # samples=None draws them
    assert torch.isfinite(loss)
