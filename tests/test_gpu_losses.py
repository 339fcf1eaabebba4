"""csrc/losses.hip and morig_amd/losses.py on the device, against the reference's recorded float32 results (tests/golden/loss_*.npz).

Bounds are measured, not chosen: per case the generator stored the deviation of the reference's float32 result from the float64 oracle
(relative for a loss, relative to max |grad| for a gradient); the device has to stay within TEN times that of the reference's result
(the convention of tests/test_gpu_tracking.py), and a bound is never tighter than one float32 ulp (2^-23) of the quantity's largest
magnitude. Every figure is printed before it is asserted (run with -s); the stored deviations are tabulated in DESIGN.md section 14.
"""
import numpy as np
import pytest
import torch

import loss_oracle as lo
from morig_amd import losses, models, synth
from test_loss_oracle import CH, CH_META, MP, MP_META, NCE_IN, NCE_META, ids, load, nce_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, ULP = 10.0, 2.0 ** -23
_cache = {}


@pytest.fixture(autouse=True)
def _grad_on():
    """conftest.py runs every test under torch.no_grad(); these need the graph"""
    with torch.enable_grad():
        yield
    losses.check_inputs()                                  # no launch of the test found its inputs wrong


def bound(dev):
    return max(FACTOR * dev, ULP)


def rel_max(got, want):
    scale = np.abs(want).max()
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / scale) if scale > 0 else float(np.abs(got).max())


def report(what, got, b):
    print(f"\n{what}: {got:.3e} (bound {b:.3e})")
    return got <= b


# ------------------------------------------------------------------------------------------------------------------- infoNCE
def nce_device(scale, sel=None):
    """the fixture's batch (or pair ``sel`` alone, as a batch of one) on the device -> (vtx, pts, index tensors)"""
    t = {k: ids(v) for k, v in NCE_IN.items() if v.dtype == np.uint16}
    vtx, pts = torch.from_numpy(NCE_IN["vtx"]) * np.float32(scale), torch.from_numpy(NCE_IN["pts"]) * np.float32(scale)
    if sel is not None:
        keep = {k: t[k if k.endswith("batch") else k + "_batch"] == sel for k in t}
        vtx, pts = vtx[keep["vtx_batch"]], pts[keep["pts_batch"]]
        t = {k: (v[keep[k]] * 0 if k.endswith("batch") else v[keep[k]]) for k, v in t.items()}
    return vtx.to(DEV).requires_grad_(True), pts.to(DEV).requires_grad_(True), {k: v.to(DEV) for k, v in t.items()}


def nce_run(case, sel=None):
    key = (case, sel)
    if key not in _cache:
        par = NCE_META["cases"][case]
        vtx, pts, t = nce_device(par["scale"], sel)
        loss = losses.infoNCE(*nce_args(vtx, pts, t), par["tau"], num_graphs=5 if sel is None else 1)
        loss.backward()
        _cache[key] = (float(loss), vtx.grad.cpu().numpy(), pts.grad.cpu().numpy())
    return _cache[key]


@pytest.mark.parametrize("case", list(NCE_META["cases"]))
def test_infonce_against_the_reference(case):
    """five pairs in one launch -- an ordinary one, one without v2p rows (both terms skipped), one without p2v rows, (1, 1, 1, 1), and
    300 rows on 129 vertices with repeating labels -- at tau 0.07, at tau 0.01, and with rows of norm 3 (logits beyond +-100: without the
    running maximum exp overflows)"""
    meta, ref = load(f"loss_nce_{case}")
    loss, gv, gp = nce_run(case)
    dev = meta["deviations"]
    ok = report(f"infoNCE {case} loss rel", abs(loss - float(ref["loss"])) / abs(float(ref["loss"])), bound(dev["dev_loss"]))
    ok &= report(f"infoNCE {case} grad_vtx rel", rel_max(gv, ref["grad_vtx"]), bound(dev["dev_grad_vtx"]))
    ok &= report(f"infoNCE {case} grad_pts rel", rel_max(gp, ref["grad_pts"]), bound(dev["dev_grad_pts"]))
    assert ok
    vb, pb = NCE_IN["vtx_batch"], NCE_IN["pts_batch"]
    for pair in (1, 3):                                    # the skipped pair and the (1, 1, 1, 1) pair: exactly zero
        assert (gv[vb == pair] == 0).all() and (gp[pb == pair] == 0).all()
    assert np.isfinite(gv).all() and np.isfinite(gp).all()


def test_infonce_two_runs_are_bit_identical():
    first = nce_run("tau007")
    par = NCE_META["cases"]["tau007"]
    vtx, pts, t = nce_device(par["scale"])
    loss = losses.infoNCE(*nce_args(vtx, pts, t), par["tau"], num_graphs=5)
    loss.backward()
    assert float(loss) == first[0]
    assert np.array_equal(vtx.grad.cpu().numpy(), first[1]) and np.array_equal(pts.grad.cpu().numpy(), first[2])


def test_infonce_each_pair_alone_is_its_share_of_the_batch():
    meta, _ = load("loss_nce_tau007")
    dev = meta["deviations"]
    loss, gv, gp = nce_run("tau007")
    alone = [nce_run("tau007", b) for b in range(5)]
    assert alone[1][0] == 0.0 and alone[3][0] == 0.0       # no v2p rows; one key: the loss is exactly 0
    assert (alone[3][1] == 0).all() and (alone[3][2] == 0).all()
    ok = report("infoNCE sum of pairs alone / 5 against the batch, rel", abs(sum(a[0] for a in alone) / 5 - loss) / loss, bound(dev["dev_loss"]))
    gv_alone, gp_alone = np.concatenate([a[1] for a in alone]) / 5, np.concatenate([a[2] for a in alone]) / 5
    ok &= report("infoNCE grad_vtx alone / 5 against the batch, rel", rel_max(gv_alone, gv), bound(dev["dev_grad_vtx"]))
    ok &= report("infoNCE grad_pts alone / 5 against the batch, rel", rel_max(gp_alone, gp), bound(dev["dev_grad_pts"]))
    assert ok


def test_infonce_allocates_nothing_of_the_size_of_the_logits():
    """(4096, 8192, 2048, 2048): forward and backward grow the peak by less than ONE rows x keys matrix"""
    g = torch.Generator().manual_seed(0)
    nv, npt, r = 4096, 8192, 2048
    vtx = torch.nn.functional.normalize(torch.randn(nv, 64, generator=g), dim=1).to(DEV).requires_grad_(True)
    pts = torch.nn.functional.normalize(torch.randn(npt, 64, generator=g), dim=1).to(DEV).requires_grad_(True)
    cv = torch.stack([torch.randint(0, nv, (r,), generator=g), torch.randint(0, npt, (r,), generator=g)], 1).to(DEV)
    cp = torch.stack([torch.randint(0, npt, (r,), generator=g), torch.randint(0, nv, (r,), generator=g)], 1).to(DEV)
    z = lambda n: torch.zeros(n, dtype=torch.long, device=DEV)
    args = (vtx, pts, cv, cp, z(nv), z(npt), z(r), z(r))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    loss = losses.infoNCE(*args, 0.07, num_graphs=1)
    loss.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"\ninfoNCE (4096, 8192, 2048, 2048): peak grew by {grown} bytes (one logits matrix: {r * npt * 4})")
    assert grown < r * npt * 4
    assert np.isfinite(float(loss)) and 0.5 * np.log(nv) < float(loss)


def test_wrong_indices_are_reported_not_followed():
    vtx, pts, t = nce_device(1.0)
    corr = t["corr_v2p"].clone()
    corr[3, 1] = 200                                        # pair 0 has 200 points
    loss = losses.infoNCE(*nce_args(vtx, pts, dict(t, corr_v2p=corr)), 0.07, num_graphs=5)
    assert torch.isnan(loss)
    with pytest.raises(losses.LossInputError, match="index"):
        losses.check_inputs()


# ------------------------------------------------------------------------------------------------------------------- multi-positive
def multipos_run(view):
    if ("mp", view) not in _cache:
        f = torch.from_numpy(MP["feat"])
        samples = tuple(ids(MP[k]).to(DEV) for k in ("sample_ids", "pos_ids", "neg_ids"))
        if view:
            stack = torch.randn(len(f), 3, 32, generator=torch.Generator().manual_seed(1))
            stack[:, 1, :] = f
            leaf = stack.to(DEV).requires_grad_(True)
            feat = leaf[:, 1, :]
        else:
            leaf = f.to(DEV).requires_grad_(True)
            feat = leaf
        loss = losses.multi_pos_infoNCE(feat, None, ids(MP["batch"]).to(DEV), samples=samples, num_graphs=2)
        loss.backward()
        _cache[("mp", view)] = (float(loss), leaf.grad.cpu().numpy())
    return _cache[("mp", view)]


@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "keyframe_view"])
def test_multipos_against_the_reference(view):
    """meshes of 512 and 700 vertices, width 32, the reference's own draws; once contiguous, once as the [:, t, :] view of an [N, 3, 32]
    tensor (training/train_rig.py:154-156); vertex 5 shares its skin row with nobody: all of its positives are itself"""
    loss, grad = multipos_run(view)
    dev = MP_META["deviations"]
    if view:
        assert (grad[:, 0, :] == 0).all() and (grad[:, 2, :] == 0).all()
        grad = grad[:, 1, :]
    ok = report("multi-pos loss rel", abs(loss - float(MP["loss"])) / abs(float(MP["loss"])), bound(dev["dev_loss"]))
    ok &= report("multi-pos grad rel", rel_max(grad, MP["grad"]), bound(dev["dev_grad"]))
    assert ok
    sampled = np.zeros(len(grad), dtype=bool)
    for b in range(2):
        sampled[np.nonzero(MP["batch"] == b)[0][MP["sample_ids"][b]]] = True
    assert (grad[~sampled] == 0).all() and (~sampled).sum() == 188            # unsampled rows: exactly zero


def test_multipos_two_runs_are_bit_identical():
    first = multipos_run(False)
    _cache.pop(("mp", False))
    again = multipos_run(False)
    assert first[0] == again[0] and np.array_equal(first[1], again[1])
    assert first[0] == multipos_run(True)[0] and np.array_equal(first[1], multipos_run(True)[1][:, 1, :])


# ------------------------------------------------------------------------------------------------------------------- chamfer
def chamfer_alone(name):
    if ("ch", name) not in _cache:
        p = torch.from_numpy(CH[f"{name}_p"]).to(DEV).requires_grad_(True)
        q = torch.from_numpy(CH[f"{name}_q"]).to(DEV).requires_grad_(True)
        loss = losses.chamfer_distance_with_average(p.unsqueeze(0), q.unsqueeze(0))
        loss.backward()
        _cache[("ch", name)] = (float(loss), p.grad.cpu().numpy(), q.grad.cpu().numpy())
    return _cache[("ch", name)]


@pytest.mark.parametrize("name", CH_META["batch"] + ["coincide"])
def test_chamfer_alone_through_the_reference_signature(name):
    loss, gp, gq = chamfer_alone(name)
    dev = CH_META["deviations"][name]
    ok = report(f"chamfer {name} loss rel", abs(loss - float(CH[f"{name}_loss"])) / float(CH[f"{name}_loss"]), bound(dev["dev_loss"]))
    ok &= report(f"chamfer {name} grad_p rel", rel_max(gp, CH[f"{name}_grad_p"]), bound(dev["dev_grad_p"]))
    ok &= report(f"chamfer {name} grad_q rel", rel_max(gq, CH[f"{name}_grad_q"]), bound(dev["dev_grad_q"]))
    assert ok
    if name == "coincide":                                  # joint 2 IS vertex 7: finite everywhere, nothing through the zero distance
        c = CH_META["coincide"]
        assert np.isfinite(loss) and np.isfinite(gp).all() and np.isfinite(gq).all()
        assert (gp[c["vertex"]] == 0).all()
        assert np.array_equal(gq[c["joint"]] == 0, CH["coincide_grad_q"][c["joint"]] == 0)


def test_chamfer_batched_in_one_launch():
    """(N, M) = (600, 17), (1, 1), (64, 1), (65, 33), (1025, 3) as one batch: the mean of the reference's five losses, its gradients / 5;
    bit-identical when run again"""
    names = CH_META["batch"]
    cat = lambda k: torch.cat([torch.from_numpy(CH[f"{n}_{k}"]) for n in names])
    bvec = lambda k: torch.cat([torch.full((len(CH[f"{n}_{k}"]),), i, dtype=torch.long) for i, n in enumerate(names)]).to(DEV)
    out = []
    for _ in range(2):
        p, q = cat("p").to(DEV).requires_grad_(True), cat("q").to(DEV).requires_grad_(True)
        loss = losses.chamfer_batched(p, bvec("p"), q, bvec("q"), num_graphs=len(names))
        loss.backward()
        out.append((float(loss), p.grad.cpu().numpy(), q.grad.cpu().numpy()))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    loss, gp, gq = out[0]
    devs = [CH_META["deviations"][n] for n in names]
    want = float(np.mean([np.float64(CH[f"{n}_loss"]) for n in names]))
    ok = report("chamfer batch loss rel", abs(loss - want) / want, bound(max(d["dev_loss"] for d in devs)))
    ok &= report("chamfer batch grad_p rel", rel_max(gp, cat("grad_p").numpy() / 5), bound(max(d["dev_grad_p"] for d in devs)))
    ok &= report("chamfer batch grad_q rel", rel_max(gq, cat("grad_q").numpy() / 5), bound(max(d["dev_grad_q"] for d in devs)))
    assert ok


# ------------------------------------------------------------------------------------------------------------------- one training step
def test_one_training_step_of_the_rig_loop():
    """training/train_rig.py:162-190 on a two-mesh batch: jointnet_motion in train mode, loss = 0.1 sum multi_pos_infoNCE + chamfer + l1.
    The loss equals the float64 oracle on the same device outputs; backward() leaves a finite gradient on every parameter, and one that is
    not all zero on every parameter this loss reaches."""
    torch.manual_seed(5)
    b = synth.make_batch([31, 32], n_side=23)
    n, batch = b.pos.shape[0], b.batch
    assert int(torch.bincount(batch).min()) >= 512
    g = torch.Generator().manual_seed(6)
    bone = (b.pos[:, 0] > b.pos[:, 0].median()).long() * 3 + torch.randint(0, 3, (n,), generator=g)
    gt_skin = torch.nn.functional.one_hot(bone, 6).float()
    joints = torch.rand(60, 3, generator=g) - 0.5
    joints_batch = torch.arange(2).repeat_interleave(30)
    offsets = torch.rand(n, 3, generator=g) * 0.2 - 0.1
    model = synth.load_recipe(models.jointnet_motion(num_keyframes=5, chn_output=3, aggr_method="attn"), 3, mild=True).to(DEV).train()
    d = b.to(DEV)
    samples = [tuple(t.to(DEV) for t in losses.draw_multi_pos_samples(gt_skin, batch, generator=g, num_graphs=2)) for _ in range(6)]
    motion_all, motion_aggr, disp = model(d, d.pred_flow)
    disp = torch.tanh(disp)
    y_pred = disp + d.pos
    emb = 0.0
    for t in range(motion_all.shape[1]):
        emb = emb + losses.multi_pos_infoNCE(motion_all[:, t, :], gt_skin.to(DEV), d.batch, samples=samples[t], num_graphs=2)
    emb = emb + losses.multi_pos_infoNCE(motion_aggr, gt_skin.to(DEV), d.batch, samples=samples[5], num_graphs=2)
    chamfer = losses.chamfer_batched(y_pred, d.batch, joints.to(DEV), joints_batch.to(DEV), num_graphs=2)
    l1 = torch.nn.functional.l1_loss(disp, offsets.to(DEV))
    loss = 0.1 * emb + chamfer + l1
    loss.backward()
    f64 = lambda t: t.detach().cpu().double()
    want = 0.0
    for t in range(6):
        feat = f64(motion_all[:, t, :]) if t < 5 else f64(motion_aggr)
        want = want + 0.1 * lo.multipos_loss(feat, batch, *(s.cpu() for s in samples[t]), 2)
    want = float(want + lo.chamfer_loss(f64(y_pred), batch, joints.double(), joints_batch, 2) + (f64(disp) - offsets.double()).abs().mean())
    fwd = bound(max(MP_META["deviations"]["dev_loss"], max(v["dev_loss"] for v in CH_META["deviations"].values())))
    assert report("training step loss against the oracle on the device outputs, rel", abs(float(loss) - want) / want, fwd)
    named = list(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in named)
    dead = [k for k, p in named if not bool((p.grad != 0).any())]
    print(f"\ntraining step: loss {float(loss):.6f}, {len(named)} parameters, all-zero gradients on {dead}")
    assert not dead, dead                                   # every parameter of jointnet_motion feeds motion_all, motion_aggr or the shift
