"""csrc/losses_skin.hip and the skin losses of morig_amd/losses.py on the device, against the reference's recorded float32 results
(tests/golden/loss_logratio_*.npz, loss_skin_ce.npz; tools/make_skin_loss_golden.py).

Bounds follow tests/test_gpu_losses.py: per case the generator stored the deviation of the reference's float32 result from the float64
oracle (relative for a loss, relative to max |grad| for a gradient); the device has to stay within TEN times that of the reference's
result, and a bound is never tighter than one float32 ulp (2^-23) of the quantity's largest magnitude. Every figure is printed before it
is asserted (run with -s); the figures are tabulated in DESIGN.md section 14.
"""
import numpy as np
import pytest
import torch

import skin_loss_oracle as so
from morig_amd import losses, models, synth
from test_gpu_losses import bound, rel_max, report
from test_loss_oracle import ids
from test_skin_loss_oracle import CE, CE_META, LR, LR_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}


@pytest.fixture(autouse=True)
def _grad_on():
    """conftest.py runs every test under torch.no_grad(); these need the graph"""
    with torch.enable_grad():
        yield
    losses.check_inputs()                                  # no launch of the test found its inputs wrong


# ------------------------------------------------------------------------------------------------------------------- log-ratio
def lr_inputs(case, mesh=None):
    """the fixture's batch (or mesh ``mesh`` alone, as a batch of one) -> (feat, gt, batch, samples, B) on the host"""
    meta, z = LR[case]
    feat, gt, batch, samples = torch.from_numpy(z["feat"]), torch.from_numpy(z["gt"]), ids(z["batch"]), ids(z["samples"])
    if mesh is None:
        return feat, gt, batch, samples, len(meta["sizes"])
    keep = batch == mesh
    return feat[keep], gt[keep], batch[keep] * 0, samples[mesh:mesh + 1], 1


def lr_run(case, mesh=None, view=False):
    key = ("lr", case, mesh, view)
    if key not in _cache:
        feat, gt, batch, samples, B = lr_inputs(case, mesh)
        if view:
            kv = LR[case][0]["keyframe_view"]
            stack = torch.randn(len(feat), kv["T"], feat.shape[1], generator=torch.Generator().manual_seed(kv["seed"]))
            stack[:, kv["t"], :] = feat
            leaf = stack.to(DEV).requires_grad_(True)
            f = leaf[:, kv["t"], :]
        else:
            leaf = feat.to(DEV).requires_grad_(True)
            f = leaf
        loss = losses.log_ratio_loss(f, gt.to(DEV), batch.to(DEV), samples=samples.to(DEV), num_graphs=B)
        loss.backward()
        _cache[key] = (float(loss), leaf.grad.cpu().numpy())
    return _cache[key]


def lr_check(what, case, loss, grad):
    meta, z = LR[case]
    dev = meta["deviations"]
    ok = report(f"log-ratio {what} loss rel", abs(loss - float(z["loss"])) / abs(float(z["loss"])), bound(dev["dev_loss"]))
    ok &= report(f"log-ratio {what} grad rel", rel_max(grad, z["grad"]), bound(dev["dev_grad"]))
    assert ok
    batch, samples = z["batch"].astype(np.int64), z["samples"].astype(np.int64)
    sampled = np.zeros(len(grad), dtype=bool)
    for b in range(len(meta["sizes"])):
        sampled[np.nonzero(batch == b)[0][samples[b]]] = True
    assert (grad[~sampled] == 0).all() and np.isfinite(grad).all()                          # unsampled rows: exactly zero


@pytest.mark.parametrize("case", LR_CASES)
def test_log_ratio_against_the_reference(case):
    """one mesh of exactly 50 vertices; meshes of 50, 67, 130 at width 32 / 48; width 4 / 4; two identical sampled feature rows and two
    identical gt_skin rows -- the reference's own draws, its float32 loss and autograd gradient"""
    loss, grad = lr_run(case)
    lr_check(case, case, loss, grad)
    if case == "coincident":                                # the pair of identical rows: finite, and 1 / (0 + eps) multiplies an exact zero
        assert np.isfinite(loss)
        i, j = LR[case][0]["coincident"]["feature_rows"]
        others = np.delete(np.abs(grad).max(axis=1), [i, j])
        print(f"\nlog-ratio coincident: max |grad| of rows {i}, {j}: {np.abs(grad[[i, j]]).max():.3e}, of the other rows: {others.max():.3e}")
        assert np.abs(grad[[i, j]]).max() <= 10 * others.max()


def test_log_ratio_as_a_keyframe_view():
    """the ragged case as the [:, t, :] view of an [N, 5, 32] tensor, read in place: the same bits, the other keyframes exact zeros"""
    loss, grad = lr_run("ragged", view=True)
    t = LR["ragged"][0]["keyframe_view"]["t"]
    assert (np.delete(grad, t, axis=1) == 0).all()
    lr_check("keyframe view", "ragged", loss, grad[:, t, :])
    base = lr_run("ragged")
    assert loss == base[0] and np.array_equal(grad[:, t, :], base[1])


def test_log_ratio_identical_rows_give_exactly_zero_gradient():
    """three samples whose feature rows are all the same: every distance is 0, the loss is finite and every f_i - f_j an exact zero"""
    _, z = LR["coincident"]
    feat = torch.from_numpy(np.repeat(z["feat"][3:4], 3, axis=0)).to(DEV).requires_grad_(True)
    gt = torch.from_numpy(z["gt"][:3]).to(DEV)
    loss = losses.log_ratio_loss(feat, gt, torch.zeros(3, dtype=torch.long, device=DEV), samples=torch.arange(3, device=DEV)[None], num_graphs=1)
    loss.backward()
    want = float(so.logratio_loss(feat.detach().cpu().double(), gt.cpu().double(), torch.zeros(3, dtype=torch.long), torch.arange(3)[None], 1))
    assert report("log-ratio three identical rows loss rel", abs(float(loss) - want) / want, 1e-6)
    assert (feat.grad == 0).all()


def test_log_ratio_two_runs_are_bit_identical():
    first = lr_run("ragged")
    _cache.pop(("lr", "ragged", None, False))
    again = lr_run("ragged")
    assert first[0] == again[0] and np.array_equal(first[1], again[1])


def test_log_ratio_each_mesh_alone_is_its_share_of_the_batch():
    loss, grad = lr_run("ragged")
    meta, z = LR["ragged"]
    B = len(meta["sizes"])
    alone = [lr_run("ragged", b) for b in range(B)]
    assert report("log-ratio sum of meshes alone / B against the batch, rel", abs(sum(a[0] for a in alone) / B - loss) / loss, 2.0 ** -22)
    # the division by the number of meshes is the last operation on a gradient row: the same bits
    scaled = np.concatenate([a[1] for a in alone]) / np.float32(B)
    assert scaled.dtype == np.float32 and np.array_equal(grad, scaled)


def frames_inputs():
    feat, gt, batch, _, B = lr_inputs("ragged")
    g = torch.Generator().manual_seed(2)
    motion_all = (torch.randn(len(feat), 5, 32, generator=g) * 0.5).to(DEV).requires_grad_(True)
    motion_aggr = feat.to(DEV).requires_grad_(True)
    samples = losses.draw_log_ratio_samples(batch, n_sets=6, generator=g, num_graphs=B).to(DEV)
    return motion_all, motion_aggr, gt.to(DEV), batch.to(DEV), samples, B


def test_log_ratio_frames_against_six_single_calls():
    """one launch for the five keyframes and the aggregate: gradients bit-identical to six single calls, the loss -- a float64 sum over
    the sets rounded once, against a Python sum of float32 losses rounded six times -- to 2^-22"""
    motion_all, motion_aggr, gt, batch, samples, B = frames_inputs()
    loss = losses.log_ratio_frames(motion_all, motion_aggr, gt, batch, samples=samples, num_graphs=B)
    loss.backward()
    got = (float(loss), motion_all.grad.clone(), motion_aggr.grad.clone())
    motion_all.grad = motion_aggr.grad = None
    single, total64 = 0.0, 0.0
    for t in range(6):
        f = motion_all[:, t, :] if t < 5 else motion_aggr
        l = losses.log_ratio_loss(f, gt, batch, samples=samples[t], num_graphs=B)
        single, total64 = single + l, total64 + float(l)
    single.backward()
    assert report("log_ratio_frames against the sum of six calls, rel", abs(got[0] - total64) / total64, 2.0 ** -22)
    assert torch.equal(got[1], motion_all.grad) and torch.equal(got[2], motion_aggr.grad)
    assert bool((got[1] != 0).any(dim=2).any(dim=0).all())
    # and again: the same bits
    motion_all.grad = motion_aggr.grad = None
    again = losses.log_ratio_frames(motion_all, motion_aggr, gt, batch, samples=samples, num_graphs=B)
    again.backward()
    assert float(again) == got[0] and torch.equal(got[1], motion_all.grad) and torch.equal(got[2], motion_aggr.grad)
    # against the float64 oracle on the same inputs, under the bound of the ragged case
    want = so.logratio_frames(motion_all.detach().cpu().double(), motion_aggr.detach().cpu().double(), gt.cpu().double(), batch.cpu(),
                              samples.cpu(), B)
    dev = LR["ragged"][0]["deviations"]
    ok = report("log_ratio_frames loss against the float64 oracle, rel", abs(got[0] - float(want[0])) / float(want[0]), bound(dev["dev_loss"]))
    ok &= report("log_ratio_frames grad motion_all rel", rel_max(got[1].cpu().numpy(), want[1].numpy()), bound(dev["dev_grad"]))
    ok &= report("log_ratio_frames grad motion_aggr rel", rel_max(got[2].cpu().numpy(), want[2].numpy()), bound(dev["dev_grad"]))
    assert ok


def test_log_ratio_allocates_nothing_of_the_size_of_the_pair_tables():
    """forward and backward of the three-mesh case grow the peak by less than ONE 1225 x 1225 float32 matrix (the reference holds
    [3, 1225, 1225, 48] of them)"""
    feat, gt, batch, samples, B = (t.to(DEV) if torch.is_tensor(t) else t for t in lr_inputs("ragged"))
    feat.requires_grad_(True)
    losses.log_ratio_loss(feat, gt, batch, samples=samples, num_graphs=B).backward()       # warm: the library, the pinned status word
    feat.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    loss = losses.log_ratio_loss(feat, gt, batch, samples=samples, num_graphs=B)
    loss.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"\nlog-ratio (50, 67, 130): peak grew by {grown} bytes (one pair table: {1225 * 1225 * 4})")
    assert grown < 1225 * 1225 * 4
    assert float(loss) == lr_run("ragged")[0]


def test_wrong_samples_are_reported_not_followed():
    feat, gt, batch, samples, B = (t.to(DEV) if torch.is_tensor(t) else t for t in lr_inputs("ragged"))
    for row, col, value in ((0, 4, 50), (2, 0, -3), (1, 7, int(samples[1, 8]))):           # past the mesh, negative, a repeat
        s = samples.clone()
        s[row, col] = value
        f = feat.clone().requires_grad_(True)
        loss = losses.log_ratio_loss(f, gt, batch, samples=s, num_graphs=B)
        assert torch.isnan(loss)
        with pytest.raises(losses.LossInputError, match="index"):
            losses.check_inputs()


# ------------------------------------------------------------------------------------------------------------------- masked soft-label CE
def ce_run():
    if "ce" not in _cache:
        x = torch.from_numpy(CE["x"]).to(DEV).requires_grad_(True)
        loss, vm = losses.skin_ce_loss(x, torch.from_numpy(CE["label"]).to(DEV), ids(CE["mask"]).to(DEV), nearest_bone=CE_META["K"],
                                       return_vert_mask=True)
        loss.backward()
        _cache["ce"] = (float(loss), x.grad.cpu().numpy(), vm.cpu().numpy())
    return _cache["ce"]


def test_skin_ce_against_the_reference():
    """384 rows with 0 .. 5 non-zero labels, masked-out columns, a sixth label column outside the picked five: vert_mask equal on every
    row (the rows are order-independent), the reference's float32 loss and gradient"""
    loss, grad, vm = ce_run()
    assert np.array_equal(vm > 0, CE["vert_mask"])
    dev = CE_META["deviations"]
    ok = report("skin CE loss rel", abs(loss - float(CE["loss"])) / abs(float(CE["loss"])), bound(dev["dev_loss"]))
    ok &= report("skin CE grad rel", rel_max(grad, CE["grad"]), bound(dev["dev_grad"]))
    assert ok
    assert (grad[~CE["vert_mask"]] == 0).all()                                              # a masked-out vertex: exactly zero


def test_skin_ce_known_answers_of_the_order_rule():
    """a dozen rows whose vert_mask DEPENDS on the order of the two sums: the device gives what index order in float32 gives"""
    label, mask = torch.from_numpy(CE["known_label"]).to(DEV), ids(CE["known_mask"]).to(DEV)
    x = torch.zeros(len(label), CE_META["K"], device=DEV)
    _, vm = losses.skin_ce_loss(x, label, mask, nearest_bone=CE_META["K"], return_vert_mask=True)
    print(f"\nskin CE known answers: device {vm.cpu().numpy().astype(int).tolist()} want {CE['known_vert_mask'].astype(int).tolist()}")
    assert np.array_equal(vm.cpu().numpy() > 0, CE["known_vert_mask"])


def test_skin_ce_all_masked_is_nan_and_two_runs_are_bit_identical():
    x = torch.from_numpy(CE["x"]).to(DEV)
    label, mask = torch.from_numpy(CE["label"]).to(DEV), ids(CE["mask"]).to(DEV)
    assert torch.isnan(losses.skin_ce_loss(x, label, torch.zeros_like(mask), nearest_bone=CE_META["K"]))
    first = ce_run()
    _cache.pop("ce")
    again = ce_run()
    assert first[0] == again[0] and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weight"])
def test_cross_entropy_with_probs_against_torch(weighted):
    """the three reductions, with and without weight, at K = 5 and K = 128, against the same formula in torch on the device (float64)"""
    g = torch.Generator().manual_seed(8)
    for n, K in ((384, 5), (300, 128)):
        x = (torch.randn(n, K, generator=g) * 2.0).to(DEV)
        target = torch.softmax(torch.randn(n, K, generator=g), dim=1).to(DEV)
        weight = torch.rand(K, generator=g).to(DEV) if weighted else None
        up = torch.rand(n, K, generator=g).to(DEV)
        for reduction, u in (("none", up), ("mean", 1.5), ("sum", 0.25)):
            out = []
            for _ in range(2):
                leaf = x.clone().requires_grad_(True)
                val = losses.cross_entropy_with_probs(leaf, target, weight, reduction)
                (val * u).sum().backward()
                out.append((val.detach(), leaf.grad))
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
            w64 = None if weight is None else torch.broadcast_to(weight, x.shape).double()
            want, grad = so.ce_probs(x.double(), target.double(), w64, reduction, up.double() if reduction == "none" else u)
            # float32 exp / log / the subtraction of the maximum at logits up to |8|: 16 ulp (2^-19) of the largest entry
            ok = report(f"cross_entropy_with_probs K {K} {reduction} value rel", rel_max(out[0][0].cpu().numpy().reshape(-1), want.cpu().numpy().reshape(-1)), 2e-6)
            ok &= report(f"cross_entropy_with_probs K {K} {reduction} grad rel", rel_max(out[0][1].cpu().numpy(), grad.cpu().numpy()), 2e-6)
            assert ok


# ------------------------------------------------------------------------------------------------------------------- one training step
def test_one_training_step_of_the_skin_loop():
    """training/train_skin.py:145-178 on a two-mesh batch: skinnet_motion in train mode, loss = skin_ce_loss + 0.1 log_ratio_frames,
    backward(), optimizer.step(): the loss equals the float64 oracle on the same device outputs, every parameter gradient is finite"""
    torch.manual_seed(5)
    b = synth.make_batch(range(31, 33), n_side=9, with_skin=True)
    n, batch = b.pos.shape[0], b.batch
    assert int(torch.bincount(batch).min()) >= 50
    g = torch.Generator().manual_seed(6)
    gt_skin = torch.zeros(n, 48)
    bones = torch.randint(0, 12, (n, 3), generator=g)
    gt_skin.scatter_(1, bones, torch.rand(n, 3, generator=g) + 0.05)
    gt_skin = gt_skin / gt_skin.sum(1, keepdim=True)
    skin_label = torch.rand(n, 5, generator=g) * (torch.rand(n, 5, generator=g) < 0.6)
    skin_label = skin_label / (skin_label.sum(1, keepdim=True) + 1e-8)
    loss_mask = (torch.rand(n, 5, generator=g) < 0.85).long()
    kw = dict(nearest_bone=5, use_Dg=False, use_Lf=False, num_keyframes=5, use_motion=True, motion_dim=32)
    model = synth.load_recipe(models.skinnet_motion(**kw), 204).to(DEV).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-4)
    d = b.to(DEV)
    samples = losses.draw_log_ratio_samples(batch, n_sets=6, generator=g, num_graphs=2).to(DEV)
    optimizer.zero_grad()
    motion_all, motion_aggr, skin_pred = model(d, d.pred_flow)
    loss_skin, vert_mask = losses.skin_ce_loss(skin_pred, skin_label.to(DEV), loss_mask.to(DEV), nearest_bone=5, return_vert_mask=True)
    loss_emb = 0.1 * losses.log_ratio_frames(motion_all, motion_aggr, gt_skin.to(DEV), d.batch, samples=samples, num_graphs=2)
    loss = loss_skin + loss_emb
    loss.backward()
    before = [p.detach().clone() for p in model.parameters()]
    optimizer.step()
    losses.check_inputs()
    f64 = lambda t: t.detach().cpu().double()
    want = so.skin_ce_loss(f64(skin_pred), skin_label.double(), loss_mask, 5, vert_mask.cpu() > 0)
    want = float(want + 0.1 * so.logratio_frames(f64(motion_all), f64(motion_aggr), gt_skin.double(), batch, samples.cpu(), 2)[0])
    fwd = bound(max(CE_META["deviations"]["dev_loss"], max(LR[c][0]["deviations"]["dev_loss"] for c in LR_CASES)))
    assert report("skin training step loss against the oracle on the device outputs, rel", abs(float(loss) - want) / want, fwd)
    assert np.array_equal(vert_mask.cpu().numpy() > 0, so.vert_mask_sequential(skin_label.numpy(), loss_mask.float().numpy(), 5))
    named = list(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in named)
    dead = [k for k, p in named if not bool((p.grad != 0).any())]
    moved = sum(not torch.equal(p.detach(), q) for (_, p), q in zip(named, before))
    print(f"\nskin training step: loss {float(loss):.6f} (CE {float(loss_skin):.6f}), {len(named)} parameters, {moved} moved, all-zero gradients on {dead}")
    assert moved > 0
