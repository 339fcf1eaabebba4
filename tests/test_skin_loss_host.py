"""The skin losses of morig_amd/losses.py on an emulated op layer (tests/skin_loss_emulate.py through ``runtime._test_ops``): autograd
wiring, log_ratio_frames against single calls, num_graphs handling, the sampler, what is refused, the status word, the reductions."""
import numpy as np
import pytest
import torch

import skin_loss_emulate
import skin_loss_oracle as so
from morig_amd import losses, runtime
from test_loss_oracle import ids
from test_skin_loss_oracle import CE, CE_META, LR


@pytest.fixture()
def ops(monkeypatch):
    o = skin_loss_emulate.SkinLossOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


@pytest.fixture(autouse=True)
def _grad_on():
    with torch.enable_grad():
        yield


def ragged():
    meta, z = LR["ragged"]
    return torch.from_numpy(z["feat"]), torch.from_numpy(z["gt"]), ids(z["batch"]), ids(z["samples"]), len(meta["sizes"])


def test_log_ratio_autograd_wiring(ops):
    feat, gt, batch, samples, B = ragged()
    leaf = feat.clone().requires_grad_(True)
    loss = losses.log_ratio_loss(leaf, gt, batch, samples=samples, num_graphs=B)
    (3.0 * loss).backward()
    want, grad = so.logratio(feat.double(), gt.double(), batch, samples, B)
    assert loss.shape == () and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert (leaf.grad.double() - 3.0 * grad).abs().max() <= 1e-4 * grad.abs().max() * 3
    assert ops.calls == ["logratio_forward", "logratio_backward"]
    sampled = torch.zeros(len(feat), dtype=torch.bool)
    sampled[so._rows(batch, samples, B).reshape(-1)] = True
    assert (leaf.grad[~sampled] == 0).all() and int((~sampled).sum()) == 97
    # a strided keyframe view is read in place: the same loss, the gradient lands in its slab only
    stack = torch.randn(len(feat), 5, 32, generator=torch.Generator().manual_seed(1))
    stack[:, 2, :] = feat
    stack.requires_grad_(True)
    view = losses.log_ratio_loss(stack[:, 2, :], gt, batch, samples=samples[None], num_graphs=B)
    view.backward()
    assert abs(float(view) - float(loss)) <= 1e-6 * float(loss) and (stack.grad[:, [0, 1, 3, 4], :] == 0).all()
    assert (stack.grad[:, 2, :] * 3.0 - leaf.grad).abs().max() <= 1e-5 * leaf.grad.abs().max()


def test_log_ratio_frames_is_the_sum_of_single_calls(ops):
    feat, gt, batch, _, B = ragged()
    g = torch.Generator().manual_seed(2)
    motion_all = torch.randn(len(feat), 5, 32, generator=g).requires_grad_(True)
    motion_aggr = feat.clone().requires_grad_(True)
    samples = losses.draw_log_ratio_samples(batch, n_sets=6, generator=g, num_graphs=B)
    assert samples.shape == (6, B, 50)
    loss = losses.log_ratio_frames(motion_all, motion_aggr, gt, batch, samples=samples, num_graphs=B)
    (0.1 * loss).backward()
    assert ops.calls == ["logratio_forward", "logratio_backward"]
    got_all, got_aggr = motion_all.grad.clone(), motion_aggr.grad.clone()
    motion_all.grad = motion_aggr.grad = None
    single = 0.0
    for t in range(5):
        single = single + losses.log_ratio_loss(motion_all[:, t, :], gt, batch, samples=samples[t], num_graphs=B)
    single = single + losses.log_ratio_loss(motion_aggr, gt, batch, samples=samples[5], num_graphs=B)
    (0.1 * single).backward()
    assert abs(float(loss) - float(single)) <= 1e-6 * float(single)
    # (bit-identical on the device, tests/test_gpu_skin_losses.py; the emulation's float32 sums depend on the memory layout)
    assert (got_all - motion_all.grad).abs().max() <= 1e-5 * got_all.abs().max() and (got_aggr - motion_aggr.grad).abs().max() <= 1e-5 * got_aggr.abs().max()
    assert bool((got_all != 0).any(dim=2).any(dim=0).all())                                 # every keyframe received its gradient


def test_num_graphs(ops):
    feat, gt, batch, samples, B = ragged()
    a = float(losses.log_ratio_loss(feat, gt, batch, samples=samples))                     # read from the batch vector
    b = float(losses.log_ratio_loss(feat, gt, batch, samples=samples, num_graphs=B))
    assert a == b
    # three empty meshes more: they add nothing and the divisor doubles
    more = torch.cat([samples, torch.zeros(3, 50, dtype=torch.long)])
    c = float(losses.log_ratio_loss(feat, gt, batch, samples=more, num_graphs=2 * B))
    assert abs(c - b / 2) <= 1e-6 * b
    with pytest.raises(losses.LossInputError, match="outside"):
        losses.log_ratio_loss(feat, gt, batch, samples=samples[:2], num_graphs=2)


def test_sampler_properties(ops):
    _, _, batch, _, B = ragged()
    g = torch.Generator().manual_seed(9)
    s = losses.draw_log_ratio_samples(batch, n_sets=4, generator=g, num_graphs=B)
    sizes = torch.bincount(batch)
    assert s.shape == (4, B, 50) and s.dtype == torch.int64
    assert bool((s >= 0).all()) and bool((s < sizes[None, :, None]).all())
    srt = torch.sort(s, dim=2).values
    assert not bool((srt[:, :, 1:] == srt[:, :, :-1]).any())
    assert sorted(s[0, 0].tolist()) == list(range(50))                                      # a mesh of exactly 50: every vertex
    assert not torch.equal(s[0], s[1])                                                      # every set has its own draws
    assert losses.draw_log_ratio_samples(batch, n_sample=7, num_graphs=B).shape == (1, B, 7)
    with pytest.raises(losses.LossInputError, match="fewer than 51"):
        losses.draw_log_ratio_samples(batch, n_sample=51, num_graphs=B)
    feat, gt, batch, _, B = ragged()
    assert np.isfinite(float(losses.log_ratio_loss(feat, gt, batch)))                       # draws its own, as the reference does
    with pytest.raises(losses.LossInputError, match="fewer than 50"):
        losses.log_ratio_loss(feat[:49], gt[:49], batch[:49])


def test_refused_shapes_are_named(ops):
    feat, gt, batch, samples, B = ragged()
    kw = dict(samples=samples, num_graphs=B)
    for bad_feat, what in ((feat[:, :30], "feature widths"), (torch.zeros(len(feat), 132), "feature widths"), (feat[:, :0], "feature widths")):
        with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*" + what):
            losses.log_ratio_loss(bad_feat, gt, batch, **kw)
    for bad_gt in (gt[:, :46], torch.zeros(len(feat), 132)):
        with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*gt_skin widths"):
            losses.log_ratio_loss(feat, bad_gt, batch, **kw)
    with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*n_sample = 2"):
        losses.log_ratio_loss(feat, gt, batch, samples=samples[:, :2], num_graphs=B)
    big = torch.arange(65)[None].repeat(B, 1)
    with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*n_sample from 3 to 64"):
        losses.log_ratio_loss(feat, gt, batch, samples=big, num_graphs=B)
    with pytest.raises(losses.LossInputError, match="float32"):
        losses.log_ratio_loss(feat.double(), gt, batch, **kw)
    with pytest.raises(losses.LossInputError, match="samples"):
        losses.log_ratio_loss(feat, gt, batch, samples=samples[:2], num_graphs=B)
    with pytest.raises(losses.LossInputError, match="motion_aggr"):
        losses.log_ratio_frames(torch.zeros(len(feat), 5, 32), feat[:, :16], gt, batch, num_graphs=B)
    assert float(losses.log_ratio_loss(feat, gt, batch, samples=samples[:, :3], num_graphs=B)) > 0      # three samples: three pairs
    x = torch.zeros(4, 9)
    with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*nearest_bone"):
        losses.skin_ce_loss(x, torch.zeros(4, 9), torch.ones(4, 9))
    with pytest.raises(losses.LossInputError, match="skin_pred"):
        losses.skin_ce_loss(torch.zeros(4, 6), torch.zeros(4, 6), torch.ones(4, 6), nearest_bone=5)
    with pytest.raises(losses.LossInputError, match="skin_label"):
        losses.skin_ce_loss(torch.zeros(4, 5), torch.zeros(4, 4), torch.ones(4, 5))
    with pytest.raises(losses.LossInputError, match="MORIG_E_UNSUPPORTED.*128 classes"):
        losses.cross_entropy_with_probs(torch.zeros(2, 129), torch.zeros(2, 129))
    with pytest.raises(ValueError, match="Keyword 'reduction' must be one of"):
        losses.cross_entropy_with_probs(torch.zeros(2, 3), torch.zeros(2, 3), reduction="avg")


def test_wrong_samples_give_nan_and_the_status_error(ops):
    feat, gt, batch, samples, B = ragged()
    for bad in (50, -1):                                    # mesh 0 has 50 vertices
        s = samples.clone()
        s[0, 4] = bad
        with pytest.raises(losses.LossInputError, match="index"):
            losses.log_ratio_loss(feat, gt, batch, samples=s, num_graphs=B)
    s = samples.clone()
    s[1, 7] = s[1, 8]                                       # a repeat inside a mesh
    with pytest.raises(losses.LossInputError, match="index"):
        losses.log_ratio_loss(feat, gt, batch, samples=s, num_graphs=B)
    status = torch.zeros(1, dtype=torch.int32)
    ptr = ops.segment_ptr(batch, B, status)
    loss, _ = ops.logratio_forward(None, feat, gt, ptr, s[None].int(), status)
    assert torch.isnan(loss).all() and int(status) == losses.ST_INDEX
    g_all, g_aggr = ops.logratio_backward(None, feat, gt, ptr, s[None].int(), torch.zeros(1, B, 2, 50, 50), torch.ones(1), status)
    assert g_all is None and (g_aggr == 0).all()


def ce_inputs():
    return torch.from_numpy(CE["x"]), torch.from_numpy(CE["label"]), ids(CE["mask"]), CE_META["K"]


def test_skin_ce_wiring_and_the_all_masked_batch(ops):
    x, label, mask, K = ce_inputs()
    leaf = x.clone().requires_grad_(True)
    loss, vm = losses.skin_ce_loss(leaf, label, mask, nearest_bone=K, return_vert_mask=True)
    (2.0 * loss).backward()
    want, grad = so.skin_ce(x.double(), label.double(), mask, K)
    assert loss.shape == () and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert (leaf.grad.double() - 2.0 * grad).abs().max() <= 1e-5 * grad.abs().max() * 2
    assert np.array_equal(vm.numpy() > 0, CE["vert_mask"]) and not vm.requires_grad
    assert ops.calls == ["skin_ce_forward", "skin_ce_backward"]
    assert float(losses.skin_ce_loss(x, label, mask)) == float(loss)                        # K: the width of skin_pred
    assert float(losses.skin_ce_loss(x, label, mask.bool(), nearest_bone=K)) == float(loss)
    assert torch.isnan(losses.skin_ce_loss(x, label, torch.zeros_like(mask), nearest_bone=K))            # 0 / 0, as the reference
    assert torch.isnan(losses.skin_ce_loss(x, torch.zeros_like(label), mask, nearest_bone=K))


def test_cross_entropy_with_probs_reductions_and_weight(ops):
    x, label, _, K = ce_inputs()
    g = torch.Generator().manual_seed(8)
    target = torch.softmax(torch.randn(x.shape, generator=g), dim=1)
    up = torch.rand(x.shape, generator=g)
    for weight in (None, torch.rand(K, generator=g), torch.rand(x.shape, generator=g)):
        w = None if weight is None else torch.broadcast_to(weight, x.shape)
        for reduction, u in (("none", up), ("mean", 1.5), ("sum", 0.25)):
            leaf = x.clone().requires_grad_(True)
            out = losses.cross_entropy_with_probs(leaf, target, weight, reduction)
            (out * u).sum().backward()
            want, grad = so.ce_probs(x.double(), target.double(), None if w is None else w.double(), reduction, u if reduction != "none" else up.double())
            assert out.shape == (x.shape if reduction == "none" else ())
            assert (out.double() - want).abs().max() <= 1e-5 * want.abs().max()
            assert (leaf.grad.double() - grad).abs().max() <= 1e-5 * grad.abs().max()
    cum = -target * torch.log_softmax(x, dim=1)
    assert (losses.cross_entropy_with_probs(x, target, reduction="none") - cum).abs().max() <= 1e-6
    assert abs(float(losses.cross_entropy_with_probs(x, target)) - float(cum.sum(1).mean())) <= 1e-6
    assert abs(float(losses.cross_entropy_with_probs(x, target, reduction="sum")) - float(cum.sum())) <= 1e-4
