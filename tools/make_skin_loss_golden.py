"""Fixtures of the skin-training losses (tests/golden/loss_logratio_*.npz, loss_skin_ce.npz), made by the reference's own functions:
log_ratio_loss and cross_entropy_with_probs of models/customized_losses.py, imported from where the reference lies as
tools/make_loss_golden.py does. Nothing of the reference is written into the repository: only inputs, recorded draws and results.

  loss_logratio_all50       one mesh of exactly 50 vertices (every vertex is sampled), feature width 32, gt_skin width 48
  loss_logratio_ragged      meshes of 50, 67 and 130 vertices at 32 / 48; tests/test_gpu_skin_losses.py also runs it as the [:, t, :] view of
                            an [N, 5, 32] tensor (meta "keyframe_view"; the generator checks that the reference returns the same loss there)
  loss_logratio_d4          meshes of 50 and 61 vertices at feature width 4, gt_skin width 4
  loss_logratio_coincident  one mesh of 50 vertices; feature rows 3 and 17 are identical, gt_skin rows 5 and 9 are identical
  loss_skin_ce              384 rows of the masked soft-label cross-entropy of the skin training step (K = 5 of 6 stored columns), and a dozen
                            rows whose vert_mask depends on the order of the sums, with the answer of the sequential float32 rule

The reference's log_ratio_loss moves an index tensor with ``.cuda()``: ``torch.Tensor.cuda`` is the identity while it runs here, and
``np.random.choice`` is wrapped to record its draws. The masking arithmetic around cross_entropy_with_probs lives inside the reference's
training loop, not in a function; it is stated here from its formula (``masked_ce``) around the reference's own cross_entropy_with_probs.

Per case the deviation of the reference's float32 result from tests/skin_loss_oracle.py (float64, closed-form gradients) is stored:
relative for the loss, relative to max |grad| for the gradient. The device is held to ten times these.

Conditions enforced here (the run fails rather than write a fixture that misses one) and re-checked by tests/test_skin_loss_oracle.py:
every mesh has at least 50 vertices; every off-diagonal feature distance among a mesh's samples is at least 1e-3 (``coincident``: but
for its one identical pair); every CE row gives the same vert_mask under all 105 x 105 association orders of its two sums (rows that do
not are redrawn, the number is stored); the CE rows cover 0 .. 5 non-zero labels, both outcomes of vert_mask on non-empty rows, and
masked-out columns. No file is larger than the largest loss fixture there was (loss_multipos.npz).

Run from the repository root:  python tools/make_skin_loss_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_loss_golden as mlg                                                 # noqa: E402  (reference, rel, rel_max)
import make_skin_golden as msg                                                 # noqa: E402  (save)
import skin_loss_oracle as so                                                  # noqa: E402

N_SAMPLE, MIN_DIST = 50, 1e-3
MAX_BYTES = os.path.getsize(os.path.join(msg.OUT, "loss_multipos.npz"))
CE_ROWS, CE_K, CE_COLS, CE_KNOWN = 384, 5, 6, 12
LOGRATIO_CASES = {
    "all50": dict(sizes=[50], D=32, W=48),
    "ragged": dict(sizes=[50, 67, 130], D=32, W=48),
    "d4": dict(sizes=[50, 61], D=4, W=4),
    "coincident": dict(sizes=[50], D=32, W=48),
}
COINCIDENT = dict(feature_rows=[3, 17], skin_rows=[5, 9])
KEYFRAME_VIEW = dict(T=5, t=2, seed=1)


def save(name, meta, **arrs):
    msg.save(name, meta, **arrs)
    size = os.path.getsize(os.path.join(msg.OUT, name + ".npz"))
    assert size <= MAX_BYTES, (name, size, MAX_BYTES)


# ------------------------------------------------------------------------------------------------------------------- log-ratio
def skin_rows(rng, n, width):
    """skin weights as the dataset stores them: a few bones per vertex, rows summing to 1, zero padding"""
    bones = min(width, 20)
    skin = np.zeros((n, width), dtype=np.float32)
    for v in range(n):
        k = int(rng.integers(1, min(4, bones) + 1))
        cols = rng.choice(bones, k, replace=False)
        w = rng.uniform(0.05, 1.0, k)
        skin[v, cols] = (w / w.sum()).astype(np.float32)
    return skin


def run_log_ratio(ref, feat, gt, batch):
    """the reference's log_ratio_loss on float32 CPU tensors -> (loss, the draws [B, 50])"""
    draws = []
    real_choice, real_cuda = np.random.choice, torch.Tensor.cuda

    def choice(*a, **kw):
        r = real_choice(*a, **kw)
        draws.append(np.asarray(r).copy())
        return r
    np.random.choice, torch.Tensor.cuda = choice, lambda self, *a, **kw: self
    try:
        loss = ref.log_ratio_loss(feat, gt, batch)
    finally:
        np.random.choice, torch.Tensor.cuda = real_choice, real_cuda
    return loss, np.stack(draws)


def logratio_case(ref, rng, name, sizes, D, W):
    n = sum(sizes)
    feat = (rng.standard_normal((n, D)) * 0.5).astype(np.float32)
    gt = skin_rows(rng, n, W)
    if name == "coincident":
        (i, j), (k, l) = COINCIDENT["feature_rows"], COINCIDENT["skin_rows"]
        feat[j], gt[l] = feat[i], gt[k]
    batch = np.repeat(np.arange(len(sizes)), sizes)
    f = torch.from_numpy(feat).requires_grad_(True)
    np.random.seed(11)
    loss, samples = run_log_ratio(ref, f, torch.from_numpy(gt), torch.from_numpy(batch))
    loss.backward()
    assert np.isfinite(loss.item()) and np.isfinite(f.grad.numpy()).all()
    check_logratio_conditions(name, feat, batch, samples)
    tl = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64))
    want = so.logratio(f.detach().double(), torch.from_numpy(gt).double(), tl(batch), tl(samples), len(sizes))
    dev = dict(dev_loss=mlg.rel(loss, want[0]), dev_grad=mlg.rel_max(f.grad.numpy(), want[1].numpy()))
    meta = dict(sizes=sizes, D=D, W=W, n_sample=N_SAMPLE, deviations=dev)
    if name == "coincident":
        meta["coincident"] = COINCIDENT
    if name == "ragged":                                   # the same rows as a keyframe view: the reference returns the same loss
        stack = torch.randn(n, KEYFRAME_VIEW["T"], D, generator=torch.Generator().manual_seed(KEYFRAME_VIEW["seed"]))
        stack[:, KEYFRAME_VIEW["t"], :] = torch.from_numpy(feat)
        stack.requires_grad_(True)
        np.random.seed(11)
        loss_v, samples_v = run_log_ratio(ref, stack[:, KEYFRAME_VIEW["t"], :], torch.from_numpy(gt), torch.from_numpy(batch))
        loss_v.backward()
        assert np.array_equal(samples_v, samples) and loss_v.item() == loss.item()
        view_grad = stack.grad.numpy()                     # (autograd sums the view's gradient in another order: not the same bits)
        assert mlg.rel_max(view_grad[:, KEYFRAME_VIEW["t"], :], f.grad.numpy()) <= 1e-6 and (np.delete(view_grad, KEYFRAME_VIEW["t"], 1) == 0).all()
        meta["keyframe_view"] = KEYFRAME_VIEW
    print(f"  {name}: loss {loss.item():.6f}  deviations {dev}")
    save(f"loss_logratio_{name}", meta, feat=feat, gt=gt, batch=batch.astype(np.uint16), samples=samples.astype(np.uint16),
         loss=np.float32(loss.item()), grad=f.grad.numpy())


def check_logratio_conditions(name, feat, batch, samples):
    for b in range(int(batch.max()) + 1):
        rows = np.nonzero(batch == b)[0]
        assert len(rows) >= N_SAMPLE and len(set(samples[b].tolist())) == N_SAMPLE
        d = so.sq_dist(torch.from_numpy(feat[rows[samples[b]]]).double()).numpy()
        d[np.diag_indices(N_SAMPLE)] = np.inf
        close = np.argwhere(d < MIN_DIST)
        if name == "coincident":
            i, j = (int(np.nonzero(samples[b] == r)[0][0]) for r in COINCIDENT["feature_rows"])
            assert sorted(map(tuple, close.tolist())) == sorted([(i, j), (j, i)]) and d[i, j] == 0.0
        else:
            assert len(close) == 0, (name, b, close)


# ------------------------------------------------------------------------------------------------------------------- masked CE
def ce_rows(rng, n):
    """label [n, 6] float32 and mask [n, 6] int64: 0 .. 5 weights among the first five columns, the rest of a vertex's weight in the sixth
    (a bone outside the picked five); every column masked out with probability 0.15"""
    label = np.zeros((n, CE_COLS), dtype=np.float32)
    for v in range(n):
        k = int(rng.integers(0, CE_K + 1))
        cols = rng.choice(CE_K, k, replace=False)
        w = rng.uniform(0.02, 1.0, k + 1)
        w = w / w.sum()
        if rng.random() < 0.5:                              # all of the weight inside the picked bones
            w[:k] = w[:k] / max(w[:k].sum(), 1e-30)
            w[k] = 0.0
        label[v, cols] = w[:k].astype(np.float32)
        label[v, CE_K] = np.float32(w[k])
    mask = (rng.random((n, CE_COLS)) >= 0.15).astype(np.int64)
    return label, mask


def order_independent(label, mask):
    m = so.vert_mask_orders(label, mask.astype(np.float32), CE_K)
    return (m == m[0, 0]).all(axis=(0, 1))


def masked_ce(ref, x, label, mask):
    """the skin loss of the training step around the reference's cross_entropy_with_probs -> (loss, vert_mask)"""
    m = mask.float()[:, :CE_K]
    g = label[:, :CE_K] * m
    q = g / (g.abs().sum(dim=1, keepdim=True) + 1e-8)
    v = ((q.sum(dim=1) - 1.0).abs() < 1e-8).float()
    w = m * v[:, None]
    return (ref.cross_entropy_with_probs(x, q, reduction="none") * w).sum() / w.sum(), v


def skin_ce_case(ref, rng):
    label, mask = ce_rows(rng, CE_ROWS)
    redrawn, known_l, known_m = 0, [], []
    while True:
        bad = np.nonzero(~order_independent(label, mask))[0]
        if len(bad) == 0:
            break
        known_l.append(label[bad].copy()); known_m.append(mask[bad].copy())
        redrawn += len(bad)
        label[bad], mask[bad] = ce_rows(rng, len(bad))
    nz = ((label[:, :CE_K] * mask[:, :CE_K]) != 0).sum(1)
    vm = so.vert_mask_sequential(label, mask.astype(np.float32), CE_K)
    assert set(nz.tolist()) == set(range(CE_K + 1)), "a count of non-zero labels is missing"
    assert (vm & (nz > 0)).any() and (~vm & (nz > 0)).any(), "both outcomes of vert_mask on non-empty rows"
    assert (mask[:, :CE_K] == 0).any() and not vm[nz == 0].any()
    x = torch.from_numpy((rng.standard_normal((CE_ROWS, CE_K)) * 2.0).astype(np.float32)).requires_grad_(True)
    loss, v = masked_ce(ref, x, torch.from_numpy(label), torch.from_numpy(mask))
    loss.backward()
    assert np.array_equal(v.numpy() > 0, vm), "torch and the sequential rule disagree on an order-independent row"
    want = so.skin_ce(x.detach().double(), torch.from_numpy(label).double(), torch.from_numpy(mask), CE_K, torch.from_numpy(vm))
    dev = dict(dev_loss=mlg.rel(loss, want[0]), dev_grad=mlg.rel_max(x.grad.numpy(), want[1].numpy()))
    # a dozen of the rows that were redrawn, both answers among them, with what the sequential float32 rule gives
    kl, km = np.concatenate(known_l), np.concatenate(known_m)
    ka = so.vert_mask_sequential(kl, km.astype(np.float32), CE_K)
    pick = np.concatenate([np.nonzero(ka)[0][:CE_KNOWN // 2], np.nonzero(~ka)[0][:CE_KNOWN // 2]])
    assert len(pick) == CE_KNOWN, "too few order-dependent rows of one of the two answers"
    kl, km, ka = kl[pick], km[pick], ka[pick]
    assert not order_independent(kl, km).any()
    print(f"  skin_ce: loss {loss.item():.6f}  deviations {dev}  redrawn {redrawn}  masked in {int(vm.sum())} of {CE_ROWS}")
    save("loss_skin_ce", dict(K=CE_K, deviations=dev, redrawn=redrawn, known_rows=CE_KNOWN), x=x.detach().numpy(), label=label,
         mask=mask.astype(np.uint8), vert_mask=vm, loss=np.float32(loss.item()), grad=x.grad.numpy(), known_label=kl,
         known_mask=km.astype(np.uint8), known_vert_mask=ka)


def main():
    ref = mlg.reference()
    rng = np.random.default_rng(20241018)
    print("log-ratio")
    for name, par in LOGRATIO_CASES.items():
        logratio_case(ref, rng, name, **par)
    print("masked soft-label cross-entropy")
    skin_ce_case(ref, rng)


if __name__ == "__main__":
    main()
