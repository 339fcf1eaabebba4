"""Timing of the device training losses (morig_amd/losses.py, csrc/losses.hip), forward + backward, at workload size:

  infonce    8 pairs of 4 096 vertices x 8 192 points, width 64, 2 048 correspondences per direction, tau 0.07
  multipos   8 meshes of 4 096 vertices, width 32: the six calls of a rig training step (5 keyframe views of an [N, 5, 32] tensor and the
             aggregate), draws made beforehand
  chamfer    the same meshes against about 30 joints each, one call
  log_ratio_frames   --skin-meshes (64) meshes of 4 096 vertices, T = 5, width 32, gt_skin width 48: the six log-ratio calls of a skin
             training step as one launch, draws made beforehand
  skin_ce_loss       the masked soft-label cross-entropy of the same step on those vertices, K = 5 (the torch side is handed vert_mask:
             its order rule is not a torch expression)

against the only thing the project offered before: the same formulas as plain torch operations with the per-mesh loop (tests/loss_oracle.py
and tests/skin_loss_oracle.py in float32, autograd backward) on the same device. Protocol (measuring guide): both versions alternate in ONE process, every shape is
warmed up, a timing is the host clock around a device synchronise of forward + backward, medians over --repeats; the spread is read from
the same version measured twice (the A/A ratio of the two halves of its samples). No GPU: this tool fails, it does not fall back.

    python tools/loss_bench.py [--repeats 30] [--warmup 5] [--pairs 8] [--skin-meshes 64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEP_MS = 77.0                                             # one training step without any loss


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(device_fn, torch_fn, warmup, repeats):
    for _ in range(warmup):
        device_fn(); torch_fn()
    a, b = [], []
    for _ in range(repeats):                               # alternate: drift of the clock hits both alike
        a.append(timed(device_fn)); b.append(timed(torch_fn))
    a, b = np.array(a), np.array(b)
    half = lambda x: float(np.median(x[0::2]) / np.median(x[1::2]))
    return dict(device_ms=round(float(np.median(a)), 3), torch_ms=round(float(np.median(b)), 3),
                ratio=round(float(np.median(b) / np.median(a)), 2), aa_device=round(half(a), 3), aa_torch=round(half(b), 3),
                share_of_step=round(float(np.median(a)) / STEP_MS, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--skin-meshes", type=int, default=64)
    args = ap.parse_args()
    import loss_oracle as lo
    import skin_loss_oracle as so
    from morig_amd import losses, native
    assert torch.cuda.is_available(), "loss_bench needs a GPU"
    native.get_ops()
    dev, B = "cuda", args.pairs
    g = torch.Generator().manual_seed(11)
    res = {}

    # ---- infoNCE
    nv, npt, r = 4096, 8192, 2048
    unit = lambda n, c: torch.nn.functional.normalize(torch.randn(n, c, generator=g), dim=1)
    vtx, pts = unit(B * nv, 64).to(dev).requires_grad_(True), unit(B * npt, 64).to(dev).requires_grad_(True)
    cv = torch.stack([torch.randint(0, nv, (B * r,), generator=g), torch.randint(0, npt, (B * r,), generator=g)], 1).to(dev)
    cp = torch.stack([torch.randint(0, npt, (B * r,), generator=g), torch.randint(0, nv, (B * r,), generator=g)], 1).to(dev)
    rep = lambda n: torch.arange(B).repeat_interleave(n).to(dev)
    nce = (vtx, pts, cv, cp, rep(nv), rep(npt), rep(r), rep(r))

    def clear(*ts):
        for t in ts:
            t.grad = None

    def nce_device():
        clear(vtx, pts)
        losses.infoNCE(*nce, 0.07, num_graphs=B).backward()

    def nce_torch():
        clear(vtx, pts)
        lo.infonce_loss(*nce, 0.07, B).backward()
    res["infonce"] = ab(nce_device, nce_torch, args.warmup, args.repeats)

    # ---- the six multi-positive calls and the chamfer of a rig step
    n = 4096
    motion = (1.5 * torch.nn.functional.normalize(torch.randn(B * n, 5, 32, generator=g), dim=2)).to(dev).requires_grad_(True)
    aggr = (1.5 * unit(B * n, 32)).to(dev).requires_grad_(True)
    batch = rep(n)
    skin = torch.nn.functional.one_hot(torch.randint(0, 6, (B * n,), generator=g), 6).float().to(dev)
    draws = [losses.draw_multi_pos_samples(skin, batch, num_graphs=B) for _ in range(6)]

    def mp_device():
        clear(motion, aggr)
        total = losses.multi_pos_infoNCE(aggr, skin, batch, samples=draws[5], num_graphs=B)
        for t in range(5):
            total = total + losses.multi_pos_infoNCE(motion[:, t, :], skin, batch, samples=draws[t], num_graphs=B)
        total.backward()

    def mp_torch():
        clear(motion, aggr)
        total = lo.multipos_loss(aggr, batch, *draws[5], B)
        for t in range(5):
            total = total + lo.multipos_loss(motion[:, t, :], batch, *draws[t], B)
        total.backward()
    res["multipos_x6"] = ab(mp_device, mp_torch, args.warmup, args.repeats)

    y = (torch.rand(B * n, 3, generator=g) - 0.5).to(dev).requires_grad_(True)
    counts = torch.randint(26, 35, (B,), generator=g)
    joints = (torch.rand(int(counts.sum()), 3, generator=g) - 0.5).to(dev)
    jb = torch.arange(B).repeat_interleave(counts).to(dev)

    def ch_device():
        clear(y)
        losses.chamfer_batched(y, batch, joints, jb, num_graphs=B).backward()

    def ch_torch():
        clear(y)
        lo.chamfer_loss(y, batch, joints, jb, B).backward()
    res["chamfer"] = ab(ch_device, ch_torch, args.warmup, args.repeats)

    # ---- the six log-ratio calls and the masked cross-entropy of a skin step
    Bs = args.skin_meshes
    sbatch = torch.arange(Bs).repeat_interleave(n).to(dev)
    smotion = torch.randn(Bs * n, 5, 32, generator=g).to(dev).requires_grad_(True)
    saggr = torch.randn(Bs * n, 32, generator=g).to(dev).requires_grad_(True)
    gt = torch.zeros(Bs * n, 48)
    gt.scatter_(1, torch.randint(0, 20, (Bs * n, 3), generator=g), torch.rand(Bs * n, 3, generator=g) + 0.05)
    gt = (gt / gt.sum(1, keepdim=True)).to(dev)
    sdraws = losses.draw_log_ratio_samples(sbatch, n_sets=6, num_graphs=Bs)

    def lr_device():
        clear(smotion, saggr)
        losses.log_ratio_frames(smotion, saggr, gt, sbatch, samples=sdraws, num_graphs=Bs).backward()

    def lr_torch():
        clear(smotion, saggr)
        total = so.logratio_loss(saggr, gt, sbatch, sdraws[5], Bs)
        for t in range(5):
            total = total + so.logratio_loss(smotion[:, t, :], gt, sbatch, sdraws[t], Bs)
        total.backward()
    res["log_ratio_frames"] = ab(lr_device, lr_torch, args.warmup, args.repeats)

    logits = torch.randn(Bs * n, 5, generator=g).to(dev).requires_grad_(True)
    label = torch.rand(Bs * n, 5, generator=g) * (torch.rand(Bs * n, 5, generator=g) < 0.6)
    label = (label / (label.sum(1, keepdim=True) + 1e-8)).to(dev)
    lmask = (torch.rand(Bs * n, 5, generator=g) < 0.85).long().to(dev)
    vm = losses.skin_ce_loss(logits.detach(), label, lmask, nearest_bone=5, return_vert_mask=True)[1] > 0

    def ce_device():
        clear(logits)
        losses.skin_ce_loss(logits, label, lmask, nearest_bone=5).backward()

    def ce_torch():
        clear(logits)
        so.skin_ce_loss(logits, label, lmask, 5, vm).backward()
    res["skin_ce_loss"] = ab(ce_device, ce_torch, args.warmup, args.repeats)
    losses.check_inputs()
    for k, v in res.items():
        print(f"{k:16s} device {v['device_ms']:8.3f} ms   torch loop {v['torch_ms']:8.3f} ms   x{v['ratio']:<6} A/A device {v['aa_device']} torch "
              f"{v['aa_torch']}   {100 * v['share_of_step']:.2f} % of the {STEP_MS:.0f} ms step")
    print(json.dumps(dict(tool="loss_bench", pairs=B, skin_meshes=Bs, repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
