"""Timing of the device scoring path (morig_amd/metrics.py: evaluate_rigs with predicted rigs, i.e. CD-J2J, the matching, IoU / precision
/ recall, CD-J2B and CD-B2B) on a batch of synthetic rigs, next to the host loop of tests/metrics_oracle.py (numpy + scipy, one mesh at a
time: what a user had to run before). Rigs: random trees of --joints +- 8 joints in the unit box (coordinates on the 1 / 256 grid), the
prediction a perturbed copy with a few joints dropped or added. The device time is wall time around a device-synchronised call after a
warm-up, median over the repeats (the host loop runs once); it includes the host work of the call (listing the bones, the uploads, the one host read). The results
of the two paths are compared before anything is printed. One JSON line; there is NO threshold: the point of the stage is that scoring
stays on the device, and no speed is claimed until this has been run on one.

    python tools/metrics_bench.py [--meshes 64] [--joints 16] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_oracle as mo              # noqa: E402
from morig_amd import formats, metrics   # noqa: E402


def tree(rng, pos):
    return formats.Rig.from_arrays(pos, [-1] + [int(rng.integers(0, j)) for j in range(1, len(pos))], 0)


def make_batch(n_meshes, joints, seed=0):
    rng = np.random.default_rng([0x4D657472, seed])
    gt_rigs, pred_rigs, fss = [], [], []
    for _ in range(n_meshes):
        n_gt = int(rng.integers(max(joints - 8, 2), joints + 9))
        gt = rng.integers(0, 257, (n_gt, 3)) / 256.0
        keep = rng.permutation(n_gt)[:max(n_gt - int(rng.integers(0, 4)), 2)]
        pred = np.concatenate([gt[keep] + np.round(rng.normal(0.0, 0.03, (len(keep), 3)) * 256) / 256, rng.integers(0, 257, (int(rng.integers(0, 4)), 3)) / 256.0])
        gt_rigs.append(tree(rng, gt))
        pred_rigs.append(tree(rng, pred))
        fss.append(rng.uniform(0.02, 0.08, n_gt))
    return gt_rigs, pred_rigs, fss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--joints", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    gt_rigs, pred_rigs, fss = make_batch(a.meshes, a.joints)
    preds = [r.pos for r in pred_rigs]
    pred, ptr = np.concatenate(preds), np.concatenate([[0], np.cumsum([len(p) for p in preds])])

    def device():
        res = metrics.evaluate_rigs(pred, ptr, gt_rigs, fss, pred_rigs=pred_rigs, device="cuda")
        torch.cuda.synchronize()
        return res

    res = device()                                           # warm-up
    dev_s = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        res = device()
        dev_s.append(time.perf_counter() - t)
    t = time.perf_counter()                                  # once: tens of seconds at the defaults
    want = mo.evaluate(preds, gt_rigs, fss, pred_rigs)
    host_s = [time.perf_counter() - t]
    worst = max(abs(float(res["mean"][k]) - want["mean"][k]) for k in want["mean"])
    assert worst <= 1e-11 and metrics.format_report(res) == mo.format_report(want), worst
    n_samples = int(sum(len(mo.sample_skel(r)) for r in gt_rigs + pred_rigs))
    print(json.dumps(dict(meshes=a.meshes, joints=a.joints, bone_samples=n_samples, device_ms=round(statistics.median(dev_s) * 1e3, 3),
                          device_ms_all=[round(x * 1e3, 3) for x in dev_s], host_loop_ms=round(statistics.median(host_s) * 1e3, 3),
                          max_mean_diff=worst)))


if __name__ == "__main__":
    main()
