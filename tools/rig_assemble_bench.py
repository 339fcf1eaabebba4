"""Timing of the rig assembly (morig_amd/rigging.py: assemble_rigs, i.e. assemble_skel_skin + remove_dup_joints for a batch) next to the
per-vertex host loop of tests/rigging_oracle.py (numpy, one vertex and one bone at a time: what a user had to run on the host before).
Rigs: random trees of about --bones bones; weights: up to five bones per vertex, normalised, on the device as one block (what
skin_weights leaves). The device time is wall time around a device-synchronised call after a warm-up, median over the repeats; it
includes everything the call does: the host plans, the table uploads, the kernels and the copy of the dense block to the host.
``plan_ms`` is the host plans alone, ``entries_ms`` the same call with the sparse form added. The host loop runs once. The results of the
two paths are compared bit for bit before anything is printed. One JSON line; there is NO threshold.

    python tools/rig_assemble_bench.py [--meshes 64] [--vertices 4096] [--bones 30] [--repeats 5]
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
import rigging_oracle as ro              # noqa: E402
from morig_amd import formats, rigging, skinning   # noqa: E402


def make_batch(n_meshes, n_vertices, n_bones, seed=0):
    rng = np.random.default_rng([0x52696741, seed])
    rigs, weights = [], []
    for _ in range(n_meshes):
        nb = 0
        while abs(nb - n_bones) > 4:                         # a tree of J joints has J - 1 bones plus one per leaf
            j = int(rng.integers(max(n_bones // 2, 2), n_bones + 1))
            rig = formats.Rig.from_arrays(rng.uniform(-0.5, 0.5, (j, 3)), [-1] + [int(rng.integers(0, i)) for i in range(1, j)], 0)
            nb = len(skinning.get_bones(rig)[0])
        w = np.zeros((n_vertices, nb))
        idx = np.argsort(rng.random((n_vertices, nb)), axis=1)[:, :5]
        np.put_along_axis(w, idx, rng.uniform(0.0, 1.0, idx.shape) * (rng.random(idx.shape) < 0.8), axis=1)
        rigs.append(rig)
        weights.append(w / (w.sum(axis=1, keepdims=True) + 1e-10))
    return rigs, weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--bones", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    rigs, weights = make_batch(a.meshes, a.vertices, a.bones)
    wide = max(w.shape[1] for w in weights)
    block = torch.zeros(a.meshes * a.vertices, wide, dtype=torch.float64, device="cuda")
    views = []
    for b, w in enumerate(weights):
        block[b * a.vertices:(b + 1) * a.vertices, :w.shape[1]] = torch.from_numpy(w).to("cuda")
        views.append(block[b * a.vertices:(b + 1) * a.vertices, :w.shape[1]])

    def timed(fn):
        fn()                                                 # warm-up
        out = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t)
        return res, out

    got, dev_s = timed(lambda: rigging.assemble_rigs(rigs, views))
    _, ent_s = timed(lambda: rigging.assemble_rigs(rigs, views, entries=True))
    _, plan_s = timed(lambda: [rigging.assembly_plan(r) for r in rigs])
    t = time.perf_counter()                                  # once: the V x B double loop in Python
    want = [ro.assemble_rig((r.names, np.asarray(r.hierarchy), r.pos, r.root_id), w) for r, w in zip(rigs, weights)]
    host_s = time.perf_counter() - t
    for g, w in zip(got, want):
        assert g.names == w["final"][0] and g.skins.tobytes() == w["skins"].tobytes() and g.pos.tobytes() == w["final"][2].tobytes()
    ms = lambda xs: round(statistics.median(xs) * 1e3, 3)
    print(json.dumps(dict(meshes=a.meshes, vertices=a.vertices, bones=[int(min(w.shape[1] for w in weights)), int(wide)],
                          device_ms=ms(dev_s), device_ms_all=[round(x * 1e3, 3) for x in dev_s], entries_ms=ms(ent_s), plan_ms=ms(plan_s),
                          host_loop_ms=round(host_s * 1e3, 3), bit_equal=True)))


if __name__ == "__main__":
    main()
