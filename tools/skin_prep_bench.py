"""Timing of the device skinning path (morig_amd/skinning.py) on a batch of synthetic meshes: volumetric geodesic distances of every
(mesh, bone), bind rows + SkinNet inputs, and the post-processing of seeded logits (train_skin order), each timed with CUDA events
after warm-up. Meshes: synth torus meshes voxelised as solid tubes, skeletons of 20-40 bones along the tube's centre circle. The
reference's CPU time per mesh (calc_volumetric_geodesic with its 8-process pool, recorded by tools/make_skin_golden.py in the
fixtures) is printed next to it.

    python tools/skin_prep_bench.py [--meshes 64] [--n-side 32] [--repeats 3]
"""
import argparse
import glob
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morig_amd import skinning, synth   # noqa: E402

T = np.array([-0.55, -0.40, -0.55])
S = 1.1


def mesh_case(seed, n_side, n_bones):
    m = synth.make_mesh(seed, n_side=n_side, with_skin=False)
    rng = np.random.default_rng([0x4D6F5269, seed])
    R = 0.35 * (1.0 + 0.1 * rng.uniform(-1, 1))
    r = 0.12 * (1.0 + 0.1 * rng.uniform(-1, 1))
    i = np.arange(88)
    X, Y, Z = np.meshgrid(*[T[a] + (i / 88.0) * S for a in range(3)], indexing="ij")
    grid = ((np.sqrt(X ** 2 + Z ** 2) - R) ** 2 + (Y - r) ** 2) <= (r + 0.012) ** 2
    vox = types.SimpleNamespace(data=grid, translate=list(T), scale=S, dims=[88, 88, 88])
    # root at 0 deg, two chains around the circle: n_bones = l1 + l2 + 2 leaf bones
    l1 = (n_bones - 2) // 2
    l2 = n_bones - 2 - l1
    names, pos, hier = ["j0"], [[R, r, 0.0]], [-1]
    for sgn, L in ((1, l1), (-1, l2)):
        prev = 0
        for t in range(1, L + 1):
            a = np.deg2rad(sgn * 170.0 * t / L)
            names.append(f"j{len(names)}")
            pos.append([R * np.cos(a), r, R * np.sin(a)])
            hier.append(prev)
            prev = len(names) - 1
    rig = types.SimpleNamespace(names=names, pos=np.array(pos), hierarchy=np.array(hier), root_id=0)
    bones, bnames, leaf = skinning.get_bones(rig)
    assert len(bones) == n_bones
    return m, vox, rig, bones, bnames, leaf


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--n-side", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    cases = [mesh_case(100 + i, args.n_side, int(rng.integers(20, 41))) for i in range(args.meshes)]
    batch = synth.collate([c[0] for c in cases]).to(dev)
    pos = batch.pos.double().contiguous()
    voxes = [c[1] for c in cases]
    bones = [c[3] for c in cases]
    sj = [skinning.start_joints(c[2], c[4]) for c in cases]
    leaf = [c[5] for c in cases]

    ms_dist, dists = timed(lambda: skinning.volumetric_geodesic_batched(pos, batch.batch, voxes, bones), args.repeats)
    ms_bind, o = timed(lambda: skinning.skin_bind_batched(dists, bones, leaf, sj, None, 20), args.repeats)
    logits = torch.from_numpy(np.random.default_rng(2).normal(0, 2, size=(pos.shape[0], 20)).astype(np.float32)).to(dev)
    nbs = [len(b) for b in bones]
    ms_post, _ = timed(lambda: skinning.skin_weights(logits, o["skin_nn"], o["loss_mask"], batch.tpl_edge_index, batch.batch, nbs),
                       args.repeats)
    ref = []
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "skin_*.npz"))):
        z = np.load(f)
        meta = json.loads(bytes(z["meta"]).decode())
        ref.append(dict(case=meta["case"], bones=len(meta["bone_names"]), vertices=int(z["pos"].shape[0]),
                        cpu_seconds=round(meta["ref_seconds"], 3)))
    print(json.dumps(dict(meshes=args.meshes, vertices=int(pos.shape[0]), bones_total=int(sum(nbs)), ms_distances=round(ms_dist, 3),
                          ms_bind=round(ms_bind, 3), ms_post=round(ms_post, 3), ms_total=round(ms_dist + ms_bind + ms_post, 3),
                          gpu=torch.cuda.get_device_name(0), reference_cpu_per_mesh=ref)))


if __name__ == "__main__":
    main()
