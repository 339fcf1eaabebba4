"""Timing of the device skeleton stage (morig_amd/skeleton.py) on a batch of synthetic meshes: 64 torus meshes of 4 096 vertices with
24-48 joints each, voxelised as solid tubes. Reported, each as the median over repeated calls after warm-up, host clock around a device
synchronise (the stage ends in host reads, so host time is part of it): the ROOTNET forward, the PairCls forward, the pair geometry
(the public call, which uploads the voxel grids, and the kernel alone on resident grids), cost matrix + Prim, and the whole
``predict_skeleton``. The shader clock is sampled while the timed calls run (bench.py's ClockSampler). The reference's CPU time for ONE
such mesh (create_one_data + predict_skeleton, recorded by tools/make_skeleton_golden.py in tests/golden/skel_nets.npz) is printed
next to it. No GPU: this tool fails, it does not fall back.

    python tools/skeleton_bench.py [--meshes 64] [--n-side 64] [--repeats 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ClockSampler                          # noqa: E402
from morig_amd import skeleton, synth                   # noqa: E402
from morig_amd.models import bonenet, rootnet           # noqa: E402
from morig_amd.runtime import get_ops                   # noqa: E402

T = np.array([-0.55, -0.40, -0.55])
S = 1.1


def mesh_case(seed, n_joints):
    """-> (voxel grid of the mesh's solid tube, joints inside the tube)"""
    rng = np.random.default_rng([0x4D6F5269, seed])       # the first two draws of synth.make_mesh
    R = 0.35 * (1.0 + 0.1 * rng.uniform(-1, 1))
    r = 0.12 * (1.0 + 0.1 * rng.uniform(-1, 1))
    i = np.arange(88)
    X, Y, Z = np.meshgrid(*[T[a] + (i / 88.0) * S for a in range(3)], indexing="ij")
    grid = ((np.sqrt(X ** 2 + Z ** 2) - R) ** 2 + (Y - r) ** 2) <= (r + 0.012) ** 2
    vox = types.SimpleNamespace(data=grid, translate=list(T), scale=S, dims=[88, 88, 88])
    g = np.random.default_rng([0x6A6E74, seed])
    a = g.uniform(0, 2 * np.pi, size=n_joints)
    rho = R + g.uniform(-0.04, 0.04, size=n_joints)
    joints = np.stack([rho * np.cos(a), r + g.uniform(-0.04, 0.04, size=n_joints), rho * np.sin(a)], axis=1)
    return vox, joints


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--n-side", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "skeleton_bench needs the GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    seeds = [300 + i for i in range(args.meshes)]
    cases = [mesh_case(s, int(rng.integers(24, 49))) for s in seeds]
    voxes, joints = [c[0] for c in cases], [c[1] for c in cases]
    batch = synth.make_batch_device(seeds, dev, n_side=args.n_side, with_skin=False)
    root_net = synth.load_recipe(rootnet.ROOTNET().eval(), 701, mild=True).to(dev)
    bone_net = synth.load_recipe(bonenet.PairCls().eval(), 702, mild=True).to(dev)

    w, k = args.warmup, args.repeats
    sampler = ClockSampler(index=0).start()
    t_start = time.perf_counter()
    res = {}
    res["pair_attr_call"], data = timed(lambda: skeleton.make_data(batch, joints, voxes), w, k)
    ops = get_ops()
    grids, tf = skeleton.vox_arrays(voxes, dev)
    counts = [len(j) for j in joints]
    _, pptr, _, jp, pp, _ = skeleton._ptrs(counts, dev)
    j64 = torch.from_numpy(np.concatenate(joints, 0)).to(dev)
    j32 = j64.float()
    res["pair_attr_kernel"], _ = timed(lambda: ops.pair_attr(j64, j32, jp, pp, int(pptr[-1]), grids, tf), w, k)
    with torch.no_grad():
        res["rootnet_forward"], root_out = timed(lambda: root_net(data, shuffle=False), w, k)
        res["bonenet_forward"], pair_out = timed(lambda: bone_net(data, permute_joints=False), w, k)

        def cost_and_tree():
            cost, root = skeleton._connectivity_cost(pair_out[0], root_out[0], data.joints, None, data.joints_batch, data.outside_count)
            parent, _, status = skeleton._prim(cost, root)
            return parent.cpu(), root.cpu(), status.cpu()
        res["cost_and_mst"], _ = timed(cost_and_tree, w, k)
        res["predict_skeleton"], rigs = timed(lambda: skeleton.predict_skeleton(data, None, root_net, bone_net), w, k)
    t_end = time.perf_counter()
    clocks = sampler.stop().summary(t_start, t_end)
    ref = None
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", "skel_nets.npz"))
        ref = json.loads(bytes(z["meta"]).decode())["reference_cpu"]
    except Exception:
        pass
    stage_ms = res["pair_attr_call"]["median_ms"] + res["predict_skeleton"]["median_ms"]
    print(json.dumps(dict(meshes=args.meshes, vertices=int(batch.pos.shape[0]), joints_total=int(sum(counts)), pairs_total=int(pptr[-1]),
                          repeats=k, warmup=w, **res, stage_ms=round(stage_ms, 3), rigs=len(rigs),
                          note="stage_ms = pair_attr_call + predict_skeleton, the batch's counterpart of the reference's "
                               "create_one_data + predict_skeleton per mesh",
                          reference_cpu_one_mesh=ref, gpu=torch.cuda.get_device_name(0), clocks=clocks, date=time.strftime("%Y-%m-%d"))))


if __name__ == "__main__":
    main()
