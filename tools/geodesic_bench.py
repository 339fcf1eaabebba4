"""Timing of the device geodesic path (morig_amd/geodesic.py) on a batch of synthetic meshes, per stage: the surface geodesic of every
mesh (5-NN graph, all-pairs shortest paths, the V x V gather), the visibility of every (vertex, bone) by ray casting against the
mesh's own triangles, the vertex-to-bone matrix, and the bind rows. Meshes: synth torus meshes (V = n_side^2), S random samples on the
analytic torus with analytic normals, skeletons of ~30 bones along the tube's centre circle. Each stage is timed with device events
after a warm-up run, device-synchronised, median over the repeats; the batch runs in chunks of --chunk meshes (the S x S matrices of
a chunk are dropped after its gather). The reference's CPU time per mesh (calc_surface_geodesic at S = 4000, V = 1024, recorded by
tools/make_geodesic_golden.py in the geo_4000 fixture) is printed next to it. One JSON line.

    python tools/geodesic_bench.py [--meshes 64] [--samples 4000] [--n-side 64] [--repeats 5] [--chunk 8]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morig_amd import geodesic, synth   # noqa: E402


def torus_params(seed):
    rng = np.random.default_rng([0x4D6F5269, seed])
    return 0.35 * (1.0 + 0.1 * rng.uniform(-1, 1)), 0.12 * (1.0 + 0.1 * rng.uniform(-1, 1))


def mesh_case(seed, n_side, n_samples, n_bones):
    R, r = torus_params(seed)
    pos = synth.make_mesh(seed, n_side=n_side, with_skin=False, geo="none").pos.numpy().astype(np.float64)
    rng = np.random.default_rng([0x47656F42, seed])
    u, v = rng.uniform(0, 2 * np.pi, n_samples), rng.uniform(0, 2 * np.pi, n_samples)
    pts = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v) + r, (R + r * np.cos(v)) * np.sin(u)], 1)
    nrm = np.stack([np.cos(v) * np.cos(u), np.sin(v), np.cos(v) * np.sin(u)], 1)
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    a, b, c, d = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0).astype(np.int32)
    # two chains around the centre circle from 0 deg and a zero-length leaf bone at either end
    l1 = (n_bones - 2) // 2
    bones, leaf = [], []
    for sgn, L in ((1, l1), (-1, n_bones - 2 - l1)):
        ang = [np.deg2rad(sgn * 170.0 * t / L) for t in range(L + 1)]
        jt = [np.array([R * np.cos(x), r, R * np.sin(x)]) for x in ang]
        for t in range(L):
            bones.append(np.concatenate([jt[t], jt[t + 1]]))
            leaf.append(False)
        bones.append(np.concatenate([jt[-1], jt[-1]]))
        leaf.append(True)
    return dict(pos=pos, pts=pts, normals=nrm, faces=faces, bones=np.stack(bones), leaf=leaf)


class Clock:
    def __init__(self):
        self.ms = {}

    def run(self, key, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        self.ms[key] = self.ms.get(key, 0.0) + a.elapsed_time(b)
        return out


def one_pass(cases, dev, chunk, stats):
    clk = Clock()
    for c0 in range(0, len(cases), chunk):
        cs = cases[c0:c0 + chunk]
        pts = torch.cat([c["pts"] for c in cs])
        nrm = torch.cat([c["normals"] for c in cs])
        verts = torch.cat([c["pos"] for c in cs])
        p_ptr = np.concatenate([[0], np.cumsum([len(c["pts"]) for c in cs])])
        v_ptr = np.concatenate([[0], np.cumsum([len(c["pos"]) for c in cs])])
        mats, st = clk.run("paths", lambda: geodesic.surface_geodesic_samples(pts, nrm, ptr=p_ptr, return_stats=True))
        for k in ("total_sweeps", "jobs", "entries"):
            stats[k] = stats.get(k, 0) + st[k]
        stats["max_sweeps"] = max(stats.get("max_sweeps", 0), st["max_sweeps"])
        stats["nsrc"] = st["nsrc"]

        def gather():
            nn = geodesic.nearest_sample(verts, pts, v_ptr, p_ptr).long()
            return [m[nn[int(v_ptr[i]):int(v_ptr[i + 1])]][:, nn[int(v_ptr[i]):int(v_ptr[i + 1])]] for i, m in enumerate(mats)]
        sgs = clk.run("gather", gather)
        del mats
        pos, bones = [c["pos"] for c in cs], [c["bones"] for c in cs]
        vis = clk.run("visibility", lambda: geodesic.bone_visibility_batched(pos, bones, pos, [c["faces"] for c in cs]))
        geo = clk.run("bone_matrix", lambda: geodesic.bone_geodesic_matrix_batched(pos, bones, sgs, vis))
        clk.run("bind", lambda: geodesic.skin_inputs_joint2rig_batched(geo, bones, [c["leaf"] for c in cs], 5))
        del sgs
    return clk.ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--n-side", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    cases = [mesh_case(200 + i, args.n_side, args.samples, int(rng.integers(26, 35))) for i in range(args.meshes)]
    for c in cases:
        for k in ("pos", "pts", "normals", "bones"):
            c[k] = torch.from_numpy(c[k]).to(dev)
        c["faces"] = torch.from_numpy(c["faces"]).to(dev)
    one_pass(cases, dev, args.chunk, {})                    # warm-up
    runs, stats = [], {}
    for _ in range(args.repeats):
        stats = {}
        runs.append(one_pass(cases, dev, args.chunk, stats))
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    stage1 = med["paths"] + med["gather"]
    # relaxations d[v] = min(d[v], d[u] + w): per job and sweep, every directed adjacency entry of its mesh for each of its nsrc sources
    relax = stats["total_sweeps"] * (stats["entries"] / args.meshes) * stats["nsrc"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "geo_4000.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    print(json.dumps(dict(meshes=args.meshes, samples=args.samples, vertices=args.n_side ** 2, bones_total=int(sum(len(c["bones"]) for c in cases)),
                          ms={k: round(v, 3) for k, v in med.items()}, ms_total=round(sum(med.values()), 3),
                          ms_surface_geodesic_per_mesh=round(stage1 / args.meshes, 3), sweeps_max=stats["max_sweeps"],
                          sweeps_mean=round(stats["total_sweeps"] / stats["jobs"], 2), adjacency_entries_per_mesh=round(stats["entries"] / args.meshes, 1),
                          relaxations=relax, relaxations_per_second=relax / (med["paths"] * 1e-3), gpu=torch.cuda.get_device_name(0),
                          reference_cpu_seconds_per_mesh=dict(case=meta["case"], S=meta["S"], V=meta["V"], seconds=round(meta["ref_seconds"], 3)))))


if __name__ == "__main__":
    main()
