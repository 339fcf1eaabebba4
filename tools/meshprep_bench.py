"""Timing of the mesh front end (morig_amd/meshprep.py) per stage for a batch: --meshes closed meshes of --vertices vertices and
2 V - 4 faces (the convex hull of random points on a sphere, then every vertex moved radially: 4096 vertices give 8188 faces), already on
the device. Each stage is timed between two device events around the whole public call after a warm-up pass, median over the repeats:
that is everything the call does -- the concatenation of the inputs, the plumbing in torch (the key sort of tpl_edges, the index check),
the host reads (frames, sizes, status, the grids coming back to the host in voxelize) and the kernels. ``*_kernel_ms`` are the library's
own event pairs around the voxeliser's two launches. The reference's get_tpl_edges seconds are those recorded in
tests/golden/meshprep_tpl_edges.npz for ONE mesh of 4096 vertices. One JSON line; there is NO threshold.

    python tools/meshprep_bench.py [--meshes 64] [--vertices 4096] [--dims 88] [--samples 4000] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
from scipy.spatial import ConvexHull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morig_amd import meshprep, native        # noqa: E402


def make_batch(n_meshes, V, seed=0):
    rng = np.random.default_rng([0x4D657368, seed])
    verts, faces = [], []
    for _ in range(n_meshes):
        p = rng.normal(size=(V, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        f = ConvexHull(p).simplices
        bump = 1.0 + 0.25 * np.sin(3.0 * p[:, :1]) * np.cos(2.0 * p[:, 1:2])
        verts.append(p * bump * [0.3, 0.5, 0.2] + rng.normal(size=3))
        faces.append(f.astype(np.int32))
    return verts, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--dims", type=int, default=88)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    verts, faces = make_batch(a.meshes, a.vertices)
    dv, df = [torch.from_numpy(v).cuda() for v in verts], [torch.from_numpy(f).cuda() for f in faces]
    nv = [len(v) for v in verts]

    def timed(fn):
        fn()                                                 # warm-up
        out = []
        for _ in range(a.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            res = fn()
            stop.record()
            torch.cuda.synchronize()
            out.append(start.elapsed_time(stop))
        return res, round(statistics.median(out), 3)

    normed, normalize_ms = timed(lambda: meshprep.normalize(dv))
    nverts = [v for v, _, _ in normed]
    edges, edges_ms = timed(lambda: meshprep.tpl_edges(df, nv))
    _, sample_ms = timed(lambda: meshprep.sample_surface(nverts, df, n_samples=a.samples))
    native.prof_enable(True)
    native.prof_reset()
    (vox, info), voxel_ms = timed(lambda: meshprep.voxelize(nverts, df, dims=a.dims, return_info=True))
    prof = native.prof_collect()
    native.prof_enable(False)
    calls = a.repeats + 1
    kernel = lambda name: round(prof[name]["ms"] / calls, 3) if name in prof else None
    meta = json.loads(bytes(np.load(os.path.join(ROOT, "tests", "golden", "meshprep_tpl_edges.npz"))["meta"]).decode())
    print(json.dumps(dict(meshes=a.meshes, vertices=a.vertices, faces=int(faces[0].shape[0]), dims=a.dims, samples=a.samples,
                          normalize_ms=normalize_ms, tpl_edges_ms=edges_ms, edges_per_mesh=int(edges[0].shape[1]), sample_surface_ms=sample_ms,
                          voxelize_ms=voxel_ms, voxel_surface_kernel_ms=kernel("voxel_surface"), voxel_fill_kernel_ms=kernel("voxel_fill"),
                          fill_sweeps=[int(info[:, 1].min()), int(info[:, 1].max())], solid_share=round(float(np.mean([v.data.mean() for v in vox])), 4),
                          reference_get_tpl_edges_s_per_mesh=round(meta["ref_seconds_torus64"], 3))))


if __name__ == "__main__":
    main()
