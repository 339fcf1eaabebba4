"""Timing of the rig-free tracker (morig_amd/piecewise.py: kernel_kmeans and piecewise_ransac for a batch) next to the numpy restatement
of tests/piecewise_oracle.py on the host (the per-segment, 100-iteration loop a user had to run before). Meshes: --vertices points in
blobs, unit embeddings of width --dim that follow the blobs, every segment moved rigidly with 1 % noise and a visibility mask that keeps
about 80 % of the vertices. The segments of the RANSAC stage are the k-means labels. The device time is wall time around a
device-synchronised call after a warm-up, median over the repeats; it includes everything the call does: the concatenation and upload of
the inputs, the plumbing in torch, the host read of the handle counts, the upload of the samples and the kernels. ``draw_ms`` is the host
time of the sample draws alone (numpy's legacy generator, one permutation per hypothesis), which a caller may do ahead. The host oracle
runs on the first --host-meshes meshes only and is reported per mesh. Labels, inlier counts and chosen hypotheses of the two paths are
compared first. One JSON line; there is NO threshold.

    python tools/piecewise_bench.py [--meshes 64] [--vertices 4096] [--clusters 20] [--dim 64] [--segments 30] [--repeats 5] [--host-meshes 1]
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
import piecewise_oracle as po             # noqa: E402
from morig_amd import piecewise           # noqa: E402


def make_batch(n_meshes, V, D, n_blobs, seed=0):
    rng = np.random.default_rng([0x50696563, seed])
    X, verts = [], []
    for _ in range(n_meshes):
        blob = rng.integers(0, n_blobs, V)
        verts.append(rng.uniform(-1, 1, (n_blobs, 3))[blob] + rng.normal(size=(V, 3)) * 0.12)
        proto = rng.normal(size=(n_blobs, D))
        x = proto[blob] + rng.normal(size=(V, D)) * 0.4
        X.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    return X, verts, rng


def move_segments(rng, verts, seg):
    out = verts.copy()
    for l in np.unique(seg):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        a = rng.uniform(0.1, 0.5)
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        m = seg == l
        out[m] = verts[m] @ R.T + rng.uniform(-0.1, 0.1, 3) + rng.normal(size=(int(m.sum()), 3)) * 0.01
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--segments", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-meshes", type=int, default=1)
    a = ap.parse_args()
    X, verts, rng = make_batch(a.meshes, a.vertices, a.dim, a.clusters)
    first = [int(rng.integers(0, a.vertices)) for _ in range(a.meshes)]

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

    dX, dv = [torch.from_numpy(x).cuda() for x in X], [torch.from_numpy(v).cuda() for v in verts]
    (labels, state), km_s = timed(lambda: piecewise.kernel_kmeans(dX, dv, n_clusters=a.clusters, first=first, return_state=True))
    # the RANSAC stage on about --segments segments per mesh: blobs of the positions, as a rig's arg-max skins would give
    seg = [np.argmin(((v[:, None] - v[rng.choice(a.vertices, a.segments, replace=False)][None]) ** 2).sum(-1), axis=1) for v in verts]
    dst = [move_segments(rng, v, s) for v, s in zip(verts, seg)]
    vis = [rng.uniform(0.1, 1.0, a.vertices) for _ in range(a.meshes)]
    counts = [len(h) for v, s in zip(vis, seg) for h in po.segment_handles(v, s, 0.3)[1]]
    t = time.perf_counter()
    samples = piecewise.draw_ransac_samples(counts, rng=np.random.RandomState(1))
    draw_s = time.perf_counter() - t
    up = lambda xs: [torch.from_numpy(x).cuda() for x in xs]
    d_src, d_dst, d_vis, d_seg = up(verts), up(dst), up(vis), up(seg)
    details = []
    (moved), rs_s = timed(lambda: piecewise.piecewise_ransac(d_src, d_dst, d_vis, d_seg, samples=samples))
    piecewise.piecewise_ransac(d_src, d_dst, d_vis, d_seg, samples=samples, details=details)

    n_host = min(a.host_meshes, a.meshes)
    t = time.perf_counter()
    want_km = [po.kernel_kmeans(X[m], verts[m], a.clusters, 100, 0.2, 1e-4, first[m]) for m in range(n_host)]
    host_km = (time.perf_counter() - t) / max(n_host, 1)
    t, at, same = time.perf_counter(), 0, True
    for m in range(n_host):
        n = sum(1 for h in po.segment_handles(vis[m], seg[m], 0.3)[1] if len(h) >= 4)
        out, det = po.piecewise_ransac(verts[m], dst[m], vis[m], seg[m], samples[at:at + n])
        for d, g in zip(det, [x for x in details if x["mesh"] == m]):
            same &= bool(np.array_equal(d["counts"], g["counts"]) and d["by_count"] == g["by_count"] and d["refit"] == g["refit"])
        same &= bool(np.abs(out - moved[m].cpu().numpy()).max() < 1e-9)
        at += n
    host_rs = (time.perf_counter() - t) / max(n_host, 1)
    for m in range(n_host):
        same &= bool(np.array_equal(want_km[m][0], labels[m].cpu().numpy()) and want_km[m][1]["n_iter"] == state[m]["n_iter"])
    ms = lambda xs: round(statistics.median(xs) * 1e3, 3)
    print(json.dumps(dict(meshes=a.meshes, vertices=a.vertices, clusters=a.clusters, dim=a.dim, segments=a.segments, problems=len(samples),
                          kmeans_iterations=[int(min(s["n_iter"] for s in state)), int(max(s["n_iter"] for s in state))],
                          kmeans_device_ms=ms(km_s), ransac_device_ms=ms(rs_s), draw_ms=round(draw_s * 1e3, 3),
                          host_meshes=n_host, kmeans_host_ms_per_mesh=round(host_km * 1e3, 3), ransac_host_ms_per_mesh=round(host_rs * 1e3, 3),
                          agrees_with_host=same)))


if __name__ == "__main__":
    main()
