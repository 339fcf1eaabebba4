"""Timing of the mesh BVH (morig_amd.spatial, csrc/bvh.hip) against the brute-force kernels of the same library, in one run, at three
sizes, everything already on the device:

    transfer   tools/transfer_bench.py's surface workload: --meshes pairs, the skins of a torus of 8 192 faces carried to the 30 276
               vertices of the original (``transfer.transfer_skins``)
    labels     tools/labels_bench.py's workload: 14 rays about each of 30 joints in --meshes tori of 8 192 faces (``labels.cast_rays``)
    asset      ONE torus of --asset-side x --asset-side vertices (708: 1 002 528 faces) with --asset-queries points near its surface
               (``transfer.transfer_skins``, 4 joints) and as many rays from its core circle (``labels.cast_rays``)

Per size and query kind: ``brute_ms`` the public call with ``accel=None``, ``bvh_ms`` the same call with ``accel="bvh"`` (the tree is
built inside the call), ``prebuilt_ms`` the ``spatial`` query on a tree built before, ``build_ms`` ``spatial.build`` alone. Each is the
whole call between two device events after a warm-up of every variant, the variants ALTERNATING within a repeat, median of the repeats.
``kernels_ms`` are the library's own event pairs per call (transfer_pairs, ray_cast: brute force; bvh_build: keys and boxes, without the
sort; bvh_query). ``equal``: the outputs of the variants hold the same bits. ``tests_share``: the box and face tests of the tree over
queries x faces. The shader clock is sampled (bench.py's ClockSampler) over the timed repeats of each size. One JSON line per size with
the date; there is NO threshold.

    python tools/spatial_bench.py [--meshes 64] [--asset-side 708] [--asset-queries 100000] [--repeats 5] [--only transfer,labels,asset]
"""
import argparse
import datetime
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
from bench import ClockSampler                          # noqa: E402
from morig_amd import labels, native, spatial, transfer  # noqa: E402
import labels_oracle as lo                              # noqa: E402
import transfer_oracle as to                            # noqa: E402

KINDS = ("transfer_pairs", "ray_cast", "bvh_build", "bvh_query")


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    """two results of lists / tuples of device tensors hold the same bits"""
    if isinstance(a, torch.Tensor):
        return bool(torch.equal(bits(a), bits(b)))
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def timed(variants, repeats):
    """variants: name -> callable. -> name -> (median ms, kernel ms per call by kind), the variants alternating within every repeat"""
    for fn in variants.values():
        fn()                                                                              # warm-up of every shape
    torch.cuda.synchronize()
    times, kernels = {k: [] for k in variants}, {k: {} for k in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            native.prof_reset()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            times[name].append(start.elapsed_time(stop))
            prof = native.prof_collect()
            for kind in KINDS:
                if kind in prof:
                    kernels[name].setdefault(kind, []).append(prof[kind]["ms"])
    return {k: dict(ms=round(statistics.median(times[k]), 3), kernels_ms={kind: round(statistics.median(v), 3) for kind, v in kernels[k].items()})
            for k in variants}


def report(size, detail, results, equal, shares, clocks):
    print(json.dumps(dict(date=datetime.date.today().isoformat(), size=size, **detail, **results, equal=equal, tests_share=shares,
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])), flush=True)


def point_variants(verts, faces, skins, dst):
    tree = spatial.build(verts, faces)
    return dict(brute=lambda: transfer.transfer_skins(verts, faces, skins, dst), bvh=lambda: transfer.transfer_skins(verts, faces, skins, dst, accel="bvh"),
                prebuilt=lambda: spatial.closest_points(tree, dst), build=lambda: spatial.build(verts, faces)), tree


def ray_variants(verts, faces, o, d, rp):
    tree = spatial.build(verts, faces)
    return dict(brute=lambda: labels.cast_rays(o, d, rp, verts, faces), bvh=lambda: labels.cast_rays(o, d, rp, verts, faces, accel="bvh"),
                prebuilt=lambda: spatial.cast_rays(tree, o, d, rp), build=lambda: spatial.build(verts, faces)), tree


def point_checks(v, tree, dst, n_faces):
    a, b, c = v["brute"](), v["bvh"](), spatial.closest_points(tree, dst, return_visits=True)
    equal = same(a, b) and same([x[1:] for x in a], [x[:3] for x in c])
    return equal, round(float(sum(int(x[3].sum()) for x in c)) / (sum(len(p) for p in dst) * n_faces), 5)


def ray_checks(v, tree, o, d, rp, n_faces):
    a, b, c = v["brute"](), v["bvh"](), spatial.cast_rays(tree, o, d, rp, return_visits=True)
    return same(a, b) and same(a, c[:3]), round(float(sum(int(x.sum()) for x in c[3])) / (len(o) * n_faces), 5)


def rename(prefix, res):
    return {f"{prefix}_{name}_ms": r["ms"] for name, r in res.items()} | {f"{prefix}_kernels_ms": {name: r["kernels_ms"] for name, r in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--asset-side", type=int, default=708)
    ap.add_argument("--asset-queries", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="transfer,labels,asset")
    a = ap.parse_args()
    only = a.only.split(",")
    native.prof_enable(True)
    cuda = lambda x: torch.from_numpy(x).cuda()
    if "transfer" in only:
        vr, fr = to.torus(64, 64)
        vo, _ = to.torus(174, 174)
        shifts = [np.random.default_rng(m).uniform(-0.1, 0.1, 3) for m in range(a.meshes)]
        verts, faces, dst = [cuda(vr + s) for s in shifts], [cuda(fr)] * a.meshes, [cuda(vo + s) for s in shifts]
        skins = [cuda(to.random_skins(len(vr), 30, 1000 + m)) for m in range(a.meshes)]
        v, tree = point_variants(verts, faces, skins, dst)
        equal, share = point_checks(v, tree, dst, len(fr))
        sampler, t0 = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
        res = timed(v, a.repeats)
        report("transfer", dict(meshes=a.meshes, faces=len(fr), points_per_mesh=len(vo), pairs=a.meshes * len(vo) * len(fr), repeats=a.repeats),
               rename("points", res), equal, share, sampler.stop().summary(t0, time.perf_counter()))
    if "labels" in only:
        scenes = [(lo.torus_mesh(64, seed=m), lo.torus_chain(30, seed=m)) for m in range(a.meshes)]
        verts, faces = [cuda(s[0][0]) for s in scenes], [cuda(s[0][1]) for s in scenes]
        table = labels.bone_rays([lo.PlainRig(*s[1]) for s in scenes], 14)
        o, d, rp = cuda(table.origins), cuda(table.dirs), table.ray_ptr
        v, tree = ray_variants(verts, faces, o, d, rp)
        equal, share = ray_checks(v, tree, o, d, rp, len(scenes[0][0][1]))
        sampler, t0 = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
        res = timed(v, a.repeats)
        report("labels", dict(meshes=a.meshes, faces=len(scenes[0][0][1]), rays=len(o), pairs=len(o) * len(scenes[0][0][1]), repeats=a.repeats),
               rename("rays", res), equal, share, sampler.stop().summary(t0, time.perf_counter()))
    if "asset" in only:
        vh, fh = lo.torus_mesh(a.asset_side, noise=1e-4, seed=1)
        rng = np.random.default_rng(2)
        n = a.asset_queries
        pts = vh[rng.integers(0, len(vh), n)] + rng.normal(0, 0.004, (n, 3))
        ang = rng.uniform(0, 2 * np.pi, n)
        org = np.stack([0.35 * np.cos(ang), np.zeros(n), 0.35 * np.sin(ang)], 1) + rng.uniform(-0.02, 0.02, (n, 3))
        verts, faces, dst = [cuda(vh)], [cuda(fh)], [cuda(pts)]
        skins = [cuda(to.random_skins(len(vh), 4, 3))]
        o, d, rp = cuda(org), cuda(rng.normal(size=(n, 3))), np.array([0, n])
        pv, tree = point_variants(verts, faces, skins, dst)
        rv, _ = ray_variants(verts, faces, o, d, rp)
        rv["prebuilt"] = lambda: spatial.cast_rays(tree, o, d, rp)
        pe, ps = point_checks(pv, tree, dst, len(fh))
        re_, rs = ray_checks(rv, tree, o, d, rp, len(fh))
        sampler, t0 = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
        pres = timed(pv, a.repeats)
        del rv["build"]
        rres = timed(rv, a.repeats)
        report("asset", dict(meshes=1, faces=len(fh), vertices=len(vh), points=n, rays=n, pairs=n * len(fh), repeats=a.repeats),
               rename("points", pres) | rename("rays", rres), dict(points=pe, rays=re_), dict(points=ps, rays=rs),
               sampler.stop().summary(t0, time.perf_counter()))
    native.prof_enable(False)


if __name__ == "__main__":
    main()
