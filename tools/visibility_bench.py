"""Timing of the two visibility rules on the mesh BVH (csrc/bvh.hip) against the brute-force kernels of the same
library, in one run, everything already on the device:

    scan         tools/scan_bench.py's workload: --meshes tori of 4 096 vertices / 8 192 faces turning through --frames frames, every
                 (mesh, frame) a pinhole view of 128 x 128 pixels thinned to 1 024 points (``scan.scan_trajectory``)
    bones        tools/geodesic_bench.py's workload: --meshes tori of 4 096 vertices with about 30 bones, against occluders of at most
                 3 000 faces (``rigging.occluders``) and against the mesh's own 8 192 faces (``geodesic.bone_visibility_batched``)
    asset        ONE torus of --asset-side x --asset-side vertices (354: 250 632 faces): --asset-frames views of it, and --asset-verts of
                 its vertices seen from 30 bones with the whole mesh as the occluder

Per size: ``brute_ms`` the public call with ``accel=None``, ``bvh_ms`` the same call with ``accel="bvh"`` (the tree is built inside the
call), and for the stage alone ``stage_brute_ms`` / ``stage_prebuilt_ms`` the two operators on the same tables (for ``scan`` the first
chunk of views) with ``build_ms`` the tree's construction. Each is the whole call between two device events after a warm-up of every
variant, the variants ALTERNATING within a repeat, median of the repeats. ``kernels_ms`` are the library's own event pairs per call
(scan: the scope the brute-force scan kernel shares with its stage's other kernels -- the bone kernel's scope is not collected;
bvh_build: keys and boxes, without the sort; bvh_query). ``equal``: the outputs of the variants hold the same bits, checked before
anything is timed. ``tests_share``: the box and face tests of the tree over queries x faces. The shader clock is sampled (bench.py's ClockSampler) over the timed repeats of each size. One JSON line per size with
the date; there is NO threshold.

    python tools/visibility_bench.py [--meshes 64] [--frames 100] [--asset-side 354] [--repeats 5] [--only scan,bones,asset]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import ClockSampler                                        # noqa: E402
from morig_amd import geodesic, native, ragged, rigging, scan, spatial  # noqa: E402
from geodesic_bench import mesh_case                                  # noqa: E402
from scan_bench import torus, turning                                 # noqa: E402
import labels_oracle as lo                                            # noqa: E402

KINDS = ("scan", "bvh_build", "bvh_query")
DEV = torch.device("cuda", 0)


def same(a, b):
    """two results of lists / tuples of device tensors hold the same bits"""
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b))
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
    return ({f"{k}_ms": round(statistics.median(times[k]), 3) for k in variants},
            {k: {kind: round(statistics.median(v), 3) for kind, v in kernels[k].items()} for k in variants})


def report(size, detail, variants, checks, repeats):
    """checks() -> (equal, tests_share) runs before the clock starts"""
    equal, share = checks()
    sampler, t0 = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    ms, kernels = timed(variants, repeats)
    clocks = sampler.stop().summary(t0, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), size=size, **detail, repeats=repeats, **ms, kernels_ms=kernels, equal=equal,
                          tests_share=share, sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])), flush=True)


# ------------------------------------------------------------------------------------------------------------------------- scans
def scan_size(name, meshes, frames, image, points, repeats, stage_views):
    ops = native.get_ops()
    trajs = [turning(v, frames) for v, _ in meshes]
    faces = [torch.from_numpy(f).cuda() for _, f in meshes]
    cam = scan.Camera.pinhole((0.4, 0.6, 2.8), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, image, image)
    cams = [cam] * len(meshes)
    # the stage alone: the first views of the job as one chunk, the tables as scan._Chunk makes them
    verts, view_mesh = [], []
    for m, t in enumerate(trajs):
        per_frame = t.permute(1, 0, 2).contiguous()
        verts += [per_frame[k] for k in range(frames)]
        view_mesh += [m] * frames
    verts, view_mesh = verts[:stage_views], view_mesh[:stage_views]
    tree = spatial.build_views(verts, faces, view_mesh)
    views = np.stack([view_mesh, [image] * len(verts), [image] * len(verts), [cam.kind] * len(verts)], 1).astype(np.int32)
    tables = (tree.verts, tree.vptr, tree.faces, tree.fptr, torch.from_numpy(np.stack([cam.row()] * len(verts))).cuda(), torch.from_numpy(views).cuda())
    blk, n_blk = ragged.blocks([v.shape[0] for v in verts], ops.SCAN_BLOCK, DEV, "bench")
    stage_bvh = lambda visits=False: ops.bvh_scan_visibility(*tables, 1e-4, tree.order, tree.boxes, tree.node_ptr, tree.flags, visits)
    variants = dict(brute=lambda: scan.scan_trajectory(trajs, faces, cams, n_pts=points),
                    bvh=lambda: scan.scan_trajectory(trajs, faces, cams, n_pts=points, accel="bvh"),
                    stage_brute=lambda: ops.scan_visibility(*tables, blk, n_blk, 1e-4), stage_prebuilt=stage_bvh,
                    build=lambda: spatial.build_views(verts, faces, view_mesh))

    def checks():
        a, b = variants["brute"](), variants["bvh"]()
        vis, _, visits = stage_bvh(True)
        n_faces = np.array([len(meshes[m][1]) for m in view_mesh], dtype=np.float64)
        pairs = float(sum(v.shape[0] * f for v, f in zip(verts, n_faces)))
        return same(a, b) and same(vis, variants["stage_brute"]()), round(float(visits.sum()) / pairs, 5)

    n_faces = len(meshes[0][1])
    report(name, dict(meshes=len(meshes), vertices=len(meshes[0][0]), faces=n_faces, frames=frames, views=len(meshes) * frames, image=image,
                      n_pts=points, stage_views=len(verts)), variants, checks, repeats)


# ------------------------------------------------------------------------------------------------------------------------- bones
def bone_size(name, pos, bones, tri_pos, tri_faces, repeats):
    ops = native.get_ops()
    pr = geodesic._Pairs(pos, bones, "bench").to(DEV)
    tree = spatial.build(tri_pos, tri_faces)
    m = tree.mesh
    blk, n_blk = ragged.blocks([v * n for v, n in zip(pr.nv, pr.nb)], geodesic._VIS_BLOCK, DEV, "bench")
    stage_bvh = lambda visits=False: ops.bvh_bone_visibility(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, m.verts, m.vptr, m.faces, m.fptr, pr.d_off,
                                                              pr.n, tree.order, tree.boxes, tree.node_ptr, tree.flags, visits)
    variants = dict(brute=lambda: geodesic.bone_visibility_batched(pos, bones, tri_pos, tri_faces),
                    bvh=lambda: geodesic.bone_visibility_batched(pos, bones, tri_pos, tri_faces, accel="bvh"),
                    stage_brute=lambda: ops.bone_visibility(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, m.verts, m.vptr, m.faces, m.fptr, pr.d_off, blk,
                                                            n_blk, pr.n),
                    stage_prebuilt=stage_bvh, build=lambda: spatial.build(tri_pos, tri_faces))

    def checks():
        a, b = variants["brute"](), variants["bvh"]()
        vis, _, visits = stage_bvh(True)
        pairs = float(sum(v * n * f for v, n, f in zip(pr.nv, pr.nb, m.nf)))
        return same(a, b) and same(vis, variants["stage_brute"]()), round(float(visits.sum()) / pairs, 5)

    report(name, dict(meshes=len(pos), vertices=int(np.mean(pr.nv)), bones_total=int(sum(pr.nb)), rays=pr.n, occluder_faces=int(np.mean(m.nf))),
           variants, checks, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--asset-side", type=int, default=354)
    ap.add_argument("--asset-frames", type=int, default=4)
    ap.add_argument("--asset-verts", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="scan,bones,asset")
    a = ap.parse_args()
    only = a.only.split(",")
    native.prof_enable(True)
    if "scan" in only:
        scan_size("scan", [torus(64, m) for m in range(a.meshes)], a.frames, 128, 1024, a.repeats, scan.KEY_BUDGET // (8 * 128 * 128))
    if "bones" in only:
        rng = np.random.default_rng(1)
        cases = [mesh_case(200 + i, 64, 8, int(rng.integers(26, 35))) for i in range(a.meshes)]
        pos, bones = [torch.from_numpy(c["pos"]).cuda() for c in cases], [torch.from_numpy(c["bones"]).cuda() for c in cases]
        faces = [torch.from_numpy(c["faces"]).cuda() for c in cases]
        occ = rigging.occluders(pos, faces, 3000)
        bone_size("bones_3000", pos, bones, [o[0] for o in occ], [o[1] for o in occ], a.repeats)
        bone_size("bones_8192", pos, bones, pos, faces, a.repeats)
    if "asset" in only:
        scan_size("asset_scan", [torus(a.asset_side, 1)], a.asset_frames, 128, 1024, a.repeats, a.asset_frames)
        vh, fh = lo.torus_mesh(a.asset_side, noise=1e-4, seed=1)
        joints, _ = lo.torus_chain(31, seed=1)
        pos, faces = torch.from_numpy(vh).cuda(), torch.from_numpy(fh).cuda()
        pick = torch.from_numpy(np.random.default_rng(3).choice(len(vh), min(a.asset_verts, len(vh)), replace=False)).cuda()
        bone_size("asset_bones", [pos[pick].contiguous()], [torch.from_numpy(np.concatenate([joints[:-1], joints[1:]], 1)).cuda()], [pos], [faces],
                  a.repeats)
    native.prof_enable(False)


if __name__ == "__main__":
    main()
