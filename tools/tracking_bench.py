"""Timing of the device tracking stage (morig_amd/tracking.py, csrc/track.hip) on a batch of synthetic problems: 64 rigs of about 30
joints on 4 096-vertex meshes with 5 influences per vertex and 4 096 target points each. Reported, each as the median over repeated calls
after warm-up: the first solve alone (morig_ik_solve on resident inputs, device events: 64 problems x 200 iterations in one launch) and
per iteration, the second solve's launch on the kept pairs, and the whole ``ik_drag`` (host clock around a device synchronise: the stage
does its per-rig algebra on the host). The shader clock is sampled while the timed calls run (bench.py's ClockSampler). The reference's
CPU time for ONE such problem (its ik_drag, recorded by tools/make_tracking_golden.py in tests/golden/track_drag.npz) is printed next to
it. No GPU: this tool fails, it does not fall back.

    python tools/tracking_bench.py [--problems 64] [--vertices 4096] [--repeats 5] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_scene(seed, n_vtx=4096, n_joints=30, n_pts=4096, influences=5, width=64):
    """one synthetic tracking problem -> dict(pos, parent, root, skins, vtx_src, vtx_dst, pts, vtx_feature, pts_feature, vismask): a random
    tree of joints in the unit box, ``influences`` weights per vertex, the targets a small pose away, points sampled near the target
    vertices with features that match their vertex"""
    from morig_amd import formats, tracking
    rng = np.random.default_rng([0x74626E, seed])
    root = int(rng.integers(n_joints))
    parent = np.full(n_joints, -1, dtype=np.int64)
    placed = [root]
    for j in rng.permutation([j for j in range(n_joints) if j != root]):
        parent[j] = placed[int(rng.integers(len(placed)))]
        placed.append(int(j))
    pos = rng.uniform(-0.4, 0.4, size=(n_joints, 3))
    skins = np.zeros((n_vtx, n_joints))
    cols = np.argsort(rng.uniform(size=(n_vtx, n_joints)), axis=1)[:, :influences]
    w = rng.uniform(0.1, 1.0, size=(n_vtx, influences))
    skins[np.arange(n_vtx)[:, None], cols] = np.round(w / w.sum(1, keepdims=True), 4)
    vtx = rng.uniform(-0.5, 0.5, size=(n_vtx, 3))
    rig = formats.Rig.from_arrays(pos, parent, root, skins=skins)
    # the target: the mesh under a small random pose (float64 forward kinematics on the host)
    posed = copy_pose(rig, rng.uniform(-0.2, 0.2, size=(n_joints, 3)), rng.uniform(-0.05, 0.05, size=3))
    vptr, ev, ej, wt = tracking.skin_entries(skins)
    loc, _ = tracking.local_vertices(rig.global_transforms_homogeneous, vtx, ev, ej)
    target = tracking.skin_vertices(posed.global_transforms_homogeneous, loc, ev, ej, wt, n_vtx)
    src = rng.integers(n_vtx, size=n_pts)
    fv = rng.normal(size=(n_vtx, width))
    fv /= np.linalg.norm(fv, axis=1, keepdims=True)
    fp = fv[src] + 0.45 * rng.normal(size=(n_pts, width)) / np.sqrt(width)
    fp /= np.linalg.norm(fp, axis=1, keepdims=True)
    return dict(pos=pos, parent=parent, root=root, skins=skins, vtx_src=vtx, vtx_dst=target + rng.normal(0, 2e-3, size=target.shape),
                pts=target[src] + rng.normal(0, 5e-3, size=(n_pts, 3)), vtx_feature=fv.astype(np.float32), pts_feature=fp.astype(np.float32),
                vismask=rng.uniform(size=n_vtx).astype(np.float32))


def copy_pose(rig, angles, trans):
    """a copy of the rig posed by Euler angles (R = Rx Ry Rz per joint) and a root translation"""
    import copy
    c, s = np.cos(angles), np.sin(angles)
    out = copy.deepcopy(rig)
    for j in range(len(angles)):
        rx = np.array([[1, 0, 0], [0, c[j, 0], -s[j, 0]], [0, s[j, 0], c[j, 0]]])
        ry = np.array([[c[j, 1], 0, s[j, 1]], [0, 1, 0], [-s[j, 1], 0, c[j, 1]]])
        rz = np.array([[c[j, 2], -s[j, 2], 0], [s[j, 2], c[j, 2], 0], [0, 0, 1]])
        out.local_frames[j] = rx @ (ry @ rz)
    out.pos = out.pos.copy()
    out.pos[out.root_id] = out.pos[out.root_id] + trans
    out.fk()
    return out


def main():
    import torch
    from bench import ClockSampler
    from morig_amd import formats, tracking
    from morig_amd.runtime import get_ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--joints", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tracking_bench needs the GPU"
    rng = np.random.default_rng(2)
    scenes = [make_scene(500 + i, args.vertices, int(rng.integers(args.joints - 4, args.joints + 5)), args.vertices) for i in range(args.problems)]
    rigs = [formats.Rig.from_arrays(s["pos"], s["parent"], s["root"], skins=s["skins"]) for s in scenes]
    ops = get_ops()

    def events(fn, warmup, repeats):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3))

    def stage_problems(kw):
        probs = []
        for s, rig in zip(scenes, rigs):
            vptr, ev, ej, w = tracking.skin_entries(rig.skins)
            loc, _ = tracking.local_vertices(rig.global_transforms_homogeneous, s["vtx_src"], ev, ej)
            probs.append(tracking.make_problem(rig.local_frames, rig.offset, rig.hierarchy, rig.root_id, vptr, ej, w, loc[:, :3], s["vtx_dst"],
                                               s["vismask"], thrd=tracking.VISMASK_THRD, **kw))
        return probs

    sampler = ClockSampler(index=0).start()
    t_start = time.perf_counter()
    res = {}
    for label, kw in (("solve_stage1", tracking.STAGE1), ("solve_400_iterations_all_vertices", tracking.STAGE2)):
        t, n, mj, mv, mi, _, _ = tracking.pack_problems(stage_problems(kw), "cuda")
        res[label] = events(lambda: ops.ik_solve(t, n, mj, mv, mi), args.warmup, args.repeats)
        res[label]["us_per_iteration"] = round(res[label]["median_ms"] * 1e3 / kw["iter_time"], 2)
        res[label]["lds_bytes"] = ops.ik_solve_lds_bytes(mj, mv)
    ts, kept = [], None
    for r in range(args.warmup + args.repeats):
        details = []
        t0 = time.perf_counter()
        tracking.ik_drag([s["vtx_src"] for s in scenes], [s["vtx_dst"] for s in scenes], [s["pts"] for s in scenes], rigs,
                         [s["vtx_feature"] for s in scenes], [s["pts_feature"] for s in scenes], [s["vismask"] for s in scenes], details=details)
        torch.cuda.synchronize()
        if r >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
        kept = [len(d["pairs"]) for d in details]
    res["ik_drag"] = dict(median_ms=round(float(np.median(ts)), 1), min_ms=round(float(np.min(ts)), 1), max_ms=round(float(np.max(ts)), 1))
    t_end = time.perf_counter()
    clocks = sampler.stop().summary(t_start, t_end)
    ref = None
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", "track_drag.npz"))
        ref = json.loads(bytes(z["meta"]).decode()).get("reference_cpu")
    except Exception:
        pass
    print(json.dumps(dict(problems=args.problems, vertices=args.vertices, joints=[len(r.pos) for r in rigs],
                          entries=int(sum(int(np.count_nonzero(r.skins)) for r in rigs)), kept_pairs_mean=float(np.mean(kept)),
                          repeats=args.repeats, warmup=args.warmup, **res, reference_cpu_one_problem=ref,
                          gpu=torch.cuda.get_device_name(0), clocks=clocks, date=time.strftime("%Y-%m-%d"))))


if __name__ == "__main__":
    main()
