"""Timing of the depth scans (morig_amd/scan.py) for a batch: --meshes tori of --side x --side vertices (4 096 at the default 64, twice as
many faces), each turning through --frames frames, every (mesh, frame) one pinhole view of --image x --image pixels thinned to --points
points; the trajectories are on the device before the clock starts. ``scan_trajectory_ms`` is the whole public call between two device
events after a warm-up, median over the repeats: the tables built on the host and uploaded, the chunks, every launch and every host read.
``stage_ms`` sums, per stage, the time between a pair of device events around each of its calls in the op layer (raster, resolve, compact,
fps, visibility, nearest) in the last repeat; what is left is torch glue and the host. The shader clock is sampled (bench.py's
ClockSampler) over the timed repeats. One JSON line with the date; there is NO threshold.

    python tools/scan_bench.py [--meshes 64] [--side 64] [--frames 100] [--image 128] [--points 1024] [--repeats 3]
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
from bench import ClockSampler                          # noqa: E402
from morig_amd import native, scan                      # noqa: E402

STAGES = ("scan_raster", "scan_resolve", "scan_compact", "fps", "scan_visibility", "scan_nearest")


class TimedOps:
    """the op layer with a pair of device events around every call of a stage"""

    def __init__(self, ops):
        self.ops, self.events = ops, {s: [] for s in STAGES}

    def __getattr__(self, name):
        attr = getattr(self.ops, name)
        if name not in STAGES:
            return attr

        def run(*args, **kw):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = attr(*args, **kw)
            stop.record()
            self.events[name].append((start, stop))
            return out
        return run

    def totals(self):
        torch.cuda.synchronize()
        return {s: round(sum(a.elapsed_time(b) for a, b in ev), 3) for s, ev in self.events.items()}


def torus(side, seed):
    rng = np.random.default_rng([0x5363616E, seed])
    R, r = rng.uniform(0.5, 0.65), rng.uniform(0.15, 0.3)
    a = 2 * np.pi * np.arange(side) / side
    u, v = np.meshgrid(a, a, indexing="ij")
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    at = lambda i, j: (i % side) * side + j % side
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    faces = np.concatenate([np.stack([at(i, j), at(i + 1, j), at(i + 1, j + 1)], -1).reshape(-1, 3),
                            np.stack([at(i, j), at(i + 1, j + 1), at(i, j + 1)], -1).reshape(-1, 3)])
    return verts @ q.T, faces


def turning(verts, frames):
    """[V, T, 3] on the device: the mesh turning about y by 0.03 rad per frame"""
    a = torch.arange(frames, dtype=torch.float64, device="cuda") * 0.03
    c, s, z, o = torch.cos(a), torch.sin(a), torch.zeros_like(a), torch.ones_like(a)
    R = torch.stack([torch.stack([c, z, s], 1), torch.stack([z, o, z], 1), torch.stack([-s, z, c], 1)], 1)      # [T, 3, 3]
    return torch.einsum("tij,vj->vti", R, torch.from_numpy(verts).cuda()).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    meshes = [torus(a.side, m) for m in range(a.meshes)]
    trajs = [turning(v, a.frames) for v, _ in meshes]
    faces = [torch.from_numpy(f).cuda() for _, f in meshes]
    cam = scan.Camera.pinhole((0.4, 0.6, 2.8), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, a.image, a.image)
    run = lambda: scan.scan_trajectory(trajs, faces, [cam] * a.meshes, n_pts=a.points)
    out = run()                                              # warm-up
    times, timed = [], None
    real_ops = scan.get_ops
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    try:
        for _ in range(a.repeats):
            timed = TimedOps(native.get_ops())
            scan.get_ops = lambda: timed
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            out = run()
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
    finally:
        scan.get_ops = real_ops
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    stage = timed.totals()
    total = statistics.median(times)
    views = a.meshes * a.frames
    print(json.dumps(dict(date=datetime.date.today().isoformat(), meshes=a.meshes, vertices=a.side * a.side, faces=2 * a.side * a.side,
                          frames=a.frames, views=views, image=[a.image, a.image], n_pts=a.points, key_budget_bytes=scan.KEY_BUDGET,
                          chunks=len(timed.events["scan_raster"]), scan_trajectory_ms=round(total, 3), last_repeat_ms=round(times[-1], 3),
                          stage_ms=stage, glue_and_host_ms=round(times[-1] - sum(stage.values()), 3),
                          views_per_s=round(views / (total * 1e-3), 1),
                          visible_share=round(float(sum(o[1].float().mean() for o in out)) / len(out), 4),
                          corr_v2p_rows=int(sum(o[2].shape[0] for o in out)), corr_p2v_rows=int(sum(o[3].shape[0] for o in out)),
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
