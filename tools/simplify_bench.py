"""Timing of the mesh simplification (morig_amd.meshprep.simplify, csrc/simplify.hip) on two batches of --meshes closed meshes already on
the device: tori of --side x --side vertices (64: 4 096 vertices, 8 192 faces) and of --large-side (180: 32 400 vertices, 64 800 faces),
each under a rotation of its own, brought to --target faces. ``simplify_ms`` is the whole public call between two device events after a
warm-up, median of the repeats: the index check, the bounding boxes, every step of the joint bisection (two sorts and one host read
each), the face compaction, the corner sort and the quadric kernel. ``quadrics_kernel_ms`` and ``key_kernels_ms`` are the library's own
event pairs, per call. The first mesh of every batch also goes through the numpy oracle (tests/simplify_oracle.py), results compared
first: discrete results equal, positions in units of the cell size. The shader clock is sampled (bench.py's ClockSampler) over the timed
repeats. One JSON line with the date; there is NO threshold.

    python tools/simplify_bench.py [--meshes 64] [--side 64] [--large-side 180] [--target 3000] [--repeats 5]
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
from morig_amd import meshprep, native                  # noqa: E402
import meshprep_oracle as mo                            # noqa: E402
import simplify_oracle as so                            # noqa: E402


def batch(n_meshes, side):
    v, f = mo.torus(side)
    return [so.rotated(v * (1.0 + 0.01 * m), 100 + m) for m in range(n_meshes)], [f] * n_meshes


def measure(n_meshes, side, target, repeats):
    verts, faces = batch(n_meshes, side)
    dv, df = [torch.from_numpy(v).cuda() for v in verts], [torch.from_numpy(f).cuda() for f in faces]
    out, info = meshprep.simplify(dv, df, target_faces=target, return_info=True)                   # warm-up
    t0 = time.perf_counter()
    want = so.simplify(verts[0], faces[0], target)
    oracle_s = time.perf_counter() - t0
    v, f, m, r = out[0]
    equal = bool(r == want["resolution"] and np.array_equal(m.cpu().numpy(), want["vertex_map"]) and np.array_equal(f.cpu().numpy(), want["faces"])
                 and info[0] == want["trace"])
    dev = float(np.abs(v.cpu().numpy() - want["verts"]).max() / want["h"]) if equal else None
    native.prof_enable(True)
    native.prof_reset()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        out = meshprep.simplify(dv, df, target_faces=target)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    prof = native.prof_collect()
    native.prof_enable(False)
    kernel = lambda name: round(prof[name]["ms"] / repeats, 3) if name in prof else None
    total = statistics.median(times)
    return dict(meshes=n_meshes, vertices=side * side, faces=2 * side * side, simplify_ms=round(total, 3), meshes_per_s=round(n_meshes / (total * 1e-3), 1),
                quadrics_kernel_ms=kernel("simplify_quadrics"), key_kernels_ms=kernel("simplify_keys"),
                passes=len(info[0]), resolutions=[min(o[3] for o in out), max(o[3] for o in out)],
                out_vertices=[min(o[0].shape[0] for o in out), max(o[0].shape[0] for o in out)],
                out_faces=[min(o[1].shape[0] for o in out), max(o[1].shape[0] for o in out)],
                oracle_first_mesh_s=round(oracle_s, 3), oracle_discrete_equal=equal, oracle_position_deviation_h=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--large-side", type=int, default=180)
    ap.add_argument("--target", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    small = measure(a.meshes, a.side, a.target, a.repeats)
    large = measure(a.meshes, a.large_side, a.target, a.repeats)
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), target_faces=a.target, repeats=a.repeats, small=small, large=large,
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
