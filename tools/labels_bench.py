"""Timing of the bone-ray labels (morig_amd.labels.bone_ray_labels, csrc/labels.hip) on a batch of --meshes tori of --side x --side vertices
(64: 4 096 vertices, 8 192 faces) already on the device, each with a chain of --joints jittered joints on its core circle (14 rays per
joint). ``labels_ms`` is the whole public call between two device events after a warm-up, median of the repeats: the host ray plan, the
uploads, the three kernels and the status read. ``cast_kernel_ms``, ``select_kernel_ms`` and ``attention_kernel_ms`` are the library's
own event pairs, per call. The first mesh also goes through the numpy oracle (tests/labels_oracle.py), timed and compared. The shader
clock is sampled (bench.py's ClockSampler) over the timed repeats. One JSON line with the date; there is NO threshold.

    python tools/labels_bench.py [--meshes 64] [--side 64] [--joints 30] [--repeats 5]
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
from morig_amd import labels, native                    # noqa: E402
import labels_oracle as lo                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--joints", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    scenes = [(lo.torus_mesh(a.side, seed=m), lo.torus_chain(a.joints, seed=m)) for m in range(a.meshes)]
    verts = [torch.from_numpy(s[0][0]).cuda() for s in scenes]
    faces = [torch.from_numpy(s[0][1]).cuda() for s in scenes]
    rigs = [lo.PlainRig(*s[1]) for s in scenes]
    out = labels.bone_ray_labels(verts, faces, rigs)                                     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = lo.labels(scenes[0][0][0], scenes[0][0][1], *scenes[0][1])
    oracle_s = time.perf_counter() - t0
    attn, fs, det = out[0]
    equal = bool(np.array_equal(det["face"].cpu().numpy(), want["face"]) and np.array_equal(det["kept"].cpu().numpy(), want["kept"])
                 and np.array_equal(attn.cpu().numpy(), want["attn"]))
    fs_dev = float(np.abs(fs.cpu().numpy() - want["featuresize"]).max())
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    native.prof_enable(True)
    native.prof_reset()
    times = []
    for _ in range(a.repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        out = labels.bone_ray_labels(verts, faces, rigs)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    prof = native.prof_collect()
    native.prof_enable(False)
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    kernel = lambda name: round(prof[name]["ms"] / a.repeats, 3) if name in prof else None
    total = statistics.median(times)
    rays = sum(int(o[2]["t"].numel()) for o in out)
    print(json.dumps(dict(date=datetime.date.today().isoformat(), meshes=a.meshes, vertices=a.side * a.side, faces=2 * a.side * a.side, joints=a.joints,
                          rays=rays, ray_face_tests=rays * 2 * a.side * a.side, repeats=a.repeats, labels_ms=round(total, 3),
                          meshes_per_s=round(a.meshes / (total * 1e-3), 1), cast_kernel_ms=kernel("ray_cast"), select_kernel_ms=kernel("ray_select"),
                          attention_kernel_ms=kernel("ray_attention"), labelled_share=round(float(torch.cat([o[0] for o in out]).mean()), 4),
                          featuresize_range=[round(float(min(o[1].min() for o in out)), 4), round(float(max(o[1].max() for o in out)), 4)],
                          oracle_first_mesh_s=round(oracle_s, 3), oracle_discrete_equal=equal, oracle_featuresize_deviation=fs_dev,
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
