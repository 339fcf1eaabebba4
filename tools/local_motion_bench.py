"""Timing of the local rigid motion (morig_amd.local_motion, csrc/local_motion.hip) on --meshes jittered grids of --side x --side vertices
(64: 4 096 vertices) at spacing --spacing with --frames frames of a bend, already on the device. ``patches_ms`` and ``motion_ms`` are the
whole public calls ``patches`` and ``local_rigid_motion`` between two device events after a warm-up, median of the repeats: uploads of
the tables, the key sort, the kernels, the scan and the host reads. ``kernels_ms`` are the three launches alone (count pass, fill pass,
fit), each between its own device events on prepared inputs; ``fit_write_gbs`` is the fit kernel's 88 bytes of results per fit over its
time. The first mesh also goes through the numpy oracle (tests/local_motion_oracle.py), timed; its patches are compared bit for bit and
its fits under the tests' criterion first. The shader clock is sampled (bench.py's ClockSampler) over the timed repeats. One JSON line
with the date; there is NO threshold.

    python tools/local_motion_bench.py [--meshes 64] [--side 64] [--spacing 0.012] [--frames 20] [--repeats 5]
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
from morig_amd import local_motion as lm                # noqa: E402
from morig_amd.meshbatch import MeshBatch, vertex_adjacency   # noqa: E402
from morig_amd.runtime import get_ops                   # noqa: E402
import local_motion_oracle as lo                        # noqa: E402


def timed(fn, repeats):
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--spacing", type=float, default=0.012)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    v0, f0 = lo.grid_mesh(a.side, a.side, a.spacing, seed=1)
    clip0 = lo.bend_clip(v0, a.frames, 2)
    verts, faces, trajs = [], [], []
    for m in range(a.meshes):
        shift = np.random.default_rng(m).uniform(-0.1, 0.1, 3) * (m > 0)
        verts.append(torch.from_numpy(v0 + shift).cuda())
        faces.append(torch.from_numpy(f0).cuda())
        trajs.append(torch.from_numpy(clip0 + shift).cuda())
    pat = lm.patches(verts, faces)                                                        # warm-up
    out = lm.local_rigid_motion(verts, trajs, pat)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want_p = lo.patch_lists(v0, f0)
    oracle_p = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_m = lo.local_motion(v0, clip0, want_p["lists"])
    oracle_m = time.perf_counter() - t0
    got_lists = pat.split()[0]
    equal = bool(all(np.array_equal(x, y) for x, y in zip(got_lists, want_p["lists"])))
    got = dict(zip(("rot6d", "trans", "gap", "residual"), (t.cpu().numpy() for t in out.split()[0])))
    worst = lo.assert_motion_close(got, want_m, v0, clip0, want_p["lists"], "first mesh")
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    patches_ms = timed(lambda: lm.patches(verts, faces), a.repeats)
    motion_ms = timed(lambda: lm.local_rigid_motion(verts, trajs, pat), a.repeats)
    mesh, ops = MeshBatch("bench", verts, faces), get_ops()                                 # the three launches alone, on prepared inputs
    n, dev = int(mesh.vptr_host[-1]), mesh.device
    words = torch.zeros(mesh.n + 1 + 3, dtype=torch.int32, device=dev)
    keys, rowptr = vertex_adjacency(ops, mesh, 6, words[:mesh.n + 1])
    status, most, flat = words[mesh.n + 1:], int(mesh.nv.max()), torch.cat(trajs, 0).contiguous()
    count_ms = timed(lambda: ops.local_patches(mesh.verts, mesh.vptr, most, rowptr, keys, lm.RUNGS, status), a.repeats)
    fill_ms = timed(lambda: ops.local_patches(mesh.verts, mesh.vptr, most, rowptr, keys, lm.RUNGS, status, ptr=pat.ptr, rung=pat.rung,
                                              n_ids=pat.ids.numel()), a.repeats)
    fit_ms = timed(lambda: ops.local_fit(mesh.verts, flat, mesh.vptr, pat.ptr, pat.ids, status), a.repeats)
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    n_fits, sizes = n * a.frames, np.diff(pat.ptr.cpu().numpy())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), meshes=a.meshes, vertices=len(v0), faces=len(f0), frames=a.frames, fits=n_fits,
                          patch_size_mean=round(float(sizes.mean()), 2), patch_size_max=int(sizes.max()), repeats=a.repeats,
                          patches_ms=round(patches_ms, 3), motion_ms=round(motion_ms, 3),
                          kernels_ms=dict(count=round(count_ms, 3), fill=round(fill_ms, 3), fit=round(fit_ms, 3)),
                          fit_write_gbs=round(n_fits * 88 / (fit_ms * 1e-3) / 1e9, 1), oracle_patches_first_mesh_s=round(oracle_p, 2),
                          oracle_motion_first_mesh_s=round(oracle_m, 2), oracle_patches_equal=equal,
                          oracle_motion_worst_error_over_bound=round(max(worst.values()), 4), sclk_under_load_mhz=clocks["sclk_under_load_mhz"],
                          clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
