"""Timing of the rig transfer (morig_amd.transfer, csrc/transfer.hip) on --meshes pairs of tori already on the device: a remeshed torus of
--side x --side vertices (64: 4 096 vertices, 8 192 faces) and an original of --large-side x --large-side vertices (174: 30 276), every
--every-th remeshed vertex also being an original one, --joints joints. ``remesh_ms`` is ``transfer_to_remesh`` (original -> remeshed,
the reference's neighbour set), ``surface_ms`` is ``transfer_skins`` (remeshed surface -> original vertices); each is the whole public
call between two device events after a warm-up, median of the repeats: uploads of the tables, the sort, the kernels, the status read and,
for ``transfer_to_remesh``, the copy of the skin block into the returned rigs. The ``*_kernel_ms`` are the library's own event pairs per
call (pairs: the two all-pairs kernels; flood: keys and flood; rows: the row kernels). The first pair also goes through the numpy oracle
(tests/transfer_oracle.py), timed and compared bit for bit; the closest-point oracle runs on the first --host-points destination
vertices only and its time is scaled to all of them. The shader clock is sampled (bench.py's ClockSampler) over the timed repeats. One
JSON line with the date; there is NO threshold.

    python tools/transfer_bench.py [--meshes 64] [--side 64] [--large-side 174] [--joints 30] [--every 10] [--repeats 5] [--host-points 1024]
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
from morig_amd import native, transfer                  # noqa: E402
import transfer_oracle as to                            # noqa: E402


def timed(fn, repeats):
    native.prof_reset()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    prof = native.prof_collect()
    kernel = lambda name: round(prof[name]["ms"] / repeats, 3) if name in prof else None
    return statistics.median(times), {k: kernel("transfer_" + k) for k in ("pairs", "flood", "rows")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--large-side", type=int, default=174)
    ap.add_argument("--joints", type=int, default=30)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=1024)
    a = ap.parse_args()
    pairs = []
    for m in range(a.meshes):
        rng = np.random.default_rng(m)
        shift = rng.uniform(-0.1, 0.1, 3)
        vr, fr = to.torus(a.side, a.side)
        vo, _ = to.torus(a.large_side, a.large_side)
        vr, vo = vr + shift, vo + shift
        keep = np.arange(0, len(vr), a.every)
        vo[rng.permutation(len(vo))[:len(keep)]] = vr[keep]
        pairs.append((vo, vr, fr, to.random_skins(len(vo), a.joints, m), to.random_skins(len(vr), a.joints, 1000 + m)))
    dev = lambda k, dt=None: [torch.from_numpy(p[k]).cuda() for p in pairs]
    vo, vr, fr, so, sr = (dev(k) for k in range(5))
    rigs = [to.PlainRig(p[3]) for p in pairs]
    for r, s in zip(rigs, so):
        r.skins = s                                                                       # device skins: no upload inside the timed call
    remesh = lambda: transfer.transfer_to_remesh(vo, vr, fr, rigs, return_info=True)
    surface = lambda: transfer.transfer_skins(vr, fr, sr, vo)
    out_a, out_b = remesh(), surface()                                                    # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want_a = to.remesh_loop(*pairs[0][:4])
    oracle_a = time.perf_counter() - t0
    n_host = min(a.host_points, len(pairs[0][0]))
    t0 = time.perf_counter()
    want_b = to.transfer_skins(pairs[0][1], pairs[0][2], pairs[0][4], pairs[0][0][:n_host])
    oracle_b = (time.perf_counter() - t0) * len(pairs[0][0]) / n_host
    equal_a = bool(np.array_equal(out_a[0][1].cpu().numpy(), want_a["source"]) and out_a[0][0].skins.tobytes() == want_a["skins"].tobytes())
    equal_b = bool(np.array_equal(out_b[0][1][:n_host].cpu().numpy(), want_b["face"])
                   and out_b[0][0][:n_host].cpu().numpy().tobytes() == want_b["skins"].tobytes())
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    native.prof_enable(True)
    ms_a, k_a = timed(remesh, a.repeats)
    ms_b, k_b = timed(surface, a.repeats)
    native.prof_enable(False)
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), meshes=a.meshes, remeshed_vertices=len(pairs[0][1]), remeshed_faces=len(pairs[0][2]),
                          original_vertices=len(pairs[0][0]), joints=a.joints, repeats=a.repeats, sweeps_first_mesh=want_a["n_sweeps"],
                          coincident_first_mesh=int((want_a["sweep"] == 0).sum()), remesh_ms=round(ms_a, 3), remesh_kernels_ms=k_a,
                          surface_ms=round(ms_b, 3), surface_kernels_ms=k_b, point_triangle_pairs=a.meshes * len(pairs[0][0]) * len(pairs[0][2]),
                          oracle_remesh_first_mesh_s=round(oracle_a, 3), oracle_surface_first_mesh_s=round(oracle_b, 1), oracle_surface_points=n_host,
                          oracle_remesh_equal=equal_a, oracle_surface_equal=equal_b, sclk_under_load_mhz=clocks["sclk_under_load_mhz"],
                          clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
