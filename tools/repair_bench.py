"""Timing of the mesh repair (morig_amd.meshprep.repair, csrc/meshfix.hip) on meshes already on the device, on the three workloads of
tools/topology_bench.py: --meshes seam tori of --side x --side quads in one call, then ONE of --large-side and one of --huge-side. Every
torus has 1 % of its faces reversed (numpy's default_rng, seeded by the mesh number) and eight single quads taken out, far apart: eight
simple loops of four edges.

``repair_ms`` is the whole public call ``repair(fill_holes="all", return_report=True)``, host reads included, between two host clock
readings around a synchronised device, median of the repeats after a warm-up; ``clean_ms`` the ``clean`` call it contains, measured the
same way. ``kernels_ms`` / ``clean_kernels_ms`` are the library's own event pairs per call (meshcheck_* and meshfix_*):
``cover_components_ms`` is what the component rounds of the double cover cost, the repair's meshcheck_components less the clean's, and
``cover_rounds`` / ``diagnose_rounds`` their round counts. ``sort_ms`` / ``host_read_ms`` are the time one more repair call spends in
``torch.sort`` and in reading tensors back (each bracketed by a synchronisation, so their sum with the kernels exceeds the undisturbed
call); ``host_reads`` counts those reads. ``oracle_s`` is the numpy oracle (tests/repair_oracle.py) on the first mesh of the batch on this
machine's CPU, its result compared first. The shader clock is sampled (bench.py's ClockSampler) over the timed repeats. One JSON line
with the date; there is NO threshold.

    python tools/repair_bench.py [--meshes 64] [--side 64] [--large-side 354] [--huge-side 708] [--repeats 5]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench import ClockSampler                          # noqa: E402
from morig_amd import meshprep, native                  # noqa: E402
from topology_bench import seam_torus, shares, timed    # noqa: E402
import repair_oracle as ro                              # noqa: E402

KINDS = ("meshcheck_weld", "meshcheck_faces", "meshcheck_edges", "meshcheck_components", "meshcheck_compact", "meshfix_orient", "meshfix_loops",
         "meshfix_fill")


def damaged_torus(n, seed, scale=1.0):
    v, f = seam_torus(n, scale)
    rng = np.random.default_rng(seed)
    turn = rng.random(len(f)) < 0.01
    f[turn] = f[turn][:, [0, 2, 1]]
    keep = np.ones(len(f), dtype=bool)
    for k in range(8):                                                           # quad (i, j) is the faces i n + j and n^2 + i n + j
        q = ((4 + 7 * k) % (n - 1)) * n + (9 + 5 * k) % (n - 1)
        keep[[q, n * n + q]] = False
    return v, f[keep]


def kernels_of(fn, repeats):
    native.prof_enable(True)
    native.prof_reset()
    ms = timed(fn, repeats)
    prof = native.prof_collect()
    native.prof_enable(False)
    return ms, {k: round(prof[k]["ms"] / repeats, 3) for k in KINDS if k in prof}


def measure(n_meshes, side, repeats, with_oracle):
    meshes = [damaged_torus(side, m, 1.0 + 0.01 * m) for m in range(n_meshes)]
    dv, df = [torch.from_numpy(v).cuda() for v, _ in meshes], [torch.from_numpy(f).cuda() for _, f in meshes]
    call = lambda: meshprep.repair(dv, df, fill_holes="all", return_report=True)
    out, rep = call()                                                                              # warm-up
    meshprep.clean(dv, df)
    oracle_s = equal = None
    if with_oracle:
        print(f"oracle on {len(meshes[0][1])} faces ...", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = ro.repair(*meshes[0], fill_holes="all")
        oracle_s = round(time.perf_counter() - t0, 3)
        equal = (all(rep[0][k] == want["report"][k] for k in ro.FIELDS + ("orient_rounds",)) and
                 all(np.array_equal(x.cpu().numpy(), want[k]) for x, k in zip(out[0], ("verts", "faces", "vertex_map", "face_map", "flipped"))))
    repair_ms, kernels = kernels_of(call, repeats)
    clean_ms, clean_kernels = kernels_of(lambda: meshprep.clean(dv, df), repeats)
    sort_ms, read_ms, reads = shares(call)
    r = rep[0]
    return dict(meshes=n_meshes, vertices=len(meshes[0][0]), faces=len(meshes[0][1]), repair_ms=round(repair_ms, 3), clean_ms=round(clean_ms, 3),
                kernels_ms=kernels, kernels_total_ms=round(sum(kernels.values()), 3), clean_kernels_ms=clean_kernels,
                cover_components_ms=round(kernels.get("meshcheck_components", 0.0) - clean_kernels.get("meshcheck_components", 0.0), 3),
                cover_rounds=r["orient_rounds"], diagnose_rounds=r["input"]["rounds"], sort_ms=sort_ms, host_read_ms=read_ms, host_reads=reads,
                flipped_faces=r["flipped_faces"], filled_loops=r["filled_loops"], tangled_boundary_edges=r["tangled_boundary_edges"],
                oracle_s=oracle_s, oracle_equal=equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--large-side", type=int, default=354)
    ap.add_argument("--huge-side", type=int, default=708)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    batch = measure(a.meshes, a.side, a.repeats, True)
    large = measure(1, a.large_side, a.repeats, False)
    huge = measure(1, a.huge_side, a.repeats, False)
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), repeats=a.repeats, batch=batch, large=large, huge=huge,
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
