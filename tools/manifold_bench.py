"""Timing of the non-manifold split (morig_amd.meshprep.split_nonmanifold / repair(split=True), csrc/meshsplit.hip) on meshes already on
the device, on the three workloads of tools/topology_bench.py: --meshes seam tori of --side x --side quads in one call, then ONE of
--large-side and one of --huge-side. Every torus gets two kinds of defect, made by coincident copies that the exact weld joins: on 3 % of
its vertices (numpy's default_rng, seeded by the mesh number) a small open cone of three faces whose apex is a copy of the vertex -- a
pinched vertex with two fans --, and on 16 of its edges a pair of triangles on copies of the edge's ends -- an edge with four faces.

``split_ms`` is the whole public call ``split_nonmanifold(return_report=True)``, host reads included, between two host clock readings
around a synchronised device, median of the repeats after a warm-up; ``clean_ms`` the ``clean`` call it contains, ``repair_ms`` the call
``repair(fill_holes="all", return_report=True)`` WITHOUT the split on the same inputs and ``repair_split_ms`` the same call with
``split=True``, all measured the same way: ``added_ms`` = repair_split_ms - repair_ms is what the split costs a repair. ``kernels_ms`` /
``clean_kernels_ms`` are the library's own event pairs per call of ``split_nonmanifold`` / ``clean``: ``fan_components_ms`` is what the
component rounds on the corner nodes cost, the split's meshcheck_components less the clean's, ``split_rounds`` / ``diagnose_rounds`` their
round counts, ``meshsplit_*`` the new kernels. ``sort_ms`` / ``host_read_ms`` are the time one more ``split_nonmanifold`` call spends in
``torch.sort`` and in reading tensors back (each bracketed by a synchronisation, so their sum with the kernels exceeds the undisturbed
call); ``host_reads`` counts those reads. ``oracle_s`` is the numpy oracle (tests/manifold_oracle.py ``repair_split``) on the first mesh of
the batch on this machine's CPU, its result compared first with that of ``repair(split=True)``. The shader clock is sampled (bench.py's
ClockSampler) over the timed repeats. One JSON line with the date; there is NO threshold.

    python tools/manifold_bench.py [--meshes 64] [--side 64] [--large-side 354] [--huge-side 708] [--repeats 5]
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
import manifold_oracle as mo                            # noqa: E402
import repair_oracle as ro                              # noqa: E402

KINDS = ("meshcheck_weld", "meshcheck_faces", "meshcheck_edges", "meshcheck_components", "meshcheck_compact", "meshfix_orient", "meshfix_loops",
         "meshfix_fill", "meshsplit_links", "meshsplit_apply")


def defective_torus(n, seed, scale=1.0):
    v, f = seam_torus(n, scale)
    rng = np.random.default_rng(seed)
    V = len(v)
    apex = rng.choice(V, max(1, int(0.03 * V)), replace=False)
    new_v, new_f = [v], [f]
    base = V
    for a in apex:                                                               # an open cone of three faces on a copy of vertex a
        rim = v[a] + 0.01 * scale * np.array([[1.0, 0, 1], [0, 1.0, 1], [-1.0, 0, 1], [0, -1.0, 1]])
        new_v.append(np.concatenate([v[a][None], rim]))
        new_f.append(np.array([[base, base + 1 + i, base + 2 + i] for i in range(3)]))
        base += 5
    for k in rng.choice(len(f), 16, replace=False):                              # two more triangles on the edge (f[k, 0], f[k, 1])
        a, b = f[k, 0], f[k, 1]
        mid = 0.5 * (v[a] + v[b])
        new_v.append(np.stack([v[a], v[b], mid + [0, 0, 0.02 * scale], mid - [0, 0, 0.02 * scale]]))
        new_f.append(np.array([[base, base + 1, base + 2], [base + 1, base, base + 3]]))
        base += 4
    return np.concatenate(new_v), np.concatenate(new_f).astype(np.int64)


def kernels_of(fn, repeats):
    native.prof_enable(True)
    native.prof_reset()
    ms = timed(fn, repeats)
    prof = native.prof_collect()
    native.prof_enable(False)
    return ms, {k: round(prof[k]["ms"] / repeats, 3) for k in KINDS if k in prof}


def measure(n_meshes, side, repeats, with_oracle):
    meshes = [defective_torus(side, m, 1.0 + 0.01 * m) for m in range(n_meshes)]
    dv, df = [torch.from_numpy(v).cuda() for v, _ in meshes], [torch.from_numpy(f).cuda() for _, f in meshes]
    split = lambda: meshprep.split_nonmanifold(dv, df, return_report=True)
    repair = lambda: meshprep.repair(dv, df, fill_holes="all", return_report=True)
    repair_split = lambda: meshprep.repair(dv, df, fill_holes="all", return_report=True, split=True)
    _, rep = split()                                                                               # warm-up
    out, rrep = repair_split()
    _, plain = repair()
    meshprep.clean(dv, df)
    oracle_s = equal = None
    if with_oracle:
        print(f"oracle on {len(meshes[0][1])} faces ...", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = mo.repair_split(*meshes[0], fill_holes="all")
        oracle_s = round(time.perf_counter() - t0, 3)
        equal = (all(rrep[0][k] == want["report"][k] for k in ro.FIELDS + ("orient_rounds",)) and rrep[0]["split"] == want["report"]["split"] and
                 all(np.array_equal(x.cpu().numpy(), want[k]) for x, k in zip(out[0], ("verts", "faces", "vertex_map", "face_map", "flipped", "source"))))
    split_ms, kernels = kernels_of(split, repeats)
    clean_ms, clean_kernels = kernels_of(lambda: meshprep.clean(dv, df), repeats)
    repair_ms = timed(repair, repeats)
    repair_split_ms, repair_split_kernels = kernels_of(repair_split, repeats)
    sort_ms, read_ms, reads = shares(split)
    r = rep[0]
    return dict(meshes=n_meshes, vertices=len(meshes[0][0]), faces=len(meshes[0][1]), split_ms=round(split_ms, 3), clean_ms=round(clean_ms, 3),
                repair_ms=round(repair_ms, 3), repair_split_ms=round(repair_split_ms, 3), added_ms=round(repair_split_ms - repair_ms, 3),
                kernels_ms=kernels, kernels_total_ms=round(sum(kernels.values()), 3), clean_kernels_ms=clean_kernels,
                repair_split_kernels_ms=repair_split_kernels,
                fan_components_ms=round(kernels.get("meshcheck_components", 0.0) - clean_kernels.get("meshcheck_components", 0.0), 3),
                split_rounds=r["split_rounds"], diagnose_rounds=r["input"]["rounds"], sort_ms=sort_ms, host_read_ms=read_ms, host_reads=reads,
                nonmanifold_edges=r["nonmanifold_edges"], nonmanifold_verts=r["nonmanifold_verts"], added_verts=r["added_verts"], max_fans=r["max_fans"],
                tangled_without_split=plain[0]["tangled_boundary_edges"], tangled_with_split=rrep[0]["tangled_boundary_edges"],
                filled_without_split=plain[0]["filled_loops"], filled_with_split=rrep[0]["filled_loops"], oracle_s=oracle_s, oracle_equal=equal)


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
