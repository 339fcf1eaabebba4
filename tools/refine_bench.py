"""Timing of the mesh refinement (morig_amd.meshprep.refine, csrc/refine.hip) on meshes already on the device: --meshes seam tori of
--side x --side quads (about 500 vertices each) refined to --min-verts vertices in one call, then ONE seam torus of --large-side (354:
250 632 faces) refined with a ``max_edge`` of --factor times its median edge length, which about quadruples it.

``refine_ms`` is the whole public call ``refine(..., return_report=True)``, host reads included, between two host clock readings around a
synchronised device, median of the repeats after a warm-up. ``kernels_ms`` are the library's own event pairs per call (refine_* and the run
marking under mesh_prep); ``sort_ms`` / ``host_read_ms`` are the time one more call spends in ``torch.sort`` and in reading tensors back
(each bracketed by a synchronisation, so their sum with the kernels exceeds the undisturbed call); ``host_reads`` counts those reads and
``looks`` the passes with the looks that found nothing. ``interpolate_ms`` carries a float32 [V, 64] table up the result. ``oracle_s`` is
the numpy oracle (tests/refine_oracle.py) on the first mesh of the case on this machine's CPU, its result compared first. The shader clock
is sampled (bench.py's ClockSampler) over the timed repeats. One JSON line with the date; there is NO threshold.

    python tools/refine_bench.py [--meshes 64] [--side 22] [--min-verts 4096] [--large-side 354] [--factor 0.93] [--repeats 5] [--no-large-oracle]
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
import refine_oracle as fo                              # noqa: E402

KINDS = ("refine_edges", "refine_emit", "refine_interpolate", "mesh_prep")


def median_edge(v, f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return float(np.median(np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1)))


def measure(meshes, repeats, with_oracle, **kw):
    dv, df = [torch.from_numpy(v).cuda() for v, _ in meshes], [torch.from_numpy(f).cuda() for _, f in meshes]
    call = lambda: meshprep.refine(dv, df, return_report=True, **kw)
    out, rep = call()                                                                              # warm-up
    oracle_s = equal = None
    if with_oracle:
        print(f"oracle on {len(meshes[0][1])} faces ...", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = fo.refine(*meshes[0], **kw)
        oracle_s = round(time.perf_counter() - t0, 3)
        equal = rep[0] == want["report"] and all(np.array_equal(x.cpu().numpy(), want[k]) for x, k in zip(out[0], ("verts", "faces", "parents", "face_map")))
    native.prof_enable(True)
    native.prof_reset()
    refine_ms = timed(call, repeats)
    prof = native.prof_collect()
    native.prof_enable(False)
    kernels = {k: round(prof[k]["ms"] / repeats, 3) for k in KINDS if k in prof}
    sort_ms, read_ms, reads = shares(call)
    values = [torch.rand(len(v), 64, dtype=torch.float32, device="cuda") for v, _ in meshes]
    parents = [o[2] for o in out]
    meshprep.interpolate(values, parents)
    interpolate_ms = timed(lambda: meshprep.interpolate(values, parents), repeats)
    return dict(meshes=len(meshes), vertices=len(meshes[0][0]), faces=len(meshes[0][1]), settings={k: round(float(x), 6) for k, x in kw.items()},
                out_vertices=rep[0]["verts"], out_faces=rep[0]["faces"], passes=max(r["passes"] for r in rep), looks=reads,
                refine_ms=round(refine_ms, 3), kernels_ms=kernels, kernels_total_ms=round(sum(kernels.values()), 3), sort_ms=round(sort_ms, 3),
                host_read_ms=round(read_ms, 3), host_reads=reads, interpolate_ms=round(interpolate_ms, 3), oracle_s=oracle_s, oracle_equal=equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=22)
    ap.add_argument("--min-verts", type=int, default=4096)
    ap.add_argument("--large-side", type=int, default=354)
    ap.add_argument("--factor", type=float, default=0.93)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-large-oracle", action="store_true")
    a = ap.parse_args()
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    batch = measure([seam_torus(a.side, 1.0 + 0.01 * m) for m in range(a.meshes)], a.repeats, True, min_verts=a.min_verts)
    big = seam_torus(a.large_side)
    large = measure([big], a.repeats, not a.no_large_oracle, max_edge=a.factor * median_edge(*big))
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), repeats=a.repeats, batch=batch, large=large,
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
