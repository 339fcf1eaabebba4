"""Timing of the mesh diagnosis and cleaning (morig_amd.meshprep.diagnose / clean, csrc/meshcheck.hip) on meshes already on the device:
--meshes tori of --side x --side quads with duplicated seam vertices (64: 4 225 vertices, 8 192 faces) in one call, then ONE such torus
of --large-side (354: 250 632 faces) and one of --huge-side (708: 1 002 528 faces). A torus is built as an OBJ exporter would write it,
with the seam rows and columns present twice, so the weld has work to do and the unwelded mesh is an open sheet.

``diagnose_ms`` / ``clean_ms`` are the whole public calls, host reads included, between two host clock readings around a synchronised
device, median of the repeats after a warm-up. ``kernels_ms`` are the library's own event pairs per diagnose call (meshcheck_*), and
``sort_ms`` / ``host_read_ms`` the time one more diagnose call spends in ``torch.sort`` and in reading tensors back (each bracketed by a
synchronisation, so their sum with the kernels exceeds the undisturbed call); ``host_reads`` counts those reads. ``oracle_s`` is the numpy
oracle (tests/topology_oracle.py) on the first mesh on this machine's CPU, its report compared first. The shader clock is sampled
(bench.py's ClockSampler) over the timed repeats. One JSON line with the date; there is NO threshold.

    python tools/topology_bench.py [--meshes 64] [--side 64] [--large-side 354] [--huge-side 708] [--repeats 5] [--no-large-oracle]
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
import topology_oracle as to                            # noqa: E402

KINDS = ("meshcheck_weld", "meshcheck_faces", "meshcheck_edges", "meshcheck_components", "meshcheck_compact")


def seam_torus(n, scale=1.0):
    """(n + 1)^2 vertices, 2 n^2 faces: row n repeats row 0 and column n column 0"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    a, b = 2 * np.pi * (i % n) / n, 2 * np.pi * (j % n) / n
    v = np.stack([(2 + np.cos(b)) * np.cos(a), (2 + np.cos(b)) * np.sin(a), np.sin(b)], -1).reshape(-1, 3) * scale
    q = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([q, q + n + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + 1], 1)])
    return v, f


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def shares(fn):
    """one call with torch.sort and Tensor.cpu bracketed by synchronisations -> (sort ms, host read ms, host reads)"""
    acc = dict(sort=0.0, read=0.0, reads=0)
    sort, cpu = torch.sort, torch.Tensor.cpu

    def bracket(key, inner):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = inner(*a, **kw)
            torch.cuda.synchronize()
            acc[key] += (time.perf_counter() - t0) * 1e3
            return r
        return run

    def read(t, *a, **kw):
        acc["reads"] += 1 if t.is_cuda else 0
        return bracket("read", cpu)(t, *a, **kw)
    torch.sort, torch.Tensor.cpu = bracket("sort", sort), read
    try:
        fn()
    finally:
        torch.sort, torch.Tensor.cpu = sort, cpu
    return round(acc["sort"], 3), round(acc["read"], 3), acc["reads"]


def measure(n_meshes, side, repeats, with_oracle):
    meshes = [seam_torus(side, 1.0 + 0.01 * m) for m in range(n_meshes)]
    dv, df = [torch.from_numpy(v).cuda() for v, _ in meshes], [torch.from_numpy(f).cuda() for _, f in meshes]
    rep = meshprep.diagnose(dv, df)                                                                # warm-up
    meshprep.clean(dv, df)
    oracle_s = equal = None
    if with_oracle:
        print(f"oracle on {len(meshes[0][1])} faces ...", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = to.diagnose(*meshes[0])
        oracle_s = round(time.perf_counter() - t0, 3)
        equal = all(rep[0][k] == want[k] for k in to.FIELDS + ("watertight", "rounds"))
    native.prof_enable(True)
    native.prof_reset()
    diag = timed(lambda: meshprep.diagnose(dv, df), repeats)
    prof = native.prof_collect()
    native.prof_enable(False)
    kernels = {k: round(prof[k]["ms"] / repeats, 3) for k in KINDS if k in prof}
    cleaning = timed(lambda: meshprep.clean(dv, df), repeats)
    sort_ms, read_ms, reads = shares(lambda: meshprep.diagnose(dv, df))
    r = rep[0]
    return dict(meshes=n_meshes, vertices=len(meshes[0][0]), faces=len(meshes[0][1]), diagnose_ms=round(diag, 3), clean_ms=round(cleaning, 3),
                kernels_ms=kernels, kernels_total_ms=round(sum(kernels.values()), 3), sort_ms=sort_ms, host_read_ms=read_ms, host_reads=reads,
                rounds=r["rounds"], duplicate_verts=r["duplicate_verts"], watertight=r["watertight"], oracle_s=oracle_s, oracle_equal=equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--large-side", type=int, default=354)
    ap.add_argument("--huge-side", type=int, default=708)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-large-oracle", action="store_true")
    a = ap.parse_args()
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    batch = measure(a.meshes, a.side, a.repeats, True)
    large = measure(1, a.large_side, a.repeats, not a.no_large_oracle)
    huge = measure(1, a.huge_side, a.repeats, not a.no_large_oracle)
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), repeats=a.repeats, batch=batch, large=large, huge=huge,
                          sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
