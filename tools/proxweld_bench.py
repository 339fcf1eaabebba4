"""Timing of the tolerance weld (morig_amd.meshprep.clean with weld_tol, csrc/proxweld.hip) on seam tori: tori cut into bands with vertices
of their own along the cuts, every coordinate jittered by at most 1e-9, welded at 1e-8. Three workloads: --meshes tori of --side x
--side vertices in one batch (64 x 64: about 4 k vertices each), one torus of about 250 k faces and one of about 1 M faces. Per workload
``clean_tol_ms`` is the whole public call ``clean(weld_tol=1e-8)`` with its host reads between two device events after a warm-up, median
of the repeats, and ``clean_exact_ms`` the whole call ``clean()`` on the UNJITTERED copies (the exact weld closes those): the difference
is what the tolerance costs. The exact path is the code of the commits before the tolerance weld, unchanged. ``stages_ms`` breaks the
added work down on prepared inputs, each stage between its own device events: the cell keys (four launches), the sorts with their
gathers, the count walk, the prefix sum with the ONE added host read, the emit walk, the component rounds on the links (with their
reads) and the spread. The first small mesh also goes through the numpy oracle (tests/proxweld_oracle.py: brute force over all pairs,
no grid), timed, and ``clean``'s outputs are compared bit for bit; the oracle is not run on the large meshes (n^2 / 2 pairs). The
shader clock is sampled (bench.py's ClockSampler) over the timed repeats. One JSON line with the date; there is NO threshold.

    python tools/proxweld_bench.py [--meshes 64] [--side 64] [--large 354 708] [--repeats 5] [--exact-only] [--root DIR]

``--exact-only`` times ``clean()`` alone, and ``--root DIR`` takes the package from another checkout (built there): together they
measure the exact baseline AT THE PARENT COMMIT with this file's meshes. Run the two alternately in one visit and repeat both to see the
spread.
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

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else HERE    # the checkout whose package is timed
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))
from bench import ClockSampler                          # noqa: E402
from morig_amd import meshprep                          # noqa: E402
from morig_amd.meshbatch import MeshBatch               # noqa: E402
from morig_amd.runtime import get_ops                   # noqa: E402

TOL, JITTER, STRIPS = 1e-8, 1e-9, 8


def seam_torus(n, seed):
    """(jittered vertices, unjittered vertices, faces) of an n x n torus in STRIPS bands with their own vertices along the cuts"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = 2 * np.pi * i.ravel() / n, 2 * np.pi * j.ravel() / n
    v = np.stack([(2 + np.cos(b)) * np.cos(a), (2 + np.cos(b)) * np.sin(a), np.sin(b)], 1)
    idx = lambda p, q: (p % n) * n + (q % n)
    i, j = i.ravel(), j.ravel()
    f = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], 1), np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], 1)])
    patch = np.concatenate([i, i]) * STRIPS // n
    own, inverse = np.unique(patch[:, None] * len(v) + f, return_inverse=True)
    sv, sf = v[own % len(v)], inverse.reshape(-1, 3).astype(np.int64)
    return sv + np.random.default_rng(seed).uniform(-JITTER, JITTER, sv.shape), sv, sf


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


def stages(verts, faces, repeats):
    """the added work of ``meshprep._tolerance_weld`` stage by stage, on the inputs the stage in front of it made"""
    ops, batch = get_ops(), MeshBatch("bench", verts=verts, faces=faces)
    dev, N = batch.device, int(batch.vptr_host[-1])
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    keys, nonfinite = ops.meshcheck_coord_keys(batch.verts)
    order = torch.arange(N, dtype=torch.int64, device=dev)
    for c in (2, 1, 0):
        order = order[torch.sort(keys[c][order], stable=True).indices]
    flags = ops.meshcheck_weld_mark(keys, nonfinite, order.contiguous(), batch.vptr)
    rep0 = ops.meshcheck_run_rep(order.contiguous(), flags, torch.cumsum(flags, 0, dtype=torch.int64))
    vp = torch.from_numpy(batch.vptr_host).to(dev)
    eps = torch.full((batch.n,), TOL, dtype=torch.float64, device=dev)
    eps2 = eps * eps
    out = {}
    out["cell_keys"] = timed(lambda: ops.proxweld_cell_keys(batch.verts, nonfinite, rep0, batch.vptr, eps), repeats)
    ckeys, _ = ops.proxweld_cell_keys(batch.verts, nonfinite, rep0, batch.vptr, eps)

    def sort():
        o = torch.sort(ckeys, stable=True).indices
        if batch.n > 1:
            o = o[torch.sort(torch.searchsorted(vp[1:].contiguous(), o, right=True), stable=True).indices]
        o = o.contiguous()
        return o, ckeys[o].contiguous(), batch.verts[o].contiguous()
    out["sorts_and_gathers"] = timed(sort, repeats)
    o, skeys, spos = sort()
    out["count_links"] = timed(lambda: ops.proxweld_count_links(skeys, o, spos, batch.vptr, eps2), repeats)
    count = ops.proxweld_count_links(skeys, o, spos, batch.vptr, eps2)
    out["prefix_and_read"] = timed(lambda: (torch.cumsum(count, 0, dtype=torch.int64), meshprep._seg_sum(count, vp).cpu()), repeats)
    lrank = torch.cumsum(count, 0, dtype=torch.int64)
    total = int(lrank[-1].cpu())
    out["emit_links"] = timed(lambda: ops.proxweld_emit_links(skeys, o, spos, batch.vptr, eps2, count, lrank, total), repeats)
    links = ops.proxweld_emit_links(skeys, o, spos, batch.vptr, eps2, count, lrank, total)
    rounds = lambda: meshprep._component_rounds(ops, rows, links, batch.vptr, int(batch.nv.max()) + 2, "bench")
    out["component_rounds"] = timed(rounds, repeats)
    label, last = rounds()
    rep = label[rep0.long()].contiguous()
    out["spread"] = timed(lambda: ops.proxweld_spread(batch.verts, rep, nonfinite, batch.vptr), repeats)
    return {k: round(x, 3) for k, x in out.items()}, total, int(last.max()) + 1


def workload(name, meshes, repeats, exact_only=False):
    jit = [torch.from_numpy(m[0]).cuda() for m in meshes]
    flat = [torch.from_numpy(m[1]).cuda() for m in meshes]
    faces = [torch.from_numpy(m[2]).cuda() for m in meshes]
    if exact_only:
        exact = meshprep.clean(flat, faces, return_report=True)[1]                    # warm-up
        torch.cuda.synchronize()
        return dict(name=name, meshes=len(meshes), vertices=len(meshes[0][0]), faces=len(meshes[0][2]),
                    clean_exact_ms=round(timed(lambda: meshprep.clean(flat, faces), repeats), 3), watertight=bool(all(x["watertight"] for x in exact))), None
    out, reports = meshprep.clean(jit, faces, weld_tol=TOL, return_report=True)       # warm-up
    exact = meshprep.clean(flat, faces, return_report=True)[1]
    loose = meshprep.clean(jit[:1], faces[:1], return_report=True)[1][0]
    torch.cuda.synchronize()
    tol_ms = timed(lambda: meshprep.clean(jit, faces, weld_tol=TOL), repeats)
    exact_ms = timed(lambda: meshprep.clean(flat, faces), repeats)
    st, links, link_rounds = stages(jit, faces, repeats)
    r = reports[0]
    return dict(name=name, meshes=len(meshes), vertices=len(meshes[0][0]), faces=len(meshes[0][2]), clean_tol_ms=round(tol_ms, 3),
                clean_exact_ms=round(exact_ms, 3), stages_ms=st, links=links, link_rounds=link_rounds,
                watertight=bool(all(x["watertight"] for x in reports) and all(x["watertight"] for x in exact)), components_without_tolerance=loose["components"],
                near_verts=r["near_verts"], weld_spread=r["weld_spread"]), out[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--large", type=int, nargs="*", default=[354, 708])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--exact-only", action="store_true")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    small = [seam_torus(a.side, m) for m in range(a.meshes)]
    rows, first = workload("batch", small, a.repeats, a.exact_only)
    results = [rows]
    oracle = {}
    if not a.exact_only:
        import proxweld_oracle as po
        t0 = time.perf_counter()
        want = po.clean(small[0][0], small[0][2], TOL)
        oracle = dict(oracle_first_mesh_s=round(time.perf_counter() - t0, 2),
                      oracle_equal=bool(all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(first, want))))
    for side in a.large:
        results.append(workload(f"torus_{side}", [seam_torus(side, 1)], a.repeats, a.exact_only)[0])
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    print(json.dumps(dict(date=datetime.date.today().isoformat(), package=os.path.relpath(ROOT, HERE), tolerance=TOL, jitter=JITTER, repeats=a.repeats,
                          workloads=results, **oracle, sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
