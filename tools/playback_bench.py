"""Timing of motion playback (morig_amd/playback.py) for a batch: --meshes rigs of about --joints joints (random trees, float32 joints)
with --vertices vertices of up to four weights each, a clip of --frames random-walk frames, inputs already on the device. ``replay_ms``
is the whole public call between two device events after a warm-up, median over the repeats: the tables built on the host and uploaded,
the concatenations, the five launches and the status read. ``*_kernel_ms`` are the library's own event pairs: ``pose_skin`` is the
skinning kernel alone, and ``skin_write_GBps`` its 24 bytes per (vertex, frame) over that time; ``pose_prep`` is validate + quaternions +
forward kinematics + local vertices together. ``host_s`` is the path this replaces -- per frame a deep copy of the rig, ``Rig.fk`` and
``tracking.skin_vertices`` in numpy, with scipy's Rotation for the matrices -- measured on the first --host-meshes meshes on this
machine's CPU and scaled to the batch; its trajectories are compared with the device's first. The shader clock is sampled (bench.py's
ClockSampler) while the call runs back to back for --clock-seconds after the timed repeats. One JSON line; there is NO threshold.

    python tools/playback_bench.py [--meshes 64] [--vertices 4096] [--joints 30] [--frames 100] [--repeats 5] [--host-meshes 2]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ClockSampler                          # noqa: E402
from morig_amd import native, playback, tracking        # noqa: E402
from morig_amd.formats import Rig                       # noqa: E402


def make_batch(n_meshes, V, J, T, seed=0):
    rng = np.random.default_rng([0x506C6179, seed])
    rigs, vtx, quats = [], [], []
    for _ in range(n_meshes):
        j = int(J + rng.integers(-3, 4))
        hier = np.array([-1] + [int(rng.integers(0, i)) for i in range(1, j)])
        pick = rng.random((V, j)).argsort(1)[:, :4]                              # up to four distinct joints per vertex
        w = rng.uniform(0.1, 1.0, pick.shape) * (np.arange(pick.shape[1])[None, :] < rng.integers(1, 5, V)[:, None])
        skins = np.zeros((V, j))
        np.put_along_axis(skins, pick, w / w.sum(1, keepdims=True), 1)
        rigs.append(Rig.from_arrays(rng.uniform(-0.5, 0.5, (j, 3)).astype(np.float32), hier, 0, skins=skins))
        vtx.append(rng.uniform(-0.5, 0.5, (V, 3)))
        r, q = Rotation.from_rotvec(rng.normal(size=(j, 3))), np.zeros((j, T, 4))
        for t in range(T):                                   # steps of about 0.15 rad about random axes
            q[:, t] = r.as_quat()
            r = Rotation.from_rotvec(rng.normal(size=(j, 3)) * 0.09) * r
        quats.append(q)
    return rigs, vtx, quats


def host_replay(rig, vtx, quats):
    """the host path: smoothing in numpy, then per frame Rotation -> Rig.fk on a copy -> tracking.skin_vertices"""
    q = quats.copy()
    for _ in range(2):
        q[:, 1:-1] = (q[:, 1:-1] + 0.5 * q[:, 2:] + 0.5 * q[:, :-2]) / 2.0
    _, ev, ej, w = tracking.skin_entries(rig.skins)
    local, _ = tracking.local_vertices(rig.global_transforms_homogeneous, vtx, ev, ej)
    frames = []
    for t in range(q.shape[1]):
        upd = copy.deepcopy(rig)
        upd.local_frames = Rotation.from_quat(q[:, t]).as_matrix()
        upd.fk()
        frames.append(tracking.skin_vertices(upd.global_transforms_homogeneous, local, ev, ej, w, len(vtx)))
    return np.stack(frames, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--joints", type=int, default=30)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-meshes", type=int, default=2)
    ap.add_argument("--clock-seconds", type=float, default=1.5)
    a = ap.parse_args()
    rigs, vtx, quats = make_batch(a.meshes, a.vertices, a.joints, a.frames)
    for r in rigs:                                           # the entries on the device, as rigging.assemble_rigs(entries=True) leaves them
        vptr, ev, ej, w = tracking.skin_entries(r.skins)
        r.skin_entries_device = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (vptr, ev.astype(np.int32), ej.astype(np.int32), w))
    dv, dq = [torch.from_numpy(v).cuda() for v in vtx], [torch.from_numpy(q).cuda() for q in quats]
    native.prof_enable(True)
    native.prof_reset()
    res = playback.replay(rigs, dv, dq)                      # warm-up
    times = []
    for _ in range(a.repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        res = playback.replay(rigs, dv, dq)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    prof = native.prof_collect()
    native.prof_enable(False)
    calls = a.repeats + 1
    kernel = lambda name: round(prof[name]["ms"] / calls, 4) if name in prof else None
    sampler, t_start = ClockSampler(index=0, period=0.02).start(), time.perf_counter()
    while time.perf_counter() - t_start < a.clock_seconds:
        playback.replay(rigs, dv, dq)
    torch.cuda.synchronize()
    clocks = sampler.stop().summary(t_start, time.perf_counter())
    gt = [r[0] + 0.01 for r in res]
    mask = [torch.ones(r[0].shape[:2], device="cuda") for r in res]
    playback.trajectory_errors([r[0] for r in res], gt, mask)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    playback.trajectory_errors([r[0] for r in res], gt, mask)
    stop.record()
    torch.cuda.synchronize()
    errors_ms = start.elapsed_time(stop)
    worst, t0 = 0.0, time.perf_counter()
    host = [host_replay(rigs[m], vtx[m], quats[m]) for m in range(min(a.host_meshes, a.meshes))]
    host_s = (time.perf_counter() - t0) / max(1, len(host)) * a.meshes
    for m, h in enumerate(host):
        worst = max(worst, float(np.abs(res[m][0].cpu().numpy() - h).max()))
    cells = sum(len(v) for v in vtx) * a.frames
    skin_ms = kernel("pose_skin")
    print(json.dumps(dict(meshes=a.meshes, vertices=a.vertices, joints=[min(len(r.names) for r in rigs), max(len(r.names) for r in rigs)],
                          frames=a.frames, skin_entries=int(sum(np.count_nonzero(r.skins) for r in rigs)), vertex_frames=cells,
                          replay_ms=round(statistics.median(times), 3), pose_prep_kernels_ms=kernel("pose_prep"), pose_skin_kernel_ms=skin_ms,
                          skin_write_GBps=round(24.0 * cells / (skin_ms * 1e-3) / 1e9, 1) if skin_ms else None,
                          trajectory_errors_ms=round(errors_ms, 3), host_meshes=len(host), host_s=round(host_s, 2),
                          host_vs_device_max_abs=worst, sclk_under_load_mhz=clocks["sclk_under_load_mhz"], clock_source=clocks["source"])))


if __name__ == "__main__":
    main()
