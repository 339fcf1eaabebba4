"""CPU: (1) the host logic of morig_amd/piecewise.py and tracking.track_piecewise on an emulated op layer (tests/piecewise_emulate.py
through ``runtime._test_ops``): the label renumbering, the handle CSR, the order of the sample draws and their reproduction from a seed
alone, the slicing of a batch, the error paths; (2) the rigid-fit core csrc/kabsch_core.h as the stand-alone program
tools/kabsch_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program (never loaded into Python),
against the rotations recorded from the reference's own fits."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import piecewise_emulate
import piecewise_oracle as po
from morig_amd import piecewise, runtime, tracking
from morig_amd.abi import MorigNativeError
from test_piecewise_oracle import K_META, KCASES, MESHES, ORACLE_TOL, PROBLEMS, R_ARR, R_META, SAMPLES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = piecewise_emulate.PiecewiseOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def lists(meshes=MESHES):
    return tuple([m[k] for m in meshes] for k in ("src", "dst", "vis", "seg"))


_cache = {}


def batch_run():
    """the golden batch through piecewise.py over the emulated ops, once (the caller holds the ``ops`` fixture)"""
    if "b" not in _cache:
        details, before = [], len(runtime._test_ops.calls)
        out = piecewise.piecewise_ransac(*lists(), samples=SAMPLES, details=details)
        _cache["b"] = (out, details, runtime._test_ops.calls[before:])
    return _cache["b"]


# ------------------------------------------------------------------------------------------------------------------------- draws
def test_draws_reproduce_the_reference_run_from_its_seed_alone():
    counts = [h for m in MESHES for h in m["handle_counts"]]
    got = piecewise.draw_ransac_samples(counts, rng=np.random.RandomState(R_META["seed"]))
    assert got.dtype == np.int32 and got.shape == SAMPLES.shape and np.array_equal(got, SAMPLES)
    state = np.random.get_state()
    try:
        np.random.seed(R_META["seed"])                                         # rng=None: numpy's global generator, as the reference uses it
        assert np.array_equal(piecewise.draw_ransac_samples(counts), SAMPLES)
    finally:
        np.random.set_state(state)
    assert piecewise.draw_ransac_samples([3, 0, 2]).shape == (0, 100, 3)       # nothing below 4 handles draws
    few = piecewise.draw_ransac_samples([3, 5, 1, 4], n_iter=7, rng=np.random.RandomState(1))
    want = np.random.RandomState(1)
    assert few.shape == (2, 7, 3) and np.array_equal(few[0, 0], want.permutation(5)[:3]) and few[1].max() < 4
    for row in few.reshape(-1, 3):
        assert len(set(row)) == 3


def test_samples_are_drawn_inside_when_none_are_given(ops):
    rng = np.random.RandomState(R_META["seed"])
    out = piecewise.piecewise_ransac(*lists(), rng=rng)                        # the same draws as the recorded ones
    for a, b in zip(out, batch_run()[0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------- plumbing
def test_plan_renumbers_labels_and_lists_handles_in_vertex_order(ops):
    src, dst, vis, seg = lists()
    n = [len(s) for s in src]
    mesh_of = torch.repeat_interleave(torch.arange(len(n)), torch.tensor(n))
    plan = piecewise.RansacPlan(torch.from_numpy(np.concatenate(vis)), torch.from_numpy(np.concatenate(seg)), mesh_of, 0.3)
    assert list(plan.handle_counts) == [h for m in MESHES for h in m["handle_counts"]]
    assert plan.n_problems == len(PROBLEMS) and plan.hptr.dtype == plan.handles.dtype == plan.problem_of.dtype == torch.int32
    off = np.concatenate([[0], np.cumsum(n)])
    hp, h = plan.hptr.numpy(), plan.handles.numpy()
    for p, want in enumerate(PROBLEMS):
        s = plan.problem_segment[p]
        assert (int(plan.segment_mesh[s]), int(plan.segment_label[s])) == (want["mesh"], want["label"])
        assert np.array_equal(h[hp[p]:hp[p + 1]] - off[want["mesh"]], want["handles"])
        members = np.nonzero(plan.problem_of.numpy() == p)[0] - off[want["mesh"]]
        assert np.array_equal(members, np.nonzero(MESHES[want["mesh"]]["seg"] == want["label"])[0])
    assert np.sum(plan.problem_of.numpy() == -1) == sum(np.sum(po.renumber(m["seg"]) == l) for m in MESHES
                                                        for l, c in enumerate(m["handle_counts"]) if c < 4)


def test_batch_over_the_emulated_ops_equals_the_reference(ops):
    out, details, calls = batch_run()
    assert calls == ["ransac_vote", "ransac_fit", "ransac_apply"]              # three launches for the whole batch
    for o, m, s in zip(out, MESHES, lists()[0]):
        assert o.dtype == torch.float64 and o.shape == m["out"].shape and np.abs(o.numpy() - m["out"]).max() < ORACLE_TOL
        assert o.data_ptr() != torch.as_tensor(s).data_ptr()                   # a new tensor: vert_src is not written
    assert len(details) == len(PROBLEMS)
    for d, p in zip(details, PROBLEMS):
        assert (d["mesh"], d["label"], d["by_count"], d["best_count"], d["refit"]) == (p["mesh"], p["label"], p["by_count"], p["best_count"], p["refit"])
        assert np.array_equal(d["handles"], p["handles"]) and np.array_equal(d["counts"], p["counts"])
        assert p["refit"] or d["by_sum"] == p["by_sum"]
        assert np.abs(d["R"] - p["R"]).max() < ORACLE_TOL and np.abs(d["t"] - p["t"]).max() < ORACLE_TOL


def test_a_mesh_alone_equals_its_slice_of_the_batch(ops):
    out = batch_run()[0]
    at = 0
    for i, m in enumerate(MESHES):
        n = sum(h >= 4 for h in m["handle_counts"])
        alone, = piecewise.piecewise_ransac(*lists([m]), samples=SAMPLES[at:at + n])
        assert torch.equal(alone, out[i])
        at += n


def test_float32_inputs_are_promoted(ops):
    m = MESHES[2]
    out, = piecewise.piecewise_ransac([m["src"].astype(np.float32)], [torch.from_numpy(m["dst"]).float()], [m["vis"].astype(np.float32)],
                                      [m["seg"].astype(np.int32)], samples=SAMPLES[-1:])
    assert out.dtype == torch.float64 and np.abs(out.numpy() - m["out"]).max() < 1e-5


# ------------------------------------------------------------------------------------------------------------------------- errors
def test_error_paths(ops):
    src, dst, vis, seg = lists([MESHES[2]])
    with pytest.raises(ValueError, match="one entry per mesh"):
        piecewise.piecewise_ransac(src, dst, vis, [])
    with pytest.raises(ValueError, match="samples of shape"):
        piecewise.piecewise_ransac(src, dst, vis, seg, samples=SAMPLES[:2])
    bad = SAMPLES[-1:].copy()
    bad[0, 3, 1] = 29                                                          # the segment has 29 handles
    with pytest.raises(ValueError, match="names no handle"):
        piecewise.piecewise_ransac(src, dst, vis, seg, samples=bad)
    # every distance sum is 1e10 or more: the reference ends on R = None
    far = [MESHES[1]["dst"].copy()]
    far[0][MESHES[1]["seg"] == 40] *= 1e12                                     # (a shift alone would be fitted away)
    with pytest.raises(ValueError, match="mesh 0, label 40"):
        piecewise.piecewise_ransac([MESHES[1]["src"]], far, [MESHES[1]["vis"]], [MESHES[1]["seg"]], samples=SAMPLES[4:7])


def test_kmeans_size_refusal(ops):
    v = np.zeros((80, 3))
    with pytest.raises(ValueError, match="n_clusters 65"):
        piecewise.kernel_kmeans([np.zeros((80, 8), dtype=np.float32)], [v], n_clusters=65, first=[0])
    with pytest.raises(ValueError, match="D 129"):
        piecewise.kernel_kmeans([np.zeros((80, 129), dtype=np.float32)], [v], first=[0])
    assert ops.calls == []                                                     # refused before any op
    with pytest.raises(MorigNativeError):                                      # the op layer refuses by status on its own
        ops.kernel_kmeans(torch.zeros(80, 129), torch.zeros(80, 3, dtype=torch.float64), torch.tensor([0, 80], dtype=torch.int32),
                          torch.tensor([0], dtype=torch.int32), 20, 100, 0.2, 1e-4)
    with pytest.raises(ValueError, match="first names one vertex"):
        piecewise.kernel_kmeans([np.zeros((80, 8), dtype=np.float32)], [v], first=[80])
    with pytest.raises(ValueError, match="no cluster keeps"):                  # 8 vertices: no cluster can have more than 8 members
        piecewise.kernel_kmeans([np.eye(8, dtype=np.float32)], [np.arange(24.0).reshape(8, 3)], n_clusters=2, first=[0])


# ------------------------------------------------------------------------------------------------------------------------- k-means
def test_kmeans_over_the_emulated_ops(ops):
    rng = np.random.RandomState(K_META["seed"])                                # one randint per mesh, in the reference's order
    for c in KCASES:
        (labels,), (st,) = piecewise.kernel_kmeans([c["X"]], [c["verts"]], n_clusters=c["K"], max_iter=c["max_iter"], rng=rng,
                                                   return_state=True)
        assert labels.dtype == torch.int64 and np.array_equal(labels.numpy(), c["labels"]), c["name"]
        assert np.array_equal(st["seeds"], c["seeds"]) and st["seeds"][0] == c["first"]
        assert (st["n_iter"], st["n_kept"]) == (c["n_iter"], c["n_kept"]) and np.array_equal(st["members"], c["members"])
    a, b = KCASES[3], KCASES[4]                                                # two meshes of one width in one call
    both = piecewise.kernel_kmeans([a["X"], b["X"]], [a["verts"], b["verts"]], n_clusters=6, first=[a["first"], b["first"]])
    assert np.array_equal(both[0].numpy(), a["labels"]) and len(both[1]) == b["V"]


# ------------------------------------------------------------------------------------------------------------------------- segments
def test_segments_from_skins_dense_and_entries():
    rng = np.random.default_rng(5)
    skins = rng.uniform(0, 1, (50, 7)) * (rng.uniform(0, 1, (50, 7)) > 0.5)
    skins[3] = 0.0                                                             # an empty row: joint 0
    skins[4] = [0, 0.4, 0.4, 0, 0.1, 0, 0]                                     # a tie: the first
    skins[:, 6] = 0.0                                                          # a trailing joint without an entry
    want = np.argmax(skins, axis=1)
    vptr, ev, ej, w = tracking.skin_entries(skins)
    entries = tuple(torch.from_numpy(np.asarray(a)) for a in (vptr, ev, ej, w))
    dense, from_entries, from_tensor = piecewise.segments_from_skins([skins, entries, torch.from_numpy(skins)])
    for got in (dense, from_entries, from_tensor):
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert want[3] == 0 and want[4] == 1


# ------------------------------------------------------------------------------------------------------------------------- the loop
def test_track_piecewise_equals_its_per_frame_composition(ops, monkeypatch):
    meshes = [MESHES[1], MESHES[2]]
    T = 3
    rng = np.random.default_rng(9)
    pts_traj = [rng.normal(size=(11, T, 3)) for _ in meshes]

    def stub(net, vtx, pts, tpl_e, geo_e, device):                             # the target: the recorded motion applied again, shifted by the frame's points
        return [(np.asarray(v) + (m["dst"] - m["src"]) + p.mean(), m["vis"].astype(np.float32), None, None)
                for v, p, m in zip(vtx, pts, meshes)]

    monkeypatch.setattr(tracking, "deform_inference", stub)
    segs = [m["seg"] for m in meshes]
    got = tracking.track_piecewise([m["src"] for m in meshes], segs, pts_traj, [None, None], [None, None], None, rng=np.random.RandomState(4))
    draws = np.random.RandomState(4)
    prev = [m["src"] for m in meshes]
    for t in range(1, T):
        inf = stub(None, prev, [p[:, t] for p in pts_traj], None, None, None)
        prev = [o.numpy() for o in piecewise.piecewise_ransac(prev, [i[0] for i in inf], [i[1] for i in inf], segs, rng=draws)]
        for m in range(2):
            assert np.array_equal(got[m][0][:, t - 1], prev[m]) and np.array_equal(got[m][1][:, t - 1], inf[m][1])
    assert got[0][0].shape == (180, T - 1, 3) and got[0][1].shape == (180, T - 1)
    full, vis = tracking.flow_errors(got[0][0], np.repeat(meshes[0]["src"][:, None], T, 1), np.ones((180, T)))
    assert np.isfinite(full) and np.isfinite(vis)


# ------------------------------------------------------------------------------------------------------------ the host program
def test_kabsch_core_under_the_sanitizers_equals_the_recorded_rotations(tmp_path):
    exe = str(tmp_path / "kabsch_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "kabsch_host_check.cpp"), "-o", exe], check=True)
    M, R = R_ARR["fit_M"], R_ARR["fit_R"]
    extra = np.stack([np.zeros((3, 3)), np.eye(3), np.diag([1.0, 0.0, 0.0]), np.full((3, 3), np.nan)])      # degenerate input must not trip
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(M) + len(extra)))
        f.write(np.ascontiguousarray(np.concatenate([M, extra])).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    raw = open(dst, "rb").read()
    n = len(M) + len(extra)
    got = np.frombuffer(raw[:n * 72], dtype=np.float64).reshape(n, 3, 3)
    sweeps = np.frombuffer(raw[n * 72:], dtype=np.int32)
    worst = float(np.abs(got[:len(M)] - R).max())
    print(f"kabsch_core.h vs the reference's SVD rotations on {len(M)} recorded fits: {worst:.2e}, at most {sweeps[:len(M)].max()} sweeps")
    assert worst < ORACLE_TOL and sweeps.max() <= 16
    assert np.array_equal(got[len(M)], np.eye(3)) and np.array_equal(got[len(M) + 1], np.eye(3))
    for r in got[:len(M) + 3]:                                                 # proper rotations
        assert np.abs(r @ r.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(r) - 1) < 1e-14
