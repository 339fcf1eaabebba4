"""GPU: morig_amd/local_motion.py (csrc/local_motion.hip) against tests/local_motion_oracle.py. Every discrete result -- ``ptr``, ``ids``,
``rung``, the status counts -- bit-equal to the oracle with nothing excused, at the smallest shapes at which the patch kernel branches
(a bitset word of 32 vertices, a wave of 64, one pass of 64 x 32 bits, the vertex limit), on fans, strips, every rung of the ladder,
coincident vertices, a degenerate face and vertices in no face. The fits under the continuous criterion of DESIGN.md section 26
(``local_motion_oracle.assert_motion_close``: 16 K0 2^-52 / gap from the oracle's singular values), with the recorded reference numbers
for the golden cases; degenerate patches by their properties only."""
import numpy as np
import pytest
import torch

import local_motion_oracle as lo
from morig_amd import local_motion as lm

pytestmark = pytest.mark.gpu


def host(t):
    return t.cpu().numpy()


def ribbon(n, spacing=0.004, seed=None):
    """a triangle strip of n vertices, faces (i, i + 1, i + 2), zigzagging along x; seed: renumbered at random"""
    i = np.arange(n, dtype=np.float64)
    v = np.stack([i * spacing, (np.arange(n) % 2) * spacing, 0.001 * np.sin(0.7 * i)], 1)
    f = np.stack([np.arange(n - 2), np.arange(n - 2) + 1, np.arange(n - 2) + 2], 1).astype(np.int64) if n >= 3 else np.zeros((0, 3), dtype=np.int64)
    return lo.shuffled(v, f, seed) if seed is not None else (v, f)


def named_meshes():
    m = {"one_vertex": (np.array([[0.1, -0.2, 0.3]]), np.zeros((0, 3), dtype=np.int64)), "triangle": ribbon(3)}
    for n in (31, 32, 33, 63, 64, 65, 2047, 2048, 2049):
        m[f"ribbon_{n}"] = ribbon(n, seed=n if n > 100 else None)
    for k in (62, 63, 64, 65, 100):                                                    # hub valence; patches of k + 1 = 63, 64, 65 members
        m[f"fan_{k}"] = lo.fan_mesh(k)
    m["strip"] = lo.strip_mesh(14)
    for k, (near, far) in enumerate(((3, (0.045, 0.07)), (4, (0.07,)), (3, (0.07, 0.07)), (2, (0.045, 0.055, 0.07)), (2, (0.045, 0.07, 0.07)),
                                     (1, (0.045, 0.045, 0.055)))):
        m[f"rung_{k}"] = lo.rung_mesh(near, far)
    m["exact_rung"] = lo.exact_rung_mesh()
    v, f = lo.grid_mesh(6, 6, 0.01, seed=5)
    v[7], v[20] = v[8], v[8]                                                           # coincident vertices
    v[3] = [-0.0, 0.0, -0.0]
    v[4] = [0.0, -0.0, 0.0]
    m["coincident"] = (v, f)
    m["degenerate_alone"] = (np.array([[0.0, 0, 0], [0.01, 0, 0]]), np.array([[0, 0, 1]]))
    v, f = lo.grid_mesh(5, 5, 0.01, seed=6)
    m["degenerate_among"] = (np.concatenate([v, [[0.021, 0.02, 0.0]]]), np.concatenate([f, [[12, 12, 25]], [[3, 3, 3]]]))
    m["isolated"] = lo.isolated_mesh()
    m["shuffled_grid"] = lo.shuffled(*lo.grid_mesh(12, 11, 0.011, seed=7), seed=8)
    return m


@pytest.fixture(scope="module")
def meshes():
    return named_meshes()


@pytest.fixture(scope="module")
def wanted(meshes):
    return {name: lo.patch_lists(v, f) for name, (v, f) in meshes.items()}


@pytest.fixture(scope="module")
def batch(meshes):
    names = list(meshes)
    return names, lm.patches([meshes[n][0] for n in names], [meshes[n][1] for n in names])


def check_patches(pat, b, want):
    """mesh b of pat against the oracle: ptr, ids, rung bit for bit"""
    p = host(pat.ptr).astype(np.int64)
    v0, v1 = pat.vptr_host[b], pat.vptr_host[b + 1]
    want_ptr, want_ids = lo.flat(want["lists"])
    assert pat.ptr.dtype == pat.ids.dtype == pat.rung.dtype == torch.int32 and pat.ptr.is_cuda
    assert np.array_equal(p[v0:v1 + 1] - p[v0], want_ptr)
    assert np.array_equal(host(pat.ids)[p[v0]:p[v1]], want_ids)
    assert np.array_equal(host(pat.rung)[v0:v1], want["rung"])


def test_patches_of_every_named_mesh_in_one_batch_equal_the_oracle(meshes, wanted, batch):
    names, pat = batch
    assert pat.n_isolated == sum(w["n_isolated"] for w in wanted.values()) == 2 and int(host(pat.ptr)[-1]) == pat.ids.numel()
    for b, name in enumerate(names):
        check_patches(pat, b, wanted[name])
    split = pat.split()
    assert [r.tolist() for r in split[names.index("degenerate_alone")]] == [[0], [1]]   # the walks of four edges, not depth <= 4
    assert split[names.index("one_vertex")][0].tolist() == [0]
    hub = split[names.index("fan_100")][0]
    assert hub.dtype == np.int64 and hub.tolist() == list(range(101))
    assert [len(split[names.index(f"fan_{k}")][0]) for k in (62, 63, 64)] == [63, 64, 65]
    assert 10 not in split[names.index("strip")][0] and 8 in split[names.index("strip")][0]
    assert 1 not in split[names.index("exact_rung")][0] and host(pat.rung)[pat.vptr_host[names.index("exact_rung")]] == 2
    rungs = [(int(host(pat.rung)[pat.vptr_host[names.index(f"rung_{k}")]]), len(split[names.index(f"rung_{k}")][0])) for k in range(6)]
    assert rungs == [(1, 5), (0, 5), (2, 4), (2, 5), (2, 4), (2, 5)]


@pytest.mark.parametrize("name", ["one_vertex", "triangle", "ribbon_33", "ribbon_2049", "fan_100", "coincident", "isolated"])
def test_a_mesh_alone_gives_the_bits_it_gives_in_the_batch_and_twice(meshes, wanted, batch, name):
    names, pat = batch
    v, f = meshes[name]
    alone, again = lm.patches([v], [f]), lm.patches([torch.as_tensor(v, device="cuda")], [torch.as_tensor(f, device="cuda")])
    check_patches(alone, 0, wanted[name])
    b = names.index(name)
    p = host(pat.ptr).astype(np.int64)
    assert np.array_equal(host(alone.ids), host(pat.ids)[p[pat.vptr_host[b]]:p[pat.vptr_host[b + 1]]])
    assert torch.equal(alone.ptr, again.ptr) and torch.equal(alone.ids, again.ids) and torch.equal(alone.rung, again.rung)
    assert alone.n_isolated == again.n_isolated == wanted[name]["n_isolated"]


def test_the_vertex_limit_and_one_more():
    v, f = ribbon(lm.MAX_VERTS, seed=11)
    pat = lm.patches([v], [f])
    check_patches(pat, 0, lo.patch_lists(v, f))
    with pytest.raises(ValueError, match="at most 32768 per mesh"):
        lm.patches([np.concatenate([v, v[:1]])], [f])


def test_refusals_come_from_the_status_words(meshes):
    v, f = meshes["shuffled_grid"]
    for bad in (f + len(v), np.concatenate([f, [[0, -1, 2]]])):
        with pytest.raises(ValueError, match="outside its mesh"):
            lm.patches([meshes["triangle"][0], v], [meshes["triangle"][1], bad])
    for bad in (np.nan, np.inf, -np.inf):
        moved = v.copy()
        moved[17, 2] = bad
        with pytest.raises(ValueError, match="no finite number"):
            lm.patches([meshes["triangle"][0], moved], [meshes["triangle"][1], f])
    bad_lists = lm.Patches.from_lists([[[0, 1, 2]] * 3])
    bad_lists.ids[1] = 7                                                                # behind the host check: the kernel clamps and flags
    with pytest.raises(ValueError, match="outside its mesh"):
        lm.local_rigid_motion([meshes["triangle"][0]], [meshes["triangle"][0][:, None]], bad_lists)


# --------------------------------------------------------------------------------------------------------------------------- fits
def run_fit(verts, trajs, pat):
    out = lm.local_rigid_motion(verts, trajs, pat)
    return out, [dict(zip(("rot6d", "trans", "gap", "residual"), (host(t) for t in part))) for part in out.split()]


@pytest.mark.parametrize("frames", [1, 2, 63, 64, 65])
def test_fits_over_clips_of_every_wave_boundary(frames):
    v, f = lo.grid_mesh(6, 5, 0.012, seed=frames)
    v2, f2 = lo.grid_mesh(4, 4, 0.015, seed=100 + frames)
    trajs = [lo.bend_clip(v, frames, 3), lo.bend_clip(v2, frames, 4)]
    pat = lm.patches([v, v2], [f, f2])
    out, got = run_fit([v, v2], trajs, pat)
    assert out.n_empty == 0 and out.rot6d.is_cuda and tuple(out.rot6d.shape) == (len(v) + len(v2), frames, 6)
    lists = pat.split()
    for b, (vb, tb) in enumerate(((v, trajs[0]), (v2, trajs[1]))):
        lo.assert_motion_close(got[b], lo.local_motion(vb, tb, lists[b]), vb, tb, lists[b], f"T {frames}, mesh {b}")
    alone, _ = run_fit([v2], trajs[1:], lm.patches([v2], [f2]))                         # alone: the bits of the batch; and twice
    again, _ = run_fit([v, v2], trajs, pat)
    for name in ("rot6d", "trans", "gap", "residual"):
        assert torch.equal(getattr(alone, name), getattr(out, name)[len(v):]) and torch.equal(getattr(again, name), getattr(out, name))


def test_patch_sizes_three_and_above_a_wave_and_an_empty_row():
    v, f = lo.fan_mesh(100)
    lists = [list(map(int, r)) for r in lo.patch_lists(v, f)["lists"]]
    lists[1], lists[4], lists[5] = [], [1, 40, 80], [5, 6, 7, 60]
    traj = lo.bend_clip(v, 3, 12)
    pat = lm.Patches.from_lists([lists], device="cuda")
    out, got = run_fit([v], [traj], pat)
    assert pat.n_empty == out.n_empty == 1 and len(lists[0]) == 101
    lo.assert_motion_close(got[0], lo.local_motion(v, traj, lists), v, traj, lists, "fan")
    assert np.isnan(got[0]["rot6d"][1]).all() and np.isnan(got[0]["residual"][1]).all()


def test_degenerate_patches_by_their_properties():
    v, f = lo.fan_mesh(12)
    v[9] = v[8]                                                                         # two coincident points
    lists = [[k] for k in range(6)] + [[0, 3], [2, 11], [8, 9], [3, 3], [1, 4], [5, 5]] + [[6]]
    traj = lo.bend_clip(v, 4, 13)
    traj[9] = traj[8]
    out, (got,) = run_fit([v], [traj], lm.Patches.from_lists([lists], device="cuda"))
    assert out.n_empty == 0 and np.isfinite(got["rot6d"]).all() and np.isfinite(got["trans"]).all()
    R = lo.rotation_of(got["rot6d"])
    assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() <= 64 * lo.EPS and np.abs(np.linalg.det(R) - 1).max() <= 64 * lo.EPS
    assert (np.abs(got["gap"]) <= 1e-9).all()                                           # rank <= 1: no unique answer, and the gap says so
    for k in list(range(6)) + [12]:                                                     # one point: the identity exactly, t = q - p
        assert (got["rot6d"][k] == [1, 0, 0, 0, 1, 0]).all() and np.array_equal(got["trans"][k], traj[lists[k][0]] - v[lists[k][0]])
    for k in (8, 9, 11):                                                                # two coincident points: M = 0, the identity too
        assert (got["rot6d"][k] == [1, 0, 0, 0, 1, 0]).all()
    for k in (6, 7, 10):                                                                  # two points: the segment's direction is carried over
        a, b = lists[k]
        d0, d1 = v[b] - v[a], traj[b] - traj[a]
        cos = np.einsum("tij,j,ti->t", R[k], d0, d1) / (np.linalg.norm(d0) * np.linalg.norm(d1, axis=1))
        assert np.abs(cos - 1).max() <= 1e-12


def test_half_turns_mirrored_planar_patches_identity_and_float32():
    v, f = lo.grid_mesh(7, 6, 0.012, seed=21)
    flat_v, flat_f = lo.grid_mesh(6, 6, 0.013, seed=22, bump=0.0)
    half = lo.rotation([1.0, -2.0, 0.5], np.pi)
    traj = np.stack([v @ half.T + 0.3, v, v @ lo.rotation([0, 0, 1], np.pi).T], 1)       # a half turn, the identity, a half turn about z
    mirrored = np.stack([flat_v * [1, -1, 1], flat_v * [-1, 1, 1] + 0.1], 1)            # reflections within the plane: the determinant rule decides
    mirrored = np.concatenate([mirrored, mirrored[:, :1]], 1)
    pat = lm.patches([v, flat_v], [f, flat_f])
    lists = pat.split()
    out, got = run_fit([v, flat_v], [traj, mirrored], pat)
    want = [lo.local_motion(v, traj, lists[0]), lo.local_motion(flat_v, mirrored, lists[1])]
    assert np.abs(lo.rotation_of(want[0]["rot6d"][:, 0]) - half).max() < 1e-12 and np.abs(want[0]["rot6d"][:, 1] - [1, 0, 0, 0, 1, 0]).max() < 1e-12
    assert np.abs(lo.rotation_of(want[1]["rot6d"][:, 0]) - np.diag([1.0, -1.0, -1.0])).max() < 1e-12
    lo.assert_motion_close(got[0], want[0], v, traj, lists[0], "half turns and identity")
    lo.assert_motion_close(got[1], want[1], flat_v, mirrored, lists[1], "mirrored planar")
    R = host(lm.rotation_matrices(out.rot6d))
    assert np.array_equal(R[..., :2].swapaxes(-1, -2).reshape(R.shape[:2] + (6,)), host(out.rot6d)) and np.abs(np.linalg.det(R) - 1).max() <= 64 * lo.EPS
    bent = lo.bend_clip(v, 2, 23).astype(np.float32)
    _, (got32,) = run_fit([v], [torch.as_tensor(bent)], lm.patches([v], [f]))
    lo.assert_motion_close(got32, lo.local_motion(v, bent, lists[0]), v, bent.astype(np.float64), lists[0], "float32 clip")


@pytest.mark.parametrize("name", sorted(lo.load_golden()))
def test_golden_cases_against_the_recorded_reference(name):
    c = lo.load_golden()[name]
    R_all, T_all, nnids = lm.gt_rotation_icp(c["verts0"], c["faces"], c["verts_t"])
    assert len(nnids) == len(c["nnids"]) and all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(nnids, c["nnids"]))
    out, (got,) = run_fit([c["verts0"]], [c["verts_t"][:, None]], lm.patches([c["verts0"]], [c["faces"]]))
    assert np.array_equal(host(R_all), got["rot6d"][:, 0]) and np.array_equal(host(T_all), got["trans"][:, 0])
    again = lm.gt_rotation_icp(c["verts0"], c["faces"], c["verts_t"], nnids)            # the recorded lists handed back
    assert torch.equal(again[0], R_all) and torch.equal(again[1], T_all)
    oracle = lo.local_motion(c["verts0"], c["verts_t"][:, None], c["nnids"])
    recorded = dict(oracle, rot6d=c["R_all"][:, None], trans=c["T_all"][:, None])
    lo.assert_motion_close(got, recorded, c["verts0"], c["verts_t"][:, None], c["nnids"], name)
