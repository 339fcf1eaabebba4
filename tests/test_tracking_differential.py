"""GPU: ``ik_solve_kernel`` and ``corr_select`` (csrc/track.hip) through morig_amd.tracking / morig_amd.native against the float64 oracle
(tests/tracking_oracle.py) on the generated cases of tests/track_cases.py: vertex counts around the second pass of the vertex loop and
the 256 -> 1 024 thread switch, joint counts that wrap step D's waves and the per-thread joint loops, a chain of depth 64, a star of 300
leaves, a full binary tree, joints owning 0 / 1 / 63 / 64 / 65 / 129 entries, vertices owning 0 / 1 / 8, dynamic LDS just under, exactly
at and just over 64 KiB on either workgroup size and up to the last vertex that fits in 160 KiB. tests/test_track_cases.py proves the
case conditions, the packing and this file's comparison code without a device.

Bounds: ten times the family maximum of the float32 twin's deviation from the float64 oracle, floored at 2^-23, positions capped at
1e-5; computed at test time and printed next to every device figure before the assert (run with -s). Where the project claims bits -- a
second run, a problem inside a batch on either workgroup size, ``with_grad=False``, joints without entries below them, a healthy
problem next to a refused one -- bits are asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_cases as tc
import tracking_oracle as tk
from morig_amd import native, tracking

pytestmark = pytest.mark.gpu
BIT_KEYS = ("angles", "trans", "locals", "globals", "jpos", "grad_angles", "grad_trans")
_cache = {}


def alone(name):
    """the case alone in a launch, computed once for the module"""
    if ("alone", name) not in _cache:
        _cache["alone", name] = tracking.ik_solve([tc.problem(name)], with_grad=True)[0]
    return _cache["alone", name]


def batch(key, with_grad=True):
    if (key, with_grad) not in _cache:
        _cache[key, with_grad] = tracking.ik_solve([tc.problem(n) for n in tc.BATCHES[key]], with_grad=with_grad)
    return _cache[key, with_grad]


# ------------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("name", tc.NAMES)
def test_against_the_float64_oracle(name):
    tc.compare("device", name, alone(name))


def test_bounds_in_use():
    print("\n" + tc.table(device={n: tc.deviation_of(alone(n), tc.case(n)["want"]) for n in tc.NAMES}))


# ------------------------------------------------------------------------------------------------------------------- bits
def test_every_case_runs_twice_with_the_same_bits():
    for name in tc.NAMES:
        again = tracking.ik_solve([tc.problem(name)], with_grad=True)[0]
        for k in again:
            assert np.array_equal(again[k], alone(name)[k]), (name, k)


@pytest.mark.parametrize("key", list(tc.BATCHES))
def test_a_case_in_a_batch_is_the_case_alone(key):
    """one launch of the 256-thread cases; the same cases forced onto 1 024 threads by neighbours of up to 2 049 vertices; the LDS giants
    with two small cases: LDS is laid out for the largest problem, max_iter exceeds most problems' own, and every problem gives the bits of
    its lone run (the loss, summed per wave, to rel 1e-6)"""
    for name, got in zip(tc.BATCHES[key], batch(key)):
        for k in BIT_KEYS:
            assert np.array_equal(got[k], alone(name)[k]), (key, name, k)
        assert float(got["loss"]) == pytest.approx(float(alone(name)["loss"]), rel=1e-6, abs=0)


@pytest.mark.parametrize("key", list(tc.BATCHES))
def test_without_the_gradient_outputs(key):
    for name, got, full in zip(tc.BATCHES[key], batch(key, with_grad=False), batch(key)):
        assert set(got) == {"angles", "trans", "locals", "globals", "jpos"}
        for k in got:
            assert np.array_equal(got[k], full[k]), (key, name, k)


# ------------------------------------------------------------------------------------------------------------------- LDS limits
def flat_problem(J, V):
    """a star of identity frames, every vertex on joint 0: the cheapest problem of a given size"""
    eye = np.repeat(np.eye(3, dtype=np.float32)[None], J, 0)
    return tracking.make_problem(eye, np.zeros((J, 3)), [-1] + [0] * (J - 1), 0, np.arange(V + 1), np.zeros(V, dtype=np.int32), np.ones(V),
                                 np.zeros((V, 3)), np.zeros((V, 3)), np.ones(V), iter_time=1)


def test_lds_limits():
    """between 64 KiB and the whole LDS of a CU the entry point raises the kernel's dynamic-LDS attribute; the last size that fits runs,
    one vertex more is refused before anything is launched"""
    ops, s = native.get_ops(), tc.lds_sizes()
    info = native.device_info()
    print(f"\ndevice: LDS per CU {info['lds_bytes_per_cu']} B, shared memory per block (the attribute the entry point asks) "
          f"{torch.cuda.get_device_properties(0).shared_memory_per_block} B")
    for name in tc.LDS_CASES:                                                   # they ran, within the same bounds
        sp = tc.SPECS[name]
        print(f"{name}: J {sp['J']} V {sp['V']} dynamic LDS {tc.lds_bytes(sp['J'], sp['V'])} B on {1024 if sp['V'] > 512 else 256} threads")
        tc.compare("device", name, alone(name))
    J, V = tc.LDS_JOINTS, s["largest"]
    fits, over = tc.lds_bytes(J, V) + tc.LDS_STATIC, tc.lds_bytes(J, V + 1) + tc.LDS_STATIC
    print(f"accepted: {fits} B (dynamic + {tc.LDS_STATIC} static) at {V} vertices; refused: {over} B at {V + 1}")
    assert fits <= tc.LDS_LIMIT < over
    t, n, max_j, max_v, max_iter, _, _ = tracking.pack_problems([flat_problem(J, V + 1)], "cuda")
    with pytest.raises(native.MorigNativeError, match="unsupported"):
        ops.ik_solve(t, n, max_j, max_v, max_iter)
    out = torch.zeros(J * 9, dtype=torch.float32, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    a = native._args(native.IkArgs)
    a.n_problems, a.max_joints, a.max_vertices, a.max_iter, a.n_entries = n, max_j, max_v, max_iter, V + 1
    for k in ops.IK_FIELDS_I32 + ops.IK_FIELDS_F32 + ops.IK_FIELDS_F64:
        setattr(a, k, t[k].data_ptr())
    for k in ("angles", "trans", "locals", "globals", "jpos"):
        setattr(a, k, out.data_ptr())
    a.status = status.data_ptr()
    assert ops.lib.morig_ik_solve(C.byref(a), None) == native._K["MORIG_E_UNSUPPORTED"]
    torch.cuda.synchronize()
    assert status.item() == -1 and float(out.abs().max()) == 0                  # nothing was launched
    # the same arrays one vertex shorter are accepted
    t, n, max_j, max_v, max_iter, _, _ = tracking.pack_problems([flat_problem(J, V)], "cuda")
    assert ops.ik_solve(t, n, max_j, max_v, max_iter)["status"].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------- the kernel's input check
HEALTHY, SMALL = "v257_j16_root_mid_w_invis", "v40_j6_binary"


def _set(key, at, value):
    def f(t, i):
        t[key][i[at[0]] + at[1]] = value(t, i) if callable(value) else value
    return f


def _swap_root(t, i):
    t["order"][i["j0"]], t["order"][i["j0"] + 1] = t["order"][i["j0"] + 1].clone(), t["order"][i["j0"]].clone()


# every corrupted value still indexes inside the launch's buffers and the LDS the launch declares: it is at most the small problem's
# J = 6 < max_joints = 16, V = 40 < max_vertices = 257, or an entry offset inside n_entries
CORRUPTIONS = {
    "parent_is_the_joint_itself": (_set("parent", ("j0", 3), 3), 2),
    "second_joint_with_parent_-1": (_set("parent", ("j0", 4), -1), 2),
    "order_entry_is_J": (_set("order", ("j0", 5), 6), 2),
    "root_not_first_in_order": (_swap_root, 2),
    "child_hi_below_child_lo": (_set("child_hi", ("j0", 0), lambda t, i: int(t["child_lo"][i["j0"]]) - 1), 2),
    "level_ptr_not_ascending": (_set("level_ptr", ("lv0", 1), 4), 2),                        # [0, 1, 3, 6] -> [0, 4, 3, 6]
    "level_ptr_starts_at_1": (_set("level_ptr", ("lv0", 0), 1), 2),
    "vptr_descending": (_set("vptr", ("v0", 5), lambda t, i: int(t["vptr"][i["v0"] + 6]) + 1), 2),
    "jptr_descending": (_set("jptr", ("j0", 2), lambda t, i: int(t["jptr"][i["j0"] + 3]) + 1), 2),
    "vent_j_is_J": (_set("vent_j", ("e0", 7), 6), 2),
    "jent_v_is_V": (_set("jent_v", ("e0", 7), 40), 2),
    "root_is_J": (_set("root", ("one", 0), 6), 1),
    "iter_time_is_0": (_set("iter_time", ("one", 0), 0), 1),
}


def input_check_batch():
    if "check" not in _cache:
        t, n, max_j, max_v, max_iter, joint_ptr, vert_ptr = tracking.pack_problems([tc.problem(HEALTHY), tc.problem(SMALL)], "cuda")
        info = dict(j0=joint_ptr[1], v0=vert_ptr[1], lv0=int(t["level_off"][1]), e0=len(tc.case(HEALTHY)["prob"]["ent_j"]), one=1)
        assert (max_j, max_v, joint_ptr[2] - joint_ptr[1], vert_ptr[2] - vert_ptr[1]) == (16, 257, 6, 40)
        assert t["level_ptr"][info["lv0"]:].tolist() == [0, 1, 3, 6] and int(t["child_lo"][info["j0"]]) == 1
        assert int(t["vptr"][info["v0"] + 6]) + 1 <= t["vent_j"].numel() and int(t["jptr"][info["j0"] + 3]) + 1 <= t["vent_j"].numel()
        _cache["check"] = (t, (n, max_j, max_v, max_iter), info)
    return _cache["check"]


def test_input_check_batch_is_healthy_before_it_is_corrupted():
    t, sizes, info = input_check_batch()
    out = native.get_ops().ik_solve(t, *sizes, with_grad=True)
    assert out["status"].tolist() == [0, 0]
    for k in BIT_KEYS[:5]:
        assert np.array_equal(out[k][info["j0"] if k != "trans" else 1:].cpu().numpy().reshape(alone(SMALL)[k].shape), alone(SMALL)[k]), k


@pytest.mark.parametrize("what", list(CORRUPTIONS))
def test_the_kernel_refuses_a_corrupted_table(what):
    """a batch of two: the smaller problem carries ONE corrupted table entry and is refused by its workgroup (status 2; 1 for the size
    checks), the healthy problem in front of it keeps the bits of its lone run"""
    clean, sizes, info = input_check_batch()
    t = {k: v.clone() for k, v in clean.items()}
    corrupt, status = CORRUPTIONS[what]
    corrupt(t, info)
    assert sum(int((t[k] != clean[k]).sum()) for k in t) == (2 if what == "root_not_first_in_order" else 1)
    out = native.get_ops().ik_solve(t, *sizes, with_grad=True)
    assert out["status"].tolist() == [0, status]
    want, J = alone(HEALTHY), info["j0"]
    for k in BIT_KEYS:
        got = out[k][0] if k in ("trans", "grad_trans") else out[k][:J]
        assert np.array_equal(got.cpu().numpy(), want[k]), (what, k)
    assert float(out["loss"][0]) == float(want["loss"])


# ------------------------------------------------------------------------------------------------------------------- corr_select
def select(nn, sim, n_pts):
    """device against tracking_oracle.select_pairs; a vertex that names no point of the range takes no part"""
    nn, sim = np.asarray(nn, dtype=np.int32), np.asarray(sim, dtype=np.float32)
    winner, wsim = native.get_ops().corr_select(torch.from_numpy(nn).cuda(), torch.from_numpy(sim).cuda(), n_pts)
    valid = (nn >= 0) & (nn < n_pts)
    with np.errstate(invalid="ignore"):                                         # the oracle's runner-up margin meets inf - inf
        want, best, _ = tk.select_pairs(np.where(valid, sim, np.float32(-1.0)), np.where(valid, nn, 0), n_pts)
    assert np.array_equal(winner.cpu().numpy(), want), (winner.cpu().numpy(), want)
    assert np.array_equal(wsim.cpu().numpy(), best.astype(np.float32))
    return want, best


@pytest.mark.parametrize("n_pts", [1, 257])
@pytest.mark.parametrize("n_vtx", [1, 255, 256, 257, 1000])
def test_corr_select_against_the_oracle(n_vtx, n_pts):
    rng = np.random.default_rng([tc.TAG, n_vtx, n_pts])
    # random: some points nobody names (n_pts = 257 has more points than most vertex counts), similarities of either sign
    nn, sim = rng.integers(0, n_pts, size=n_vtx), rng.uniform(-0.2, 1.0, size=n_vtx).astype(np.float32)
    want, _ = select(nn, sim, n_pts)
    assert n_pts == 1 or (want < 0).any()
    # every vertex names point 0 with one similarity: the lowest vertex wins, across every block boundary
    want, _ = select(np.zeros(n_vtx), np.full(n_vtx, 0.75), n_pts)
    assert want[0] == 0 and np.all(want[1:] == -1)
    # the two largest, equal, on either side of a block boundary (or the last two vertices): the lower one wins
    hi = min(256, n_vtx - 1)
    sim = rng.uniform(0.1, 0.9, size=n_vtx).astype(np.float32)
    sim[[max(hi - 1, 0), hi]] = 0.95
    want, best = select(np.zeros(n_vtx), sim, n_pts)
    assert want[0] == max(hi - 1, 0) and best[0] == np.float32(0.95)
    # nn of -1 and of n_pts take no part, although they carry the largest similarity
    nn, sim = rng.integers(0, n_pts, size=n_vtx), rng.uniform(0.1, 0.9, size=n_vtx).astype(np.float32)
    nn[::3], sim[::3] = np.where(np.arange(len(nn[::3])) % 2 == 0, -1, n_pts), 2.0
    want, best = select(nn, sim, n_pts)
    assert best.max(initial=0) < 1.0 and not np.isin(want, np.arange(n_vtx)[::3]).any()


@pytest.mark.parametrize("n_vtx", [6, 257])
def test_corr_select_special_similarities(n_vtx):
    """-0.0 and 0.0 win nothing (similarity has to be positive), the smallest positive denormal does, +inf beats every finite value, NaN
    takes no part: one point per value, then all of them on one point"""
    tiny = np.float32(np.finfo(np.float32).smallest_subnormal)
    values = np.array([-0.0, 0.0, tiny, np.inf, np.nan, 0.5], dtype=np.float32)
    sim = np.resize(values, n_vtx)
    nn = np.arange(n_vtx) % 6
    want, best = select(nn, sim, 7)
    assert want.tolist() == [-1, -1, 2, 3, -1, 5, -1] and best[2] == tiny and best[3] == np.inf
    want, _ = select(np.zeros(n_vtx), sim, 2)
    assert want.tolist() == [3, -1]
    want, _ = select(np.zeros(n_vtx), np.where(np.isinf(sim), np.float32(np.nan), sim), 2)      # NaN in front of the winner
    assert want.tolist() == [5, -1]
    want, best = select(np.zeros(n_vtx), np.resize(values[:3], n_vtx), 1)                        # the denormal alone is positive
    assert want.tolist() == [2] and best[0] == tiny
