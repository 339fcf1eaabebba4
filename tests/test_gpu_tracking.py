"""csrc/track.hip and morig_amd/tracking.py on the device, against the reference's recorded results (tests/golden/track_*.npz).

Tolerances are measured, not chosen: per case the generator stored the deviation of the reference's float32 result from the float64
oracle; the device -- the same arithmetic in another summation order -- has to stay within TEN times that of the reference's result, with
1e-5 absolute as the outer cap on every position-like quantity (meshes live in the unit box). Every figure is printed before it is
asserted (run with -s); the stored deviations are tabulated in DESIGN.md section 13.
"""
import numpy as np
import pytest
import torch

import tracking_oracle as tk
from morig_amd import formats, models, native, synth, tracking
from test_tracking_host import drag_rig
from test_tracking_oracle import DRAG, DRAG_META, SOLVE, SOLVE_META, solve_problem

pytestmark = pytest.mark.gpu
FACTOR, CAP = 10.0, 1e-5
_cache = {}


def problem(name):
    par, p = SOLVE_META["params"][name], solve_problem(SOLVE, SOLVE_META, name)
    return tracking.make_problem(p["locals_in"], p["offsets"], p["parent"], p["root"], p["vptr"], p["ent_j"], p["ent_w"], p["ent_x"],
                                 p["constraints"], p["vismask"], par["iter_time"], par["lr"], par["w_invis"], par["thrd"])


def single(name):
    """the case alone in a launch, computed once for the module"""
    if name not in _cache:
        _cache[name] = tracking.ik_solve([problem(name)], with_grad=True)[0]
    return _cache[name]


def batch():
    if "batch" not in _cache:
        _cache["batch"] = tracking.ik_solve([problem(n) for n in SOLVE_META["cases"]], with_grad=True)
    return _cache["batch"]


def posed_f32(res, prob):
    """the posed vertices of a result, float32 sums in entry order as the kernel forms them"""
    ev = np.repeat(np.arange(len(prob["vismask"])), np.diff(prob["vptr"]))
    contrib = prob["ent_w"][:, None].astype(np.float64) * (np.einsum("eab,eb->ea", res["globals"][prob["ent_j"]].astype(np.float64),
                                                                     prob["ent_x"].astype(np.float64)) + res["jpos"][prob["ent_j"]])
    out = np.zeros((len(prob["vismask"]), 3))
    np.add.at(out, ev, contrib)
    return out


@pytest.mark.parametrize("name", SOLVE_META["cases"])
def test_solve_against_the_reference(name):
    """J = 1, J = 2 with one vertex, a chain, a star rooted at joint 3, zero-weight joints, V in {1, 63, 65, 1025}, an all-invisible mask,
    w_invis > 0, iter_time 1 / 2 / 200 / 400, both learning rates: angles, translation, locals, globals, jpos, posed vertices, and the last
    iteration's loss and gradient"""
    got, dev, prob = single(name), SOLVE_META["deviations"][name], problem(name)
    d_ang = max(np.abs(got["angles"] - SOLVE[f"{name}_angles"]).max(), np.abs(got["trans"] - SOLVE[f"{name}_trans"]).max())
    d_vtx = max(np.abs(got[k] - SOLVE[f"{name}_{k}"]).max() for k in ("locals", "globals", "jpos"))
    d_vtx = max(d_vtx, np.abs(posed_f32(got, prob) - SOLVE[f"{name}_posed"]).max())
    want_loss = float(SOLVE[f"{name}_loss"])
    d_loss = abs(float(got["loss"]) - want_loss) / max(abs(want_loss), 1e-30)
    g_scale = max(np.abs(SOLVE[f"{name}_g_angles"]).max(), np.abs(SOLVE[f"{name}_g_trans"]).max(), 1e-30)
    d_grad = max(np.abs(got["grad_angles"] - SOLVE[f"{name}_g_angles"]).max(), np.abs(got["grad_trans"] - SOLVE[f"{name}_g_trans"]).max()) / g_scale
    print(f"\n{name}: device - reference: angles {d_ang:.3e} (bound {FACTOR * dev['dev_angles']:.3e}), positions {d_vtx:.3e} "
          f"(bound {min(FACTOR * dev['dev_vertices'], CAP):.3e}), loss rel {d_loss:.3e} (bound {FACTOR * dev['dev_loss']:.3e}), "
          f"gradient rel {d_grad:.3e} (bound {FACTOR * dev['dev_grad']:.3e})")
    assert d_ang <= FACTOR * dev["dev_angles"]
    assert d_vtx <= min(FACTOR * dev["dev_vertices"], CAP)
    assert d_loss <= FACTOR * dev["dev_loss"]
    assert d_grad <= FACTOR * dev["dev_grad"]
    silent = np.setdiff1d(np.arange(len(prob["parent"])), prob["ent_j"])
    assert np.all(got["grad_angles"][silent] == 0)                              # quirk (iii): exactly zero, not skipped, not noisy


def test_one_iteration_returns_the_initial_pose():
    """quirk (i): the returned frames are the last forward's -- after one iteration forward kinematics at 0.01 -- the parameters have stepped"""
    got, prob = single("one_iteration"), solve_problem(SOLVE, SOLVE_META, "one_iteration")
    J = len(prob["parent"])
    L, G, P = tk.forward(np.full((J, 3), np.float32(0.01), dtype=np.float64), np.full(3, np.float64(np.float32(0.01))), prob)
    assert np.abs(got["locals"] - L).max() <= 3e-7 and np.abs(got["globals"] - G).max() <= 3e-7 and np.abs(got["jpos"] - P).max() <= 3e-7
    assert np.abs(got["angles"] - 0.01).min() > 1e-3


def test_ragged_batch_in_one_launch():
    """eight problems with different J, V, depth, iter_time, lr and w_invis in ONE launch: every problem as when it runs alone, bit for
    bit (the sums of a problem do not depend on its neighbours or on the workgroup size the batch picks; the loss is reduced per wave)"""
    for name, got in zip(SOLVE_META["cases"], batch()):
        alone = single(name)
        for k in ("angles", "trans", "locals", "globals", "jpos", "grad_angles", "grad_trans"):
            assert np.array_equal(got[k], alone[k]), (name, k)
        assert float(got["loss"]) == pytest.approx(float(alone["loss"]), rel=1e-6, abs=0)


def test_two_runs_are_bit_identical():
    again = tracking.ik_solve([problem(n) for n in SOLVE_META["cases"]], with_grad=True)
    for a, b in zip(again, batch()):
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_a_problem_too_large_for_lds_is_refused():
    """16 384 vertices need 192 KiB of residuals: more than a workgroup can hold, so the launch is refused with a status and nothing runs"""
    V = 16384
    eye = np.eye(3, dtype=np.float32)[None]
    big = tracking.make_problem(eye, np.zeros((1, 3)), [-1], 0, np.arange(V + 1), np.zeros(V, dtype=np.int32), np.ones(V), np.zeros((V, 3)),
                                np.zeros((V, 3)), np.ones(V), iter_time=1)
    ops = native.get_ops()
    assert ops.ik_solve_lds_bytes(1, V) > 160 * 1024
    t, n, max_j, max_v, max_iter, _, _ = tracking.pack_problems([big], "cuda")
    a = native._args(native.IkArgs)
    with pytest.raises(native.MorigNativeError, match="unsupported"):
        ops.ik_solve(t, n, max_j, max_v, max_iter)
    # and straight through the C ABI: MORIG_E_UNSUPPORTED (-2)
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    a.n_problems, a.max_joints, a.max_vertices, a.max_iter, a.n_entries = n, max_j, max_v, max_iter, V
    for k in ops.IK_FIELDS_I32 + ops.IK_FIELDS_F32 + ops.IK_FIELDS_F64:
        setattr(a, k, t[k].data_ptr())
    for k in ("angles", "trans", "locals", "globals", "jpos"):
        setattr(a, k, out.data_ptr())
    a.status = status.data_ptr()
    import ctypes as C
    assert ops.lib.morig_ik_solve(C.byref(a), None) == -2
    torch.cuda.synchronize()
    assert status.item() == -1 and float(out.abs().max()) == 0                  # nothing ran
    # a problem larger than the sizes the launch declares is refused by its workgroup, the others run
    small = problem("one_iteration")
    t2, n2, mj, mv, mi, _, _ = tracking.pack_problems([small, problem("chain")], "cuda")
    res = ops.ik_solve(t2, n2, mj, 63, mi)                                      # chain has 65 vertices
    assert res["status"].tolist() == [0, 1]
    assert np.array_equal(res["angles"][:5].cpu().numpy(), single("one_iteration")["angles"])


def drag_inputs(name):
    return ([DRAG[f"{name}_vtx_src"]], [DRAG[f"{name}_vtx_dst"]], [DRAG[f"{name}_pts"]], [drag_rig(name)])


@pytest.mark.parametrize("name", DRAG_META["cases"])
def test_ik_drag_end_to_end(name):
    """both solves, the selection from the features on the device (similarity GEMM with row arg-max, per-point winner, no V x P matrix),
    rig updates, final skinning, quaternions: the kept pair lists EXACTLY, vertices and frames within ten times the stored deviations"""
    details = []
    vtx, rigs, quats = tracking.ik_drag(*drag_inputs(name), vtx_feature=[DRAG[f"{name}_vtx_feature"]], pts_feature=[DRAG[f"{name}_pts_feature"]],
                                        vismask=[DRAG[f"{name}_vismask"]], details=details)
    d, dev = details[0], DRAG_META["deviations"][name]
    assert np.array_equal(d["pairs_similarity"], DRAG[f"{name}_pairs_similarity"]) and np.array_equal(d["pairs"], DRAG[f"{name}_pairs"])
    figures = {}
    for stage in (1, 2):
        s, b = d[f"solve{stage}"], dev[f"stage{stage}"]
        figures[f"angles{stage}"] = (max(np.abs(s["angles"] - DRAG[f"{name}_solve{stage}_angles"]).max(),
                                         np.abs(s["trans"] - DRAG[f"{name}_solve{stage}_trans"]).max()), FACTOR * b["dev_angles"])
        figures[f"frames{stage}"] = (max(np.abs(s["locals"] - DRAG[f"{name}_solve{stage}_locals"]).max(),
                                         np.abs(s["jpos"] - DRAG[f"{name}_solve{stage}_jpos"]).max()), min(FACTOR * b["dev_vertices"], CAP))
    bound_v = min(FACTOR * max(dev["stage1"]["dev_vertices"], dev["stage2"]["dev_vertices"]), CAP)
    figures["stage1_vtx"] = (np.abs(d["stage1_vtx"] - DRAG[f"{name}_stage1_vtx"]).max(), min(FACTOR * dev["stage1"]["dev_vertices"], CAP))
    figures["vtx"] = (np.abs(vtx[0] - DRAG[f"{name}_vtx"]).max(), bound_v)
    figures["local_frames"] = (np.abs(rigs[0].local_frames - DRAG[f"{name}_rig2_local_frames"]).max(), bound_v)
    figures["quats"] = (tk.quat_distance(quats[0], DRAG[f"{name}_quats"]), bound_v)
    print(f"\n{name}: " + ", ".join(f"{k} {v:.3e} (bound {b:.3e})" for k, (v, b) in figures.items()))
    for k, (v, b) in figures.items():
        assert v <= b, k
    # the explicit matrix takes the same road from the selection on
    corr = np.matmul(DRAG[f"{name}_vtx_feature"], DRAG[f"{name}_pts_feature"].T)
    vtx_c, _, _ = tracking.ik_drag(*drag_inputs(name), vismask=[DRAG[f"{name}_vismask"]], corrmat=[corr])
    assert np.array_equal(vtx_c[0], vtx[0])


def test_corr_select_ties_and_sign():
    """the first vertex wins an exact tie, similarity has to be positive, an unchosen point has no winner"""
    nn = torch.tensor([0, 0, 2, 1, 1, 0], dtype=torch.int32, device="cuda")
    sim = torch.tensor([0.9, 0.9, -0.5, 0.3, 0.95, 0.0], dtype=torch.float32, device="cuda")
    winner, wsim = native.get_ops().corr_select(nn, sim, 4)
    assert winner.tolist() == [0, 4, -1, -1] and wsim.tolist() == [np.float32(0.9), np.float32(0.95), 0.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------- the frame loop
def small_scene(seed, n_side=16, n_pts=512, frames=3, joints=4):
    mesh = synth.make_mesh(seed, n_side=n_side, with_skin=False)
    V = n_side * n_side
    rng = np.random.default_rng([0x747263, seed])
    pos = mesh.pos.numpy().astype(np.float64)
    jpos = pos[rng.choice(V, size=joints, replace=False)] * 0.9
    skins = np.zeros((V, joints))
    d = np.linalg.norm(pos[:, None] - jpos[None], axis=-1)
    near = np.argsort(d, axis=1)[:, :2]
    w = rng.uniform(0.2, 1.0, size=(V, 2))
    skins[np.arange(V)[:, None], near] = np.round(w / w.sum(1, keepdims=True), 4)
    rig = formats.Rig.from_arrays(jpos, [-1] + list(range(joints - 1)), 0, skins=skins)
    pick = rng.integers(V, size=n_pts)
    pts0 = pos[pick] + rng.normal(0, 2e-3, size=(n_pts, 3))
    traj = np.stack([pts0 + t * np.array([0.01, 0.0, 0.005]) for t in range(frames)], 1)
    strip = lambda e: e[:, :-V].numpy()                                        # synth appends the self loops; tracking adds its own
    return pos, rig, traj, strip(mesh.tpl_edge_index), strip(mesh.geo_edge_index), pick


def by_hand(vtx0, rigs, pts_traj, tpl, geo, net):
    prev, out = vtx0, []
    for t in range(1, pts_traj[0].shape[1]):
        pts = [p[:, t, :] for p in pts_traj]
        inf = tracking.deform_inference(net, prev, pts, tpl, geo)
        prev, _, q = tracking.ik_drag(vtx0, [i[0] for i in inf], pts, rigs, [i[2] for i in inf], [i[3] for i in inf], [i[1] for i in inf])
        out.append((prev, [i[1] for i in inf], q))
    return out


def check_track(net, scenes):
    vtx0, rigs, traj, tpl, geo = ([s[k] for s in scenes] for k in range(5))
    torch.manual_seed(11)                                  # CorrNet's farthest-point sampling draws its starts
    got = tracking.track(vtx0, rigs, traj, tpl, geo, net)
    torch.manual_seed(11)
    want = by_hand(vtx0, rigs, traj, tpl, geo, net)
    for m in range(len(scenes)):
        v, vis, q = got[m]
        assert v.shape == (len(vtx0[m]), 2, 3) and vis.shape == (len(vtx0[m]), 2) and q.shape == (len(rigs[m].pos), 2, 4)
        for t in range(2):
            assert np.array_equal(v[:, t], want[t][0][m]) and np.array_equal(vis[:, t], want[t][1][m]) and np.array_equal(q[:, t], want[t][2][m])
        assert np.isfinite(v).all() and np.isfinite(q).all()
    return got


def test_track_two_frames_of_two_meshes():
    """DeformNet (synthetic weights) on the previous posed vertices, then ik_drag from the frame-0 vertices: track() equals the same calls
    made by hand, frame after frame"""
    net = synth.load_recipe(models.deformnet(tau_nce=0.07, num_interp=5).eval(), 61, mild=True).to("cuda")
    check_track(net, [small_scene(91), small_scene(92)])


class ScriptedDeformNet:
    """stands in for DeformNet where the second solve has to run: a small rigid flow, unit features that match a point to the vertex it
    was sampled from, a visibility mask away from the threshold"""

    def __init__(self, scenes):
        self.picks = [s[5] for s in scenes]

    def __call__(self, data):
        rng = np.random.default_rng(5)
        V = data.vtx.shape[0]
        fv = rng.normal(size=(V, 64))
        fv /= np.linalg.norm(fv, axis=1, keepdims=True)
        off, fp = 0, []
        for pick in self.picks:
            f = fv[off + pick] + 0.05 * rng.normal(size=(len(pick), 64))
            fp.append(f / np.linalg.norm(f, axis=1, keepdims=True))
            off += int((data.vtx_batch == len(fp) - 1).sum())
        dev = data.vtx.device
        flow = torch.tensor([0.01, 0.0, 0.005], device=dev).expand(V, 3).contiguous()
        vis = torch.linspace(0.0, 1.0, V, device=dev).add(0.0123).clamp(0, 1).reshape(V, 1)
        return (flow, torch.tensor(fv, dtype=torch.float32, device=dev), torch.tensor(np.concatenate(fp), dtype=torch.float32, device=dev), vis,
                torch.tensor(0.07))


def test_track_runs_both_solves_and_flow_errors():
    scenes = [small_scene(93, n_side=8, n_pts=128), small_scene(94, n_side=12, n_pts=200, joints=5)]
    net = ScriptedDeformNet(scenes)
    got = check_track(net, scenes)
    # the scripted features do keep correspondences, so the loop above went through the second solve
    vtx0, rigs, traj, tpl, geo = ([s[k] for s in scenes] for k in range(5))
    pts = [p[:, 1, :] for p in traj]
    inf, details = tracking.deform_inference(net, vtx0, pts, tpl, geo), []
    tracking.ik_drag(vtx0, [i[0] for i in inf], pts, rigs, [i[2] for i in inf], [i[3] for i in inf], [i[1] for i in inf], details=details)
    assert all(len(d["pairs"]) >= 16 and d["solve2"] is not None for d in details)
    for m, s in enumerate(scenes):
        v = got[m][0]
        gt = np.stack([s[0] + t * np.array([0.01, 0.0, 0.005]) for t in range(3)], 1)
        vis = np.random.default_rng(m).uniform(size=gt.shape[:2])
        full, seen = tracking.flow_errors(v, gt, vis)
        d = np.linalg.norm(v - gt[:, 1:], axis=2)
        assert full == pytest.approx(d.mean(), rel=1e-13) and seen == pytest.approx(d[vis[:, 1:] > 0.5].mean(), rel=1e-12)
        assert full < 0.1                                                        # the rig stays on the slowly moving points
