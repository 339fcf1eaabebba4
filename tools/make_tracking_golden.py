"""Fixtures of the tracking stage (tests/golden/track_*.npz), made by the reference's own code: utils/deform_ik.py (Deform_IK.run),
utils/rig_parser.py (Rig.FK, global_transforms_homogeneous) and the function ik_drag of evaluate/eval_tracking.py, compiled out of that
file at generation time (the module itself imports cv2, open3d and torch_geometric). Nothing of the reference is written into the
repository: only inputs and results.

  track_solve   Deform_IK.run on synthetic rigs: J = 1, J = 2 with one vertex, a chain of depth J - 1, a star rooted at joint 3, a random
                tree with zero-weight leaves and w_invis > 0, an all-invisible mask (weight decay alone), iter_time 1, 2, 200, 400 and
                both learning rates. Inputs: locals_in, offsets, parent, root, the sparse skin with the local vertices, constraints,
                vismask, the hyper-parameters. Results: final angles and translation, locals, globals, jpos, the posed vertices, the last
                loss and the last gradients.
  track_drag    ik_drag on a rig with features and points: every input, the pairs kept after each filter, the rig after each update, the
                solver's results of both stages, posed vertices and quaternions.

Per case the deviation of the reference's float32 result from tests/tracking_oracle.py (float64, analytic gradient) is stored: dev_angles
(angles and translation), dev_vertices (locals, globals, jpos, posed vertices), dev_grad and dev_loss (relative). The device is held to
ten times these (tests/test_gpu_tracking.py).

Conditions enforced here (the run fails rather than write a fixture that misses one) and re-checked by tests/test_tracking_oracle.py: no
vismask value within 1e-6 of the threshold; every vertex's best and second-best similarity at least 1e-4 apart; every per-point winner
at least 1e-4 ahead of the runner-up; no kept similarity within 1e-4 of 0.5; no squared distance within 1e-5 of 1e-2; the quaternion
branch choice clear by 1e-6.

Run from the repository root:  python tools/make_tracking_golden.py
"""
import ast
import copy
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from morig_amd import formats                                                  # noqa: E402
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (_compile_from, save)
import tracking_oracle as tk                                                   # noqa: E402

VIS_MARGIN, SIM_MARGIN, DIST_MARGIN, QUAT_MARGIN = 1e-6, 1e-4, 1e-5, 1e-6
THRD = 0.3                                                                     # ik_drag's Deform_IK(vismask_thrd=0.3)


class _Recorder:
    """stands in for a module inside ik_drag: the same attributes, the results of ``where`` recorded"""

    def __init__(self, mod, log):
        self._mod, self._log = mod, log

    def __getattr__(self, name):
        return getattr(self._mod, name)

    def where(self, *a, **kw):
        r = self._mod.where(*a, **kw)
        self._log.append(np.asarray(r[0]).copy())
        return r


def reference():
    sys.path.insert(0, shim.REFERENCE_ROOT)
    dik = __import__("utils.deform_ik", fromlist=["Deform_IK"])
    rp = __import__("utils.rig_parser", fromlist=["Rig"])
    from scipy.spatial.transform import Rotation
    path = os.path.join(shim.REFERENCE_ROOT, "evaluate", "eval_tracking.py")
    code = msg._compile_from(path, lambda t: [n for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "ik_drag"])

    class Recording(dik.Deform_IK):
        runs = []

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            inner, seen = self.crit, {}
            self.seen = seen

            def crit(a, b):
                seen["a"], seen["b"] = a.detach().clone(), b.detach().clone()
                return inner(a, b)
            self.crit = crit

        def run(self, **kw):
            out = super().run(**kw)
            with torch.no_grad():
                loss = (torch.nn.functional.mse_loss(self.seen["a"], self.seen["b"], reduction="none") * self.vismask[:, None]).mean()
            Recording.runs.append(dict(kw=kw, out=[o.detach().numpy().copy() for o in out], posed=self.seen["a"].numpy().copy(),
                                       angles=self.rotation_angles.detach().numpy().copy(), trans=self.translation.detach().numpy().copy(),
                                       g_angles=self.rotation_angles.grad.numpy().copy(), g_trans=self.translation.grad.numpy().copy(),
                                       loss=float(loss)))
            return out
    return types.SimpleNamespace(Deform_IK=Recording, Rig=rp.Rig, code=code, Rotation=Rotation)


# ------------------------------------------------------------------------------------------------------------------- synthetic rigs
def random_rotations(rng, n, angle):
    return tk.euler_matrix(rng.uniform(-angle, angle, size=(n, 3)))


def make_parent(kind, J, root, rng):
    parent = np.full(J, -1, dtype=np.int64)
    others = [j for j in range(J) if j != root]
    if kind == "chain":
        prev = root
        for j in others:
            parent[j], prev = prev, j
    elif kind == "star":
        parent[others] = root
    else:
        placed = [root]
        for j in rng.permutation(others):
            parent[j] = placed[int(rng.integers(len(placed)))]
            placed.append(int(j))
    return parent


def make_skin(rng, V, J, parent, root, zero_leaves):
    """dense [V, J] float32 weights with 1..4 influences per vertex, rounded to 4 decimals as a rig file holds them; the leaves of the
    tree carry no weight when asked"""
    carriers = np.arange(J)
    if zero_leaves:
        leaves = [j for j in range(J) if not (parent == j).any() and j != root][::2]          # every other leaf
        carriers = np.array([j for j in range(J) if j not in leaves])
        assert len(carriers) < J
    skins = np.zeros((V, J))
    for v in range(V):
        k = int(rng.integers(1, min(4, len(carriers)) + 1))
        js = rng.choice(carriers, size=k, replace=False)
        w = rng.uniform(0.1, 1.0, size=k)
        skins[v, js] = np.round(w / w.sum(), 4)
    return skins


def vismask_with_margin(rng, V, lo=0.0, hi=1.0):
    m = rng.uniform(lo, hi, size=V).astype(np.float32)
    bad = np.abs(m.astype(np.float64) - THRD) < 10 * VIS_MARGIN
    m[bad] += np.float32(1e-3)
    return m


def reference_rig(ref, pos, parent, root, skins):
    rig = ref.Rig()
    rig.names = [f"joint_{i}" for i in range(len(pos))]
    rig.pos = np.array(pos, dtype=np.float64)
    rig.hierarchy = np.array(parent, dtype=int)
    rig.root_id, rig.root_name = int(root), f"joint_{root}"
    rig.skins = np.array(skins, dtype=np.float64)
    rig.calc_frames_and_offsets()
    rig.pos_in = np.array(pos, dtype=np.float64)                              # the positions as a rig file holds them (FK rebuilds rig.pos)
    return rig


def posed_by(rig, vtx, angles, trans):
    """the mesh under a pose of the rig: float64 forward kinematics and skinning (the targets of the synthetic problems)"""
    prob = dict(locals_in=rig.local_frames, offsets=rig.offset, parent=rig.hierarchy, root=rig.root_id)
    prob["vptr"], prob["ent_j"], prob["ent_w"], prob["ent_x"] = tk.local_entries(rig.global_transforms_homogeneous, vtx, rig.skins)
    _, G, P = tk.forward(angles, trans, prob)
    return tk.skin(G, P, prob)


# ------------------------------------------------------------------------------------------------------------------- track_solve
SOLVE_CASES = {
    # name: (J, V, tree, root, zero-weight leaves, iter_time, lr, w_invis, vismask range)
    "one_joint": (1, 63, "chain", 0, False, 200, 5e-2, 0.0, (0.0, 1.0)),
    "two_joints_one_vertex": (2, 1, "chain", 0, False, 2, 5e-2, 0.0, (0.5, 1.0)),
    "chain": (8, 65, "chain", 0, False, 200, 5e-2, 0.0, (0.0, 1.0)),
    "star_root3": (7, 1025, "star", 3, True, 400, 1e-3, 0.0, (0.0, 1.0)),
    "tree_w_invis": (16, 600, "tree", 5, True, 200, 5e-2, 0.25, (0.0, 1.0)),
    "all_invisible": (5, 65, "tree", 1, False, 200, 5e-2, 0.0, (0.0, 0.25)),
    "one_iteration": (5, 63, "tree", 2, True, 1, 5e-2, 0.0, (0.0, 1.0)),
    "two_iterations": (6, 64, "tree", 0, False, 2, 1e-3, 0.5, (0.0, 1.0)),
}


def dense_inputs(prob):
    J, V = len(prob["parent"]), len(prob["vptr"]) - 1
    ev = tk.entry_vertex(prob)
    vert_local = np.zeros((J, 4, V), dtype=np.float32)
    vert_local[:, 3, :] = 1
    vert_local[prob["ent_j"], 0:3, ev] = prob["ent_x"]
    skinning = np.zeros((V, J), dtype=np.float32)
    skinning[ev, prob["ent_j"]] = prob["ent_w"]
    return vert_local, skinning


def deviations(run, want):
    """the reference's float32 results against the float64 oracle"""
    locals_, globals_, jpos = run["out"]
    dev = dict(
        dev_angles=max(np.abs(run["angles"] - want["angles"]).max(), np.abs(run["trans"] - want["trans"]).max()),
        dev_vertices=max(np.abs(locals_ - want["locals"]).max(), np.abs(globals_ - want["globals"]).max(), np.abs(jpos - want["jpos"]).max(),
                         np.abs(run["posed"] - want["posed"]).max()),
        dev_loss=abs(run["loss"] - want["loss"]) / max(abs(want["loss"]), 1e-30),
        dev_grad=max(np.abs(run["g_angles"] - want["g_angles"]).max(), np.abs(run["g_trans"] - want["g_trans"]).max())
        / max(np.abs(want["g_angles"]).max(), np.abs(want["g_trans"]).max(), 1e-30))
    return {k: float(v) for k, v in dev.items()}


def oracle_solve(prob, iter_time, lr, w_invis):
    want = tk.solve(prob, iter_time, lr, w_invis, THRD)
    want["posed"] = tk.skin(want["globals"], want["jpos"], prob)
    return want


def group_solve(ref):
    arrs, meta = {}, dict(cases=[], params={}, deviations={}, reference_seconds={})
    for ci, (name, (J, V, kind, root, zero_leaves, iters, lr, w_invis, vis)) in enumerate(SOLVE_CASES.items()):
        rng = np.random.default_rng([0x747261, ci])
        parent = make_parent(kind, J, root, rng)
        pos = rng.uniform(-0.4, 0.4, size=(J, 3))
        skins = make_skin(rng, V, J, parent, root, zero_leaves)
        rig = reference_rig(ref, pos, parent, root, skins)
        rig.local_frames = random_rotations(rng, J, 0.3)                      # a posed rig, as the second solve of ik_drag meets one
        rig.FK()
        vtx = rng.uniform(-0.5, 0.5, size=(V, 3))
        target = posed_by(rig, vtx, rng.uniform(-0.25, 0.25, size=(J, 3)), rng.uniform(-0.05, 0.05, size=3))
        prob = dict(locals_in=rig.local_frames.astype(np.float32), offsets=rig.offset.astype(np.float32), parent=parent.astype(np.int32),
                    root=root, constraints=(target + rng.normal(0, 2e-3, size=target.shape)).astype(np.float32),
                    vismask=vismask_with_margin(rng, V, *vis))
        prob["vptr"], prob["ent_j"], prob["ent_w"], prob["ent_x"] = tk.local_entries(rig.global_transforms_homogeneous, vtx, skins)
        assert np.abs(prob["vismask"].astype(np.float64) - THRD).min() >= VIS_MARGIN
        vert_local, skinning = dense_inputs(prob)
        ref.Deform_IK.runs.clear()
        t0 = time.perf_counter()
        ref.Deform_IK(vismask_thrd=THRD).run(
            locals_in=torch.from_numpy(prob["locals_in"]), offsets=torch.from_numpy(prob["offsets"]), parent=parent, root_id=root,
            vert_local=torch.from_numpy(vert_local), skinning=torch.from_numpy(skinning), constraints=torch.from_numpy(prob["constraints"]),
            vismask=torch.from_numpy(prob["vismask"]), iter_time=iters, lr=lr, w_invis=w_invis)
        secs = time.perf_counter() - t0
        run = ref.Deform_IK.runs[-1]
        dev = deviations(run, oracle_solve(prob, iters, lr, w_invis))
        if name == "all_invisible":
            assert not (prob["vismask"] > THRD).any() and np.all(run["g_angles"] == 0) and np.all(run["g_trans"] == 0)
        if zero_leaves:
            silent = np.setdiff1d(np.arange(J), prob["ent_j"])
            assert len(silent) and np.all(run["g_angles"][silent] == 0)      # quirk (iii)
        meta["cases"].append(name)
        meta["params"][name] = dict(J=J, V=V, tree=kind, root=root, iter_time=iters, lr=lr, w_invis=w_invis, thrd=THRD)
        meta["deviations"][name] = dev
        meta["reference_seconds"][name] = secs
        for k in ("locals_in", "offsets", "parent", "constraints", "vismask", "vptr", "ent_j", "ent_w", "ent_x"):
            arrs[f"{name}_{k}"] = prob[k]
        arrs.update({f"{name}_angles": run["angles"], f"{name}_trans": run["trans"], f"{name}_locals": run["out"][0],
                     f"{name}_globals": run["out"][1], f"{name}_jpos": run["out"][2], f"{name}_posed": run["posed"],
                     f"{name}_loss": np.array(run["loss"], dtype=np.float64), f"{name}_g_angles": run["g_angles"],
                     f"{name}_g_trans": run["g_trans"]})
        print(f"  solve/{name}: J={J} V={V} E={len(prob['ent_j'])} iters={iters} reference {secs:.2f} s  " +
              " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    return meta, arrs


# ------------------------------------------------------------------------------------------------------------------- track_drag
DRAG_CASES = {"main": (16, 600, 800, 64), "small": (5, 150, 200, 64)}          # J, V, P, feature width


def unit_rows(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def drag_inputs(rng, ref, J, V, P, C):
    root = int(rng.integers(J))
    parent = make_parent("tree", J, root, rng)
    skins = make_skin(rng, V, J, parent, root, True)
    rig = reference_rig(ref, rng.uniform(-0.4, 0.4, size=(J, 3)), parent, root, skins)
    vtx_src = rng.uniform(-0.5, 0.5, size=(V, 3))
    target = posed_by(rig, vtx_src, rng.uniform(-0.25, 0.25, size=(J, 3)), rng.uniform(-0.05, 0.05, size=3))
    vtx_dst = target + rng.normal(0, 2e-3, size=target.shape)
    src_of = rng.integers(V, size=P)                                          # the vertex a point was sampled near
    pts = target[src_of] + rng.normal(0, 5e-3, size=(P, 3))
    far = rng.uniform(size=P) < 0.15
    pts[far] += rng.choice([-1.0, 1.0], size=(int(far.sum()), 3)) * rng.uniform(0.08, 0.2, size=(int(far.sum()), 3))
    fv = unit_rows(rng.normal(size=(V, C)))
    noise = np.where(rng.uniform(size=(P, 1)) < 0.2, 1.3, 0.45)               # a fifth of the points match their vertex poorly
    fp = unit_rows(fv[src_of].astype(np.float64) + noise * unit_rows(rng.normal(size=(P, C))))
    return rig, vtx_src, vtx_dst, pts, fv, fp, vismask_with_margin(rng, V)


def feature_margins(corr):
    s = np.sort(corr.astype(np.float64), axis=1)
    row_margin = float((s[:, -1] - s[:, -2]).min())
    winner, best, margin = tk.select_pairs(corr.max(1).astype(np.float64), corr.argmax(1), corr.shape[1])
    kept = best > 0.5
    return row_margin, float(margin.min()), float(np.abs(best[winner >= 0] - 0.5).min()), winner, best, int(kept.sum())


def run_ik_drag(ref, rig, vtx_src, vtx_dst, pts, corr, vismask):
    wheres, copies = [], []

    def deepcopy(x):
        c = copy.deepcopy(x)
        copies.append(c)
        return c
    ns = dict(np=_Recorder(np, wheres), torch=_Recorder(torch, wheres), copy=types.SimpleNamespace(deepcopy=deepcopy), Deform_IK=ref.Deform_IK,
              Rotation=ref.Rotation)
    exec(ref.code, ns)
    ref.Deform_IK.runs.clear()
    t0 = time.perf_counter()
    vtx, quats = ns["ik_drag"](vtx_src, vtx_dst, pts, rig, corr, vismask)
    secs = time.perf_counter() - t0
    rigs = [c for c in copies if isinstance(c, ref.Rig)]
    assert len(rigs) == 2 and len(wheres) == 2 and len(ref.Deform_IK.runs) == 2
    return vtx, quats, rigs, wheres, list(ref.Deform_IK.runs), secs


def group_drag(ref):
    arrs, meta = {}, dict(cases=[], params={}, deviations={}, margins={}, seeds={}, reference_seconds={})
    for ci, (name, (J, V, P, C)) in enumerate(DRAG_CASES.items()):
        for seed in range(200):
            rng = np.random.default_rng([0x647261, ci, seed])
            rig, vtx_src, vtx_dst, pts, fv, fp, vismask = drag_inputs(rng, ref, J, V, P, C)
            corr = np.matmul(fv, fp.T)                                         # run_deform_net_inference's corr_matrix, float32
            row_m, win_m, half_m, winner, best, n_half = feature_margins(corr)
            if min(row_m, win_m, half_m) < SIM_MARGIN:
                continue
            rig0 = copy.deepcopy(rig)
            vtx, quats, rigs, wheres, runs, secs = run_ik_drag(ref, rig, vtx_src, vtx_dst, pts, corr, vismask)
            stage1 = np.sum(np.matmul(rigs[0].global_transforms_homogeneous,
                                      np.linalg.inv(rig0.global_transforms_homogeneous) @ np.column_stack((vtx_src, np.ones(V))).T[None])
                            * rigs[0].skins.T[:, None, :], axis=0)[0:3].T
            pairs1, pairs2, d2 = tk.keep_pairs(winner, best, stage1, pts)
            q_mine, q_margin = tk.quat_from_matrix(rigs[1].local_frames)
            ok = (np.abs(d2 - 1e-2).min() >= DIST_MARGIN and q_margin.min() >= QUAT_MARGIN and
                  min(tk.quat_from_matrix(rigs[0].local_frames)[1].min(), q_margin.min()) >= QUAT_MARGIN)
            if ok:
                break
        else:
            raise RuntimeError(f"{name}: no seed met the fixture conditions")
        # the restated selection is the reference's: its where() results and the rows it handed to the second solve
        assert np.array_equal(wheres[0], pairs1[:, 1]) and np.array_equal(pairs1[wheres[1]], pairs2)
        assert np.array_equal(runs[1]["kw"]["constraints"].numpy(), pts[pairs2[:, 1]].astype(np.float32))
        assert tk.quat_distance(q_mine, quats) < 1e-12
        skins = rig0.skins
        sv, sj = np.nonzero(skins)
        devs = {}
        for s, run in enumerate(runs):                                          # both solves against the oracle on the reference's own inputs
            kw = run["kw"]
            vl, sk = kw["vert_local"].numpy(), kw["skinning"].numpy()
            ev, ej = np.nonzero(sk)
            prob = dict(locals_in=kw["locals_in"].numpy(), offsets=kw["offsets"].numpy(), parent=np.asarray(kw["parent"]), root=kw["root_id"],
                        constraints=kw["constraints"].numpy(), vismask=kw["vismask"].numpy(), ent_j=ej.astype(np.int32), ent_w=sk[ev, ej],
                        ent_x=vl[ej, 0:3, ev], vptr=np.concatenate([[0], np.cumsum(np.bincount(ev, minlength=len(sk)))]).astype(np.int32))
            devs[f"stage{s + 1}"] = deviations(run, oracle_solve(prob, kw["iter_time"], kw.get("lr", 5e-2), kw.get("w_invis", 0.0)))
        meta["cases"].append(name)
        meta["params"][name] = dict(J=J, V=V, P=P, C=C, root=int(rig0.root_id), kept_similarity=len(pairs1), kept=len(pairs2))
        meta["deviations"][name] = devs
        meta["margins"][name] = dict(row=row_m, winner=win_m, half=half_m, distance=float(np.abs(d2 - 1e-2).min()), quaternion=float(q_margin.min()),
                                     vismask=float(np.abs(vismask.astype(np.float64) - THRD).min()))
        meta["seeds"][name] = seed
        meta["reference_seconds"][name] = secs
        mine = formats.Rig.from_arrays(rig0.pos_in, rig0.hierarchy, rig0.root_id, skins=skins)
        assert np.array_equal(mine.pos, rig0.pos) and np.array_equal(mine.offset, rig0.offset)
        arrs.update({f"{name}_pos": rig0.pos_in, f"{name}_parent": np.asarray(rig0.hierarchy, dtype=np.int32), f"{name}_skin_v": sv.astype(np.int32),
                     f"{name}_skin_j": sj.astype(np.int32), f"{name}_skin_w": skins[sv, sj], f"{name}_vtx_src": vtx_src, f"{name}_vtx_dst": vtx_dst,
                     f"{name}_pts": pts, f"{name}_vtx_feature": fv, f"{name}_pts_feature": fp, f"{name}_vismask": vismask,
                     f"{name}_pairs_similarity": pairs1, f"{name}_pairs": pairs2, f"{name}_stage1_vtx": stage1, f"{name}_vtx": vtx,
                     f"{name}_quats": quats})
        for s, (r, run) in enumerate(zip(rigs, runs)):
            arrs.update({f"{name}_rig{s + 1}_pos": r.pos, f"{name}_rig{s + 1}_local_frames": r.local_frames,
                         f"{name}_rig{s + 1}_global_transforms": r.global_transforms, f"{name}_rig{s + 1}_offset": r.offset,
                         f"{name}_solve{s + 1}_locals": run["out"][0], f"{name}_solve{s + 1}_jpos": run["out"][2],
                         f"{name}_solve{s + 1}_angles": run["angles"], f"{name}_solve{s + 1}_trans": run["trans"]})
        print(f"  drag/{name}: J={J} V={V} P={P} seed {seed}: {len(pairs1)} pairs above 0.5, {len(pairs2)} kept; reference {secs:.2f} s; "
              f"margins {meta['margins'][name]}; deviations {devs}")
    return meta, arrs


def reference_timing(ref):
    """the reference's ik_drag on ONE problem of tools/tracking_bench.py (4 096 vertices, 30 joints, 5 influences, 4 096 points), on this CPU"""
    import tracking_bench
    sc = tracking_bench.make_scene(500, 4096, 30, 4096)
    rig = reference_rig(ref, sc["pos"], sc["parent"], sc["root"], sc["skins"])
    corr = np.matmul(sc["vtx_feature"], sc["pts_feature"].T)
    runs = []
    for rep in range(2):                                      # the machine is shared: both runs kept, the faster one quoted
        t0 = time.perf_counter()
        _, _, _, _, solves, secs = run_ik_drag(ref, rig, sc["vtx_src"], sc["vtx_dst"], sc["pts"], corr, sc["vismask"])
        runs.append(dict(ik_drag_s=secs, kept=int(len(solves[1]["kw"]["constraints"]))))
    best = min(runs, key=lambda r: r["ik_drag_s"])
    print(f"  reference ik_drag, one 4096-vertex problem with 30 joints: {[round(r['ik_drag_s'], 2) for r in runs]} s, {best['kept']} pairs kept")
    return dict(vertices=4096, joints=30, points=4096, influences=5, iterations=[200, 400], runs=runs, threads=torch.get_num_threads(),
                date=time.strftime("%Y-%m-%d"), note="the reference's Python on the generating CPU", **best)


def main():
    ref = reference()
    common = dict(numpy=np.__version__, torch=torch.__version__, threads=torch.get_num_threads(), date=time.strftime("%Y-%m-%d"),
                  margins=dict(vismask=VIS_MARGIN, similarity=SIM_MARGIN, distance=DIST_MARGIN, quaternion=QUAT_MARGIN))
    print("track_solve")
    meta, arrs = group_solve(ref)
    msg.save("track_solve", dict(common, **meta), **arrs)
    print("track_drag")
    meta, arrs = group_drag(ref)
    meta["reference_cpu"] = reference_timing(ref)
    msg.save("track_drag", dict(common, **meta), **arrs)


if __name__ == "__main__":
    main()
