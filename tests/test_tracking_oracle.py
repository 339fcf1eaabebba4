"""tests/tracking_oracle.py (NumPy float64, analytic gradient) against the reference's recorded results (tests/golden/track_*.npz, made by
tools/make_tracking_golden.py), against central differences, against torch.optim.Adam, and the conditions the fixtures promise."""
import json
import os

import numpy as np
import pytest
import torch

import tracking_oracle as tk
from conftest import GOLDEN

THRD = 0.3
KEYS = ("locals_in", "offsets", "parent", "constraints", "vismask", "vptr", "ent_j", "ent_w", "ent_x")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), z


def solve_problem(z, meta, name):
    prob = {k: z[f"{name}_{k}"] for k in KEYS}
    prob["root"] = meta["params"][name]["root"]
    return prob


SOLVE_META, SOLVE = load("track_solve")
DRAG_META, DRAG = load("track_drag")


@pytest.mark.parametrize("name", SOLVE_META["cases"])
def test_oracle_reproduces_the_reference_solve(name):
    """float64 restatement against Deform_IK.run's float32 results: the deviations the generator stored (<= 4e-7 in the angles, <= 6e-7 in
    the positions), recomputed here"""
    par = SOLVE_META["params"][name]
    prob = solve_problem(SOLVE, SOLVE_META, name)
    got = tk.solve(prob, par["iter_time"], par["lr"], par["w_invis"], par["thrd"])
    posed = tk.skin(got["globals"], got["jpos"], prob)
    dev = SOLVE_META["deviations"][name]
    d_ang = max(np.abs(got["angles"] - SOLVE[f"{name}_angles"]).max(), np.abs(got["trans"] - SOLVE[f"{name}_trans"]).max())
    d_vtx = max(np.abs(got[k] - SOLVE[f"{name}_{k}"]).max() for k in ("locals", "globals", "jpos"))
    d_vtx = max(d_vtx, np.abs(posed - SOLVE[f"{name}_posed"]).max())
    print(f"{name}: angles {d_ang:.2e} (stored {dev['dev_angles']:.2e}) positions {d_vtx:.2e} (stored {dev['dev_vertices']:.2e})")
    assert d_ang == pytest.approx(dev["dev_angles"], rel=1e-3, abs=1e-12) and d_vtx == pytest.approx(dev["dev_vertices"], rel=1e-3, abs=1e-12)
    assert d_ang <= 1e-6 and d_vtx <= 1e-6
    assert abs(got["loss"] - float(SOLVE[f"{name}_loss"])) <= 1e-5 * max(got["loss"], 1e-12)
    scale = max(np.abs(got["g_angles"]).max(), np.abs(got["g_trans"]).max(), 1e-30)
    assert max(np.abs(got["g_angles"] - SOLVE[f"{name}_g_angles"]).max(), np.abs(got["g_trans"] - SOLVE[f"{name}_g_trans"]).max()) <= 0.05 * scale + 1e-12


def test_first_iteration_returns_the_initial_pose():
    """quirk (i): iter_time = 1 returns forward kinematics at the initial 0.01 angles, while the parameters have already stepped"""
    name = "one_iteration"
    prob = solve_problem(SOLVE, SOLVE_META, name)
    L, G, P = tk.forward(np.full((len(prob["parent"]), 3), 0.01), np.full(3, 0.01), prob)
    assert np.abs(L - SOLVE[f"{name}_locals"]).max() < 2e-7 and np.abs(P - SOLVE[f"{name}_jpos"]).max() < 2e-7
    assert np.abs(SOLVE[f"{name}_angles"] - 0.01).max() > 1e-2


def test_zero_weight_joints_and_invisible_masks():
    """quirk (iii): a joint without skin weight has an exactly zero data gradient; an all-invisible mask with w_invis = 0 leaves only the
    weight decay"""
    for name in ("star_root3", "tree_w_invis", "one_iteration"):
        prob = solve_problem(SOLVE, SOLVE_META, name)
        silent = np.setdiff1d(np.arange(len(prob["parent"])), prob["ent_j"])
        assert len(silent) and np.all(SOLVE[f"{name}_g_angles"][silent] == 0)
        mask = tk.mask_of(prob["vismask"], THRD, 0.0)
        _, g, _, _ = tk.loss_and_gradient(np.full((len(prob["parent"]), 3), 0.01), np.full(3, 0.01), prob, mask)
        assert np.all(g[silent] == 0)
    assert np.all(SOLVE["all_invisible_g_angles"] == 0) and float(SOLVE["all_invisible_loss"]) == 0
    assert not (SOLVE["all_invisible_vismask"] > THRD).any()


@pytest.mark.parametrize("name", ["chain", "star_root3", "tree_w_invis"])
def test_analytic_gradient_against_central_differences(name):
    prob = solve_problem(SOLVE, SOLVE_META, name)
    rng = np.random.default_rng(3)
    J = len(prob["parent"])
    a, t = rng.uniform(-0.4, 0.4, size=(J, 3)), rng.uniform(-0.1, 0.1, size=3)
    mask = tk.mask_of(prob["vismask"], THRD, SOLVE_META["params"][name]["w_invis"])
    tree = tk.bfs(prob["parent"], prob["root"])
    _, ga, gt, _ = tk.loss_and_gradient(a, t, prob, mask, tree)
    h = 1e-6
    num_a, num_t = np.zeros_like(a), np.zeros_like(t)
    for idx in np.ndindex(*a.shape):
        up, dn = a.copy(), a.copy()
        up[idx] += h
        dn[idx] -= h
        num_a[idx] = (tk.loss_and_gradient(up, t, prob, mask, tree)[0] - tk.loss_and_gradient(dn, t, prob, mask, tree)[0]) / (2 * h)
    for k in range(3):
        up, dn = t.copy(), t.copy()
        up[k] += h
        dn[k] -= h
        num_t[k] = (tk.loss_and_gradient(a, up, prob, mask, tree)[0] - tk.loss_and_gradient(a, dn, prob, mask, tree)[0]) / (2 * h)
    scale = max(np.abs(num_a).max(), np.abs(num_t).max())
    assert np.abs(ga - num_a).max() <= 1e-8 * scale + 1e-11 and np.abs(gt - num_t).max() <= 1e-8 * scale + 1e-11


def test_adam_step_against_torch():
    """three parameters, a fixed gradient sequence: torch.optim.Adam(lr, betas (0.9, 0.999), eps 1e-8, weight_decay 1e-4) in float64"""
    rng = np.random.default_rng(0)
    p0, grads = np.array([0.01, -0.3, 2.0]), rng.normal(size=(25, 3)) * np.array([1.0, 1e-3, 10.0])
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=5e-2, betas=(0.9, 0.999), weight_decay=1e-4)
    mine, q = tk.Adam(3, 5e-2), p0.copy()
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        q = mine.step(q, g)
        assert np.abs(q - p.detach().numpy()).max() <= 1e-14
    # the known answer of the first step: m / (1 - b1) = g' and sqrt(v / (1 - b2)) = |g'|, so p moves by lr g' / (|g'| + eps)
    first = tk.Adam(3, 5e-2).step(p0, grads[0])
    gd = grads[0] + 1e-4 * p0
    assert np.allclose(first, p0 - 5e-2 * gd / (np.abs(gd) + 1e-8), rtol=0, atol=1e-15)


def test_fixture_conditions():
    m = SOLVE_META["margins"]
    for name in SOLVE_META["cases"]:
        assert np.abs(SOLVE[f"{name}_vismask"].astype(np.float64) - THRD).min() >= m["vismask"]
    for name in DRAG_META["cases"]:
        fv, fp = DRAG[f"{name}_vtx_feature"], DRAG[f"{name}_pts_feature"]
        assert np.abs(np.linalg.norm(fv, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(fp, axis=1) - 1).max() < 1e-6
        corr = np.matmul(fv, fp.T)
        s = np.sort(corr.astype(np.float64), axis=1)
        assert (s[:, -1] - s[:, -2]).min() >= m["similarity"]                   # best and second-best of every vertex
        winner, best, margin = tk.select_pairs(corr.max(1).astype(np.float64), corr.argmax(1), corr.shape[1])
        assert margin.min() >= m["similarity"]                                   # every winner ahead of its runner-up
        assert np.abs(best[winner >= 0] - 0.5).min() >= m["similarity"]
        pairs1, pairs2, d2 = tk.keep_pairs(winner, best, DRAG[f"{name}_stage1_vtx"], DRAG[f"{name}_pts"])
        assert np.abs(d2 - 1e-2).min() >= m["distance"]
        assert np.array_equal(pairs1, DRAG[f"{name}_pairs_similarity"]) and np.array_equal(pairs2, DRAG[f"{name}_pairs"])
        assert len(pairs2) < len(pairs1) < corr.shape[1]                         # both filters drop something
        assert np.abs(DRAG[f"{name}_vismask"].astype(np.float64) - THRD).min() >= m["vismask"]
        for s_ in (1, 2):
            q, lead = tk.quat_from_matrix(DRAG[f"{name}_rig{s_}_local_frames"])
            assert lead.min() >= m["quaternion"]
        assert tk.quat_distance(tk.quat_from_matrix(DRAG[f"{name}_rig2_local_frames"])[0], DRAG[f"{name}_quats"]) <= 1e-12


def test_quaternion_branches():
    """every branch of the rule (largest of m00, m11, m22, trace) gives back the rotation"""
    for angles in ([0.1, 0.2, 0.3], [3.0, 0.1, 0.1], [0.1, 3.0, 0.1], [0.1, 0.1, 3.0]):
        m = tk.euler_matrix(np.array([angles]))
        q, _ = tk.quat_from_matrix(m)
        x, y, z, w = q[0]
        back = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert np.abs(back - m[0]).max() < 1e-14
    branches = {int(np.argmax([m[0, 0], m[1, 1], m[2, 2], np.trace(m)])) for m in
                (tk.euler_matrix(np.array([a]))[0] for a in ([0.1, 0.2, 0.3], [3.0, 0.1, 0.1], [0.1, 3.0, 0.1], [0.1, 0.1, 3.0]))}
    assert branches == {0, 1, 2, 3}
