"""Fixtures of motion playback (tests/golden/playback_cases.npz), made by the reference's own ``smooth_quats``
(evaluate/visualize_tracking.py:43-61; the one function, compiled out of its file by AST at generation time because the module imports
open3d and cv2) over the reference's own ``Rig`` (utils/rig_parser.py) and scipy's ``Rotation``. The per-frame global transforms and joint
positions are recorded from ``Rig.FK`` on a copy of the rig, as that function runs it. Nothing of the reference is written into the
repository: only inputs and recorded results.

Cases (J, V, T): random trees with a root that is not index 0 (where J > 1), float32 and float64 joints, up to four weights per vertex,
random-walk rotations of about 0.15 rad per frame: (1, 5, 1), (2, 63, 2), (3, 65, 3), (23, 257, 7), (48, 130, 33); one at the skinning
kernel's frame tile (T = 64) and one at T = 65; ``posed``: a rig whose bind pose is itself posed (non-identity global_transforms);
``noweight``: a vertex without weights; ``flip``: two frames of one joint negated -- recorded as the reference smooths it
(align_signs=False) and, for align_signs=True, as the reference smooths the input the oracle aligned.

Conditions asserted here and re-asserted by tests/test_playback_oracle.py: the oracle's smoothed quaternions equal the reference's bit
for bit; the oracle's trajectory, transforms and positions lie within (8 depth + 32) 2^-53 max(1, max |coordinate|) of the reference's
(the measured deviation is stored per case); on float32 rigs every joint position's unrounded float64 value lies farther than
2^-40 |value| from a float32 rounding midpoint (the seed is redrawn until it does).

Run from the repository root:  python tools/make_playback_golden.py
"""
import ast
import copy
import os
import sys
import types

import numpy as np
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (_compile_from, save)
import playback_oracle as po                                                   # noqa: E402

MARGIN = 2.0 ** -40
STEP = 0.15
CASES = [("j1", 1, 5, 1, "float64", {}), ("j2", 2, 63, 2, "float32", {}), ("j3", 3, 65, 3, "float64", {}),
         ("j23", 23, 257, 7, "float32", {}), ("j48", 48, 130, 33, "float64", {}),
         ("tile", 5, 40, po.FRAME_TILE, "float32", {}), ("tile_plus_1", 6, 70, po.FRAME_TILE + 1, "float64", {}),
         ("posed", 7, 50, 5, "float32", dict(posed=True)), ("noweight", 4, 30, 4, "float64", dict(noweight=3)),
         ("flip", 5, 33, 6, "float64", dict(flip=(2, (3, 4))))]


def reference():
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    rp = __import__("utils.rig_parser", fromlist=["Rig"])
    ns = dict(np=np, copy=copy, Rotation=Rotation, Rig=rp.Rig)
    pick = lambda t: [n for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "smooth_quats"]
    exec(msg._compile_from(os.path.join(shim.REFERENCE_ROOT, "evaluate", "visualize_tracking.py"), pick), ns)
    return rp, ns["smooth_quats"]


def random_tree(rng, n, dtype):
    parent = [-1] + [int(rng.integers(0, i)) for i in range(1, n)]
    pos = rng.uniform(-0.5, 0.5, (n, 3))
    perm = rng.permutation(n)
    while n > 1 and perm[0] == 0:
        perm = rng.permutation(n)
    hier, out = np.zeros(n, dtype=int), np.zeros((n, 3))
    for i in range(n):
        hier[perm[i]] = perm[parent[i]] if parent[i] >= 0 else -1
        out[perm[i]] = pos[i]
    return hier, out.astype(dtype), int(perm[0])


def random_walk(rng, J, T):
    """[J, T, 4] (x, y, z, w): a random rotation per joint, then steps of about STEP radians about random axes"""
    q = np.zeros((J, T, 4))
    for j in range(J):
        r = Rotation.from_rotvec(rng.normal(size=3))
        for t in range(T):
            q[j, t] = r.as_quat()
            axis = rng.normal(size=3)
            r = Rotation.from_rotvec(axis / np.linalg.norm(axis) * STEP * rng.uniform(0.5, 1.5)) * r
    return q


def random_skins(rng, V, J):
    skins = np.zeros((V, J))
    for v in range(V):
        js = rng.choice(J, size=min(J, int(rng.integers(1, 5))), replace=False)
        w = rng.uniform(0.1, 1.0, len(js))
        skins[v, js] = w / w.sum()
    return skins


def make_case(rp, smooth_quats, name, J, V, T, dtype, opt, seed):
    rng = np.random.default_rng(seed)
    hier, pos, root = random_tree(rng, J, dtype)
    rig = rp.Rig()
    rig.pos, rig.hierarchy, rig.names = pos, hier, [f"joint_{i}" for i in range(J)]
    rig.root_id, rig.root_name = root, f"joint_{root}"
    rig.calc_frames_and_offsets()
    if opt.get("posed"):
        rig.local_frames = Rotation.from_rotvec(rng.normal(size=(J, 3)) * 0.4).as_matrix()
        rig.FK()
    rig.skins = random_skins(rng, V, J)
    if "noweight" in opt:
        rig.skins[opt["noweight"]] = 0.0
    vtx = rng.uniform(-0.5, 0.5, (V, 3))
    quats = random_walk(rng, J, T)
    if "flip" in opt:
        j, frames = opt["flip"]
        quats[j, list(frames)] *= -1.0
    state = dict(pos=rig.pos.copy(), hier=hier, offset=np.array(rig.offset, dtype=np.float64), bind_G=np.array(rig.global_transforms),
                 skins=rig.skins.copy(), vtx=vtx, quats=quats.copy())
    assert state["pos"].dtype == np.dtype(dtype)
    oracle_rig = dict(pos=state["pos"], hierarchy=hier, root_id=root, offset=state["offset"], global_transforms=state["bind_G"],
                      skins=state["skins"])
    depth = po.level_order(hier, root)[1]
    meta = dict(name=name, J=J, V=V, T=T, dtype=dtype, root_id=root, depth=depth, seed=int(seed), **{k: True for k in opt})

    def run(q_in, suffix):
        traj, q_s = smooth_quats(types.SimpleNamespace(vertices=vtx.copy()), copy.deepcopy(rig), q_in.copy())
        G, P = np.zeros((J, T, 3, 3)), np.zeros((J, T, 3), dtype=dtype)
        for t in range(T):                                                   # Rig.FK on a copy, as smooth_quats runs it
            upd = copy.deepcopy(rig)
            upd.local_frames = Rotation.from_quat(q_s[:, t, :]).as_matrix()
            upd.FK()
            G[:, t], P[:, t] = upd.global_transforms, upd.pos
        assert P.dtype == np.dtype(dtype)
        state.update({"ref_quats" + suffix: q_s, "ref_traj" + suffix: traj, "ref_G" + suffix: G, "ref_pos" + suffix: P})
        mine = po.replay(oracle_rig, vtx, q_in)
        assert np.array_equal(mine["quats"], q_s), (name, "smoothed quaternions differ from the reference's")
        scale = max(np.abs(traj).max(), np.abs(P).max())
        dev = max(np.abs(mine["traj"] - traj).max(), np.abs(mine["G"] - G).max(),
                  np.abs(mine["pos"].astype(np.float64) - P.astype(np.float64)).max())
        assert dtype == "float32" or dev <= po.bound(depth, scale), (name, dev, po.bound(depth, scale))
        assert np.abs(mine["traj"] - traj).max() <= po.bound(depth, scale) and np.abs(mine["G"] - G).max() <= po.bound(depth, scale)
        return mine, float(dev), float(scale)

    mine, meta["deviation"], meta["scale"] = run(quats, "")
    if "flip" in opt:
        aligned = po.align_signs(quats)
        assert not np.array_equal(aligned, quats)
        state["aligned_in"] = aligned
        _, meta["deviation_aligned"], _ = run(aligned, "_aligned")
    if dtype == "float32":
        exact = []
        po.fk(oracle_rig, mine["R"], unrounded=exact)
        margin = po.midpoint_margin(np.concatenate([e.reshape(-1) for e in exact])) if exact else float("inf")
        meta["midpoint_margin"] = margin if np.isfinite(margin) else None
        if margin <= MARGIN:
            return None
        assert np.array_equal(mine["pos"], state["ref_pos"]), (name, "float32 positions differ from the reference's")
    return meta, state


def main():
    rp, smooth_quats = reference()
    metas, arrs = [], {}
    for i, (name, J, V, T, dtype, opt) in enumerate(CASES):
        seed = 1900 + i
        while True:
            made = make_case(rp, smooth_quats, name, J, V, T, dtype, opt, seed)
            if made is not None:
                break
            seed += 100
        meta, state = made
        print(f"  {name}: J {J} V {V} T {T} {dtype} depth {meta['depth']} seed {meta['seed']}: deviation {meta['deviation']:.2e} "
              f"(bound {po.bound(meta['depth'], meta['scale']):.2e}, scale {meta['scale']:.3g})")
        metas.append(meta)
        arrs.update({f"c{i}_{k}": v for k, v in state.items()})
    msg.save("playback_cases", dict(cases=metas, margin=MARGIN, step=STEP, scipy=__import__("scipy").__version__), **arrs)


if __name__ == "__main__":
    main()
