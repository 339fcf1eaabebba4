"""Fixtures of the skinning preparation and post-processing (tests/golden/skin_*.npz), made by the reference's own functions:
data_proc.common_ops.calc_volumetric_geodesic (with its process pool), data_proc.gen_skin_data.get_bones, the bind-row and file-writing
statements of gen_skin_data.py's main block (:80-135, compiled from the reference file at generation time) and training/train_skin.py's
post_filter (the one function, compiled the same way). Nothing of the reference is written into the repository: only inputs and results.

Cases (synthetic torus meshes of morig_amd.synth, voxelised analytically as a solid tube):
  skin_connected  one connected tube, a skeleton along the centre circle with a side branch and three leaves (17 bones); also the
                  post-processing case: seeded logits and the reference's weights in both caller orders (train_skin, joint2rig)
  skin_islands    the same tube plus two disconnected voxel islands with vertices in them: the patch runs twice, the second time
                  after the one-call lag; every patch is checked to be tie-free (all equally near reached voxels have one distmap value)
  skin_outside    vertices in the empty hole of the torus (voxels outside the mask) and a bone that leaves the tube
  skin_fewbones   a 4-bone skeleton: slots past the bone count are -1

Run from the repository root:  python tools/make_skin_golden.py
"""
import ast
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morig_amd import synth          # noqa: E402
from oracle import shim              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N_SIDE = 24
K = 20
VOX_T = np.array([-0.55, -0.40, -0.55])
VOX_S = 1.1


class Vox:
    def __init__(self, data):
        self.data = data
        self.translate = [float(x) for x in VOX_T]
        self.scale = VOX_S
        self.dims = [88, 88, 88]


def _reference():
    sys.path.insert(0, shim.REFERENCE_ROOT)
    for name in ("open3d", "cv2", "tqdm"):                       # imported at module level by utils/ and data_proc/, unused here
        sys.modules.setdefault(name, types.ModuleType(name))
    if not hasattr(np, "int"):
        np.int = int                                     # utils/binvox_rw.py predates numpy 1.24
    if not hasattr(np, "bool"):
        np.bool = bool
    co = __import__("data_proc.common_ops", fromlist=["calc_volumetric_geodesic"])
    gs = __import__("data_proc.gen_skin_data", fromlist=["get_bones"])
    rp = __import__("utils.rig_parser", fromlist=["Rig"])
    mu = __import__("utils.mst_utils", fromlist=["sample_on_bone"])
    return co, gs, rp, mu


def _compile_from(path, pick):
    """compile statements of a reference file at generation time: pick(tree) -> list of ast statements"""
    src = open(path).read()
    mod = ast.Module(body=pick(ast.parse(src)), type_ignores=[])
    return compile(mod, path, "exec")


def _post_filter():
    path = os.path.join(shim.REFERENCE_ROOT, "training", "train_skin.py")
    code = _compile_from(path, lambda t: [n for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "post_filter"])
    ns = {"np": np}
    exec(code, ns)
    return ns["post_filter"]


def _bind_block():
    """gen_skin_data.py's statements from `num_nearest_bone = 20` through the `with open(..._skin.txt)` writer"""
    path = os.path.join(shim.REFERENCE_ROOT, "data_proc", "gen_skin_data.py")

    def pick(tree):
        main = [n for n in tree.body if isinstance(n, ast.If)][-1]
        loop = [n for n in main.body if isinstance(n, ast.For)][-1]
        body = loop.body
        start = next(i for i, n in enumerate(body) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "num_nearest_bone")
        end = next(i for i, n in enumerate(body) if isinstance(n, ast.With))
        return body[start:end + 1]
    return _compile_from(path, pick)


def torus_params(seed):
    rng = np.random.default_rng([0x4D6F5269, seed])               # the first two draws of synth.make_mesh
    R = 0.35 * (1.0 + 0.1 * rng.uniform(-1, 1))
    r = 0.12 * (1.0 + 0.1 * rng.uniform(-1, 1))
    return R, r


def voxel_centres():
    i = np.arange(88)
    c = [VOX_T[a] + (i / 88.0) * VOX_S for a in range(3)]
    return np.meshgrid(c[0], c[1], c[2], indexing="ij")


def tube_grid(R, r):
    X, Y, Z = voxel_centres()
    rho = np.sqrt(X ** 2 + Z ** 2)
    return ((rho - R) ** 2 + (Y - r) ** 2) <= (r + 0.012) ** 2


def circle(R, r, deg, inward=0.0, up=0.0):
    a = np.deg2rad(deg)
    return np.array([(R - inward) * np.cos(a), r + up, (R - inward) * np.sin(a)])


def rig_text(joints, parents, pos):
    """a _rig.txt (utils/rig_parser.py format): skins = the 3 nearest joints by inverse distance, 4 decimals"""
    names = [f"j{i}" for i in range(len(joints))]
    lines = [f"joints {n} {p[0]:.8f} {p[1]:.8f} {p[2]:.8f}" for n, p in zip(names, joints)]
    lines.append(f"root {names[parents.index(-1)]}")
    d = np.sqrt(((pos[:, None, :] - np.asarray(joints)[None]) ** 2).sum(-1))
    for v in range(len(pos)):
        nn = np.argsort(d[v], kind="stable")[:3]
        w = 1.0 / (d[v, nn] + 1e-3)
        w = np.round(w / w.sum(), 4)
        lines.append(f"skin {v} " + " ".join(f"{names[j]} {x:.4f}" for j, x in zip(nn, w)))
    for i, p in enumerate(parents):
        if p >= 0:
            lines.append(f"hier {names[p]} {names[i]}")
    return "\n".join(lines) + "\n"


def skeleton_main(R, r):
    """root at 0 deg, two chains of 6 around the circle, a 2-joint side branch from the third joint of the first chain: 17 bones"""
    j = [circle(R, r, 0)]
    par = [-1]
    prev = 0
    for s in (1, -1):
        prev = 0
        for t in range(1, 7):
            j.append(circle(R, r, s * 24.0 * t))
            par.append(prev)
            prev = len(j) - 1
    j.append(circle(R, r, 72.0, inward=0.05))
    par.append(3)
    j.append(circle(R, r, 72.0, inward=0.05, up=0.05))
    par.append(len(j) - 2)
    return j, par


def run_reference(ref, name, pos, grid, rig_txt, tie_log):
    co, gs, rp, mu = ref
    tmp = tempfile.mkdtemp()
    rig_file = os.path.join(tmp, "rig.txt")
    open(rig_file, "w").write(rig_txt)
    rig = rp.Rig(rig_file)
    bones, bone_names, bone_isleaf = gs.get_bones(rig)
    vox = Vox(grid)
    t0 = time.perf_counter()
    dist = co.calc_volumetric_geodesic(pos, vox, bones)
    secs = time.perf_counter() - t0
    ns = dict(np=np, os=os, vtx=pos, rig=rig, bones=bones, bone_names=bone_names, bone_isleaf=bone_isleaf,
              vol_geodesic_dist=dist, dataset_folder=tmp + "/", split_name="x", model_id=name)
    os.makedirs(os.path.join(tmp, "x"), exist_ok=True)
    exec(_bind_block(), ns)
    skin_file = os.path.join(tmp, "x", f"{name}_skin.txt")
    rows = np.array(ns["input_samples"], dtype=np.float64)
    labels = np.array(ns["ground_truth_labels"], dtype=np.float64)
    return dict(rig=rig, bones=bones, bone_names=bone_names, is_leaf=np.array(bone_isleaf, dtype=np.uint8), dist=dist, secs=secs,
                rows=rows, labels=labels, skin_txt=open(skin_file, "rb").read(), skin_file=skin_file)


class TieCheckingKDTree:
    """stands in for scipy.spatial.KDTree inside one_bone: the same queries, and an assertion that every patched voxel's equally near
    reached voxels all carry one distmap value (so the reference's choice among them is not arbitrary)"""
    real = None

    def __init__(self, data):
        self.data = np.asarray(data)
        self.tree = TieCheckingKDTree.real(data)

    def query(self, x):
        dd, ii = self.tree.query(x)
        distmap = sys._getframe(1).f_locals["distmap_bone"]
        x = np.asarray(x)
        for u in np.where(dd == np.min(dd))[0]:
            d2 = ((self.data - x[u][None]) ** 2).sum(1)
            tied = self.data[d2 == d2.min()]
            vals = set(int(distmap[p[0], p[1], p[2]]) for p in tied)
            assert len(vals) == 1, f"patch tie with distmaps {vals}"
        with open(os.environ["MORIG_SKIN_TIE_LOG"], "a") as f:
            f.write(f"{len(np.where(dd == np.min(dd))[0])}\n")
        return dd, ii


def islands_case(tube, pos0, R, r, shift):
    """one single-voxel island in the torus hole (reached by the patch alone: the one-call lag follows) and a larger block far above
    the ring, patched second"""
    X, Y, Z = voxel_centres()
    isl = tube.copy()
    c1 = np.array([0.0125 * (shift % 3), r, 0.0125 * (shift // 3)])
    c2 = np.array([-R + 0.0125 * shift, 2 * r + 0.3, 0.01])
    for c, h in ((c1, 0.005), (c2, 0.03)):
        isl |= (np.abs(X - c[0]) <= h) & (np.abs(Y - c[1]) <= h) & (np.abs(Z - c[2]) <= h)
    pos = np.concatenate([pos0, c1[None], c2[None] + [[0.0, 0.0, 0.0], [0.0, 0.02, 0.0]]], 0)
    return pos, isl


def post_process_reference(post_filter, logits, mask, nn, tpl_e, nb, mode):
    """train_skin.py:232-244 / joint2rig.py:447-462 on one mesh"""
    lg = torch.from_numpy(logits)
    if mode == "train_skin":
        p = torch.softmax(lg, dim=1) * torch.from_numpy(mask).float()
        ratio = 0.5
    else:
        p = torch.softmax(lg * torch.from_numpy(mask), dim=1)
        ratio = 0.35
    p = p.numpy()
    full = np.zeros((len(p), nb))
    for v in range(len(p)):
        for s in range(nn.shape[1]):
            if mask[v, s] == 1:
                full[v, nn[v, s]] = p[v, s]
    filt = post_filter(full, tpl_e, num_ring=1)
    thr = np.max(filt, axis=1, keepdims=True) * ratio
    margin = np.abs(filt - thr).min()
    out = filt.copy()
    out[out < thr] = 0.0
    out = out / (out.sum(axis=1, keepdims=True) + 1e-10)
    return out, margin


def save(name, meta, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrs)
    size = os.path.getsize(path)
    assert size <= 1 << 20, (path, size)
    print(f"  {name}: {size} bytes")


def main():
    from morig_amd import formats
    ref = _reference()
    co = ref[0]
    TieCheckingKDTree.real = co.KDTree
    co.KDTree = TieCheckingKDTree                     # before the pool forks: the workers inherit it
    log = os.path.join(tempfile.mkdtemp(), "ties.txt")
    os.environ["MORIG_SKIN_TIE_LOG"] = log
    post_filter = _post_filter()
    seed = 5
    mesh = synth.make_mesh(seed, n_side=N_SIDE, with_skin=False)
    pos0 = mesh.pos.numpy().astype(np.float64)
    R, r = torus_params(seed)
    tube = tube_grid(R, r)
    joints, parents = skeleton_main(R, r)

    cases = []
    # 1 connected
    cases.append(("skin_connected", pos0, tube, joints, parents))
    # 2 islands: two blobs, one in the torus hole, one outside the ring, vertices in them; the first placement whose patches are all
    # tie-free is kept (islands_case)
    cases.append(("skin_islands", None, None, joints, parents))
    # 3 outside the mask: vertices in the empty hole, a bone leaving the tube towards the centre
    j3 = [circle(R, r, 0), circle(R, r, 40), circle(R, r, 80), circle(R, r, 40, inward=0.2), circle(R, r, -40), circle(R, r, -80)]
    p3 = [-1, 0, 1, 1, 0, 4]
    pos_out = np.concatenate([pos0, [[0.0, r, 0.0], [0.05, r, -0.04], [-0.1, 0.02, 0.1]]], 0)
    cases.append(("skin_outside", pos_out, tube, j3, p3))
    # 4 few bones
    j4 = [circle(R, r, 0), circle(R, r, 60), circle(R, r, 120), circle(R, r, 180)]
    cases.append(("skin_fewbones", pos0, tube, j4, [-1, 0, 1, 2]))

    for name, pos, grid, jn, par in cases:
        for shift in range(12 if pos is None else 1):
            open(log, "w").close()
            if name == "skin_islands":
                pos, grid = islands_case(tube, pos0, R, r, shift)
            txt = rig_text(jn, par, pos)
            try:
                res = run_reference(ref, name, pos, grid, txt, log)
                break
            except AssertionError as e:
                if name != "skin_islands":
                    raise
                print(f"  islands placement {shift}: {e}")
        else:
            raise RuntimeError("no tie-free island placement")
        patches = [int(x) for x in open(log).read().split()]
        print(f"{name}: V={len(pos)} bones={len(res['bones'])} patches={patches} {res['secs']:.2f} s")
        if name == "skin_islands":
            assert len(patches) >= 2 * len(res["bones"]), patches
        elif name != "skin_outside":                     # there a leaf bone lies outside the mask: its seed reaches nothing
            assert not patches, patches
        meta = dict(case=name, k=K, bone_names=res["bone_names"], ref_seconds=res["secs"], n_patches=len(patches),
                    translate=[float(x) for x in VOX_T], scale=VOX_S, dims=[88, 88, 88],
                    cpu_workers=8, note="ref_seconds: calc_volumetric_geodesic with its 8-process pool on the generating CPU")
        arrs = dict(pos=pos, vox_bits=np.packbits(grid.reshape(-1).astype(np.uint8)), rig_txt=np.frombuffer(txt.encode(), dtype=np.uint8),
                    bones=res["bones"], is_leaf=res["is_leaf"], dist=res["dist"].astype(np.int32), bind_rows=res["rows"],
                    labels=res["labels"], skin_txt=np.frombuffer(res["skin_txt"], dtype=np.uint8))
        if name == "skin_connected":
            assert res["dist"].min() > 0                 # no 1e10 inputs: the network comparison runs on this case
            _, nn, _, mask, _ = formats.load_skin(res["skin_file"])
            tpl = mesh.tpl_edge_index.numpy()
            nb = len(res["bones"])
            for s in range(100):
                logits = np.random.default_rng([77, s]).normal(0.0, 2.0, size=(len(pos), K)).astype(np.float32)
                w_ts, m1 = post_process_reference(post_filter, logits, mask, nn, tpl, nb, "train_skin")
                w_jr, m2 = post_process_reference(post_filter, logits, mask, nn, tpl, nb, "joint2rig")
                if min(m1, m2) > 1e-6:
                    break
            else:
                raise RuntimeError("no logits seed with every entry clear of its threshold")
            print(f"  logits seed {s}: threshold margins {m1:.2e} {m2:.2e}")
            meta["logits_seed"] = s
            arrs.update(tpl_edge_index=tpl, logits=logits, weights_train_skin=w_ts, weights_joint2rig=w_jr)
        save(name, meta, **arrs)


if __name__ == "__main__":
    main()
