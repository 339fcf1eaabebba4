"""Fixtures of the skeleton connection stage (tests/golden/skel_*.npz), made by the reference's own code: models/rootnet.py (ROOTNET),
models/bonenet.py (PairCls), utils/mst_utils.py (sample_on_bone, inside_check, increase_cost_for_outside_bone, primMST),
utils/rig_parser.py (Rig.save) and the functions getInitId / predict_skeleton / create_one_data of evaluate/joint2rig.py, compiled out
of that file at generation time (the module itself imports open3d, cv2 and trimesh). Nothing of the reference is written into the
repository: only inputs and results.

  skel_pairs   (b) create_one_data's pair attributes and the outside-sample counts of increase_cost_for_outside_bone (read off its
               np.sum) for joints inside the tube, bones through the hole of the torus, joints outside the grid, zero-length pairs and
               joints on the symmetry plane
  skel_mst     (c) synthetic logits through predict_skeleton: root id, cost matrix, parent, key, the written _skel.txt; exact ties
               between integer costs, a saturated probability (cost <= 0: no edge), both-on-plane halving, J = 2, J = 48; one case
               also with skin rows (the _rig.txt form)
  skel_nets    (a) ROOTNET and PairCls on one mesh and on a ragged batch of three (J = 2 and J = 48 among them): logits in float32 and
               float64, the FPS start draws, state-dict names and shapes; weights are synth.load_recipe(seed), not stored

Conditions enforced here (the run fails rather than write a fixture that misses one) and re-checked by tests/test_skeleton_oracle.py:
no bone length with length / 0.01 within 1e-6 of a half-integer; no sample within 1e-9 of a voxel rounding boundary; in (c) every Prim
decision (smallest key against the next different key, a key against the cost that relaxes it) clear by 1e-5 with exact ties only
between integer-valued costs, the two largest root logits 1e-5 apart, and every stored pair logit one whose float32 sigmoid as torch
computed it is the float32 nearest to the exact value (torch's CPU sigmoid misses that for about a third of random inputs by one
unit in the last place; the device and tests/skeleton_oracle.py compute the correctly rounded one).

Run from the repository root:  python tools/make_skeleton_golden.py
"""
import ast
import itertools
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from morig_amd import synth                                                    # noqa: E402
from oracle import pyg_primitives as P                                         # noqa: E402
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (Vox, torus_params, tube_grid, circle, save)
import skeleton_oracle as sk                                                   # noqa: E402

SEED_MESH = 5
LEN_MARGIN, VOX_MARGIN, KEY_MARGIN = 1e-6, 1e-9, 1e-5


class _CountingNumpy:
    """stands in for ``np`` inside utils.mst_utils while increase_cost_for_outside_bone runs: the same module, np.sum of a boolean
    array (the outside flags; sample_on_bone sums floats) recorded"""

    def __init__(self):
        self.sums = []

    def __getattr__(self, name):
        return getattr(np, name)

    def sum(self, *a, **kw):
        r = np.sum(*a, **kw)
        if np.asarray(a[0]).dtype == bool:
            self.sums.append(r)
        return r


def reference():
    shim.install()
    sys.modules["torch_geometric.nn"].MessagePassing = P.MessagePassing       # models/bonenet.py:10
    sys.modules["torch_geometric.utils"].softmax = lambda *a, **k: None        # models/bonenet.py:11, unused
    sys.path.insert(0, shim.REFERENCE_ROOT)
    for name in ("open3d", "cv2", "tqdm", "trimesh"):
        sys.modules.setdefault(name, types.ModuleType(name))
    mu = __import__("utils.mst_utils", fromlist=["primMST"])
    rp = __import__("utils.rig_parser", fromlist=["Rig"])
    rootnet = __import__("models.rootnet", fromlist=["ROOTNET"])
    bonenet = __import__("models.bonenet", fromlist=["PairCls"])
    path = os.path.join(shim.REFERENCE_ROOT, "evaluate", "joint2rig.py")
    want = ("getInitId", "predict_skeleton", "create_one_data")
    code = msg._compile_from(path, lambda t: [n for n in t.body if isinstance(n, ast.FunctionDef) and n.name in want])
    ns = dict(np=np, torch=torch, it=itertools, Data=P.Data, add_self_loops=P.add_self_loops, Rig=rp.Rig, primMST=mu.primMST,
              sample_on_bone=mu.sample_on_bone, inside_check=mu.inside_check,
              increase_cost_for_outside_bone=mu.increase_cost_for_outside_bone)
    exec(code, ns)
    return types.SimpleNamespace(mu=mu, rp=rp, ROOTNET=rootnet.ROOTNET, PairCls=bonenet.PairCls, ns=ns)


def torus():
    R, r = msg.torus_params(SEED_MESH)
    return R, r, msg.tube_grid(R, r)


def jitter(rng, pts, s=2e-3):
    return np.asarray(pts, dtype=np.float64) + rng.uniform(-s, s, size=np.asarray(pts).shape)


def ring(R, r, rng, n, spread=0.04):
    """n joints inside the tube at random angles"""
    return np.stack([msg.circle(R, r, rng.uniform(0, 360), inward=rng.uniform(-spread, spread), up=rng.uniform(-spread, spread))
                     for _ in range(n)], 0)


def geometry_ok(joints, grid):
    o = sk.pair_attributes(joints, grid, msg.VOX_T, msg.VOX_S, 88)
    return o["length_margin"] >= LEN_MARGIN and o["voxel_margin"] >= VOX_MARGIN, o


def draw(make, grid, tries=200):
    """make(rng) -> joints; the first draw that keeps the geometric conditions"""
    for t in range(tries):
        j = make(np.random.default_rng([0x736B656C, t]))
        ok, o = geometry_ok(j, grid)
        if ok:
            return j, o, t
    raise RuntimeError("no draw met the fixture conditions")


# ------------------------------------------------------------------------------------------------------------------- group (b)
def pair_cases(R, r):
    c = msg.circle
    return {
        "inside": lambda g: jitter(g, ring(R, r, g, 12)),
        "hole": lambda g: jitter(g, [c(R, r, 0), c(R, r, 180), c(R, r, 90), c(R, r, 270), c(R, r, 45), c(R, r, 225),
                                     [0.0, r, 0.0], [0.03, r + 0.02, -0.02]]),
        "outside_grid": lambda g: jitter(g, [[0.70, r, 0.10], [-0.90, 0.50, 0.20], [0.20, -0.60, 0.30], [0.10, 0.90, -0.80],
                                             c(R, r, 10), c(R, r, 100), c(R, r, 200)]),
        "zero_length": lambda g: (lambda a: np.concatenate([a, a[[0, 2, 2]]], 0))(jitter(g, ring(R, r, g, 5))),
        "plane": lambda g: (lambda a: a * np.array([[0.0, 1, 1]] * 3 + [[1.0, 1, 1]] * 3) + np.array(
            [[0, 0, 0], [0.0199, 0, 0], [-0.0201, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]))(
            jitter(g, [c(R, r, 90), c(R, r, 270), c(R, r, 90, up=0.05), c(R, r, 0), c(R, r, 60), c(R, r, 180)])),
    }


def reference_pairs(ref, joints, vox):
    z = np.zeros((4, 3))
    data = ref.ns["create_one_data"](z, joints, np.zeros((2, 0)), np.zeros((2, 0)), vox)
    counter = _CountingNumpy()
    ref.mu.np = counter
    try:
        ref.mu.increase_cost_for_outside_bone(np.zeros((len(joints), len(joints))), data.joints.numpy(), vox)
    finally:
        ref.mu.np = np
    n_pairs = len(joints) * (len(joints) - 1) // 2
    assert len(counter.sums) == n_pairs
    return data, np.array([int(s) for s in counter.sums], dtype=np.int32)


def group_b(ref, R, r, grid):
    vox = msg.Vox(grid)
    arrs, meta = {}, dict(cases=[], draws={})
    for name, make in pair_cases(R, r).items():
        joints, o, t = draw(make, grid)
        data, outside = reference_pairs(ref, joints, vox)
        pairs = data.pairs.numpy().astype(np.int64)
        attr = data.pair_attr.numpy()
        # the oracle is the reference here, or the conditions it reports are about something else
        assert np.array_equal(pairs, o["pairs"]) and np.array_equal(outside, o["outside_count"])
        assert np.array_equal(attr[:, 1].view(np.uint32), o["pair_attr"][:, 1].view(np.uint32))
        meta["cases"].append(name)
        meta["draws"][name] = t
        arrs.update({f"{name}_joints": joints, f"{name}_pairs": pairs, f"{name}_pair_attr": attr, f"{name}_outside": outside})
        print(f"  pairs/{name}: J={len(joints)} P={len(pairs)} outside>1: {int((outside > 1).sum())} samples<=0: "
              f"{int((o['n_samples'][:, 0] == 0).sum())} margins {o['length_margin']:.2e} {o['voxel_margin']:.2e}")
    assert (arrs["zero_length_pair_attr"][:, 0] == 0).sum() >= 3 and (arrs["hole_outside"] > 1).any()
    assert (arrs["outside_grid_pair_attr"][:, 1] == 0).any()
    return meta, arrs


# ------------------------------------------------------------------------------------------------------------------- group (c)
def exact_sigmoid_logits(logits, rng, scale, fixed=()):
    """redraw every logit (nudge the ``fixed`` ones) until torch's float32 sigmoid of the WHOLE tensor (what predict_skeleton
    evaluates) is the correctly rounded one for every entry"""
    x = np.asarray(logits, dtype=np.float32).copy()
    keep = np.zeros(len(x), dtype=bool)
    keep[list(fixed)] = True
    for _ in range(400):
        got = torch.sigmoid(torch.from_numpy(x).reshape(-1, 1)).numpy().reshape(-1)
        bad = got != sk.sigmoid_f32(x)
        if not bad.any():
            return x
        x[bad & keep] = np.nextafter(x[bad & keep], np.float32(np.inf))
        x[bad & ~keep] = rng.normal(0.0, scale, size=int((bad & ~keep).sum())).astype(np.float32)
    raise RuntimeError("no exactly rounded sigmoid inputs found")


def mst_cases(R, r):
    c = msg.circle
    col = lambda x, z, n, y0: [[x, y0 + 0.05 * k, z] for k in range(n)]       # a column of joints in the hole: every sample outside
    return {
        # equally spaced joints outside the mesh: bones of 5, 10, ... samples, all outside -> integer costs with exact ties
        "ties": (lambda g: jitter(g, col(0.10, 0.05, 4, r - 0.05) + col(-0.08, -0.03, 3, r) + [c(R, r, 20), c(R, r, 50), c(R, r, 80)], 1e-4),
                 dict(scale=2.0)),
        "saturated": (lambda g: jitter(g, [c(R, r, 30.0 * k) for k in range(9)]), dict(scale=2.0, saturate=((0, 1, 30.0), (3, 4, 30.0), (1, 2, 16.0)))),
        "plane": (lambda g: np.concatenate([jitter(g, [c(R, r, 90), c(R, r, 270), c(R, r, 90, up=0.04), c(R, r, 270, inward=0.03)])
                                            * np.array([[0.0, 1, 1]]) + np.array([[0.0, 0, 0], [0.01, 0, 0], [-0.015, 0, 0], [0.0199, 0, 0]]),
                                            jitter(g, ring(R, r, g, 5))], 0), dict(scale=2.0, skins=True)),
        "two": (lambda g: jitter(g, [c(R, r, 10), c(R, r, 40)]), dict(scale=2.0)),
        "fortyeight": (lambda g: jitter(g, ring(R, r, g, 48)), dict(scale=2.0)),
    }


def reference_skeleton(ref, joints, vox, pair_logits, root_logits):
    data = ref.ns["create_one_data"](np.zeros((4, 3)), joints, np.zeros((2, 0)), np.zeros((2, 0)), vox)
    seen = {}

    def prim(graph, init_id):
        seen["cost"], seen["root"] = np.array(graph, dtype=np.float64), int(init_id)
        return ref.mu.primMST(graph, init_id)
    ref.ns["primMST"] = prim
    pl, rl = torch.from_numpy(pair_logits).reshape(-1, 1), torch.from_numpy(root_logits).reshape(-1, 1)
    t0 = time.perf_counter()
    rig = ref.ns["predict_skeleton"](data, vox, lambda d, shuffle: (rl, None), lambda d, permute_joints: (pl, None))
    secs = time.perf_counter() - t0
    ref.ns["primMST"] = ref.mu.primMST
    parent = np.array(rig.hierarchy, dtype=np.int32)
    key = np.array(ref.mu.primMST(seen["cost"], seen["root"])[1], dtype=np.float64)
    return data, rig, seen["cost"], seen["root"], parent, key, secs


def group_c(ref, R, r, grid):
    vox = msg.Vox(grid)
    arrs, meta = {}, dict(cases=[], draws={}, notes={})
    for name, (make, opt) in mst_cases(R, r).items():
        for t in range(400):
            g = np.random.default_rng([0x6D7374, t])
            joints = make(g)
            ok, o = geometry_ok(joints, grid)
            if not ok:
                continue
            n = len(joints)
            pairs = sk.pair_list(n)
            pl = g.normal(0.0, opt["scale"], size=len(pairs)).astype(np.float32)
            fixed = [int(np.where((pairs[:, 0] == i) & (pairs[:, 1] == j))[0][0]) for (i, j, _) in opt.get("saturate", ())]
            pl[fixed] = [v for (_, _, v) in opt.get("saturate", ())]
            pl = exact_sigmoid_logits(pl, g, opt["scale"], fixed)
            rl = g.normal(0.0, 1.0, size=n).astype(np.float32)
            cost, root, from_count = sk.connectivity_cost(pl, rl, joints.astype(np.float32), o["outside_count"])
            parent, key, status, info = sk.prim(cost, root)
            if status == 0 and info["margin"] >= KEY_MARGIN and info["ties_integer"] and sk.root_margin(rl) >= KEY_MARGIN:
                break
        else:
            raise RuntimeError(f"{name}: no draw met the fixture conditions")
        data, rig, rcost, rroot, rparent, rkey, secs = reference_skeleton(ref, joints, vox, pl, rl)
        assert rroot == root and np.array_equal(rparent, parent), name
        assert np.array_equal(rcost[from_count], cost[from_count]) and np.allclose(rcost, cost, rtol=1e-14, atol=0), name
        ties = int(sum(1 for a in range(n) for b in range(a + 1, n) if from_count[a, b]))
        note = dict(count_entries=ties, no_edge=int((rcost <= 0).sum() // 2), halved=int(
            sum(1 for a, b in pairs if abs(np.float32(joints[a, 0])) < np.float32(2e-2) and abs(np.float32(joints[b, 0])) < np.float32(2e-2))),
            key_margin=info["margin"], root_margin=sk.root_margin(rl))
        if name == "ties":
            ks = key[np.arange(n) != root]
            assert len(np.unique(ks)) < len(ks) and np.all(ks[np.isin(ks, [k for k in ks if (ks == k).sum() > 1])] % 1 == 0)
        if name == "saturated":
            assert note["no_edge"] >= 2
        if name == "plane":
            assert note["halved"] >= 3
        tmp = tempfile.mkdtemp()
        rig.hierarchy = np.array(rig.hierarchy)              # Rig.save compares the hierarchy with ==: it has to be an array
        rig.save(os.path.join(tmp, "skel.txt"))
        arrs.update({f"{name}_joints": joints, f"{name}_pair_logits": pl, f"{name}_root_logits": rl, f"{name}_cost": rcost,
                     f"{name}_root": np.array(rroot, dtype=np.int32), f"{name}_parent": rparent, f"{name}_key": rkey,
                     f"{name}_prob": torch.sigmoid(torch.from_numpy(pl).reshape(-1, 1)).numpy().reshape(-1),
                     f"{name}_rig_pos": np.asarray(rig.pos), f"{name}_rig_offset": np.asarray(rig.offset),
                     f"{name}_skel_txt": np.frombuffer(open(os.path.join(tmp, "skel.txt"), "rb").read(), dtype=np.uint8)})
        if opt.get("skins"):
            w = np.round(g.uniform(0, 1, size=(30, n)) * (g.uniform(0, 1, size=(30, n)) < 0.3), 4)
            rig.skins = w
            rig.save(os.path.join(tmp, "rig.txt"))
            arrs.update({f"{name}_skins": w, f"{name}_rig_txt": np.frombuffer(open(os.path.join(tmp, "rig.txt"), "rb").read(), dtype=np.uint8)})
        meta["cases"].append(name)
        meta["draws"][name] = t
        meta["notes"][name] = note
        print(f"  mst/{name}: J={n} root={rroot} {note} reference {secs * 1e3:.1f} ms")
    return meta, arrs


# ------------------------------------------------------------------------------------------------------------------- group (a)
def collate(datas):
    """PyG batching of create_one_data's objects; ``pairs`` index the concatenated joints (the forwards gather data.joints with them)"""
    out = P.Data()
    voff = joff = 0
    cat = {k: [] for k in ("pos", "tpl_edge_index", "geo_edge_index", "batch", "joints", "pairs", "pair_attr", "joints_batch", "pairs_batch")}
    for b, d in enumerate(datas):
        cat["pos"].append(d.pos)
        cat["tpl_edge_index"].append(d.tpl_edge_index + voff)
        cat["geo_edge_index"].append(d.geo_edge_index + voff)
        cat["batch"].append(d.batch + b)
        cat["joints"].append(d.joints)
        cat["pairs"].append(d.pairs + joff)
        cat["pair_attr"].append(d.pair_attr)
        cat["joints_batch"].append(d.joints_batch + b)
        cat["pairs_batch"].append(d.pairs_batch + b)
        voff += d.pos.shape[0]
        joff += d.joints.shape[0]
    for k, v in cat.items():
        setattr(out, k, torch.cat(v, dim=1 if k.endswith("edge_index") else 0))
    return out


def to_double(d):
    out = P.Data(**d.__dict__)
    for k in ("pos", "joints", "pairs", "pair_attr"):
        setattr(out, k, getattr(d, k).double())
    return out


NET_CASES = {"single": [(11, 32, 24)], "ragged": [(12, 16, 2), (13, 24, 48), (14, 20, 17)]}       # (mesh seed, n_side, joints)
NETS = (("rootnet", "ROOTNET", 701, "shuffle"), ("bonenet", "PairCls", 702, "permute_joints"))
NET_SEED, NET_SEED_RANDOM = 900, 950


def net_joints(mesh_seed, n_joints):
    R, r = msg.torus_params(mesh_seed)
    return R, r, (lambda g: jitter(g, ring(R, r, g, n_joints)))


def run_nets(ref, data, dt, seed, random):
    """both networks after ONE torch.manual_seed, ROOTNET first: the order of predict_skeleton's draws"""
    outs = {}
    models = {net: synth.load_recipe(getattr(ref, cls)(), rseed, mild=True).to(dt).eval() for net, cls, rseed, _ in NETS}
    with shim.pretend_cuda_available(), torch.no_grad():
        torch.manual_seed(seed)                              # after the constructors: their initialisers draw too
        for net, _, _, flag in NETS:
            outs[net] = models[net](data if dt == torch.float32 else to_double(data), **{flag: random})
    return outs


def group_a(ref):
    arrs, meta = {}, dict(cases={}, nets={}, numpy=np.__version__, torch=torch.__version__, torch_seed=NET_SEED,
                          random_torch_seed=NET_SEED_RANDOM)
    for net, cls, rseed, flag in NETS:
        sd = getattr(ref, cls)().state_dict()
        meta["nets"][net] = dict(cls=cls, recipe_seed=rseed, mild=True, flag=flag, state_dict=[[k, list(v.shape)] for k, v in sd.items()])
    for cname, spec in NET_CASES.items():
        datas, joints_all, voxes = [], [], []
        for mesh_seed, n_side, nj in spec:
            mesh = synth.make_mesh(mesh_seed, n_side=n_side, with_skin=False)
            R, r, make = net_joints(mesh_seed, nj)
            grid = msg.tube_grid(R, r)
            joints, _, _ = draw(make, grid)
            voxes.append(msg.Vox(grid))
            datas.append(ref.ns["create_one_data"](mesh.pos.numpy().astype(np.float64), joints, mesh.tpl_edge_index.numpy(),
                                                   mesh.geo_edge_index.numpy(), voxes[-1]))
            joints_all.append(joints)
        data = collate(datas)
        counts = [len(j) for j in joints_all]
        meta["cases"][cname] = dict(spec=spec, n_joints=counts)
        arrs[f"{cname}_joints"] = np.concatenate(joints_all, 0)
        arrs[f"{cname}_pair_attr"] = data.pair_attr.numpy()
        arrs[f"{cname}_vox_bits"] = np.stack([np.packbits(v.data.reshape(-1).astype(np.uint8)) for v in voxes], 0)
        f32, f64 = run_nets(ref, data, torch.float32, NET_SEED, False), run_nets(ref, data, torch.float64, NET_SEED, False)
        torch.manual_seed(NET_SEED)                          # the draws of those forwards: per network sa1's clouds, then sa2's
        arrs[f"{cname}_fps_starts"] = np.array([int(torch.randint(c, (1,))) for _ in range(4) for c in counts], dtype=np.int32)
        for net, _, _, _ in NETS:
            dev = float((f32[net][0].double() - f64[net][0]).abs().max())
            assert dev < 1e-3, (cname, net, dev)             # a different FPS pick in float64 would show as a gross difference
            arrs[f"{cname}_{net}_f32"], arrs[f"{cname}_{net}_f64"] = f32[net][0].numpy(), f64[net][0].numpy()
            o = f32[net][0]
            print(f"  nets/{cname}/{net}: out {tuple(o.shape)} |logit|inf {float(o.abs().max()):.3f} range {float(o.max() - o.min()):.2e} "
                  f"f32-f64 {dev:.2e}")
        # end to end: the reference's predict_skeleton per mesh on those logits (its forwards batch, its predict_skeleton does not)
        jp, pp = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum([c * (c - 1) // 2 for c in counts])])
        costs, parents, roots = [], [], []
        for b in range(len(spec)):
            _, rig, cost, root, parent, _, _ = reference_skeleton(ref, joints_all[b], voxes[b],
                                                                  f32["bonenet"][0].numpy()[pp[b]:pp[b + 1], 0].copy(),
                                                                  f32["rootnet"][0].numpy()[jp[b]:jp[b + 1], 0].copy())
            costs.append(cost.reshape(-1))
            parents.append(parent)
            roots.append(root)
        arrs[f"{cname}_ref_cost"], arrs[f"{cname}_ref_parent"] = np.concatenate(costs), np.concatenate(parents)
        arrs[f"{cname}_ref_root"] = np.array(roots, dtype=np.int32)
        if cname == "single":                                 # the random branches, with the reference's own draws
            rnd = run_nets(ref, data, torch.float32, NET_SEED_RANDOM, True)
            for net, _, _, _ in NETS:
                arrs[f"{cname}_{net}_random_f32"], arrs[f"{cname}_{net}_random_labels"] = rnd[net][0].numpy(), rnd[net][1].numpy()
    # the reference's time for one production-size mesh: create_one_data + predict_skeleton, 4096 vertices, 36 joints, this CPU
    mesh = synth.make_mesh(21, n_side=64, with_skin=False)
    R, r, make = net_joints(21, 36)
    grid = msg.tube_grid(R, r)
    joints, _, _ = draw(make, grid)
    root_net, bone_net = ref.ROOTNET().eval(), ref.PairCls().eval()
    synth.load_recipe(root_net, 701, mild=True)
    synth.load_recipe(bone_net, 702, mild=True)
    runs = []
    with shim.pretend_cuda_available():
        for rep in range(3):                                  # the machine is shared: three runs, all kept, the fastest quoted
            torch.manual_seed(1)
            t0 = time.perf_counter()
            d = ref.ns["create_one_data"](mesh.pos.numpy().astype(np.float64), joints, mesh.tpl_edge_index.numpy(),
                                          mesh.geo_edge_index.numpy(), msg.Vox(grid))
            t1 = time.perf_counter()
            rig = ref.ns["predict_skeleton"](d, msg.Vox(grid), root_net, bone_net)
            t2 = time.perf_counter()
            runs.append(dict(create_one_data_s=t1 - t0, predict_skeleton_s=t2 - t1, total_s=t2 - t0))
    best = min(runs, key=lambda r: r["total_s"])
    meta["reference_cpu"] = dict(vertices=4096, joints=36, runs=runs, threads=torch.get_num_threads(), date=time.strftime("%Y-%m-%d"),
                                 note="the reference's Python with pure-torch stand-ins for PyG, on the generating CPU", **best)
    print(f"  reference, one 4096-vertex mesh with 36 joints, best of 3: create_one_data {best['create_one_data_s']:.3f} s, "
          f"predict_skeleton {best['predict_skeleton_s']:.3f} s (root {rig.root_id}); totals {[round(r['total_s'], 3) for r in runs]}")
    return meta, arrs


def main():
    ref = reference()
    R, r, grid = torus()
    bits = np.packbits(grid.reshape(-1).astype(np.uint8))
    common = dict(mesh_seed=SEED_MESH, translate=[float(x) for x in msg.VOX_T], scale=msg.VOX_S, dims=[88, 88, 88], numpy=np.__version__,
                  torch=torch.__version__, margins=dict(length=LEN_MARGIN, voxel=VOX_MARGIN, key=KEY_MARGIN))
    print("group (b)")
    meta, arrs = group_b(ref, R, r, grid)
    msg.save("skel_pairs", dict(common, **meta), vox_bits=bits, **arrs)
    print("group (c)")
    meta, arrs = group_c(ref, R, r, grid)
    msg.save("skel_mst", dict(common, **meta), vox_bits=bits, **arrs)
    print("group (a)")
    meta, arrs = group_a(ref)
    msg.save("skel_nets", dict(common, **meta), **arrs)


if __name__ == "__main__":
    main()
