"""Fixtures of the rig assembly (tests/golden/rig_assemble_trees.npz, rig_assemble_degenerate.npz), made by the reference's own
functions: add_duplicate_joints, mapping_bone_index, assemble_skel_skin and remove_dup_joints of evaluate/joint2rig.py and get_bones of
data_proc/gen_skin_data.py, compiled out of the reference files by AST at generation time (the modules themselves import open3d, cv2 and
trimesh), over the reference's own Rig, calc_frames_and_offsets and Rig.save (utils/rig_parser.py). Nothing of the reference is written
into the repository: only inputs and recorded results.

  rig_assemble_trees       random trees of 2, 3, 23 and 48 joints with float32 and float64 joints, a root that is not index 0 and 1, 63,
                           65 or 257 vertices.
  rig_assemble_degenerate  the rigs on which "sum the bones that start at each joint" is wrong, 40 vertices each: two children of one
                           parent at one position; a leaf at its parent's position; all joints coincident; a child on a two-child
                           parent (a zero-length bone: here the naive sum agrees); and a tree with a joint already named ``x_dup_0``.

Per case: pos (before the rig's own forward pass; skel_pos after it), hier, root_id and names of the skeleton; the bone weights
[V, n_bones]; new_of_bone; names, hierarchy, positions and skins of the intermediate rig (with duplicates) and of the final one; the
bytes of the written _rig.txt. Weights: up to five bones per
vertex, normalised, then exact zeros, 1e-5 itself, its two float64 neighbours and values below it written over some entries (nothing is
renormalised: neither does the reference).

Conditions enforced here and re-asserted by tests/test_rigging_oracle.py: for every old bone the nearest and second-nearest new-bone
distances are bitwise equal (the first index wins) or more than GAP = 1e-9 apart; the naive start-joint sum differs from the expected
skins on the degenerate cases marked so, and is bit-equal on the random trees.

Run from the repository root:  python tools/make_rigging_golden.py
"""
import ast
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (_compile_from, save)
import rigging_oracle as ro                                                    # noqa: E402

GAP = 1e-9
TREES = [(2, "float32", 1), (2, "float64", 63), (3, "float32", 65), (3, "float64", 257), (23, "float32", 257), (23, "float64", 65),
         (48, "float32", 63), (48, "float64", 257)]
V_DEGENERATE = 40
SPECIALS = [0.0, 1e-5, float(np.nextafter(1e-5, 1.0)), float(np.nextafter(1e-5, 0.0)), 3e-6, 1e-7]


def reference():
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    rp = __import__("utils.rig_parser", fromlist=["Rig"])
    funcs = lambda want: (lambda t: [n for n in t.body if isinstance(n, ast.FunctionDef) and n.name in want])
    ns = dict(np=np, Rig=rp.Rig)
    exec(msg._compile_from(os.path.join(shim.REFERENCE_ROOT, "data_proc", "gen_skin_data.py"), funcs(("get_bones",))), ns)
    exec(msg._compile_from(os.path.join(shim.REFERENCE_ROOT, "evaluate", "joint2rig.py"),
                           funcs(("add_duplicate_joints", "mapping_bone_index", "assemble_skel_skin", "remove_dup_joints"))), ns)
    return rp, ns


def reference_rig(rp, names, hier, pos, root_id):
    rig = rp.Rig()
    rig.pos = np.array(pos)
    rig.hierarchy = np.array(hier)
    rig.names = list(names)
    rig.root_id = int(root_id)
    rig.root_name = names[root_id]
    rig.calc_frames_and_offsets()
    return rig


def random_tree(rng, n, dtype):
    """parents drawn among the joints placed before, then the indices shuffled so that the root is not index 0"""
    parent = [-1] + [int(rng.integers(0, i)) for i in range(1, n)]
    pos = rng.uniform(-0.5, 0.5, (n, 3))
    perm = rng.permutation(n)
    while perm[0] == 0:
        perm = rng.permutation(n)
    hier, out = np.zeros(n, dtype=int), np.zeros((n, 3))
    for i in range(n):
        hier[perm[i]] = perm[parent[i]] if parent[i] >= 0 else -1
        out[perm[i]] = pos[i]
    return [f"joint_{i}" for i in range(n)], hier, out.astype(dtype), int(perm[0])


def degenerate_rigs(rng):
    p = lambda *rows: np.array(rows, dtype=np.float64)
    same = [0.3, 0.1, 0.0]
    cases = {}
    # the root's two children share a position; both go on
    cases["twins"] = (["r", "a", "b", "a2", "b2"], np.array([-1, 0, 0, 1, 2]), p([0, 0, 0], same, same, [0.5, 0.3, 0.1], [0.4, -0.2, 0.2]), 0, True)
    # a chain whose leaf lies at its parent's position, beside a branch
    cases["leaf_on_parent"] = (["r", "a", "b", "c", "d"], np.array([-1, 0, 1, 2, 0]),
                               p([0, 0, 0], [0.2, 0.1, 0.0], [0.4, 0.2, 0.1], [0.4, 0.2, 0.1], [-0.3, 0.1, 0.2]), 0, True)
    cases["coincident"] = (["r", "a", "b", "c", "d"], np.array([-1, 0, 0, 1, 1]), p(*([[0.1, 0.2, 0.3]] * 5)), 0, True)
    # a two-child parent with one child on it: a zero-length bone
    cases["child_on_parent"] = (["r", "a", "b", "c", "d"], np.array([-1, 0, 1, 1, 2]),
                                p([0, 0, 0], [0.2, 0.1, 0.0], [0.2, 0.1, 0.0], [0.5, 0.2, 0.1], [0.1, 0.4, 0.3]), 0, False)
    inner = []
    while not inner:                                                          # a joint below the root with exactly one child
        names, hier, pos, root = random_tree(rng, 9, "float64")
        inner = [j for j in range(9) if j != root and np.sum(hier == j) == 1]
    names[inner[0]] = "x_dup_0"
    cases["named_dup"] = (names, hier, pos, root, True)
    return cases


def make_weights(rng, V, nb):
    w = np.zeros((V, nb))
    for v in range(V):
        k = int(rng.integers(1, min(5, nb) + 1))
        idx = rng.choice(nb, k, replace=False)
        w[v, idx] = rng.uniform(0.05, 1.0, k)
    w = w / (w.sum(axis=1, keepdims=True) + 1e-10)
    for v in range(V):                                                        # the special values, written over entries of most rows
        if V == 1 or v % 3 != 2:
            for s in rng.choice(len(SPECIALS), int(rng.integers(1, 3)), replace=False):
                w[v, int(rng.integers(0, nb))] = SPECIALS[s]
    return w


def gap_ok(old, new):
    d = np.sort(ro.bone_distances(old, new), axis=1)
    if d.shape[1] < 2:
        return True
    return bool(np.all((d[:, 0] == d[:, 1]) | (d[:, 1] - d[:, 0] > GAP)))


def run_case(rp, ns, rng, names, hier, pos, root_id, V):
    skel = reference_rig(rp, names, hier, pos, root_id)
    bones_old, _, _ = ns["get_bones"](skel)
    w = make_weights(rng, V, len(bones_old))
    dup = ns["assemble_skel_skin"](skel, w)
    bones_new, names_new, _ = ns["get_bones"](dup)
    if not gap_ok(bones_old, bones_new):
        return None
    bone_map = ns["mapping_bone_index"](bones_old, bones_new)
    target = np.array([dup.names.index(names_new[bone_map[i]][0]) for i in range(len(bones_old))], dtype=np.int64)
    dup_arrs = dict(dup_hier=np.array(dup.hierarchy), dup_pos=np.array(dup.pos), dup_skins=np.array(dup.skins))     # before remove mutates
    dup_names = list(dup.names)
    final = ns["remove_dup_joints"](dup)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "0_rig.txt")
        final.save(path)
        txt = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
        back = rp.Rig(path)
        assert back.names == final.names and np.array_equal(back.hierarchy, final.hierarchy)
    nv = ro.naive((list(names), np.asarray(hier), skel.pos, root_id), list(final.names), w)
    naive_rows = int(np.sum(np.any(nv != final.skins, axis=1)))
    meta = dict(names=list(names), dup_names=dup_names, fin_names=list(final.names), root_id=int(root_id), V=int(V), naive_rows=naive_rows,
                dtype=str(np.asarray(pos).dtype))
    # pos: what the rig is made from (one forward pass follows, as after predict_skeleton or a file load); skel_pos: what that pass leaves
    arrs = dict(pos=np.asarray(pos), skel_pos=np.asarray(skel.pos), hier=np.asarray(hier), weights=w, new_of_bone=target,
                fin_hier=np.array(final.hierarchy), fin_pos=np.array(final.pos), fin_skins=np.array(final.skins), rig_txt=txt, **dup_arrs)
    assert arrs["skel_pos"].dtype == arrs["pos"].dtype == arrs["dup_pos"].dtype == arrs["fin_pos"].dtype
    return meta, arrs


def main():
    rp, ns = reference()
    rng = np.random.default_rng(20261018)
    metas, arrs = [], {}
    for J, dtype, V in TREES:
        for _ in range(50):
            got = run_case(rp, ns, rng, *random_tree(rng, J, dtype), V)
            if got is not None and got[0]["naive_rows"] == 0:
                break
        else:
            raise SystemExit(f"no admissible tree of {J} joints")
        got[0]["name"] = f"tree_{J}_{dtype}"
        metas.append(got[0])
        arrs.update({f"c{len(metas) - 1}_{k}": v for k, v in got[1].items()})
    msg.save("rig_assemble_trees", dict(cases=metas, gap=GAP), **arrs)
    metas, arrs = [], {}
    for name, (names, hier, pos, root, differs) in degenerate_rigs(rng).items():
        got = run_case(rp, ns, rng, names, hier, pos, root, V_DEGENERATE)
        assert got is not None, name
        assert (got[0]["naive_rows"] > 0) == differs, (name, got[0]["naive_rows"])
        got[0]["name"], got[0]["naive_differs"] = name, differs
        print(f"  {name}: the naive sum is wrong on {got[0]['naive_rows']} of {V_DEGENERATE} rows")
        metas.append(got[0])
        arrs.update({f"c{len(metas) - 1}_{k}": v for k, v in got[1].items()})
    msg.save("rig_assemble_degenerate", dict(cases=metas, gap=GAP), **arrs)


if __name__ == "__main__":
    main()
