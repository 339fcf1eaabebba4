"""Generated cases for the rig assembly (csrc/rig_assemble.hip, morig_amd/rigging.py) at the sizes its kernels branch on, their oracle
results (tests/rigging_oracle.py), hand-made CSR tables for the op layer, and the run / compare functions that
tests/test_rigging_cases.py (CPU, on tests/rigging_emulate.py) and tests/test_rigging_differential.py (device) share. Not a test file;
nothing of the reference, no GPU, no golden file: every rig and weight matrix comes from ``np.random.default_rng(seed)``.

What a size is for:
  rig_entries_kernel    one wave per vertex walks its row in chunks of 64 columns under a ballot: J = 63, 64, 65, 128, 129 and trees
                        whose duplicated rig has more than 192 joints (four chunks); rows that are all zero; 4 vertices per workgroup
                        (V = 1, 3, 4, 5, 257)
  rig_assemble_kernel   one thread per (vertex, output joint) of the [N, max J] block: joints past a mesh's own J, segments without
                        bones, joints without segments, the strict `w > 1e-5`, MORIG_RIG_RAW, table entries that must be clamped

A chain has exactly J joints and no duplicate; a random tree (parents drawn from the previous four joints) has many. Every rig meets
the condition of the recorded fixtures (tests/test_rigging_oracle.py): for each old bone the nearest and the second-nearest new bone
are bitwise equal or more than GAP apart. The bar is bit equality throughout (``same_bits``: NaNs in the same places, every other
value with the same bits, so -0.0 is not 0.0)."""
import functools

import numpy as np
import torch

import rigging_oracle as ro
from morig_amd import formats, rigging, tracking
from test_rigging_oracle import GAP

MIN_W = 1e-5
BELOW, ABOVE = float(np.nextafter(MIN_W, 0.0)), float(np.nextafter(MIN_W, 1.0))
SPECIAL = (MIN_W, BELOW, ABOVE, 3e-6, -0.0, 0.0)
CHUNK = 64


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes())


def check_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert same_bits(got, want), f"{what}: not bit-equal ({got.shape} {got.dtype} against {want.shape} {want.dtype}; " \
                                 f"{int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))) if got.shape == want.shape else '?'} values differ)"


# ====================================================================================================================== rigs
def _rig(kind, J, dtype, rng):
    hier = np.array([-1] + [(j - 1) if kind == "chain" else int(rng.integers(max(0, j - 4), j)) for j in range(1, J)])
    pos = rng.uniform(-0.5, 0.5, size=(J, 3)).astype(dtype)
    return [f"j{i}" for i in range(J)], hier, pos, 0


def _weights(rng, V, n_bones):
    w = rng.random((V, n_bones))
    w[rng.random((V, n_bones)) < 0.5] = 0.0
    at = rng.integers(0, V * n_bones, size=min(V * n_bones, 4 * len(SPECIAL)))
    w.reshape(-1)[at] = np.resize(np.array(SPECIAL), len(at))
    w[0] = 0.25 + 0.5 * rng.random(n_bones)                                                   # every joint a bone writes to is non-zero in this row
    if V >= 3:
        w[-1] = np.resize(np.array([0.0, BELOW, 3e-6, -0.0, MIN_W]), n_bones)                    # nothing above the threshold: an all-zero row
    return w


SPECS = [("chain", 2, 1, "float64"), ("chain", 63, 3, "float32"), ("chain", 64, 4, "float64"), ("chain", 65, 5, "float32"),
         ("chain", 128, 257, "float64"), ("chain", 129, 3, "float32"), ("tree", 40, 5, "float64"), ("tree", 70, 257, "float32"),
         ("tree", 130, 4, "float64")]


@functools.lru_cache(maxsize=None)
def cases():
    """the nine rigs with their weights and the oracle's results (``want``: rigging_oracle.assemble_rig)"""
    out = []
    for k, (kind, J, V, dtype) in enumerate(SPECS):
        rng = np.random.default_rng(4000 + k)
        names, hier, pos, root = _rig(kind, J, dtype, rng)
        rig = (names, hier, ro.rebuild(hier, pos, root), root)                                 # as the pipeline holds it: after one forward pass
        n_bones = len(ro.bones(*rig)[0])
        w = _weights(rng, V, n_bones)
        out.append(dict(name=f"{kind}{J}_V{V}_{dtype}", kind=kind, J=J, V=V, dtype=dtype, names=names, hier=hier, pos=pos, rig=rig,
                        weights=w, n_bones=n_bones, want=ro.assemble_rig(rig, w)))
    return out


def nearest_bone_condition(c):
    """the fixture condition: per old bone, nearest and second-nearest new bone bitwise equal or more than GAP apart"""
    old, _ = ro.bones(*c["rig"])
    new, _ = ro.bones(*c["want"]["dup"])
    d = np.sort(ro.bone_distances(old, new), axis=1)
    return d.shape[1] == 1 or bool(np.all((d[:, 0] == d[:, 1]) | (d[:, 1] - d[:, 0] > GAP)))


def skeleton(c):
    return formats.Rig.from_arrays(c["pos"], c["hier"], 0, c["names"])


def wanted(c, keep):
    """-> (names, hierarchy, pos, skins) of the oracle for keep_duplicates = ``keep``"""
    w = c["want"]
    names, hier, pos, _ = w["dup"] if keep else w["final"]
    return names, hier, pos, (w["dup_skins"] if keep else w["skins"])


def run_batch(cs, dev, keep, weights=None):
    """the cases as ONE ragged batch through rigging.assemble_rigs(entries=True) -> per mesh dict(names, hier, pos, skins, skins_device,
    entries), the [N, max J] block"""
    ws = [torch.from_numpy(c["weights"]).to(dev) for c in cs] if weights is None else weights
    rigs = rigging.assemble_rigs([skeleton(c) for c in cs], ws, keep_duplicates=keep, entries=True, device=dev)
    block = rigs[0].skins_device._base if rigs[0].skins_device._base is not None else rigs[0].skins_device
    per = [dict(names=r.names, hier=np.asarray(r.hierarchy), pos=np.asarray(r.pos), skins=r.skins, skins_device=host(r.skins_device),
                entries=tuple(host(t) for t in r.skin_entries_device)) for r in rigs]
    return per, host(block)


def check_rig(got, c, keep):
    names, hier, pos, skins = wanted(c, keep)
    assert got["names"] == names and np.array_equal(got["hier"], hier), c["name"]
    check_bits(got["pos"], pos, f"{c['name']}: positions")
    check_bits(got["skins"], skins, f"{c['name']}: skins")
    check_bits(got["skins_device"], skins, f"{c['name']}: skins on the device")
    check_entries(got["entries"], skins, c["name"])


def check_entries(got, skins, what):
    """the sparse form against rigging_oracle.entries and tracking.skin_entries of the dense result"""
    vptr, ev, ej, ew = got
    for name, (w_vptr, w_ev, w_ej, w_ew) in (("oracle", ro.entries(skins)), ("skin_entries", tracking.skin_entries(skins))):
        assert vptr.dtype == np.int32 and np.array_equal(vptr, w_vptr), f"{what}: entry offsets ({name})"
        assert np.array_equal(ev, w_ev) and np.array_equal(ej, w_ej), f"{what}: an entry in another slot ({name})"
        check_bits(ew, np.asarray(w_ew, dtype=np.float64), f"{what}: entry weights ({name})")


def check_block(block, cs, per):
    """[N, max J]: every mesh's rows hold its skins and zeros past its J"""
    assert block.shape == (sum(c["V"] for c in cs), max(len(p["names"]) for p in per))
    r = 0
    for c, p in zip(cs, per):
        j = len(p["names"])
        check_bits(block[r:r + c["V"], :j], p["skins"], f"{c['name']}: its part of the block")
        assert not block[r:r + c["V"], j:].any() and not np.signbit(block[r:r + c["V"], j:]).any(), f"{c['name']}: not zero past its joints"
        r += c["V"]


# ====================================================================================================================== tables
def _csr(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def table_case():
    """Two meshes with hand-made tables. Mesh 0 (4 vertices, 8 joints, 12 bone columns):
      joint 0  no segment                      joint 4  one segment of 2 bones
      joint 1  one segment without bones       joint 5  one segment of 7 bones
      joint 2  an empty segment, then one bone joint 6  three segments: 1 bone, none, 2 bones
      joint 3  one segment of 1 bone           joint 7  one segment whose last bone holds NaN / -0.0 / 1e-7 in rows 0 / 1 / 2
    Rows 0, 1, 2 hold ABOVE / exactly / BELOW 1e-5 in the LAST bone of the 1-, 2- and 7-bone segments; row 3 is ordinary.
    Mesh 1 (3 vertices, 3 joints) is an ordinary neighbour that the clamped variants damage."""
    rng = np.random.default_rng(4100)
    segs0 = [[], [[]], [[], [0]], [[1]], [[2, 3]], [[4, 5, 6, 7, 8, 9, 10]], [[0], [], [3, 11]], [[1, 11]]]
    segs1 = [[[0, 2]], [[1]], [[0], [1, 2]]]
    W = 0.1 + rng.random((7, 12))
    for v, last in enumerate((ABOVE, MIN_W, BELOW)):
        W[v, [1, 3, 10]] = last
    W[0, 11], W[1, 11], W[2, 11] = np.nan, -0.0, 1e-7
    W[4:, 3:] = 0.0                                                                           # mesh 1 has 3 bone columns
    joints = [segs0, segs1]
    flat_segs = [s for segs in joints for j in segs for s in j]
    tables = dict(vtx_ptr=np.array([0, 4, 7]), joint_ptr=_csr(joints), seg_ptr=_csr([j for segs in joints for j in segs]),
                  bone_ptr=_csr(flat_segs), bones=np.array([b for s in flat_segs for b in s], dtype=np.int64))
    return dict(W=W, tables=tables, ld_out=8, n_cols=12)


def walk_tables(W, t, ld_out, raw):
    """include/morig_hip.h's rule for morig_rig_assemble with its clamps, one (vertex, joint) at a time: an entry that leaves its array
    is skipped, a joint_ptr segment past the joints and a row no mesh names give zeros"""
    vp, jp, sp, bp, bn = (np.asarray(t[k]) for k in ("vtx_ptr", "joint_ptr", "seg_ptr", "bone_ptr", "bones"))
    n_joints, n_segs, n_bones, n_cols = len(sp) - 1, len(bp) - 1, len(bn), W.shape[1]
    out = np.zeros((W.shape[0], ld_out))
    for v in range(W.shape[0]):
        m = max(int(np.searchsorted(vp[:-1], v, side="right")) - 1, 0)
        if not vp[m] <= v < vp[m + 1]:
            continue
        j0, j1 = jp[m], jp[m + 1]
        if j0 < 0 or j1 > n_joints:
            continue
        for j in range(min(ld_out, j1 - j0)):
            total = None
            for s in range(max(sp[j0 + j], 0), min(sp[j0 + j + 1], n_segs)):
                val = 0.0
                for k in range(max(bp[s], 0), min(bp[s + 1], n_bones)):
                    if 0 <= bn[k] < n_cols and (raw or W[v, bn[k]] > MIN_W):
                        val = W[v, bn[k]]
                total = val if total is None else total + val
            out[v, j] = 0.0 if total is None else total
    return out


def clamped_variants():
    """tables with ONE entry that must be clamped or skipped; each is bounded by the kernel before any access it would guide
    (csrc/rig_assemble.hip: the mesh, joint, segment and bone-range tests of rig_assemble_kernel, and `c < 0 || c >= n_cols`)
    -> (name, tables, rows whose result must equal the clean run's)"""
    t = table_case()["tables"]
    n = len(t["bones"])
    put = lambda key, at, value: {**t, key: np.concatenate([t[key][:at], [value], t[key][at + 1:]]) if at != -1 else np.concatenate([t[key][:-1], [value]])}
    mesh0, everything = list(range(4)), list(range(7))
    return [("bone_minus_one", put("bones", n - 1, -1), mesh0), ("bone_at_n_cols", put("bones", n - 4, 12), mesh0),
            ("seg_ptr_end_past", put("seg_ptr", -1, t["seg_ptr"][-1] + 3), everything),
            ("bone_ptr_end_past", put("bone_ptr", -1, t["bone_ptr"][-1] + 2), everything),
            ("joint_ptr_past", put("joint_ptr", -1, t["joint_ptr"][-1] + 2), mesh0),
            ("rows_unnamed", {**t, "vtx_ptr": np.array([1, 4, 6])}, [1, 2, 3, 4, 5])]


def run_tables(ops, W, t, ld_out, raw, dev):
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)
    return host(ops.rig_assemble(torch.from_numpy(np.ascontiguousarray(W)).to(dev), i32(t["vtx_ptr"]), i32(t["joint_ptr"]), i32(t["seg_ptr"]),
                                 i32(t["bone_ptr"]), i32(t["bones"]), ld_out, raw))
