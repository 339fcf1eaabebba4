"""Generated cases for the IK solver (csrc/track.hip, ``ik_solve_kernel``) at the sizes the kernel branches on, their float64 oracle
results (tests/tracking_oracle.py), the float32 twin's deviations the bounds are made of, and the compare functions that
tests/test_track_cases.py (CPU) and tests/test_tracking_differential.py (device) share. Not a test file.

Every input comes from a seed: ``np.random.default_rng([TAG, seed, attempt])``, drawn again (at most 50 attempts) until the ORACLE ALONE
confirms the case's conditions, so nothing is excluded afterwards. Rigs, skins and targets are built the way
tools/make_tracking_golden.py builds them: joints in the unit box, rest frames of up to 0.3 rad, 1 to 4 influences per vertex unless a
case says otherwise, weights rounded to 4 decimals, the target the mesh posed by angles of up to 0.4 rad plus 2e-3 noise.

Bounds: per family and quantity the MAXIMUM over the family's cases of the deviation of the float32 twin (``tk.solve(dtype=float32)``)
from the float64 oracle, times FACTOR, floored at 2^-23, positions capped at 1e-5 -- the convention of tests/test_gpu_tracking.py with
the reference's arithmetic restated by the twin and the deviation taken per family, because a single generated case lands on
accidentally tiny deviations. The two families are the cases of 1 to 3 iterations and those of 25 or more: rounding differences are fed
back through the optimiser, so the deviation grows with the iteration count and one maximum over both would be the long cases' alone.
The deepest tree and the rigs with about as many joints as vertices (a chain of 65, a binary tree of 255, 256 joints on 200 vertices, 300
on 600: a joint may own a single entry or none) run at most three iterations at the small learning rate: Adam's first steps are
lr * g / (|g| + 1e-8), a sign function that turns the float32 rounding of a tiny gradient entry into a step of the order of lr, in the
twin as on the device (1e-5 in the angles at lr = 5e-2, which would then be the bound of every short case), and lr * pi = 0.16 on 25
iterations of a 64-deep chain is chaos in any arithmetic. The star of 300 leaves keeps the large learning rate.
"""
import functools
import zlib

import numpy as np

import tracking_oracle as tk
from morig_amd import native, tracking

TAG = 0x74726B
ATTEMPTS = 50
THRD = 0.3
VIS_MARGIN = 1e-6
LOSS_MIN, GRAD_MIN = 1e-7, 1e-7                            # the last iteration's float64 loss / largest gradient entry: clear of zero
FACTOR, FLOOR, CAP = 10.0, 2.0 ** -23, 1e-5
LDS_LIMIT, LDS_STATIC = 160 * 1024, 512                    # a CU's LDS; what the kernel declares besides its dynamic LDS
LDS_JOINTS = 30
QUANTITIES = ("angles", "positions", "loss", "gradient")


def lds_bytes(J, V):
    """the dynamic LDS of a launch whose largest problem has J joints and V vertices, from the library (a host function)"""
    return int(native.load_library().morig_ik_solve_lds_bytes(J, V))


@functools.lru_cache(maxsize=None)
def lds_sizes():
    """-> dict(under, over: the last V at or under 64 KiB of dynamic LDS on 1 024 threads at 30 joints and the first above it;
    exact: (J, V) whose dynamic LDS is 64 KiB to the byte, if 29 joints allow it; largest: the largest V at 30 joints for which
    lds + 512 bytes fit in 160 KiB)"""
    def last_fitting(J, limit, extra):
        lo, hi = 513, 1 << 16
        assert lds_bytes(J, lo) + extra <= limit < lds_bytes(J, hi) + extra
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if lds_bytes(J, mid) + extra <= limit else (lo, mid)
        return lo
    under = last_fitting(LDS_JOINTS, 64 * 1024, 0)
    exact = [(J, last_fitting(J, 64 * 1024, 0)) for J in (29, 28, 31)]
    exact = [jv for jv in exact if lds_bytes(*jv) == 64 * 1024]
    return dict(under=under, over=under + 1, exact=exact[0] if exact else None, largest=last_fitting(LDS_JOINTS, LDS_LIMIT, LDS_STATIC))


# ------------------------------------------------------------------------------------------------------------------- rigs
def make_parent(kind, J, root, rng):
    parent = np.full(J, -1, dtype=np.int64)
    others = [j for j in range(J) if j != root]
    if kind == "chain":
        prev = root
        for j in others:
            parent[j], prev = prev, j
    elif kind == "star":
        parent[others] = root
    elif kind == "binary":                                                      # heap order: the root, then the others ascending
        label = [root] + others
        for h in range(1, J):
            parent[label[h]] = label[(h - 1) // 2]
    else:
        placed = [root]
        for j in rng.permutation(others):
            parent[j] = placed[int(rng.integers(len(placed)))]
            placed.append(int(j))
    return parent


def rest_pose(pos, L0, parent, root):
    """rest frames and the offsets that put the joints at ``pos`` under them -> (G0, offsets)"""
    order = tk.bfs(parent, root)[0]
    G0, off = np.zeros_like(L0), np.zeros_like(pos)
    G0[root], off[root] = L0[root], pos[root]
    for c in order[1:]:
        p = int(parent[c])
        G0[c] = G0[p] @ L0[c]
        off[c] = G0[p].T @ (pos[c] - pos[p])
    return G0, off


def subtree_has_entries(parent, ent_j):
    """[J] bool: the joint or one of its descendants owns a skin entry (the others have a data gradient of exactly zero)"""
    J = len(parent)
    has = np.zeros(J, dtype=bool)
    has[np.unique(ent_j)] = True
    for j in np.nonzero(has)[0]:
        p = int(parent[j])
        while p >= 0 and not has[p]:
            has[p] = True
            p = int(parent[p])
    return has


# ------------------------------------------------------------------------------------------------------------------- skins
def skin_random(rng, V, J, spec):
    carriers = np.array([j for j in range(J) if j not in spec.get("silent", ())])
    return [np.sort(rng.choice(carriers, size=int(rng.integers(1, min(4, len(carriers)) + 1)), replace=False)) for _ in range(V)]


def skin_joint_counts(rng, V, J, spec):
    """single-influence vertices dealt so that the joints of ``counts`` own exactly that many entries; the other vertices go to the
    remaining joints with one or two influences"""
    counts = spec["counts"]
    rest = np.array([j for j in range(J) if j not in counts])
    owners = [np.array([j]) for j, n in counts.items() for _ in range(n)]
    assert len(owners) < V and len(rest) >= 2
    owners += [np.sort(rng.choice(rest, size=int(rng.integers(1, 3)), replace=False)) for _ in range(V - len(owners))]
    return [owners[i] for i in rng.permutation(V)]


def skin_vertex_counts(rng, V, J, spec):
    cycle = spec["per_vertex"]
    return [np.sort(rng.choice(J, size=cycle[v % len(cycle)], replace=False)) for v in range(V)]


def skin_one_joint(rng, V, J, spec):
    return [np.array([spec["joint"]])] * V


SKINS = dict(random=skin_random, joint_counts=skin_joint_counts, vertex_counts=skin_vertex_counts, one_joint=skin_one_joint)


# ------------------------------------------------------------------------------------------------------------------- the cases
def _c(J, V, tree="tree", root="first", iters=2, lr=5e-2, w_invis=0.0, vis="mixed", skin="random", **kw):
    return dict(J=J, V=V, tree=tree, root=root, iters=iters, lr=lr, w_invis=w_invis, vis=vis, skin=skin, **kw)


ENTRY_COUNTS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 129}


def specs():
    s = lds_sizes()
    out = {
        # 256 threads (V <= 512)
        "v1_j1": _c(1, 1, "chain", iters=1, vis="all_visible"),
        "v64_j2": _c(2, 64, "chain", "last", iters=2, lr=1e-3),
        "v255_j4_all_visible": _c(4, 255, iters=3, lr=1e-3, vis="all_visible"),
        "v256_j5_root_last": _c(5, 256, root="last", iters=25),
        "v257_j16_root_mid_w_invis": _c(16, 257, root="mid", iters=25, w_invis=0.25, silent=(3, 11)),
        "v511_j17": _c(17, 511, iters=3),
        "v512_j64": _c(64, 512, iters=2, lr=1e-3, w_invis=0.25),
        "chain_depth64": _c(65, 300, "chain", iters=3, lr=1e-3),
        "star300": _c(301, 257, "star", "mid", iters=3),                                    # 300 leaves; 256 threads above 64 KiB
        "v40_j6_binary": _c(6, 40, "binary", iters=2),                                      # the small one of the input-check batches
        "j256_v200": _c(256, 200, iters=2, lr=1e-3),
        "j257_v512": _c(257, 512, root="last", iters=2, lr=1e-3),                           # 256 threads above 64 KiB
        "entries_per_joint_256": _c(8, 512, iters=3, skin="joint_counts", counts=ENTRY_COUNTS),
        "entries_per_vertex": _c(16, 257, root="mid", iters=25, lr=1e-3, skin="vertex_counts", per_vertex=(0, 1, 8, 3)),
        "all_on_one_joint": _c(5, 64, "chain", iters=25, skin="one_joint", joint=2),
        "all_invisible": _c(5, 65, root="mid", iters=25, vis="all_invisible"),
        "on_threshold": _c(5, 64, iters=3, w_invis=0.25, vis="on_threshold"),
        "long_200": _c(8, 300, root="mid", iters=200),
        # 1 024 threads
        "v513_j5": _c(5, 513, root="last", iters=3),
        "v1023_j17": _c(17, 1023, root="mid", iters=25, w_invis=0.25),
        "v1024_j16": _c(16, 1024, iters=3, lr=1e-3),
        "v2049_j65": _c(65, 2049, root="mid", iters=2),
        "binary255": _c(255, 513, "binary", iters=3, lr=1e-3),
        "j300_v600": _c(300, 600, root="last", iters=1, lr=1e-3),
        "entries_per_joint_1024": _c(8, 513, iters=3, lr=1e-3, skin="joint_counts", counts=ENTRY_COUNTS),
        # the LDS boundaries
        "lds_under_64k": _c(LDS_JOINTS, s["under"], iters=2),
        "lds_over_64k": _c(LDS_JOINTS, s["over"], root="mid", iters=2, lr=1e-3),
        "lds_largest": _c(LDS_JOINTS, s["largest"], iters=2),
    }
    if s["exact"]:
        out["lds_exactly_64k"] = _c(s["exact"][0], s["exact"][1], iters=1)
    return out


SPECS = specs()
NAMES = tuple(SPECS)
FAMILIES = dict(short=tuple(n for n in NAMES if SPECS[n]["iters"] <= 3), long=tuple(n for n in NAMES if SPECS[n]["iters"] >= 25))
LDS_CASES = tuple(n for n in NAMES if n.startswith("lds_")) + ("star300", "j257_v512")
SMALL = tuple(n for n in NAMES if SPECS[n]["V"] <= 512)
# one launch of the 256-thread cases; the same small cases next to neighbours of up to 2 049 vertices, so on 1 024 threads; the LDS
# giants with two small cases. Every case is in a batch; ``iter_time`` differs inside each.
BATCHES = dict(threads256=SMALL,
               threads1024=SMALL + tuple(n for n in NAMES if 512 < SPECS[n]["V"] <= 2049),
               lds=tuple(n for n in NAMES if n.startswith("lds_")) + ("v1_j1", "long_200"))


def family_of(name):
    return "short" if name in FAMILIES["short"] else "long"


def root_of(spec):
    return dict(first=0, last=spec["J"] - 1, mid=spec["J"] // 2)[spec["root"]]


def draw(spec, rng):
    J, V, root = spec["J"], spec["V"], root_of(spec)
    parent = make_parent(spec["tree"], J, root, rng)
    pos = rng.uniform(-0.4, 0.4, size=(J, 3))
    L0 = tk.euler_matrix(rng.uniform(-0.3, 0.3, size=(J, 3)))                # a posed rig, as the second solve of ik_drag meets one
    G0, off = rest_pose(pos, L0, parent, root)
    vtx = rng.uniform(-0.5, 0.5, size=(V, 3))
    owners = SKINS[spec["skin"]](rng, V, J, spec)
    n = np.array([len(o) for o in owners])
    ent_j = np.concatenate(owners).astype(np.int32) if n.sum() else np.zeros(0, dtype=np.int32)
    ev = np.repeat(np.arange(V), n)
    w = rng.uniform(0.1, 1.0, size=len(ent_j))
    total = np.zeros(V)
    np.add.at(total, ev, w)
    ent_w = np.round(w / total[ev], 4)
    ent_x = np.einsum("eba,eb->ea", G0[ent_j], vtx[ev] - pos[ent_j])         # inverse of [G0 | pos] on the vertex
    prob = dict(locals_in=L0.astype(np.float32), offsets=off.astype(np.float32), parent=parent.astype(np.int32), root=root,
                vptr=np.concatenate([[0], np.cumsum(n)]).astype(np.int32), ent_j=ent_j, ent_w=ent_w.astype(np.float32),
                ent_x=ent_x.astype(np.float32))
    _, G, P = tk.forward(rng.uniform(-0.4, 0.4, size=(J, 3)), rng.uniform(-0.05, 0.05, size=3), prob)
    target = tk.skin(G, P, prob)
    target[n == 0] = vtx[n == 0]                                             # a vertex nobody moves still has somewhere to be
    prob["constraints"] = (target + rng.normal(0, 2e-3, size=target.shape)).astype(np.float32)
    lo, hi = dict(mixed=(0.0, 1.0), on_threshold=(0.0, 1.0), all_visible=(0.5, 1.0), all_invisible=(0.0, 0.25))[spec["vis"]]
    prob["vismask"] = rng.uniform(lo, hi, size=V).astype(np.float32)
    c = dict(prob=prob, iter_time=spec["iters"], lr=spec["lr"], w_invis=spec["w_invis"], thrd=THRD, spec=spec, on_threshold=None, vtx=vtx)
    if spec["vis"] == "on_threshold":
        c["on_threshold"] = int(rng.integers(V))
        prob["vismask"][c["on_threshold"]] = np.float32(THRD)
    c["want"] = oracle(c, np.float64)
    return c


def oracle(c, dtype):
    """the threshold is compared as the float32 the kernel receives, on the float32 mask"""
    return tk.solve(c["prob"], c["iter_time"], c["lr"], c["w_invis"], np.float32(c["thrd"]), dtype=dtype)


def vis_margin(c):
    d = np.abs(c["prob"]["vismask"].astype(np.float64) - np.float64(np.float32(c["thrd"])))
    if c["on_threshold"] is not None:
        d = np.delete(d, c["on_threshold"])
    return float(d.min()) if len(d) else np.inf


def grad_scale(r):
    return max(np.abs(r["g_angles"]).max(), np.abs(r["g_trans"]).max())


def conditions(c):
    """from the float64 oracle alone"""
    if vis_margin(c) < VIS_MARGIN:
        return False
    if c["spec"]["vis"] == "all_invisible":
        return not (c["prob"]["vismask"] > np.float32(c["thrd"])).any()
    return c["want"]["loss"] >= LOSS_MIN and grad_scale(c["want"]) >= GRAD_MIN


@functools.lru_cache(maxsize=None)
def case(name):
    seed = zlib.crc32(name.encode())                                         # a case keeps its inputs when the list changes
    for attempt in range(ATTEMPTS):
        c = draw(SPECS[name], np.random.default_rng([TAG, seed, attempt]))
        if conditions(c):
            c["attempts"], c["name"] = attempt + 1, name
            return c
    raise AssertionError(f"{name}: no draw met the conditions")


def problem(name):
    c, p = case(name), case(name)["prob"]
    return tracking.make_problem(p["locals_in"], p["offsets"], p["parent"], p["root"], p["vptr"], p["ent_j"], p["ent_w"], p["ent_x"],
                                 p["constraints"], p["vismask"], c["iter_time"], c["lr"], c["w_invis"], c["thrd"])


# ------------------------------------------------------------------------------------------------------------------- deviations and bounds
def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want)) if want != 0 else abs(float(got))


def deviation_of(got, want):
    """a result (the twin's, the device's, the reference's) against the float64 oracle -> {quantity: figure}. ``got`` may name the
    gradients grad_* (the device) or g_* (the oracles)"""
    ga, gt = (got["grad_angles"], got["grad_trans"]) if "grad_angles" in got else (got["g_angles"], got["g_trans"])
    scale = grad_scale(want)
    g = max(np.abs(ga - want["g_angles"]).max(), np.abs(gt - want["g_trans"]).max())
    return dict(angles=float(max(np.abs(got["angles"] - want["angles"]).max(), np.abs(got["trans"] - want["trans"]).max())),
                positions=float(max(np.abs(got[k] - want[k]).max() for k in ("locals", "globals", "jpos"))),
                loss=rel(got["loss"], want["loss"]), gradient=float(g / scale) if scale > 0 else float(g))


@functools.lru_cache(maxsize=None)
def twin_deviation(name):
    c = case(name)
    return deviation_of(oracle(c, np.float32), c["want"])


@functools.lru_cache(maxsize=None)
def deviations(family):
    """the family maxima of the float32 twin's deviations from float64"""
    return {q: max(twin_deviation(n)[q] for n in FAMILIES[family]) for q in QUANTITIES}


def bounds(family):
    b = {q: max(FACTOR * d, FLOOR) for q, d in deviations(family).items()}
    b["positions"] = min(b["positions"], CAP)
    return b


def table(device=None):
    """the family maxima, float32 twin (and the device's figures where given: {name: deviation_of(...)}), both against float64"""
    rows = ["family    quantity   float32 twin  bound" + ("      device" if device else "")]
    for family in FAMILIES:
        for q in QUANTITIES:
            row = f"{family:9s} {q:10s} {deviations(family)[q]:.3e}     {bounds(family)[q]:.3e}"
            if device:
                row += f"  {max(device[n][q] for n in FAMILIES[family] if n in device):.3e}"
            rows.append(row)
    return "\n".join(rows)


def compare(label, name, got):
    """print, then assert: a result against the float64 oracle within the family's bounds; exact zeros where the oracle has them"""
    c = case(name)
    dev, b = deviation_of(got, c["want"]), bounds(family_of(name))
    print(f"\n{label} {name}: " + ", ".join(f"{q} {dev[q]:.3e} (bound {b[q]:.3e})" for q in QUANTITIES))
    for q in QUANTITIES:
        assert dev[q] <= b[q], (name, q, dev[q], b[q])
    ga, gt = (got["grad_angles"], got["grad_trans"]) if "grad_angles" in got else (got["g_angles"], got["g_trans"])
    silent = ~subtree_has_entries(c["prob"]["parent"], c["prob"]["ent_j"])
    assert np.all(c["want"]["g_angles"][silent] == 0) and np.all(np.asarray(ga)[silent] == 0)        # quirk (iii): exactly zero
    if c["spec"]["vis"] == "all_invisible":
        assert float(got["loss"]) == 0 and np.all(np.asarray(ga) == 0) and np.all(np.asarray(gt) == 0)
    return dev
