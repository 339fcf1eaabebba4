"""Generated cases for the rig evaluation metrics (csrc/metrics.hip, csrc/assign_core.h, morig_amd/metrics.py) at the sizes the kernels
branch on, their oracle results (tests/metrics_oracle.py, float64 numpy + scipy), the restated summation orders, and the run / compare
functions that tests/test_metrics_cases.py (CPU, on tests/metrics_emulate.py) and tests/test_metrics_differential.py (device) share.
Not a test file; nothing of the reference, no GPU, no golden file: every input comes from ``np.random.default_rng(seed)``.

What a size is for:
  assign_kernel          64 lanes own the columns j = lane, lane + 64, ...: 1 to 4 columns per lane, both orientations, the cost matrix in
                         LDS up to AS_LDS_COST = 6144 entries and in global memory above; ties; empty sides; non-finite joints; bad tables
  joint_scores_kernel    the strict `dist < fs`, 64 lanes striding over the matched pairs
  nearest_kernel         MORIG_NEAREST_TILE = 1024 rows of b per LDS tile, 256 rows of a per workgroup, the walk over a workgroup's meshes
  segment_mean_kernel    256 strided partial sums, then the tree h = 128 ... 1: restated here and held bit for bit
  bone_count / _sample   256 bones / samples per workgroup, half steps (round half to even), zero-length and refused bones
  valid_mean_kernel      one thread per row, 64 rows per workgroup, the valid columns in index order

Bars: everything discrete, bone samples, squared nearest distances, segment / valid means against their restated order and the three
score ratios are compared bit for bit (``same_bits``: NaNs in the same places, every other value with the same 64 bits); a distance is
the square root of a bit-equal number, at most 1 ulp (``ulps``); chamfers and means against the oracle's pairwise np.mean are held to
SUM_TOL = 1e-11, whose premises (at most 4096 terms, each below 4) ``sum_premises`` asserts per case."""
import functools
import types

import numpy as np
import torch

import metrics_oracle as mo
from morig_amd import metrics
from test_metrics_oracle import GAP, MAX_TERM, MAX_TERMS, SUM_TOL

TILE, ROWS_A, LANES, AS_LDS_COST = 1024, 256, 64, 6144
ST_SIZE, ST_PTR, ST_INFEASIBLE = 1, 2, 4
BELOW = lambda x: float(np.nextafter(x, -np.inf))
ABOVE = lambda x: float(np.nextafter(x, np.inf))


def ptr(xs):
    return np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)


def cat(xs, width=3):
    return np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, width) for x in xs], axis=0)


def host(t):
    return t.detach().cpu().numpy()


def chain_rig(pos):
    pos = np.asarray(pos, dtype=np.float64)
    return types.SimpleNamespace(pos=pos, hierarchy=np.arange(-1, len(pos) - 1), root_id=0)


def star_rig(pos):
    """joint 0 is the root, every other joint its child"""
    pos = np.asarray(pos, dtype=np.float64)
    return types.SimpleNamespace(pos=pos, hierarchy=np.array([-1] + [0] * (len(pos) - 1)), root_id=0)


# ====================================================================================================================== comparing
def same_bits(a, b):
    """NaNs in the same places; everywhere else the same bits (so -0.0 is not 0.0)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes())


def ulps(a, b):
    """the largest distance in units of the last place between two float64 arrays with NaNs in the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.isnan(a)
    assert a.shape == b.shape and np.array_equal(na, np.isnan(b)), "NaNs in different places"
    return int(np.abs(a[~na].view(np.int64) - b[~na].view(np.int64)).max(initial=0))


def check_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind != "f":
        want = want.astype(got.dtype)
    assert same_bits(got, want), f"{what}: not bit-equal (first difference at {first_difference(got, want)})"


def first_difference(a, b):
    if a.shape != b.shape:
        return f"shapes {a.shape} / {b.shape}"
    bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).reshape(-1)) if a.dtype.kind == "f" else np.flatnonzero((a != b).reshape(-1))
    return None if len(bad) == 0 else (int(bad[0]), a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


def check_matching(got, want, what):
    """(row, col, dist) of one mesh pair for pair; the distances, square roots of bit-equal numbers, within 1 ulp -> the ulps seen"""
    row, col, dist = got
    assert np.array_equal(row, want[0]) and np.array_equal(col, want[1]), f"{what}: another matching than the oracle's"
    off = ulps(dist, want[2])
    assert off <= 1, f"{what}: matched distances {off} ulp from the oracle's"
    return off


def check_valid_matching(got, d, total, what):
    """a tie case: rows ascending, distinct columns inside the matrix, the stored distances, the optimal total with =="""
    row, col, dist = got
    assert d.shape[0] <= d.shape[1] and np.array_equal(row, np.arange(d.shape[0])), what
    assert len(set(col.tolist())) == len(col) and col.min() >= 0 and col.max() < d.shape[1] and row.min() >= 0 and row.max() < d.shape[0], what
    assert np.array_equal(dist, d[row, col]) and dist.sum() == total, f"{what}: total {dist.sum()} against {total}"


def check_hits(got, want, what):
    assert np.array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)), f"{what}: hits {np.asarray(got).tolist()} against {np.asarray(want).tolist()}"


def check_sum(got, want, what):
    err = float(np.nanmax(np.abs(np.asarray(got) - np.asarray(want)), initial=0.0))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and err <= SUM_TOL, f"{what}: {err:.2e} above SUM_TOL"
    return err


def sum_premises(n_terms, largest):
    """SUM_TOL was derived for a mean of at most 4096 terms, each below 4 (tests/test_metrics_oracle.py)"""
    assert n_terms <= MAX_TERMS and largest < MAX_TERM, (n_terms, largest)


# ====================================================================================================================== matching
LANE_SHAPES = [(1, 64), (1, 256), (2, 129), (3, 63), (63, 65), (64, 64), (17, 193), (193, 17), (100, 130), (128, 128), (128, 129),
               (129, 128), (128, 256), (256, 128), (256, 1)]
LDS_SHAPES = [(78, 78), (64, 96), (96, 64), (79, 79), (49, 126)]                          # (n_gt, n_pred)


def _assign_case(k, shape, family):
    n_gt, n_pred = shape
    rng = np.random.default_rng(1000 + k)
    gt, pred = rng.random((n_gt, 3)), rng.random((n_pred, 3))
    d = mo.dist_matrix(pred, gt)
    row, col = mo.linear_sum_assignment(d)
    return dict(name=f"{family}_{n_gt}x{n_pred}", family=family, n_gt=n_gt, n_pred=n_pred, gt=gt, pred=pred, d=d, row=row, col=col,
                dist=d[row, col], cols_per_lane=-(-max(shape) // LANES), in_lds=n_gt * n_pred <= AS_LDS_COST, transposed=n_pred < n_gt)


@functools.lru_cache(maxsize=None)
def assign_cases():
    """the columns-per-lane and the LDS / global families: 20 meshes, seeds 1000 + k in this order"""
    shapes = [(s, "lanes") for s in LANE_SHAPES] + [(s, "lds") for s in LDS_SHAPES]
    return [_assign_case(k, s, f) for k, (s, f) in enumerate(shapes)]


def _line_tie(seed, n_gt, n_pred, quad, span):
    """joints on the integer lattice along one Pythagorean quadruple (x, y, z; n): every distance is n * |a - b|, an integer, exact in
    float64 under any order of the sum; the ground-truth joints come in duplicated pairs, so the optimum is not unique"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, span, size=n_gt // 2)
    a = np.concatenate([a, a, rng.integers(0, span, size=n_gt - 2 * (n_gt // 2))])           # every value twice
    b = rng.integers(0, span, size=n_pred)
    step = np.array(quad[:3], dtype=np.float64)
    gt, pred = a[:, None] * step[None, :], b[:, None] * step[None, :]
    d = mo.dist_matrix(pred, gt)
    row, col = mo.linear_sum_assignment(d)
    return dict(name=f"tie_{n_gt}x{n_pred}", n_gt=n_gt, n_pred=n_pred, gt=gt, pred=pred, d=d, total=d[row, col].sum(), norm=quad[3], a=a, b=b)


@functools.lru_cache(maxsize=None)
def tie_cases():
    return [_line_tie(2001, 6, 8, (1, 2, 2, 3), 12), _line_tie(2002, 70, 70, (2, 3, 6, 7), 40)]


@functools.lru_cache(maxsize=None)
def degenerate_batch():
    """a batch whose first and last meshes have no predictions, n_gt 1 with n_pred 1 inside: (n_gt, n_pred)"""
    rng = np.random.default_rng(2100)
    sizes = [(4, 0), (1, 1), (3, 5), (6, 2), (5, 0)]
    return [dict(n_gt=g, n_pred=p, gt=rng.random((g, 3)), pred=rng.random((p, 3))) for g, p in sizes]


@functools.lru_cache(maxsize=None)
def nonfinite_batch():
    """five meshes of 5 ground-truth joints: a NaN prediction that is not needed (6 predictions), one that is (5), an infinite one (6), a
    NaN ground-truth joint, and a healthy mesh. ``bad``: the column the rule removes; ``want``: mo.match_rule's (status, row, col, dist)"""
    rng = np.random.default_rng(2200)
    out = []
    for name, n_pred, bad, value, bad_gt in (("nan_spare", 6, 2, np.nan, None), ("nan_needed", 5, 3, np.nan, None),
                                             ("inf_spare", 6, 4, np.inf, None), ("nan_gt", 6, None, None, 1), ("healthy", 6, None, None, None)):
        gt, pred = rng.random((5, 3)), rng.random((n_pred, 3))
        if bad is not None:
            pred[bad, 1] = value
        if bad_gt is not None:
            gt[bad_gt, 2] = np.nan
        fs = np.full(5, 10.0)                                                                  # every finite matched pair is a hit
        out.append(dict(name=name, n_gt=5, n_pred=n_pred, gt=gt, pred=pred, fs=fs, bad=bad, bad_gt=bad_gt, want=mo.match_rule(pred, gt)))
    return out


def run_match(meshes, dev, fs=None):
    """the meshes as one batch through metrics.match_joints (and joint_scores with ``fs`` per mesh) -> per-mesh (row, col, dist), status
    [, scores]"""
    pred, gt = cat([m["pred"] for m in meshes]), cat([m["gt"] for m in meshes])
    pp, gp = ptr([m["pred"] for m in meshes]), ptr([m["gt"] for m in meshes])
    m = metrics.match_joints(pred, pp, gt, gp, device=dev)
    row, col, dist, mp = host(m["row_ind"]), host(m["col_ind"]), host(m["dist"]), m["match_ptr_host"]
    assert np.array_equal(np.diff(mp), [min(c["n_gt"], c["n_pred"]) for c in meshes]) and np.array_equal(host(m["match_ptr"]), mp)
    per = [(row[mp[b]:mp[b + 1]], col[mp[b]:mp[b + 1]], dist[mp[b]:mp[b + 1]]) for b in range(len(meshes))]
    if fs is None:
        return per, host(m["status"])
    sc = metrics.joint_scores(m, m["n_pred"], m["n_gt"], np.concatenate(fs), gp, device=dev)
    return per, host(m["status"]), {k: host(v) for k, v in sc.items()}


# ---- bad tables, at the ops layer -------------------------------------------------------------------------------------------------
PREFILL = dict(row=-7, col=-7, dist=777.0, status=-9)


@functools.lru_cache(maxsize=None)
def table_batch():
    """four healthy meshes and the tables morig_assign_joints takes for them. Every variant damages the tables of ONE mesh (the first or
    the last, so that no neighbour's segment moves); the kernel bounds each of these before it addresses anything of the mesh
    (csrc/metrics.hip: the uniform check at the top of assign_kernel, then `c1 - c0 < entries`)."""
    rng = np.random.default_rng(2300)
    sizes = [(5, 6), (7, 4), (3, 3), (6, 9)]
    meshes = [dict(n_gt=g, n_pred=p, gt=rng.random((g, 3)), pred=rng.random((p, 3))) for g, p in sizes]
    pp, gp = ptr([m["pred"] for m in meshes]), ptr([m["gt"] for m in meshes])
    mp = np.concatenate([[0], np.cumsum([min(s) for s in sizes])])
    cp = np.concatenate([[0], np.cumsum([g * p for g, p in sizes])])
    clean = dict(pred_ptr=pp, gt_ptr=gp, match_ptr=mp, cost_off=cp)
    edit = lambda key, at, value: {**clean, key: np.concatenate([clean[key][:at], [value], clean[key][at + 1:]]) if at >= 0 else
                                   np.concatenate([clean[key][:-1], [value]])}
    variants = [("pred_descending", 3, ST_PTR, edit("pred_ptr", -1, pp[-2] - 1)), ("pred_negative", 0, ST_PTR, edit("pred_ptr", 0, -1)),
                ("pred_past_the_array", 3, ST_PTR, edit("pred_ptr", -1, pp[-1] + 1)), ("match_wrong_length", 3, ST_PTR, edit("match_ptr", -1, mp[-1] - 1)),
                ("cost_one_short", 3, ST_SIZE, edit("cost_off", -1, cp[-1] - 1))]
    return meshes, clean, variants


def run_assign_tables(assign, meshes, tables, dev):
    """``assign(pred, pred_ptr, gt, gt_ptr, match_ptr, n_match, cost_off, n_cost, out)`` writes into prefilled outputs, as the C entry
    point does (the device file calls the library, the CPU file the emulation) -> row, col, dist, status (numpy)"""
    _, clean, _ = table_batch()
    n_match, n_cost = int(clean["match_ptr"][-1]), int(clean["cost_off"][-1])
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)
    out = (torch.full((n_match,), PREFILL["row"], dtype=torch.int32, device=dev), torch.full((n_match,), PREFILL["col"], dtype=torch.int32, device=dev),
           torch.full((n_match,), PREFILL["dist"], dtype=torch.float64, device=dev), torch.full((len(meshes),), PREFILL["status"], dtype=torch.int32, device=dev))
    pred, gt = torch.from_numpy(cat([m["pred"] for m in meshes])).to(dev), torch.from_numpy(cat([m["gt"] for m in meshes])).to(dev)
    assign(pred, i32(tables["pred_ptr"]), gt, i32(tables["gt_ptr"]), i32(tables["match_ptr"]), n_match,
           torch.from_numpy(np.asarray(tables["cost_off"]).astype(np.int64)).to(dev), n_cost, out)
    return tuple(host(t) for t in out)


def check_assign_tables(clean_out, got, bad, status, what):
    """the damaged mesh: its status word, and nothing written (ST_PTR) or -1 / NaN (ST_SIZE); every other mesh as in the clean run"""
    _, clean, _ = table_batch()
    mp = clean["match_ptr"]
    for b in range(len(mp) - 1):
        seg = slice(mp[b], mp[b + 1])
        if b != bad:
            assert got[3][b] == clean_out[3][b] == 0, (what, b)
            for k in range(3):
                check_bits(got[k][seg], clean_out[k][seg], f"{what}: mesh {b}")
        elif status == ST_PTR:
            assert got[3][b] == ST_PTR and (got[0][seg] == PREFILL["row"]).all() and (got[1][seg] == PREFILL["col"]).all() and \
                (got[2][seg] == PREFILL["dist"]).all(), f"{what}: something of mesh {b} was written"
        else:
            assert got[3][b] == status and (got[0][seg] == -1).all() and (got[1][seg] == -1).all() and np.isnan(got[2][seg]).all(), what


# ====================================================================================================================== threshold
QUADS = [(0, 3, 4, 5), (2, 3, 6, 7), (1, 4, 8, 9), (2, 6, 9, 11), (2, 10, 11, 15)]


def _fs_for(dist, k):
    """the feature size of pair k: the distance itself, one float64 below, and -- three times of five -- one above"""
    return [dist, BELOW(dist), ABOVE(dist), ABOVE(dist), ABOVE(dist)][k % 5]


@functools.lru_cache(maxsize=None)
def threshold_batch():
    """63, 64 and 65 matched pairs per mesh: ground-truth joints 100 apart on the integer lattice, prediction k displaced by a
    Pythagorean quadruple, so its distance is exactly 5, 7, 9, 11 or 15 and the matching is beyond doubt; three more predictions far off"""
    out = []
    for n in (63, 64, 65):
        gt = np.stack([100.0 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)
        pred = gt + np.array([QUADS[k % 5][:3] for k in range(n)], dtype=np.float64)
        pred = np.concatenate([pred, gt[:3] + np.array([0.0, 5000.0, 0.0])])
        pred = pred[np.random.default_rng(2400 + n).permutation(len(pred))]
        dist = np.array([float(QUADS[k % 5][3]) for k in range(n)])
        fs = np.array([_fs_for(dist[k], k + n) for k in range(n)])
        out.append(dict(name=f"threshold_{n}", n_gt=n, n_pred=n + 3, gt=gt, pred=pred, fs=fs, exact=dist, want=mo.scores(pred, gt, fs)))
    return out


@functools.lru_cache(maxsize=None)
def threshold_handmade():
    """129 matched pairs (more than one mesh of match_joints can hold) as a hand-made matching for joint_scores: rows in a seeded order,
    the same exact distances and feature sizes; two meshes, so that the second starts at an odd offset"""
    rng = np.random.default_rng(2500)
    sizes, n_pred = [129, 66], [140, 66]
    row, dist, fs, hits = [], [], [], []
    for n in sizes:
        r = rng.permutation(n)
        d = np.array([float(QUADS[k % 5][3]) for k in range(n)])
        f = np.zeros(n)
        f[r] = [_fs_for(d[k], k) for k in range(n)]
        row.append(r), dist.append(d), fs.append(f), hits.append(int(np.sum(d < f[r])))
    ratios = np.array([[2 * h / (p + g) for h, p, g in zip(hits, n_pred, sizes)], [h / p for h, p in zip(hits, n_pred)],
                       [h / g for h, g in zip(hits, sizes)]])
    return dict(sizes=sizes, n_pred=n_pred, row=row, dist=dist, fs=fs, hits=hits, ratios=ratios)


def run_handmade_scores(c, dev):
    mp = ptr(c["row"])
    match = dict(row_ind=torch.from_numpy(np.concatenate(c["row"]).astype(np.int32)).to(dev), dist=torch.from_numpy(np.concatenate(c["dist"])).to(dev),
                 match_ptr=torch.from_numpy(mp.astype(np.int32)).to(dev))
    sc = metrics.joint_scores(match, c["n_pred"], c["sizes"], np.concatenate(c["fs"]), mp, device=dev)
    return host(sc["hits"]), np.stack([host(sc[k]) for k in ("iou", "precision", "recall")])


# ====================================================================================================================== nearest
TILE_MESHES = [(1, 2049), (255, 1), (256, 1023), (257, 1024), (513, 1025), (256, 2048)]       # (rows of a, rows of b)


@functools.lru_cache(maxsize=None)
def nearest_tiles():
    """per mesh: b uniform in the unit box; source 0 sits 1e-4 beside the LAST row of b and source 1 (where there is one) beside the
    first, the others are uniform"""
    rng = np.random.default_rng(2600)
    a_sets, b_sets = [], []
    for na, nb in TILE_MESHES:
        b, a = rng.random((nb, 3)), rng.random((na, 3))
        a[0] = b[-1] + 1e-4
        if na > 1:
            a[1] = b[0] + 1e-4
        a_sets.append(a), b_sets.append(b)
    sq = [mo.nearest_sq(a, b) for a, b in zip(a_sets, b_sets)]
    arg = [mo.sqdist(a, b).argmin(axis=1) for a, b in zip(a_sets, b_sets)]
    return dict(a=a_sets, b=b_sets, sq=sq, arg=arg, oneway=np.array([mo.oneway(a, b) for a, b in zip(a_sets, b_sets)]))


WALK_A, WALK_B, WALK_START = [100, 0, 3, 0, 0, 200, 60, 300], [50, 7, 0, 5, 9, 1100, 1, 30], 37


@functools.lru_cache(maxsize=None)
def nearest_walk():
    """eight meshes in one launch behind 37 rows no mesh owns (an a_ptr that starts past row 0, as chamfer_j2b's second list does);
    mesh 2 has sources and no rows in b"""
    rng = np.random.default_rng(2700)
    a_sets, b_sets = [rng.random((n, 3)) for n in WALK_A], [rng.random((n, 3)) for n in WALK_B]
    a = np.concatenate([rng.random((WALK_START, 3))] + a_sets)
    a_ptr = WALK_START + ptr(a_sets)
    want = np.full(len(a), np.nan)
    for m, (x, y) in enumerate(zip(a_sets, b_sets)):
        if len(x) and len(y):
            want[a_ptr[m]:a_ptr[m + 1]] = mo.nearest_sq(x, y)
    return dict(a=a, a_ptr=a_ptr, b=cat(b_sets), b_ptr=ptr(b_sets), want=want, flags=[0, 0, 1, 0, 0, 0, 0, 0])


def workgroup_meshes(a_ptr, n_a):
    """per workgroup of nearest_kernel (256 consecutive rows of a) the meshes m_lo .. m_hi it walks"""
    seg = lambda i: max(int(np.searchsorted(a_ptr[:-1], i, side="right")) - 1, 0)
    return [(seg(first), seg(min(first + ROWS_A - 1, n_a - 1))) for first in range(0, n_a, ROWS_A)]


@functools.lru_cache(maxsize=None)
def nearest_nan():
    """np.min's rule: mesh 0 has a NaN coordinate in source row 3; mesh 1 a NaN row in b (past the first tile); mesh 2 is healthy"""
    rng = np.random.default_rng(2800)
    a_sets, b_sets = [rng.random((n, 3)) for n in (9, 300, 5)], [rng.random((n, 3)) for n in (20, 1030, 7)]
    a_sets[0][3, 0] = np.nan
    b_sets[1][1027, 2] = np.nan
    with np.errstate(invalid="ignore"):
        sq = np.concatenate([mo.nearest_sq(a, b) for a, b in zip(a_sets, b_sets)])
    return dict(a=a_sets, b=b_sets, sq=sq)


def run_nearest(ops, a, a_ptr, b, b_ptr, dev):
    """the op itself (device ptr tensors: the form the chamfers forward) -> squared, rooted, flags"""
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to(dev)
    ta, tb, pa, pb = up(a, np.float64), up(b, np.float64), up(a_ptr, np.int32), up(b_ptr, np.int32)
    sq, flags = ops.nearest_distance(ta, pa, tb, pb, True)
    d, flags2 = ops.nearest_distance(ta, pa, tb, pb, False)
    assert np.array_equal(host(flags), host(flags2))
    return host(sq), host(d), host(flags)


def check_nearest(sq, d, want_sq, what):
    check_bits(sq, want_sq, f"{what}: squared minima")
    with np.errstate(invalid="ignore"):
        off = ulps(d, np.sqrt(want_sq))
    assert off <= 1, f"{what}: distances {off} ulp from the square roots of the oracle's minima"
    return off


# ====================================================================================================================== means
MEAN_SIZES = [0, 1, 2, 255, 256, 257, 511, 4096]


def kernel_order_mean(x):
    """segment_mean_kernel's order: partial t = the sequential sum of x[t::256] from 0.0, then sh[t] += sh[t + h] for h = 128 ... 1"""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return np.nan
    padded = np.zeros(-(-len(x) // 256) * 256)
    padded[:len(x)] = x                                                                        # the values are positive: x + 0.0 is x
    sh = np.zeros(256)
    for r in padded.reshape(-1, 256):
        sh = sh + r
    h = 128
    while h:
        sh[:h] = sh[:h] + sh[h:2 * h]
        h >>= 1
    return sh[0] / np.float64(len(x))


@functools.lru_cache(maxsize=None)
def mean_case():
    rng = np.random.default_rng(2900)
    xs = [rng.uniform(0.0, 4.0, size=n) for n in MEAN_SIZES]
    import math
    return dict(xs=xs, x=np.concatenate(xs), ptr=ptr(xs), order=np.array([kernel_order_mean(x) for x in xs]),
                fsum=np.array([math.fsum(x) / len(x) if len(x) else np.nan for x in xs]))


def run_segment_mean(ops, x, p, dev):
    return host(ops.segment_mean(torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.asarray(p).astype(np.int32)).to(dev)))


def sequential_mean(x, valid):
    s, n = 0.0, 0
    for v, ok in zip(x, valid):
        if ok:
            s, n = s + float(v), n + 1
    return np.float64(s) / np.float64(n) if n else np.nan


@functools.lru_cache(maxsize=None)
def valid_mean_cases():
    """(x [rows, n], valid [n]): all meshes invalid, only the last valid, 1 and 65 meshes; 65 rows pass one workgroup of 64"""
    rng = np.random.default_rng(3000)
    out = []
    for name, rows, n, valid in (("all_invalid", 6, 9, np.zeros(9, int)), ("last_valid", 6, 9, np.eye(9, dtype=int)[8]),
                                 ("one_mesh", 4, 1, np.ones(1, int)), ("65_meshes", 65, 65, (rng.random(65) < 0.7).astype(int))):
        x = rng.uniform(0.0, 1.0, size=(rows, n))
        x[:, valid == 0] = np.nan                                                             # what evaluate_rigs stacks: NaN on the skipped meshes
        out.append(dict(name=name, x=x, valid=valid, want=np.array([sequential_mean(r, valid) for r in x])))
    return out


def run_valid_mean(ops, c, dev):
    return host(ops.valid_mean(torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["valid"].astype(np.int32)).to(dev)))


# ====================================================================================================================== bones
HALF = [1.5, 2.5, 4.5, 5.5, 6.5, 7.5]                                                      # steps of 0.005 that round half to even


def _bone_rigs(rng, n_bones):
    """a chain and a star with ``n_bones`` bones together. The chain walks in steps of about 0.02 and has zero-length bones at its
    start, middle and end; the star has half-step bones along every axis, in both directions"""
    n_star = 19
    n_chain = n_bones - (n_star - 1) + 1
    pos = np.cumsum(rng.normal(scale=0.012, size=(n_chain, 3)), axis=0)
    for at in (1, n_chain // 2, n_chain - 1):
        pos[at] = pos[at - 1]
    arms = [np.eye(3)[ax] * sign * np.float64(h) * mo.STEP for ax in range(3) for sign, hs in ((1.0, HALF[:3]), (-1.0, HALF[3:])) for h in hs]
    star = np.concatenate([[np.zeros(3)], arms])                                               # around the origin: the lengths stay exact
    assert len(star) == n_star
    return [chain_rig(pos), star_rig(star)]


@functools.lru_cache(maxsize=None)
def bone_batches():
    """three batches with 255, 256 and 257 bones in total (bone_count_kernel takes 256 per workgroup)"""
    out = []
    for n_bones in (255, 256, 257):
        rigs = _bone_rigs(np.random.default_rng(3100 + n_bones), n_bones)
        samples = [mo.sample_skel(r) for r in rigs]
        counts = [len(mo.sample_bone(r.pos[p], r.pos[c])) for r in rigs for p, c in mo.bones_of(r)]
        out.append(dict(n_bones=n_bones, rigs=rigs, samples=samples, counts=np.array(counts)))
    return out


@functools.lru_cache(maxsize=None)
def refused_bones():
    """the bone table of a chain of 12 joints with three bones the kernel must refuse: a child index equal to n_joints, a NaN joint
    (it spoils the two bones that touch it) and a bone of length 1e6 (2e8 steps, above MORIG_BONE_MAX_SAMPLES = 2^24)"""
    rng = np.random.default_rng(3200)
    pos = np.cumsum(rng.normal(scale=0.012, size=(12, 3)), axis=0)
    pos[5, 1] = np.nan
    pos[9:] += 1e6
    bones = np.stack([np.arange(11), np.arange(1, 12)], axis=1)
    bones[1, 1] = 12
    refused = [1, 4, 5, 8]
    with np.errstate(invalid="ignore"):
        samples = [mo.sample_bone(pos[p], pos[c]) if k not in refused else np.zeros((0, 3)) for k, (p, c) in enumerate(bones.tolist())]
    return dict(pos=pos, bones=bones, refused=refused, counts=np.array([len(s) for s in samples]), samples=np.concatenate(samples))


def run_bone_ops(ops, pos, bones, dev):
    joints, table = torch.from_numpy(pos).to(dev), torch.from_numpy(bones.astype(np.int32)).to(dev).contiguous()
    counts = ops.bone_sample_counts(joints, table)
    off = torch.zeros(len(bones) + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(counts, 0)
    return host(counts), host(ops.bone_samples(joints, table, off, int(off[-1])))


# ====================================================================================================================== whole
@functools.lru_cache(maxsize=None)
def whole_batch():
    """evaluate_rigs on a batch that mixes the families: a mesh without predictions in the middle, 64 x 64, 3 x 63, 65 x 17, a star.
    Predicted joints are the predicted rig's; feature sizes sit around the matched distances"""
    rng = np.random.default_rng(3300)
    sizes = [(64, 64), (3, 63), (9, 0), (65, 17), (19, 19), (2, 2)]                            # (n_gt, n_pred)
    preds, pred_rigs, gt_rigs, fss = [], [], [], []
    for g, p in sizes:
        walk = lambda n: rng.random(3) * 0.5 + np.cumsum(rng.normal(scale=0.03, size=(n, 3)), axis=0)
        gt = walk(g)
        pred = gt[rng.permutation(g)[:p]] + rng.normal(scale=0.01, size=(p, 3)) if p <= g else np.concatenate([gt + rng.normal(scale=0.01, size=(g, 3)), walk(p - g)])
        gt_rigs.append(star_rig(gt) if g == 19 else chain_rig(gt))
        pred_rigs.append(None if p == 0 else chain_rig(pred))
        preds.append(pred)
        fss.append(rng.uniform(0.005, 0.03, size=g))
    return dict(preds=preds, pred_rigs=pred_rigs, gt_rigs=gt_rigs, fss=fss, want=mo.evaluate(preds, gt_rigs, fss, pred_rigs),
                want_plain=mo.evaluate(preds, gt_rigs, fss))


RATIOS, CHAMFERS = ("iou", "precision", "recall"), ("chamfer_j2j", "chamfer_j2b", "chamfer_b2b")


def run_whole(c, dev, with_rigs, only=None):
    idx = range(len(c["preds"])) if only is None else [only]
    preds = [c["preds"][b] for b in idx]
    res = metrics.evaluate_rigs(cat(preds), ptr(preds), [c["gt_rigs"][b] for b in idx], [c["fss"][b] for b in idx],
                                pred_rigs=[c["pred_rigs"][b] for b in idx] if with_rigs else None, device=dev)
    out = {k: host(res[k]) for k in RATIOS + CHAMFERS + ("hits", "valid") if k in res}
    out.update(mean={k: host(v) for k, v in res["mean"].items()}, num_invalid=res["num_invalid"], report=metrics.format_report(res),
               status=host(res["match"]["status"]), row=host(res["match"]["row_ind"]), col=host(res["match"]["col_ind"]))
    return out


def check_whole(got, want, what):
    """per-mesh ratios and hits bit for bit, chamfers within SUM_TOL; the ratio means bit for bit (a sequential sum of equal bits), the
    chamfer means within SUM_TOL; the report text -> the largest chamfer error seen"""
    assert got["num_invalid"] == want["num_invalid"] and np.array_equal(got["valid"], want["valid"]), what
    check_hits(got["hits"], want["hits"], what)
    worst = 0.0
    for k in RATIOS:
        check_bits(got[k], want[k], f"{what}: {k}")
        check_bits(got["mean"][k], np.float64(want["mean"][k]), f"{what}: mean {k}")
    for k in CHAMFERS:
        if k in got:
            worst = max(worst, check_sum(got[k], want[k], f"{what}: {k}"), check_sum(got["mean"][k], np.float64(want["mean"][k]), f"{what}: mean {k}"))
    assert got["report"] == mo.format_report(want), what
    return worst
