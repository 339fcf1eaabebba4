"""NumPy float64 restatement of the skeleton connection stage (evaluate/joint2rig.py:197-264 with utils/mst_utils.py:15-108, 269-291):
pair attributes, outside-bone counts, the cost matrix, Prim. Written from the reference's definitions, vectorised over the samples of a
bone; no code of the reference, no GPU, no native library. It states the two number-format chains explicitly:

  attributes  create_one_data gets float64 joints: length, step count, unit step and samples are float64.
  cost loop   increase_cost_for_outside_bone gets Data.joints, float32: the ray, the length, length / 0.01, the rounded step count, the
              count + 1e-30 and the unit step are float32 (NumPy 2: a float32 scalar against a Python float stays float32); the sample
              positions are float64 because arange(1, n + 1) is.

Besides the results it returns the margins the fixture conditions are about: how far a bone's length / 0.01 is from a half-integer,
how far a sample's voxel coordinate is from a rounding boundary, how far apart the keys were that Prim chose between.
"""
import numpy as np

GRID = 88
STEP = 0.01


def pair_list(n_joints):
    """itertools.combinations(range(J), 2) as an int64 [P, 2] array"""
    i, j = np.triu_indices(int(n_joints), k=1)
    return np.stack([i, j], axis=1).astype(np.int64)


def sigmoid_f32(x):
    """the float32 nearest to the float64 sigmoid of a float32 logit"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


def _half_margin(q):
    """distance of q from the nearest half-integer"""
    return float(np.abs((q - np.floor(q)) - 0.5).min()) if np.size(q) else 0.5


def _bone(p, c, grid, translate, scale, dims0, single):
    """-> (samples, inside count, length as the chain has it, margin of length / step, margin of the voxel coordinates)"""
    if single:
        p, c = p.astype(np.float32), c.astype(np.float32)
        d = p - c
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        q = length / np.float32(STEP)
        n = np.rint(q)
        unit = ((c - p) / (n + np.float32(1e-30))).astype(np.float64)
        assert length.dtype == q.dtype == n.dtype == np.float32
    else:
        p, c = p.astype(np.float64), c.astype(np.float64)
        d = p - c
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        q = length / STEP
        n = np.rint(q)
        unit = (c - p) / (n + 1e-30)
    n = int(n)
    steps = np.arange(1, n + 1, dtype=np.float64)
    samples = p.astype(np.float64)[None, :] + unit[None, :] * steps[:, None]
    coord = ((samples - np.asarray(translate, dtype=np.float64)[None, :]) / float(scale)) * float(dims0)
    vc = np.rint(coord)
    ok = np.all((vc >= 0) & (vc < GRID), axis=1)
    vi = np.clip(vc, 0, GRID - 1).astype(np.int64)
    inside = ok & (grid[vi[:, 0], vi[:, 1], vi[:, 2]] != 0)
    return n, int(inside.sum()), float(length), _half_margin(np.float64(q)), _half_margin(coord)


def pair_attributes(joints64, grid, translate, scale, dims0=GRID):
    """-> dict: pairs int64 [P, 2], pair_attr float32 [P, 3] (distance, inside / (samples + 1e-10), 1), outside_count int32 [P] (float32
    chain), n_samples int64 [P, 2] (float64 chain, float32 chain), length_margin, voxel_margin (the smallest over both chains)."""
    j64 = np.asarray(joints64, dtype=np.float64).reshape(-1, 3)
    j32 = j64.astype(np.float32)
    grid = np.asarray(grid).reshape(GRID, GRID, GRID)
    pairs = pair_list(len(j64))
    attr = np.zeros((len(pairs), 3), dtype=np.float64)
    outside = np.zeros(len(pairs), dtype=np.int32)
    ns = np.zeros((len(pairs), 2), dtype=np.int64)
    lm, vm = 0.5, 0.5
    for k, (i, j) in enumerate(pairs):
        n, n_in, length, m1, m2 = _bone(j64[i], j64[j], grid, translate, scale, dims0, single=False)
        attr[k] = (length, n_in / (n + 1e-10), 1.0)
        nf, nf_in, _, m3, m4 = _bone(j32[i], j32[j], grid, translate, scale, dims0, single=True)
        outside[k] = nf - nf_in
        ns[k] = (n, nf)
        lm, vm = min(lm, m1, m3), min(vm, m2, m4)
    return dict(pairs=pairs, pair_attr=attr.astype(np.float32), outside_count=outside, n_samples=ns, length_margin=lm, voxel_margin=vm)


def connectivity_cost(pair_logits, root_logits, joints32, outside_count):
    """-> (cost float64 [J, J], root id, count-derived mask [J, J] bool: entries that come from counts, and the diagonal)"""
    j32 = np.asarray(joints32, dtype=np.float32).reshape(-1, 3)
    n = len(j32)
    pairs = pair_list(n)
    prob = np.zeros((n, n), dtype=np.float64)
    prob[pairs[:, 0], pairs[:, 1]] = sigmoid_f32(np.asarray(pair_logits).reshape(-1)).astype(np.float64)
    prob = prob + prob.T
    cost = -np.log(prob + 1e-10)
    from_count = np.eye(n, dtype=bool)
    oc = np.asarray(outside_count).reshape(-1)
    on_plane = np.abs(j32[:, 0]) < np.float32(2e-2)
    for k, (i, j) in enumerate(pairs):
        if oc[k] > 1:
            cost[i, j] = cost[j, i] = 2.0 * float(oc[k])
            from_count[i, j] = from_count[j, i] = True
        if on_plane[i] and on_plane[j]:
            cost[i, j] *= 0.5
            cost[j, i] *= 0.5
    root = int(np.argmax(sigmoid_f32(np.asarray(root_logits).reshape(-1))))
    return cost, root, from_count


def prim(cost, root):
    """-> (parent int32 [J] or None, key float64 [J], status 0 / 1 = disconnected, decision margin). The margin: over all steps, the
    smallest gap between the chosen key and the next DIFFERENT candidate key, and between a relaxed key and the cost that replaced
    or failed to replace it; ``ties_integer`` False when two exactly equal candidate keys were not integer-valued."""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    key = np.full(n, np.inf)
    parent = np.full(n, -1, dtype=np.int32)
    done = np.zeros(n, dtype=bool)
    key[root] = 0.0
    margin, ties_integer = np.inf, True
    for _ in range(n):
        cand = np.where(~done & np.isfinite(key))[0]
        if len(cand) == 0:
            return None, key, 1, dict(margin=margin, ties_integer=ties_integer)
        ks = key[cand]
        u = int(cand[np.argmin(ks)])                     # argmin: the first index among equal minima
        others = ks[ks != key[u]]
        if len(others):
            margin = min(margin, float(others.min() - key[u]))
        if (ks == key[u]).sum() > 1 and key[u] != np.rint(key[u]):
            ties_integer = False
        done[u] = True
        row = cost[u]
        live = ~done & (row > 0)
        gap = np.abs(key[live] - row[live])
        gap = gap[np.isfinite(gap) & (gap > 0)]
        if len(gap):
            margin = min(margin, float(gap.min()))
        eq = live & (key == row)
        if np.any(eq & (row != np.rint(row))):
            ties_integer = False
        relax = live & (key > row)
        key[relax] = row[relax]
        parent[relax] = u
    return parent, key, 0, dict(margin=margin, ties_integer=ties_integer)


def root_margin(root_logits):
    r = np.sort(np.asarray(root_logits, dtype=np.float64).reshape(-1))
    return float(r[-1] - r[-2]) if len(r) > 1 else np.inf


def tree_cost(cost, parent, root):
    """total cost of a parent array on a cost matrix; raises unless it is a spanning tree rooted at root"""
    parent = np.asarray(parent).astype(np.int64)
    n = len(parent)
    assert parent[root] == -1 and np.all(np.delete(parent, root) >= 0) and np.all(parent < n)
    reached = np.arange(n) == root
    for _ in range(n):
        reached = reached | np.where(parent >= 0, reached[np.maximum(parent, 0)], False)
    assert reached.all(), "not a spanning tree"
    idx = np.array([v for v in range(n) if v != root], dtype=np.int64)
    return float(np.asarray(cost)[parent[idx], idx].sum()) if len(idx) else 0.0
