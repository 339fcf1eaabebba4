"""A plain restatement of the point-cloud and deformation operators of csrc/points.hip and csrc/deform.hip: numpy only, no torch, no GPU,
no native library. tests/test_point_oracle.py pins it to oracle/pyg_primitives.py, to the known answers of tests/test_oracle_kat.py and to
the reference-made goldens; tests/test_point_deform_differential.py compares the device with it on the generated inputs at the end of
this file.

Two kinds of function:
  * index decisions (fps, ball_query, radius_sample, knn_search) are DEFINED in float32 -- the contract at the top of points.hip: the
    squared distance is ((dx*dx + dy*dy) + dz*dz) with every product and sum rounded to float32, ties go to the lowest index -- and
    must be met bit for bit;
  * values (knn_apply, sigmoid_minmax, cosine_knn, cosine_nn, flow_vote, gather_rows) are computed in float64 from the float32 inputs;
    the device is held to them within bounds the GPU tests state.
Clarity over speed: loops over clouds and samples, one vectorised line inside."""
import numpy as np

F32 = np.float32
TAU = 2e-6                     # the similarity tolerance the project asserts for cosine_knn (maxdiff(sg, sw) <= 2e-6)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def sqdist32(p, c):
    """((dx*dx + dy*dy) + dz*dz), every step rounded to float32; p [..., 3], c [3] or broadcastable"""
    p, c = _f32(p), _f32(c)
    dx, dy, dz = p[..., 0] - c[..., 0], p[..., 1] - c[..., 1], p[..., 2] - c[..., 2]
    return ((dx * dx + dy * dy) + dz * dz).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- float32 decisions
def fps(pos, ptr, out_ptr, start=None, fill=-1):
    """farthest point sampling per cloud: sample 0 = start[b] (0 where absent or outside [0, n)), then the point with the largest
    minimum squared distance to the chosen ones, lowest index among equals. -> int32 [out_ptr[-1]] GLOBAL indices; a cloud with no point
    or no sample writes nothing (``fill`` stays)."""
    pos = _f32(pos)
    out = np.full(int(out_ptr[-1]), fill, dtype=np.int32)
    for b in range(len(ptr) - 1):
        p0, n = int(ptr[b]), int(ptr[b + 1]) - int(ptr[b])
        o0, m = int(out_ptr[b]), int(out_ptr[b + 1]) - int(out_ptr[b])
        if n <= 0 or m <= 0:
            continue
        p = pos[p0:p0 + n, :3]
        cur = int(start[b]) if start is not None else 0
        if cur < 0 or cur >= n:
            cur = 0
        dist = np.full(n, np.inf, dtype=np.float32)
        for s in range(m):
            out[o0 + s] = p0 + cur
            dist = np.minimum(dist, sqdist32(p, p[cur]))
            cur = int(np.argmax(dist))                               # the first maximum
    return out


def r2_of(r):
    return F32(float(r) * float(r))                                  # float32(float64(r) * float64(r))


def _cloud_of(ptr, k):
    """the cloud whose [ptr[c], ptr[c + 1]) holds row k (empty clouds own no row)"""
    return int(np.searchsorted(np.asarray(ptr), k, side="right")) - 1


def ball_query(x, ptr_x, y, ptr_y, r, max_nbrs):
    """per centre of y the first ``max_nbrs`` points of its cloud in x, in index order, with d^2 < r^2 (strict). -> int64 [2, ny * max_nbrs]:
    row 0 the point, row 1 the centre, unused slots -1."""
    x, y = _f32(x), _f32(y)
    ny = int(ptr_y[-1])
    coo = np.full((2, ny * max_nbrs), -1, dtype=np.int64)
    r2 = r2_of(r)
    for k in range(ny):
        c = _cloud_of(ptr_y, k)
        xs, xe = int(ptr_x[c]), int(ptr_x[c + 1])
        hits = xs + np.nonzero(sqdist32(x[xs:xe, :3], y[k, :3]) < r2)[0][:max_nbrs]
        coo[0, k * max_nbrs:k * max_nbrs + len(hits)] = hits
        coo[1, k * max_nbrs:k * max_nbrs + len(hits)] = k
    return coo


def mix32(a):
    a &= 0xFFFFFFFF
    a ^= a >> 16
    a = (a * 0x7FEB352D) & 0xFFFFFFFF
    a ^= a >> 15
    a = (a * 0x846CA68B) & 0xFFFFFFFF
    a ^= a >> 16
    return a


def radius_sample(x, y, r, max_nbrs, seed):
    """per row of y all points of x with d^2 <= r^2 (inclusive, one cloud). A row with more than ``max_nbrs`` hits keeps a reservoir
    (Algorithm R): hit number t < max goes to slot t; hit number t >= max replaces slot u = (h * (t + 1)) >> 32 when u < max, with
    h = mix32(seed ^ mix32(row * 0x9E3779B9 + t)) in 32-bit arithmetic. -> (slot table int64 [2, ny * max_nbrs], hit counts int32 [ny])."""
    x, y = _f32(x), _f32(y)
    ny = len(y)
    coo = np.full((2, ny * max_nbrs), -1, dtype=np.int64)
    counts = np.zeros(ny, dtype=np.int32)
    r2 = r2_of(r)
    for k in range(ny):
        hits = np.nonzero(sqdist32(x[:, :3], y[k, :3]) <= r2)[0]
        slot = [-1] * max_nbrs
        for t, j in enumerate(hits.tolist()):
            if t < max_nbrs:
                slot[t] = j
            else:
                h = mix32((seed & 0xFFFFFFFF) ^ mix32((k * 0x9E3779B9 + t) & 0xFFFFFFFF))
                u = (h * (t + 1)) >> 32
                if u < max_nbrs:
                    slot[u] = j
        used = min(len(hits), max_nbrs)
        coo[0, k * max_nbrs:k * max_nbrs + used] = slot[:used]
        coo[1, k * max_nbrs:k * max_nbrs + used] = k
        counts[k] = len(hits)
    return coo, counts


def knn_search(x, ptr_x, y, ptr_y, k):
    """per target of y its k (<= 3) nearest sources of the same cloud of x, sorted by (d^2, index). -> (idx int32 [ny, 3], -1 padded;
    wgt float32 [ny, 3] = float32(1) / max(d^2, 1e-16), 0 in the padding)."""
    x, y = _f32(x), _f32(y)
    ny = int(ptr_y[-1])
    idx = np.full((ny, 3), -1, dtype=np.int32)
    wgt = np.zeros((ny, 3), dtype=np.float32)
    for c in range(len(ptr_y) - 1):
        xs, xe = int(ptr_x[c]), int(ptr_x[c + 1])
        kk = min(k, xe - xs)
        for t in range(int(ptr_y[c]), int(ptr_y[c + 1])):
            if kk <= 0:
                continue
            d = sqdist32(x[xs:xe, :3], y[t, :3])
            o = np.argsort(d, kind="stable")[:kk]                    # stable: the lower index first among equal distances
            idx[t, :kk] = xs + o
            wgt[t, :kk] = F32(1.0) / np.maximum(d[o], F32(1e-16))
    return idx, wgt


# ---------------------------------------------------------------------------------------------------------------- float64 values
def knn_apply(feat, idx, wgt):
    """out[t] = sum_s w_s feat[idx_s] / sum_s w_s over the slots with idx >= 0, in float64"""
    f, w = np.asarray(feat, dtype=np.float64), np.asarray(wgt, dtype=np.float64)
    ok = idx >= 0
    g = f[np.where(ok, idx, 0)]                                       # [ny, 3, C]
    w = np.where(ok, w, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (g * w[..., None]).sum(1) / w.sum(1)[:, None]


def knn_apply_scale(feat, idx):
    """max |feat| over the live neighbours of every target, per column: what the device's rounding error scales with"""
    f = np.abs(np.asarray(feat, dtype=np.float64))
    ok = idx >= 0
    return np.where(ok[..., None], f[np.where(ok, idx, 0)], 0.0).max(1)


def sigmoid_minmax(x, ptr):
    """sigmoid, then (s - min) / (max - min) per mesh; a constant mesh is 0 / 0 = NaN"""
    s = 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64).reshape(-1)))
    out = np.full(len(s), np.nan)
    rng = np.zeros(len(ptr) - 1)
    for b in range(len(ptr) - 1):
        m = s[int(ptr[b]):int(ptr[b + 1])]
        if len(m):
            rng[b] = m.max() - m.min()
            with np.errstate(invalid="ignore", divide="ignore"):
                out[int(ptr[b]):int(ptr[b + 1])] = (m - m.min()) / rng[b]
    return out, rng


class CosineRows:
    """cosine_knn's answer with everything a comparison needs: per query row q
      order[q]  the candidates it may select (its own cloud; the visible ones in split mode), GLOBAL ids sorted by (similarity
                descending, index ascending); empty for a row that does not query;
      ssort[q]  their float64 similarities in that order;
      idx       [ny, k] the first k of ``order``, -1 padded;
      lo, hi    the query's candidate cloud [lo, hi) in x."""

    def __init__(self, ny, k):
        self.order, self.ssort = [None] * ny, [None] * ny
        self.idx = np.full((ny, k), -1, dtype=np.int32)
        self.lo, self.hi = np.zeros(ny, dtype=np.int64), np.zeros(ny, dtype=np.int64)


def cosine_knn(y, ptr_y, x, ptr_x, k, vis=None, split=False):
    """the k rows of x of the same cloud with the largest dot product per row of y, most similar first, lowest index among equals.
    split: x is y, rows with vis < 0.5 query the rows with vis >= 0.5 of their own mesh, every other row is all -1."""
    y64, x64 = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    ny = int(ptr_y[-1])
    res = CosineRows(ny, k)
    v = None if vis is None else _f32(vis).reshape(-1)
    if split:
        ptr_x = ptr_y
    for c in range(len(ptr_y) - 1):
        ys, ye, xs, xe = int(ptr_y[c]), int(ptr_y[c + 1]), int(ptr_x[c]), int(ptr_x[c + 1])
        cand = np.arange(xs, xe)
        if split:
            cand = cand[v[xs:xe] >= F32(0.5)]
        for q in range(ys, ye):
            res.lo[q], res.hi[q] = xs, xe
            if split and not v[q] < F32(0.5):
                res.order[q], res.ssort[q] = np.zeros(0, dtype=np.int64), np.zeros(0)
                continue
            s = (x64[cand] * y64[q]).sum(1)
            o = np.argsort(-s, kind="stable")                        # candidates ascend, so stable = lowest index among equals
            res.order[q], res.ssort[q] = cand[o], s[o]
            kk = min(k, len(cand))
            res.idx[q, :kk] = cand[o][:kk]
    return res


def cosine_nn(v, ptr_v, p, ptr_p):
    """-> (nn int32 [nv], sim float64 [nv], the CosineRows): the k = 1 case with its similarity; -1 / 0 without a candidate"""
    res = cosine_knn(v, ptr_v, p, ptr_p, 1)
    sim = np.array([s[0] if len(s) else 0.0 for s in res.ssort])
    return res.idx[:, 0].copy(), sim, res


def well_separated(res, k, tau=TAU):
    """rows whose gaps between consecutive sorted similarities, among the first min(k, n_live) + 1, all exceed 2 tau: the device
    list must equal the oracle's there whatever the order of its float32 operations"""
    ok = np.ones(len(res.order), dtype=bool)
    for q, s in enumerate(res.ssort):
        top = s[:min(k, len(s)) + 1]
        if len(top) > 1:
            ok[q] = bool((top[:-1] - top[1:]).min() > 2 * tau)
    return ok


def cosine_rows_check(got_idx, res, k, y, x, dup_group=None, got_sim=None, tau=TAU):
    """the per-row rule of the GPU tests on a device result ``got_idx`` [ny, k] (and ``got_sim`` of cosine_nn). -> (list of violations,
    number of rows that are not well separated). Every row is checked:
      live entries lie in the row's candidate set (own cloud, visible in split mode), without duplicates;
      entry j is at least as similar as the oracle's j-th, up to tau; the list does not increase by more than tau;
      the padding is -1 exactly where the oracle's is (and sim = 0 there); rows that do not query are all -1;
      got_sim is within tau of the float64 similarity of the entry;
      a well-separated row equals the oracle's list;
      members of one group of exactly equal candidates (``dup_group`` [nx], -1 = none) come out lowest index first: an entry is preceded
      by every candidate of its group with a lower index."""
    y64, x64 = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    bad = []
    sep = well_separated(res, k, tau)
    for q in range(len(res.order)):
        g, order, ssort = got_idx[q], res.order[q], res.ssort[q]
        n_live = min(k, len(order))
        if not np.array_equal(g < 0, res.idx[q] < 0):
            bad.append(f"row {q}: padding {g.tolist()} against {res.idx[q].tolist()}")
            continue
        if got_sim is not None and n_live == 0 and got_sim[q] != 0.0:
            bad.append(f"row {q}: similarity {got_sim[q]} in the padding")
        if n_live == 0:
            continue
        live = g[:n_live].astype(np.int64)
        if len(set(live.tolist())) != n_live or not np.isin(live, order).all():
            bad.append(f"row {q}: {live.tolist()} repeats an entry or leaves the candidate set")
            continue
        s = (x64[live] * y64[q]).sum(1)
        if (s < ssort[:n_live] - tau).any():
            bad.append(f"row {q}: entry less similar than the oracle's by {float((ssort[:n_live] - s).max()):.3e}")
        if n_live > 1 and (s[1:] - s[:-1]).max() > tau:
            bad.append(f"row {q}: list increases by {float((s[1:] - s[:-1]).max()):.3e}")
        if got_sim is not None and abs(float(got_sim[q]) - s[0]) > tau:
            bad.append(f"row {q}: similarity {got_sim[q]} against {s[0]}")
        if sep[q] and not np.array_equal(live, order[:n_live]):
            bad.append(f"row {q}: well separated, {live.tolist()} against {order[:n_live].tolist()}")
        if dup_group is not None:
            for p, j in enumerate(live.tolist()):
                if dup_group[j] >= 0:
                    lower = [i for i in order.tolist() if dup_group[i] == dup_group[j] and i < j]
                    if not set(lower) <= set(live[:p].tolist()):
                        bad.append(f"row {q}: {j} of duplicate group {dup_group[j]} ahead of a lower index: {live.tolist()}")
    return bad, int((~sep).sum())


def flow_vote(mode, idx, feat_q, feat_s, pos_q, pos_s, vis, l1):
    """similarity-weighted voting in float64 on the neighbour lists ``idx`` [n, k] (-1 = skipped). l1 [n, 4] float64 = [flow | vis] is
    updated and returned with the per-row bound terms:
      mode 0, every row i:          w_t = <f_s[j_t], f_q[i]> * vis[i], flow[i] = sum w_t (pos_s[j_t] - pos_q[i]) / sum w_t, l1[i, 3] = vis[i]
      mode 1, rows with vis < 0.5:  w_t = <f_s[j_t], f_q[i]>,          flow[i] = sum w_t flow[j_t] / sum w_t
    a row without neighbours or with a zero weight sum is 0 / 0 = NaN.
    -> (l1, rows written [n] bool, wsum [n], vsum [n] = sum_t ||v_t||inf)"""
    fq, fs = np.asarray(feat_q, dtype=np.float64), np.asarray(feat_s, dtype=np.float64)
    v = np.asarray(vis, dtype=np.float64).reshape(-1)
    v32 = _f32(vis).reshape(-1)
    out = np.array(l1, dtype=np.float64)
    n, k = idx.shape
    rows = np.ones(n, dtype=bool) if mode == 0 else (v32 < F32(0.5))
    wsum, vsum = np.zeros(n), np.zeros(n)
    src = out[:, :3].copy()                                          # mode 1 reads visible rows only: final after mode 0
    for i in np.nonzero(rows)[0]:
        acc = np.zeros(3)
        for t in range(k):
            j = int(idx[i, t])
            if j < 0:
                continue
            dot = float((fs[j] * fq[i]).sum())
            if mode == 0:
                w, val = dot * v[i], np.asarray(pos_s, dtype=np.float64)[j, :3] - np.asarray(pos_q, dtype=np.float64)[i, :3]
            else:
                w, val = dot, src[j]
            acc += w * val
            wsum[i] += w
            vsum[i] += np.abs(val).max()
        with np.errstate(invalid="ignore", divide="ignore"):
            out[i, :3] = acc / wsum[i]
    if mode == 0:
        out[:, 3] = v
    return out, rows, wsum, vsum


def gather_rows(src, idx):
    """dst[r] = src[idx[r]], a zero row for idx = -1"""
    src = np.asarray(src)
    out = np.zeros((len(idx), src.shape[1]), dtype=src.dtype)
    ok = np.asarray(idx) >= 0
    out[ok] = src[np.asarray(idx)[ok]]
    return out


def ulp_distance(a, b):
    """largest distance in units of the last place between two float32 arrays of one sign pattern"""
    ia, ib = _f32(a).view(np.int32).astype(np.int64), _f32(b).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max()) if ia.size else 0


# ================================================================================================================ generated inputs
# Every input of tests/test_point_deform_differential.py is built here, from numpy's seeded generators, so that the CPU suite
# (tests/test_point_oracle.py) re-checks on every run, from the oracle alone, the conditions the GPU tests rely on.
def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _rng(*key):
    return np.random.default_rng([0x504F494E] + [int(k) for k in key])


def padded(p3, ld, fill=0.0):
    """[n, 3] -> float32 [n, ld] with the coordinates in columns 0..2 and ``fill`` behind them"""
    out = np.full((len(p3), ld), fill, dtype=np.float32)
    out[:, :3] = p3
    return out


# ---- FPS ---------------------------------------------------------------------------------------------------------------------
FPS_SIZES = [1, 2, 5, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768]


def _clustered(n, rng):
    centres = rng.uniform(-1.0, 1.0, size=(12, 3))
    return centres[rng.integers(0, 12, n)] + rng.normal(0.0, 0.004, size=(n, 3))


def _lattice(n):
    """n = 8192 points i/16 of a 32 x 16 x 16 grid: equal distances everywhere"""
    i = np.arange(n)
    return np.stack([i // 256, (i // 16) % 16, i % 16], 1) / 16.0


def near_bound_cloud():
    """four groups of 128 coincident points, one Morton cell and so one bucket each: S (the start) at the origin, A at x = 1.0001, F at
    x = 2, B at y = 0.99995. After S the farthest is F; F lowers A's distance from 1.0002 to 0.9998, by less than 0.1 %, to just under
    B's 0.9999: the next sample is B. A bucket skipped although its bound is below its maximum keeps 1.0002 and answers A."""
    pts = np.zeros((512, 3))
    pts[128:256, 0], pts[256:384, 0], pts[384:512, 1] = 1.0001, 2.0, 0.99995
    return pts


def fps_cases():
    """name -> dict(pos float32 [N, ldp], ptr, out_ptr, start or None, max_n). The deciding size of a launch is max_n."""
    cases = {}

    def add(name, clouds, samples, ldp=4, start=None):
        pos = padded(np.concatenate(clouds) if sum(len(c) for c in clouds) else np.zeros((0, 3)), ldp, fill=9.0)
        cases[name] = dict(pos=pos, ptr=_ptr([len(c) for c in clouds]), out_ptr=_ptr(samples),
                           start=None if start is None else np.asarray(start, dtype=np.int32), max_n=max(len(c) for c in clouds))

    for i, n in enumerate(FPS_SIZES):                                # uniform clouds, a small second cloud behind the deciding one
        rng = _rng(1, n)
        add(f"size_{n}", [rng.uniform(0, 1, size=(n, 3)), rng.uniform(0, 1, size=(min(n, 37), 3))], [min(n, 320), min(n, 19)], ldp=(3, 4, 7)[i % 3])
    rng = _rng(2)
    add("ragged", [rng.uniform(0, 1, size=(n, 3)) for n in (1, 63, 64, 65, 8192)], [1, 32, 64, 33, 300])
    add("clustered_8192", [_clustered(8192, rng)], [400])
    add("clustered_4096", [_clustered(4096, rng), _clustered(3000, rng)], [300, 300], ldp=7)
    add("lattice_8192", [_lattice(8192)], [1024])
    add("lattice_shuffled", [_lattice(8192)[rng.permutation(8192)]], [1024], ldp=3)
    add("lattice_old_arm", [np.concatenate([_lattice(8192), _lattice(8192) + [2.0, 0, 0]])[rng.permutation(16384)]], [600])
    add("coincident", [np.tile(rng.uniform(0, 1, size=(1, 3)), (500, 1))], [20])
    add("plane", [np.concatenate([rng.uniform(0, 1, size=(3000, 2)), np.full((3000, 1), 0.25)], 1)], [200])
    add("line", [np.outer(rng.uniform(0, 1, 2000), [1.0, 0.0, 0.0]) + [0.0, 0.5, -0.5]], [200])
    add("far_negative", [-1.0e3 + rng.uniform(-50, 50, size=(5000, 3))], [200])
    add("near_bound", [near_bound_cloud()], [6])
    add("starts", [rng.uniform(0, 1, size=(n, 3)) for n in (700, 33, 1500, 100)], [100, 17, 100, 50], start=[5, -3, 1500, 99])
    add("m_is_n_and_one", [rng.uniform(0, 1, size=(64, 3)), rng.uniform(0, 1, size=(200, 3))], [64, 1], ldp=3)
    add("empty_members", [rng.uniform(0, 1, size=(300, 3)), np.zeros((0, 3)), rng.uniform(0, 1, size=(200, 3)), rng.uniform(0, 1, size=(150, 3))],
        [50, 4, 0, 30])
    return cases


def fps_tie_steps(pos, ptr, out_ptr, start=None):
    """how many arg-max steps of the oracle's run met more than one maximum (the statement 'ties at almost every step' measured)"""
    pos, ties, steps = _f32(pos), 0, 0
    for b in range(len(ptr) - 1):
        p = pos[int(ptr[b]):int(ptr[b + 1]), :3]
        n, m = len(p), int(out_ptr[b + 1]) - int(out_ptr[b])
        if n <= 0 or m <= 0:
            continue
        cur = int(start[b]) if start is not None and 0 <= int(start[b]) < n else 0
        dist = np.full(n, np.inf, dtype=np.float32)
        for s in range(m - 1):
            dist = np.minimum(dist, sqdist32(p, p[cur]))
            cur = int(np.argmax(dist))
            ties += int((dist == dist[cur]).sum() > 1)
            steps += 1
    return ties, steps


# ---- ball query, radius sample -------------------------------------------------------------------------------------------------
def ball_case():
    """x clouds of 0, 130, 193 (= 64 * 3 + 1), 0 and 500 points, centre clouds of 0, 40, 5, 3 and 70 centres (ptr_y repeats entries; one
    centre cloud faces an empty point cloud). ldx = 4, ldy = 5. Centre 40 (cloud 2) sees only the LAST point of its 193; centre 48 (cloud 4)
    has a point at exactly r = 0.25 (excluded)."""
    rng = _rng(3)
    nx, nyc = [0, 130, 193, 0, 500], [0, 40, 5, 3, 70]
    x = rng.uniform(0, 1, size=(sum(nx), 3))
    y = rng.uniform(0, 1, size=(sum(nyc), 3))
    x[130:130 + 193] += [5.0, 0, 0]                                   # cloud 2 far from its first centre ...
    y[40] = [0.5, 0.5, 0.5]
    x[130 + 192] = [0.5, 0.5, 0.625]                                  # ... but for the point of the last lane-step
    y[48] = [0.5, 0.25, 0.25]
    x[323 + 7] = [0.75, 0.25, 0.25]                                   # d^2 = 0.0625 = r^2 exactly
    return dict(x=padded(x, 4, 3.0), ptr_x=_ptr(nx), y=padded(y, 5, -3.0), ptr_y=_ptr(nyc), radii=(0.25, 0.5), max_nbrs=(1, 16, 64, 65, 130))


def radius_case():
    """700 points, 150 centres, r = 0.3: over-full and under-full rows at max_nbrs = 64; three far centres (no hit) and one centre with
    exactly one hit, at exactly r (inclusive), for max_nbrs = 1"""
    rng = _rng(4)
    x, y = rng.uniform(0, 1, size=(700, 3)), rng.uniform(0, 1, size=(150, 3))
    y[10:13] = [[4.0, 4, 4], [-3.0, 0, 0], [0.5, 9.0, 0.5]]
    y[13] = [3.0, 3.0, 3.0]
    x[20] = [3.0, 3.0, 2.75]                                          # the only point near centre 13, at distance 0.25 exactly
    return dict(x=padded(x, 4), y=padded(y, 3), cases=((0.3, 64), (0.3, 1), (0.25, 1), (0.25, 64)), seeds=(0, 12345))


# ---- k-NN, gather --------------------------------------------------------------------------------------------------------------
KNN_SRC = [1, 2, 3, 1023, 1024, 1025, 2049]
KNN_TGT = [255, 256, 257, 10, 300, 255, 257]


def knn_case():
    """sources of 1 .. 2049 points (fewer than k, a tile boundary, an odd tail), 255 / 256 / 257 targets per cloud. In the clouds that
    reach position 1023, targets 0 / 1 / 2 have their nearest sources planted at 1023, 1024 (where it exists) and the last position;
    target 3 coincides with a source (the 1e-16 clamp); target 4 sits next to two equal sources (ranks 1 and 2); target 5 has two
    nearer sources (60, 61) and then two EQUAL sources 50 and 700 at rank 3: the tie the third slot decides, the lower index stays."""
    rng = _rng(5)
    px, py = _ptr(KNN_SRC), _ptr(KNN_TGT)
    x = rng.uniform(0, 1, size=(px[-1], 3)).astype(np.float32)
    y = rng.uniform(0, 1, size=(py[-1], 3)).astype(np.float32)
    planted = {}
    for c, ns in enumerate(KNN_SRC):
        if ns < 1023:
            continue
        xs, ys = int(px[c]), int(py[c])
        spots = sorted({1022 if ns == 1023 else 1023, min(1024, ns - 1), ns - 1})
        for t in range(3):                                            # target t: its three nearest ARE the planted spots, in a rotated order
            y[ys + t] = [2.0 + t, 2.0, 2.0]
        for r, s in enumerate(spots):
            x[xs + s] = [2.0 + r, 2.0, 2.0 + 0.001 * (r + 1)]
        planted[c] = [xs + s for s in spots]
        y[ys + 3] = x[xs + 5]
        x[xs + 40] = x[xs + 600]                                      # equal sources 40 and 600
        y[ys + 4] = x[xs + 40] + np.float32(0.0005)
        y[ys + 5] = [-2.0, -2.0, -2.0]
        x[xs + 60], x[xs + 61] = [-2.0, -2.0, -1.75], [-2.0, -1.5, -2.0]
        x[xs + 50] = x[xs + 700] = [-1.0, -2.0, -2.0]
    return dict(x=padded(x, 4), ptr_x=px, y=padded(y, 6, 1.0), ptr_y=py, planted=planted, max_t=max(KNN_TGT))


def gather_case():
    """9000 rows x 131 columns (beyond 4096 blocks of 256 elements), every 7th index -1"""
    rng = _rng(6)
    src = rng.normal(size=(700, 140)).astype(np.float32)
    idx = rng.integers(0, 700, 9000).astype(np.int32)
    idx[::7] = -1
    idx[1], idx[2] = 0, 699
    return dict(src=src, idx=idx, col0=5, cols=131)


# ---- cosine k-NN ---------------------------------------------------------------------------------------------------------------
def unit_rows(n, rng):
    a = rng.normal(size=(n, 64))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


COS_Q = [1, 63, 64, 65, 255, 256, 257, 0, 40, 70]
COS_X = [3, 900, 31, 32, 33, 1, 900, 50, 0, 900]
DUPES = (7, 37, 40, 41, 66, 899)          # local rows of one cloud: tiles 0, 1, 1, 1, 2 and the last partial tile; 7 and 37 belong to the lanes
#                                           l + 32 (rows 4..7 of every 8), 40, 41, 66 and 899 to the lanes l
LANE_DUPES = (128, 129, 130, 131, 136, 137, 138, 139, 144)          # nine rows of ONE 32-row tile that ONE lane half owns (rows 0..3 of
#                                           every 8), none in the other half: more equal candidates than any K within one lane's scan


def cosine_case():
    """unit Gaussian rows; query clouds of 1 .. 257 rows against candidate clouds of 1 .. 900 rows, an empty query cloud and an empty
    candidate cloud in the batch. In candidate cloud 6 (900 rows, 257 queries) the rows DUPES are equal and query 3 of the cloud equals
    them; in candidate cloud 9 (900 rows, 70 queries) the rows LANE_DUPES are equal and query 5 equals them. -> dict(y, x, ptr_y, ptr_x, dup_group)"""
    rng = _rng(7)
    py, px = _ptr(COS_Q), _ptr(COS_X)
    y, x = unit_rows(int(py[-1]), rng), unit_rows(int(px[-1]), rng)
    dup = np.full(len(x), -1, dtype=np.int64)
    xs = int(px[6])
    for d in DUPES:
        x[xs + d] = x[xs + DUPES[0]]
        dup[xs + d] = 0
    y[int(py[6]) + 3] = x[xs + DUPES[0]]
    xs = int(px[9])
    for d in LANE_DUPES:
        x[xs + d] = x[xs + LANE_DUPES[0]]
        dup[xs + d] = 1
    y[int(py[9]) + 5] = x[xs + LANE_DUPES[0]]
    return dict(y=y, x=x, ptr_y=py, ptr_x=px, dup_group=dup)


SPLIT_N = [1, 63, 64, 65, 255, 256, 257, 900, 0, 33, 20]


def split_case():
    """one matrix, a visibility per row: meshes of 1 .. 900 rows; mesh 9 (33 rows) has no visible row, mesh 10 (20 rows) no invisible
    one, mesh 0 is one invisible row. In mesh 7 the rows DUPES are equal and visible, row 3 equals them and is invisible; the rows LANE_DUPES are
    equal and visible, row 5 equals them and is invisible."""
    rng = _rng(8)
    ptr = _ptr(SPLIT_N)
    f = unit_rows(int(ptr[-1]), rng)
    vis = rng.uniform(0, 1, size=int(ptr[-1])).astype(np.float32)
    vis[0] = 0.2
    vis[ptr[9]:ptr[10]] = 0.1
    vis[ptr[10]:ptr[11]] = 0.9
    dup = np.full(len(f), -1, dtype=np.int64)
    s = int(ptr[7])
    for d in DUPES:
        f[s + d] = f[s + DUPES[0]]
        vis[s + d] = 0.75
        dup[s + d] = 0
    f[s + 3], vis[s + 3] = f[s + DUPES[0]], 0.25
    for d in LANE_DUPES:
        f[s + d] = f[s + LANE_DUPES[0]]
        vis[s + d] = 0.75
        dup[s + d] = 1
    f[s + 5], vis[s + 5] = f[s + LANE_DUPES[0]], 0.25
    return dict(f=f, vis=vis.reshape(-1, 1), ptr=ptr, dup_group=dup)


def near_tie_share(res, k):
    return float((~well_separated(res, k)).mean()) if len(res.order) else 0.0


# ---- flow vote, sigmoid --------------------------------------------------------------------------------------------------------
def flow_case(n):
    """n vertices in three meshes (the last has no visible vertex) against three point clouds (the last of 3 points: -1 padding for
    k > 3). Features share a common direction, so every similarity is positive (about 0.4) and the weight sums stay away from zero.
    vis is 0 exactly on every 11th vertex of mesh 0 (mode 0: flow NaN), else in [0.1, 0.45] or [0.55, 1]."""
    rng = _rng(9, n)
    counts = [n - 120, 100, 20]
    pcounts = [400, 150, 3]
    ptr, pptr = _ptr(counts), _ptr(pcounts)
    u = np.zeros(64)
    u[0] = 0.8

    def feats(m):
        a = rng.normal(size=(m, 64)) / 8.0 + u
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)

    f, pf = feats(n), feats(int(pptr[-1]))
    vis = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0.1, 0.45, n), rng.uniform(0.55, 1.0, n)).astype(np.float32)
    vis[0:counts[0]:11] = 0.0
    vis[ptr[2]:ptr[3]] = rng.uniform(0.1, 0.45, counts[2]).astype(np.float32)
    pos = rng.normal(size=(n, 3)).astype(np.float32)
    ppos = rng.normal(size=(int(pptr[-1]), 3)).astype(np.float32)
    return dict(f=f, pf=pf, vis=vis.reshape(-1, 1), ptr=ptr, pptr=pptr, pos=pos, ppos=ppos)


def punch_holes(idx):
    """-1 in the MIDDLE of every 5th list with three or more live entries (the kernel skips them wherever they are)"""
    idx = idx.copy()
    for i in range(0, len(idx), 5):
        if idx.shape[1] >= 3 and (idx[i] >= 0).sum() >= 3:
            idx[i, 1] = -1
    return idx


SIG_N = [1, 2, 255, 0, 256, 257, 5000, 100]


def sigmoid_case():
    """logits in +-30 in column 1 of 3; meshes of 1 .. 5000 vertices with an empty mesh between two others; the last is constant. In the
    mesh of 256 the smallest logit sits at local row 200 and the largest at 250 (the fourth wave of the block)."""
    rng = _rng(10)
    ptr = _ptr(SIG_N)
    x = rng.uniform(-30, 30, size=(int(ptr[-1]), 3)).astype(np.float32)
    x[ptr[1]:ptr[2], 1] = [-1.0, 2.5]
    x[ptr[4]:ptr[5], 1] = rng.uniform(-2, 2, size=256).astype(np.float32)
    x[ptr[4] + 200, 1], x[ptr[4] + 250, 1] = -30.0, 30.0
    x[ptr[7]:ptr[8], 1] = 0.37
    return dict(x=x, ptr=ptr)
