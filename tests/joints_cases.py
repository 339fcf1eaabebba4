"""Generated cases for joint extraction (csrc/joints.hip, morig_amd/joints.py) at the sizes its kernels branch on, numpy restatements of
the kernels in their operation order, small models of the kernels' control flow, and the compare helpers that tests/test_joints_cases.py
(CPU) and tests/test_joints_differential.py (device) share. Not a test file; no GPU, no torch: every input comes from
``np.random.default_rng(seed)`` or is built from dyadic numbers, except the second inside table, which takes the voxel grid of the
``joints_small`` fixture. oracle/joints.py is the independent reference; the CPU file holds every restatement below to it.

What a case is for:
  kth_nn4_kernel          K4_R = 4 rows per workgroup and 256 threads striding over the candidates; 16-bit bin halves shared by two
                          rows; K4_LIST = 64 between "list pass next" and "another histogram pass"; the hand-off to the generic 8 x 8-bit
                          passes through `need <= s_lo` and through `need > total`; rows past the end that shadow the last row
  kth_nn_kernel<true>     the one-row kernel, reached on small inputs by passing max_n = 65536; KTH_SMALL = 8 keys in the selected bin
  nms_counts_kernel       256 targets per workgroup; nms_counts_box_kernel: MSB = 32 targets; sqrt_le_threshold at, below and above a rooted
                          distance that occurs
  nms_greedy_kernel       NMS_T = 1024 order entries per look-ahead, the `first == NMS_T` skip, the float32 and the density compare at equality
  meanshift_step_kernel   MS_TGT = 32 targets x 8 slices of an MS_TILE = 256 source tile; meanshift_step_box_kernel: MSB = 32 points per box,
                          256 boxes per chunk, near boxes dealt to four waves, two box buffers, the pass-through after convergence
  inside_check_kernel     rint on exact halves, -0.5 -> voxel 0, 87.5 -> 88, 256 threads per workgroup

Bars: k-th distances, neighbour counts, survivors of the suppression, inside masks and the mean-shift step on the exact lattice are
compared bit for bit; the bandwidth is within n * 2^-53 of the correctly rounded mean; modes of the generic mean-shift cases are within
MODE_TOL = 1e-11 of the restatement (the bar tests/test_joints_host.py uses for modes of unit-box inputs: the kernels add the same terms
in another order)."""
import functools
import itertools
import math

import numpy as np

from oracle import joints as O

K4_R, K4_LIST, KTH_SMALL = 4, 64, 8
MS_TILE, MS_TGT, MSB, NMS_T = 256, 32, 32, 1024
ONE_ROW_MAX_N = 65536                  # max_n above 65535: the batched entry point launches kth_nn_kernel<true>
MODE_TOL = 1e-11
STOP, STOP_MARGIN = 1e-3, 1e-6         # the reference's stop rule and how far a generic case stays from it at every step
SMALL_SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)
BIG = 8193 + 1                         # 257 boxes of MSB points: more than one chunk of 256 boxes


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def frozen(a):
    a.flags.writeable = False
    return a


# ================================================================================================================= restatements
def sqdist(a, b):
    """[len(a), len(b)] squared distances, (dx*dx + dy*dy) + dz*dz with every operation rounded on its own (sqdist3d)"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    dx, dy, dz = (a[:, None, c] - b[None, :, c] for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def kth_distances(x, k, rows=None):
    """distance of every row (or of `rows`) to its k-th nearest point of x, the point itself included"""
    x = np.asarray(x, dtype=np.float64)
    rows = np.arange(len(x)) if rows is None else np.asarray(rows)
    out = np.empty(len(rows))
    for s in range(0, len(rows), 64):
        d2 = sqdist(x[rows[s:s + 64]], x)
        out[s:s + 64] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    return out


def k_of(n, quantile):
    """the k of the batched launch: (int)((double)n * quantile), at least 1"""
    return max(int(float(n) * quantile), 1)


def counts(x, h):
    return (np.sqrt(sqdist(x, x)) <= h).sum(0)


def greedy(x, attn, h, order, thrd_density, thrd_attn=0.7):
    """the loop of oracle/joints.py:nms_meanshift over a GIVEN visiting order; the neighbourhood's float32 maximum meets the float32
    threshold, as the kernel's `at > thrd_attn`. -> alive [n] bool"""
    n = len(x)
    near = np.sqrt(sqdist(x, x)) <= h
    attn = np.asarray(attn, dtype=np.float32).reshape(-1)
    alive = np.ones(n, dtype=bool)
    for i in order:
        if alive[i]:
            nbrs = near[:, i]
            attn_max = attn[nbrs].max()
            density = int(nbrs.sum()) / n
            alive[nbrs] = False
            if attn_max > np.float32(thrd_attn) or density > thrd_density:
                alive[i] = True
    return alive


def meanshift_sums(x, w, h):
    """the four sums of one step for every target: sum_i kk, sum_i kk x_i, ..., kk = max(h*h - d2, 0) * w_i -> (ax, ay, az, aw)"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    ww = np.ones(n) if w is None else np.asarray(w, dtype=np.float32).reshape(-1).astype(np.float64)
    h2 = h * h
    out = np.empty((4, n))
    for s in range(0, n, 512):
        kk = np.maximum(h2 - sqdist(x, x[s:s + 512]), 0.0) * ww[:, None]           # [source i, target j]
        out[3, s:s + 512] = kk.sum(0)
        for c in range(3):
            out[c, s:s + 512] = (kk * x[:, c:c + 1]).sum(0)
    return out


def meanshift_step(x, w, h):
    """one step in the device's form: den = aw + 1e-10, moved = 0.3 * (a / den - p) + p"""
    x = np.asarray(x, dtype=np.float64)
    ax, ay, az, aw = meanshift_sums(x, w, h)
    den = aw + 1e-10
    return np.stack([0.3 * (a / den - x[:, c]) + x[:, c] for c, a in enumerate((ax, ay, az))], axis=1)


def meanshift_path(x, w, h, max_iter):
    """-> (the points before every step and after the last, the rooted displacement of every step that ran)"""
    states, diffs = [np.array(x, dtype=np.float64)], []
    diff, it = 1e10, 1
    while diff > STOP and it < max_iter:
        moved = meanshift_step(states[-1], w, h)
        d = moved - states[-1]
        diff = float(np.sqrt((d * d).sum()))
        diffs.append(diff)
        states.append(moved)
        it += 1
    return states, diffs


def meanshift(x, w, h, max_iter):
    """meanshift_step looped with the reference's stop rule -> (modes, per-step diff)"""
    states, diffs = meanshift_path(x, w, h, max_iter)
    return states[-1], diffs


def inside(pts, vox, translate, scale, dims0):
    """the kernel's three IEEE operations, then round half to even -> keep [n] bool"""
    v = (np.asarray(pts, dtype=np.float64) - np.asarray(translate, dtype=np.float64)) / scale * dims0
    vc = np.round(v).astype(np.int64)
    in_grid = np.logical_and((vc >= 0).all(1), (vc < 88).all(1))
    vc = np.clip(vc, 0, 87)
    return np.logical_and(in_grid, np.asarray(vox, dtype=bool)[vc[:, 0], vc[:, 1], vc[:, 2]])


def voxel_coordinate(p, translate, scale, dims0):
    return (np.float64(p) - np.float64(translate)) / np.float64(scale) * np.float64(dims0)


# ========================================================================================================= control-flow models
def keys_of(x, row):
    """the radix keys of a row: the bit patterns of its squared distances"""
    return np.ascontiguousarray(sqdist(x[row:row + 1], x)[0]).view(np.uint64)


def model_kth4(keys, k):
    """control flow of kth_nn4_kernel for one row -> dict(path, pops, key). path: 'generic_lo' (need <= s_lo), 'generic_total'
    (need > total), 'list' (a selected bin of at most K4_LIST keys) or 'exhausted' (all five passes); pops: the population of the
    selected bin pass by pass; first_bin: the selected bin of pass 0"""
    u = np.uint64
    top = keys >> u(58)
    lo, cand, need = int((top < u(15)).sum()), keys[top == u(15)], k
    if need <= lo:
        return dict(path="generic_lo", pops=[], key=int(np.sort(keys)[k - 1]))
    need -= lo
    if need > len(cand):
        return dict(path="generic_total", pops=[], key=int(np.sort(keys)[k - 1]))
    pops, first_bin = [], None
    for p in range(5):
        shift, nbits = (46 - 12 * p, 12) if p < 4 else (0, 10)
        bins = ((cand >> u(shift)) & u((1 << nbits) - 1)).astype(np.int64)
        hist = np.bincount(bins, minlength=1 << nbits)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, need))
        need -= int(cum[b] - hist[b])
        pops.append(int(hist[b]))
        first_bin = b if p == 0 else first_bin
        cand = cand[bins == b]
        if p == 4:
            return dict(path="exhausted", pops=pops, first_bin=first_bin, key=int(cand[0]))
        if hist[b] <= K4_LIST:
            return dict(path="list", pops=pops, first_bin=first_bin, key=int(np.sort(cand)[need - 1]))


def model_kth1(keys, k):
    """control flow of kth_nn_kernel<true> for one row -> dict(stop, pop, pops, nlist, key): the pass it stops after, the population of
    the selected bin there (<= KTH_SMALL, or whatever is left after pass 0), of every pass before, and the length of the list"""
    cand, need, pops = keys, k, []
    for p in range(7, -1, -1):
        digit = ((cand >> np.uint64(8 * p)) & np.uint64(0xff)).astype(np.int64)
        hist = np.bincount(digit, minlength=256)
        b = 0
        while b < 255 and hist[b] < need:
            need -= int(hist[b])
            b += 1
        cand = cand[digit == b]
        pops.append(int(hist[b]))
        if p == 0 or hist[b] <= KTH_SMALL:
            m = min(len(cand), KTH_SMALL)
            return dict(stop=p, pop=int(hist[b]), pops=pops, nlist=len(cand), key=int(np.sort(cand)[:m][min(max(need - 1, 0), m - 1)]))


def sqrt_le_threshold(h):
    """the kernels' T: the largest double whose root is <= h, walked to from h * h"""
    T = np.float64(h) * np.float64(h)
    for _ in range(64):
        if not np.sqrt(T) > h:
            break
        T = np.nextafter(T, -np.inf)
    for _ in range(64):
        u = np.nextafter(T, np.inf)
        if not np.sqrt(u) <= h:
            break
        T = u
    return T


def greedy_walk(x, attn, h, order, thrd_density, thrd_attn=0.7):
    """nms_greedy_kernel's walk: the next living entry is looked for NMS_T order entries at a time -> (alive, the order index of every
    visit, the value of s at every skipped window)"""
    n = len(x)
    near = np.sqrt(sqdist(x, x)) <= h
    attn = np.asarray(attn, dtype=np.float32).reshape(-1)
    alive = np.ones(n, dtype=bool)
    visits, skips, s = [], [], 0
    while s < n:
        window = alive[order[s:s + NMS_T]]
        if not window.any():
            skips.append(s)
            s += NMS_T
            continue
        s += int(np.argmax(window))
        i = order[s]
        nbrs = near[:, i]
        alive[nbrs] = False
        if attn[nbrs].max() > np.float32(thrd_attn) or int(nbrs.sum()) / n > thrd_density:
            alive[i] = True
        visits.append(s)
        s += 1
    return alive, visits, skips


def morton_keys(x):
    """morton_keys_kernel without the mesh bits: 10 bits per axis of (x + 2) * 256, clamped"""
    q = np.clip((np.asarray(x, dtype=np.float64) + 2.0) * 256.0, 0.0, 1023.0).astype(np.int64)
    key = np.zeros(len(q), dtype=np.int64)
    for bit in range(10):
        for a in range(3):
            key |= ((q[:, a] >> bit) & 1) << (3 * bit + a)
    return key


def near_boxes(x, h):
    """the box test of meanshift_step_box_kernel on the Morton-sorted set -> bool [n_boxes target, n_boxes source]"""
    xs = np.asarray(x)[np.argsort(morton_keys(x), kind="stable")]
    nb = (len(xs) + MSB - 1) // MSB
    pad = np.concatenate([xs, np.repeat(xs[-1:], nb * MSB - len(xs), axis=0)]).reshape(nb, MSB, 3)
    lo, hi = pad.min(1), pad.max(1)
    g = np.maximum(np.maximum(lo[None, :, :] - hi[:, None, :], lo[:, None, :] - hi[None, :, :]), 0.0)
    return (g * g).sum(2) <= h * h


# ================================================================================================================== selection
def _cloud(seed, n, scale=0.1):
    """normal cloud whose second quarter mirrors the first (x -> -x): pairs of equal distances, as the product's mirrored sets have"""
    x = np.random.default_rng(seed).normal(0.0, scale, (n, 3))
    q = n // 4
    x[q:2 * q] = x[:q] * np.array([-1.0, 1.0, 1.0])
    return x


def _shell():
    """102 lattice points at squared distance exactly 81/256 from the origin: the six axis points, then the sign flips of the
    permutations of (1, 4, 8), (4, 4, 7), (3, 6, 6), all over 16: dyadic, so every product and sum of sqdist is exact"""
    out = []
    for base in ((9, 0, 0), (1, 4, 8), (4, 4, 7), (3, 6, 6)):
        pts = {tuple(a * b for a, b in zip(perm, sg)) for perm in itertools.permutations(base) for sg in itertools.product((1, -1), repeat=3)}
        out += sorted(pts)
    return np.array(out, dtype=np.float64) / 16.0


CENTRE = np.array([0.25, -0.125, 0.5])
TIE_D2 = 81.0 / 256.0


def _tie_set(m, others):
    """row 0 = CENTRE, m points at squared distance TIE_D2 from it, then `others`"""
    return np.concatenate([CENTRE[None], CENTRE + _shell()[:m], CENTRE + np.asarray(others, dtype=np.float64)])


def _near_set(m, step, others, seed):
    """row 0 = CENTRE, m points on its x axis at DISTINCT squared distances TIE_D2 * (1 + i * step)^2, shuffled, then `others`"""
    s = 0.5625 * (1.0 + np.random.default_rng(seed).permutation(m) * step)
    return np.concatenate([CENTRE[None], CENTRE + np.stack([s, np.zeros(m), np.zeros(m)], 1), CENTRE + np.asarray(others, dtype=np.float64)])


def _quantile_for(n, k):
    """a quantile the batched launch turns into k"""
    q = (k + 0.5) / n
    assert k_of(n, q) == k
    return q


def _select(name, aim, x, ks, qs=None, rows=None, **more):
    n = len(x)
    ks = sorted({k for k in ks if 1 <= k <= n})
    qs = [_quantile_for(n, k) for k in ks] if qs is None else list(qs)
    return dict(name=name, aim=aim, x=frozen(np.ascontiguousarray(x, dtype=np.float64)), ks=ks, qs=qs, rows=rows,
                max_n_one_row=ONE_ROW_MAX_N, **more)


@functools.lru_cache(maxsize=None)
def select_cases():
    """One point set per case; `ks` go through the one-set launch (morig_knn_bandwidth), `qs` through the batched one with
    max_n = n (kth_nn4_kernel) and with max_n = max_n_one_row = 65536 (kth_nn_kernel<true>, blocks past the set's end return at once).
      n1 .. n513     K4_R = 4: sizes with n % 4 in {0, 1, 2, 3} (rows past the end shadow the last row), one workgroup and several; the
                     256-thread stride over the candidates at 255, 256, 257, 513; k in {1, 2, n}, quantiles 0.0, 0.04, 1.0
      tie64, tie65   K4_LIST = 64: row 0's selected bin of pass 0 holds exactly 64 / 65 bit-identical keys, k inside the tie: 64 takes the
                     list pass, 65 takes all five histogram passes
      small8, small9 KTH_SMALL = 8 (one-row kernel): 8 identical keys stop the passes early with a full list; 9 identical keys never
                     reach <= KTH_SMALL, stop after pass 0 and overflow the list (all equal)
      bin64, bin65   K4_LIST with DISTINCT keys: 64 / 65 different squared distances inside one bin of pass 0 (a full list ranked by 64
                     lanes; 65 need a second histogram pass before the list), k at the first, the middle, the last two of the bin
      near8, near9   KTH_SMALL with distinct keys: 8 / 9 squared distances that differ only in their low three bytes: 8 stop the passes
                     with a full list that has to be sorted, 9 share a bin once and must NOT stop there
      coincident20   every key 0: generic passes in kth_nn4_kernel (need <= s_lo), pass 0 stop with 20 > KTH_SMALL keys in the one-row kernel
      mixed          one workgroup with rows in three states: row 0 has 5 coincident points and k <= 5 (need <= s_lo -> generic), row 1 lies
                     1000 x outside the set (need > total -> generic), rows 2 and 3 select in the histogram
      x1000, x1e-10  whole sets above / below pass 0's range: keys whose top six bits are 0b001111, squared distances in [2^-63, 2)
      x1e-6          squared distances near 2^-46: still inside that range (the kernel's comment used to say [2^-31, 2))
      full16         65 535 points, the largest set of kth_nn4_kernel: row 0's bin holds 65 534 keys in a 16-bit half whose word row 1
                     shares; rows 0..7 and every 977th are checked"""
    cases = []
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 513):
        cases.append(_select(f"n{n}", "K4_R rows per workgroup, 256-thread stride", _cloud(100 + n, n), (1, 2, n), qs=(0.0, 0.04, 1.0)))
    nearer = [(1 / 16, 0, 0), (0, 2 / 16, 0), (0, 0, 3 / 16)]
    farther = [(12 / 16, 0, 0), (0, 13 / 16, 0), (0, 0, 14 / 16), (1, 0, 0), (0, 1, 1 / 16)]
    for m in (64, 65):
        cases.append(_select(f"tie{m}", "K4_LIST", _tie_set(m, nearer + farther), (5, 4 + m // 2, 4 + m, 5 + m), tie=m, tie_k=4 + m // 2))
    rng = np.random.default_rng(7)
    for m in (8, 9):
        x = _tie_set(m, rng.normal(0.0, 0.4, (16, 3)))
        below = int((sqdist(x[:1], x)[0] < TIE_D2).sum())                                # the point itself and the nearer others
        cases.append(_select(f"small{m}", "KTH_SMALL", x, (below + 1, below + m // 2, below + m), tie=m, tie_k=below + m // 2))
    for m in (64, 65):                                                                     # 2 * 65 * 2^-14 < 1 / 64: one bin of pass 0
        cases.append(_select(f"bin{m}", "K4_LIST, distinct keys", _near_set(m, 2.0 ** -14, nearer + farther, m), (5, 4 + m // 2, 3 + m, 4 + m), near=m))
    for m in (8, 9):                                                                       # distinct in their low 3 bytes only
        x = _near_set(m, 2.0 ** -30, rng.normal(0.0, 0.4, (16, 3)), m)
        below = int((sqdist(x[:1], x)[0] < TIE_D2).sum())
        cases.append(_select(f"near{m}", "KTH_SMALL, distinct keys", x, (below + 1, below + m // 2, below + m - 1, below + m), near=m, below=below))
    cases.append(_select("coincident20", "all keys equal", np.tile(CENTRE, (20, 1)), (1, 8, 9, 20), qs=(0.0, 0.475, 1.0)))
    x = _cloud(31, 40)
    x[4:8] = x[0]
    x[1] *= 1000.0
    cases.append(_select("mixed", "s_lo / need > total hand-off next to selecting rows", x, (2, 4, 5)))
    cases.append(_select("x1000", "above pass 0's range", _cloud(32, 37) * 1000.0, (1, 2, 19), qs=(0.04, 0.5)))
    cases.append(_select("x1e-6", "low bins of pass 0", _cloud(33, 37) * 1e-6, (1, 2, 19), qs=(0.04, 0.5)))
    cases.append(_select("x1e-10", "below pass 0's range", _cloud(34, 37) * 1e-10, (1, 2, 19), qs=(0.04, 0.5)))
    axis6 = 0.5 * np.concatenate([np.eye(3), -np.eye(3)])
    x = np.concatenate([np.zeros((1, 3)), axis6[np.arange(65534) % 6]])
    rows = np.unique(np.concatenate([np.arange(8), np.arange(0, 65535, 977)]))
    cases.append(_select("full16", "16-bit bin halves", x, (5,), qs=(0.5,), rows=rows))
    return tuple(cases)


SELECT_RAGGED = (0, 1, 4, 0, 5, 3, 0)


@functools.lru_cache(maxsize=None)
def select_ragged():
    """empty sets in front of, between and behind the others (mesh_range); quantiles 0.0, 0.04, 0.5, 1.0"""
    return dict(sizes=SELECT_RAGGED, sets=tuple(frozen(_cloud(200 + b, n)) for b, n in enumerate(SELECT_RAGGED)), qs=(0.0, 0.04, 0.5, 1.0))


def bandwidth_bound(kth):
    """(the correctly rounded mean of the k-th distances, n * 2^-53 * it): any summation order of n non-negative terms stays inside"""
    want = math.fsum(kth.tolist()) / len(kth)
    return want, len(kth) * 2.0 ** -53 * want


# ===================================================================================================================== counts
COUNT_SIZES = (1, 31, 32, 33, 255, 256, 257, 513)
COUNT_RAGGED = (0, 1, 32, 0, 33, 31, 0)


def _count_set(seed, n):
    """random in the unit box, the second half in tight clusters as modes are, rows 0 and 1 coincident -> (x, the four bandwidths:
    a rooted distance d of row 0 that occurs and whose square rounds BELOW the squared distance, so that T = h * h alone would drop the
    pair and sqrt_le_threshold has to walk up; the doubles below and above d; and 0.0)"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3))
    m = n // 2
    if m:
        c = x[:max(n // 16, 1)]
        x[n - m:] = c[rng.integers(0, len(c), m)] + rng.normal(0.0, 1e-3, (m, 3))
    if n >= 2:
        x[1] = x[0]
    d2 = np.sort(sqdist(x[:1], x)[0])[min(n - 1, 7):]
    root = np.sqrt(d2)
    d = float(root[np.argmax(root * root < d2)])                  # the first one that h * h alone would miss (none: the first)
    return frozen(x), (d, float(np.nextafter(d, 0.0)), float(np.nextafter(d, np.inf)), 0.0)


@functools.lru_cache(maxsize=None)
def count_cases():
    """nms_counts_kernel (256 targets per workgroup, 256 sources per LDS tile: sizes either side of 256 and 512) and
    nms_counts_box_kernel (MSB = 32 targets and sources per box: sizes either side of 32), at the four bandwidths that decide
    sqrt_le_threshold: d itself (equality counts), one ulp below (that pair drops out), one ulp above, and 0.0 on coincident points"""
    out = []
    for n in COUNT_SIZES:
        x, hs = _count_set(300 + n, n)
        out.append(dict(name=f"n{n}", aim="256 / MSB tails, sqrt_le_threshold", x=x, hs=hs))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def count_ragged():
    sets, hs = zip(*[_count_set(400 + b, n) if n else (frozen(np.zeros((0, 3))), (0.0,) * 4) for b, n in enumerate(COUNT_RAGGED)])
    return dict(sizes=COUNT_RAGGED, sets=sets, hs=tuple(tuple(h[j] for h in hs) for j in range(4)))


# ===================================================================================================================== greedy
GREEDY_RAGGED = (0, 1, 64, 0, 1025, 63, 0)
GREEDY_NAMES = ("n1", "n63", "n64", "n65", "n1023", "n1024", "n1025", "skip2100", "attn_equal", "density_equal", "density_above")
ATTN_AT = np.float32(0.7)
ATTN_ABOVE = np.nextafter(np.float32(0.7), np.float32(1.0))


def _orders(x, h, seed):
    first = O.nms_order(counts(x, h))
    return dict(nms=frozen(np.ascontiguousarray(first)), perm=frozen(np.random.default_rng(seed).permutation(len(x))),
                rev=frozen(np.ascontiguousarray(first[::-1])))


def _modes_like(seed, n, h):
    """points in clusters tighter than the bandwidth around n // 30 + 1 centres, float32 attention"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.4, 0.4, (n // 30 + 1, 3))
    x = c[rng.integers(0, len(c), n)] + rng.normal(0.0, h / 5.0, (n, 3))
    return x, (rng.random(n) ** 2).astype(np.float32)


def _greedy(name, aim, x, attn, h, thrd_density, seed):
    return dict(name=name, aim=aim, x=frozen(np.ascontiguousarray(x)), attn=frozen(np.asarray(attn, dtype=np.float32)), h=float(h),
                thrd_density=thrd_density, thrd_attn=0.7, orders=_orders(x, h, seed))


@functools.lru_cache(maxsize=None)
def greedy_cases():
    """nms_greedy_kernel, one workgroup of NMS_T = 1024 threads, each order (numpy's nms_order, a fixed permutation, the reverse):
      n1 .. n1025    n either side of a wave (64) and of NMS_T: one look-ahead window and two, the strided loops over the points
      skip2100       one cluster of 1100 points inside the bandwidth of the first visited point, then isolated points: after visit 0 the
                     order entries 1 .. 1024 are all dead -> `first == NMS_T`, s += NMS_T (with the `nms` order)
      attn_equal     thrd_density = 1, so only `at > thrd_attn` restores: a neighbourhood maximum of exactly float32(0.7) does not, the
                     next float32 does
      density_equal  n = 50 isolated points, thrd_density = 0.02: 1 / 50 > 0.02 is false, nobody survives
      density_above  n = 50 in coincident pairs: 2 / 50 > 0.02, the visited point of every pair survives"""
    out = []
    for n in (1, 63, 64, 65, 1023, 1024, 1025):
        x, attn = _modes_like(500 + n, n, 0.05)
        out.append(_greedy(f"n{n}", "64 / NMS_T tails", x, attn, 0.05, 0.02, n))
    rng = np.random.default_rng(21)
    lattice = 0.1 * np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing="ij"), -1).reshape(-1, 3)        # 1000 points 0.1 apart
    cluster = np.array([-0.5, -0.5, -0.5]) + rng.uniform(-0.01, 0.01, (1100, 3))                         # diameter < 0.035 < h
    x = np.concatenate([cluster, lattice])[rng.permutation(2100)]
    out.append(_greedy("skip2100", "first == NMS_T", x, (0.69 * rng.random(2100)).astype(np.float32), 0.05, 0.02, 22))
    c = np.array([[-0.5, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]])
    x = np.repeat(c, 10, axis=0) + rng.uniform(-0.005, 0.005, (40, 3))
    attn = (0.5 * rng.random(40)).astype(np.float32)
    attn[3], attn[17] = ATTN_AT, ATTN_ABOVE
    out.append(_greedy("attn_equal", "at > thrd_attn at equality", x, attn, 0.05, 1.0, 23))
    iso = 0.1 * np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(2), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    out.append(_greedy("density_equal", "ct / n > thrd_density at equality", iso, np.full(50, 0.1, np.float32), 0.05, 0.02, 24))
    out.append(_greedy("density_above", "ct / n > thrd_density", np.repeat(iso[:25], 2, axis=0), np.full(50, 0.1, np.float32), 0.05, 0.02, 25))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def greedy_ragged():
    """sizes either side of 64 and NMS_T next to empty meshes, a bandwidth per mesh"""
    hs = (0.05, 0.03, 0.05, 0.05, 0.04, 0.06, 0.05)
    ms = []
    for b, n in enumerate(GREEDY_RAGGED):
        x, attn = _modes_like(600 + b, n, hs[b]) if n else (np.zeros((0, 3)), np.zeros(0, np.float32))
        ms.append(_greedy(f"mesh{b}", "mesh_range", x, attn, hs[b], 0.02, 700 + b))
    return dict(sizes=GREEDY_RAGGED, meshes=tuple(ms), thrd_density=0.02, thrd_attn=0.7)


# ================================================================================================================= mean-shift
LATTICE_H = 0.25


def _lattice_set(seed, n, weights):
    """coordinates k / 64 in [-1, 1], clustered so that points meet inside h = 0.25 (16 lattice steps); weights None, float32 multiples
    of 1/8 in [0, 1] with zeros among them, or all 0"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-52, 53, (n // 24 + 1, 3))
    steps = np.clip(c[rng.integers(0, len(c), n)] + rng.integers(-12, 13, (n, 3)), -64, 64)
    w = {"none": None, "eighths": (rng.integers(0, 9, n) / 8.0).astype(np.float32), "zero": np.zeros(n, np.float32)}[weights]
    return frozen(steps / 64.0), w


def lattice_sums_int(x, w):
    """the four sums of meanshift_sums on the scaled lattice in integer arithmetic: coordinates in 1/64, kk in 2^-12 (h*h = 256), weights
    in 1/8 -> (ax, ay, az in units of 2^-21, aw in units of 2^-15, the largest sum of |terms| in units of 2^-21)"""
    X = np.rint(np.asarray(x) * 64.0).astype(np.int64)
    assert np.array_equal(X / 64.0, x)
    W = np.full(len(X), 8, np.int64) if w is None else np.rint(np.asarray(w, dtype=np.float64) * 8.0).astype(np.int64)
    assert w is None or np.array_equal(W / 8.0, np.asarray(w, dtype=np.float64))
    out, worst = np.empty((4, len(X)), dtype=np.int64), 0
    for s in range(0, len(X), 512):
        d = X[:, None, :] - X[None, s:s + 512, :]
        kk = np.maximum(256 - (d * d).sum(2), 0) * W[:, None]
        out[3, s:s + 512] = kk.sum(0)
        for c in range(3):
            out[c, s:s + 512] = (kk * X[:, c:c + 1]).sum(0)
        worst = max(worst, int((kk * 64).sum(0).max()))
    return out, worst


@functools.lru_cache(maxsize=None)
def lattice_cases():
    """max_iter = 2 (one step) on sets where every product and every partial sum is exact in any order, so meanshift_step_kernel,
    meanshift_step_box_kernel and meanshift_step agree bit for bit: tails n % MS_TGT and n % MS_TILE (dead lanes of the last target block,
    a last source tile of 1, 31, 33 ... sources, the 8 slices of MS_TGT sources partly or wholly empty), MSB = 32 points per box with 1 to
    257 boxes (8194 points: a second chunk of 256 boxes, one box in it), zero weights, one set whose weights are all 0"""
    out = []
    for i, n in enumerate(SMALL_SIZES + (BIG,)):
        kind = "eighths" if (i % 2 or n == BIG) else "none"
        x, w = _lattice_set(800 + n, n, kind)
        out.append(dict(name=f"lattice{n}_{kind}", aim="MS_TGT / MS_TILE / MSB tails", x=x, w=w, h=LATTICE_H, max_iter=2))
    x, w = _lattice_set(799, 65, "zero")
    out.append(dict(name="lattice65_zero", aim="den = 1e-10", x=x, w=w, h=LATTICE_H, max_iter=2))
    return tuple(out)


def _generic_set(seed, n, h, max_iter, spread=0.03):
    """clustered random set with float32 weights whose restated diff stays STOP_MARGIN away from STOP at every step (the device adds the
    displacements atomically: the last bits of its diff depend on the arrival order); otherwise the next seed"""
    while True:
        rng = np.random.default_rng(seed)
        c = rng.uniform(-0.4, 0.4, (n // 30 + 1, 3))
        x = c[rng.integers(0, len(c), n)] + rng.normal(0.0, spread, (n, 3))
        w = (rng.random(n) ** 2).astype(np.float32)
        states, diffs = meanshift_path(x, w, h, max_iter)
        if all(abs(d - STOP) > STOP_MARGIN for d in diffs):
            return dict(x=frozen(x), w=frozen(w), h=float(h), states=states, diffs=diffs)
        seed += 1000


def modes_at(m, max_iter):
    """the restated result of a mesh for a max_iter up to the one its path was made with"""
    return m["states"][min(max_iter - 1, len(m["states"]) - 1)]


GENERIC_NAMES = tuple(f"n{n}" for n in SMALL_SIZES + (BIG,)) + ("stop_pair", "ragged", "ragged_big")
RAGGED_BIG = (257, 8225, 40)


@functools.lru_cache(maxsize=None)
def generic_case(name):
    """Batches of clustered sets with weights; every mesh carries its restated path, so each max_iter reads its result from it.
      n1 .. n513     one mesh per case at the tail sizes (MS_TGT, MS_TILE, MSB), max_iter in {1, 2, 3, 12}: pass-through, one step, two
                     steps (the second box buffer), eleven
      n8194          257 boxes, one step
      stop_pair      a tight set with a generous bandwidth that converges after a few steps, batched with a set that runs all eleven: the
                     per-mesh pass-through of the converged mesh while its neighbour goes on
      ragged         (0, 1, 32, 0, 33, 31, 0): empty meshes in front, between, behind (mesh_range, segment_of in the Morton keys)
      ragged_big     (257, 8225, 40), max_iter 3: two chunks of 256 boxes and both box buffers next to small meshes"""
    if name == "stop_pair":
        return dict(name=name, aim="pass-through after convergence",
                    meshes=(_generic_set(950, 29, 10.0, 12, spread=0.002), _generic_set(951, 257, 0.08, 12)), max_iters=(12,))
    if name == "ragged":
        empty = dict(x=frozen(np.zeros((0, 3))), w=frozen(np.zeros(0, np.float32)), h=0.08, states=[np.zeros((0, 3))], diffs=[])
        return dict(name=name, aim="mesh_range, segment_of",
                    meshes=tuple(_generic_set(960 + b, n, 0.08, 12) if n else empty for b, n in enumerate(COUNT_RAGGED)), max_iters=(1, 2, 3, 12))
    if name == "ragged_big":
        return dict(name=name, aim="256-box chunks, second box buffer",
                    meshes=tuple(_generic_set(970 + b, n, 0.08, 3) for b, n in enumerate(RAGGED_BIG)), max_iters=(3,))
    n = int(name[1:])
    if n == BIG:
        return dict(name=name, aim="more than 256 boxes", meshes=(_generic_set(900 + BIG, BIG, 0.08, 2),), max_iters=(2,))
    return dict(name=name, aim="MS_TGT / MS_TILE / MSB tails", meshes=(_generic_set(900 + n, n, 0.08, 12),), max_iters=(1, 2, 3, 12))


def generic_cases():
    return tuple(generic_case(name) for name in GENERIC_NAMES)


# ================================================================================================================ inside test
EXACT_TRANSLATE, EXACT_SCALE, EXACT_DIMS0 = (0.0, 0.0, 0.0), 0.6875, 88
INSIDE_SIZES = (1, 255, 256, 257)
MID_EVEN, MID_ODD = (40, 40), (40, 41)          # the other two axes sit mid-voxel; their cell sum decides which cells of the line are filled
# v on the tested axis, the cell a correct rint gives, the cell a wrong rounding (or a forgotten grid test) would read
INSIDE_EDGES = ((-0.5, 0, -1), (-0.5 - 2.0 ** -40, -1, 0), (0.5, 0, 1), (1.5, 2, 1), (2.5, 2, 3), (86.5, 86, 87),
                (float(np.nextafter(87.5, 0.0)), 87, 88), (87.5, 88, 87), (88.0, 88, 87), (-1.0, -1, 0), (1e15, 10 ** 15, 87))


def checker_grid():
    """filled where i + j + k is even: the two cells a half could round to always differ"""
    i, j, k = np.meshgrid(*[np.arange(88)] * 3, indexing="ij")
    return frozen((i + j + k) % 2 == 0)


def cell_value(vox, cell, mid):
    """what a point whose tested axis lands in `cell` (the other two in `mid`) must answer"""
    return bool(0 <= cell < 88 and vox[cell, mid[0], mid[1]])


def _coordinate_for(v):
    """a coordinate p whose voxel coordinate (p - 0) / 0.6875 * 88 is v exactly: v / 128, or a neighbouring double"""
    p = np.float64(v) / 128.0
    for _ in range(8):
        got = voxel_coordinate(p, 0.0, EXACT_SCALE, EXACT_DIMS0)
        if got == v:
            return float(p)
        p = np.nextafter(p, np.inf if got < v else -np.inf)
    return None


@functools.lru_cache(maxsize=None)
def inside_edge_table():
    """-> rows of (point, axis, v, right cell, wrong cell, mid cells). translate 0, scale 0.6875, dims0 88: v = p * 128. A v that no
    double p reaches exactly (the roundings of the division and the product decide) keeps the nearest reachable v on the same side of the
    half; the CPU test asserts which cell every row rounds to. The mid cells are chosen so that the right and the wrong cell answer
    differently in checker_grid()."""
    vox, rows = checker_grid(), []
    for v, right, wrong in INSIDE_EDGES:
        p = _coordinate_for(v)
        if p is None:
            p = float(np.float64(v) / 128.0)
            half = np.round(v * 2) / 2
            side = np.sign(v - half)
            while side != 0 and np.sign(voxel_coordinate(p, 0.0, EXACT_SCALE, EXACT_DIMS0) - half) != side:   # stay on v's side of the half
                p = float(np.nextafter(p, side * np.inf))
        mid = next(m for m in (MID_EVEN, MID_ODD) if cell_value(vox, right, m) != cell_value(vox, wrong, m))
        for axis in range(3):
            pt = np.empty(3)
            pt[axis] = p
            pt[[a for a in range(3) if a != axis]] = (np.array(mid) + 0.25) / 128.0
            rows.append((pt, axis, float(voxel_coordinate(p, 0.0, EXACT_SCALE, EXACT_DIMS0)), right, wrong, mid))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def inside_cases():
    """inside_check_kernel, 256 threads per workgroup, n in {1, 255, 256, 257}.
      exact_n        the 33 edge rows of inside_edge_table() first, then points whose voxel coordinates are random multiples of 0.5 in
                     [-2, 90] on every axis (halves and integers, in and out of the grid), in checker_grid()
      fixture_n      translate, scale and grid of the joints_small fixture: random points over and a little beyond the grid"""
    from conftest import load_golden
    rng = np.random.default_rng(41)
    edge = np.stack([r[0] for r in inside_edge_table()])
    halves = rng.integers(-4, 181, (257 - len(edge), 3)) / 256.0                          # v = p * 128 in steps of 0.5
    pool = np.concatenate([edge, halves])
    meta, a = load_golden("joints_small")
    vox = np.unpackbits(a["vox_data"].numpy())[:88 ** 3].reshape(88, 88, 88).astype(bool)
    t, s, d0 = [float(v) for v in meta["vox_translate"]], float(meta["vox_scale"]), int(meta["vox_dims"][0])
    filled = np.argwhere(vox)
    cells = filled[rng.integers(0, len(filled), 257)] + rng.uniform(-1.5, 1.5, (257, 3))    # around filled voxels: both answers occur
    fix = cells / d0 * s + np.array(t)
    out = []
    for n in INSIDE_SIZES:
        out.append(dict(name=f"exact_{n}", aim="rint on halves, grid bounds", pts=frozen(pool[:n].copy()), vox=checker_grid(),
                        translate=EXACT_TRANSLATE, scale=EXACT_SCALE, dims=(EXACT_DIMS0,) * 3))
        out.append(dict(name=f"fixture_{n}", aim="arbitrary translate and scale", pts=frozen(fix[:n].copy()), vox=frozen(vox), translate=tuple(t),
                        scale=s, dims=(d0,) * 3))
    return tuple(out)
