"""Cases for the train-mode backward operators (csrc/train_bwd.hip) at the sizes their kernels and their dispatch branch on: float64
restatements of the operators, a Python restatement of the dispatch arithmetic, two input families and the case tables that
tests/test_train_bwd_cases.py (CPU) and tests/test_train_bwd_differential.py (device) share. Not a test file; numpy only, no GPU.

The restatements are written from the operators' definitions (the header comment of train_bwd.hip), every one as a plain float64
expression over whole arrays; sums of float inputs are taken in extended precision. tests/test_train_bwd_cases.py holds them to
torch.autograd in float64 through oracle/nets.py.

Two input families:
  exact   every intermediate of the kernel is representable in float32 (and in the bf16 hi / lo pair where the operand is split), so a
          sum gives the same bits in any order and with or without fused multiply-adds; the bar is EQUALITY with the float64
          restatement rounded once to float32. GEMM: small integers ("int"), or one operand k/4 with 9-10 significant bits (its bf16
          split needs the lo half) against integers of at most 3 bits whose lo half is zero ("splitA": A needs lo, "splitB": B does);
          sum_r |a||b| stays below 2^24 grid units. Row passes: values on a quarter grid, mean / rstd / gamma / scale / shift powers of
          two or small integers; 1 / n enters the du passes, so the live row count is a power of two wherever the two BatchNorm sums
          are not zero. Edge scatter: integer gradients.
  float   seeded normals, the gradient columns spread over six decades; held to the bounds derived in the device file.

Out of scope: non-finite Z in segmax_affine_arg (the two kernels are not required to agree there), MORIG_TN_NO_BIG (read once per
process)."""
import functools
import zlib

import numpy as np

U = 2.0 ** -24                        # unit roundoff of float32
F32, F64 = np.float32, np.float64
MAX_OPERAND = 33000 * 260             # floats per operand of any case
SENTINEL = -77.25
GUARD = 3                             # guard rows behind / guard columns beside every output window


def cdiv(a, b):
    return -(-a // b)


def f64(x):
    return np.asarray(x, dtype=F64)


def once(x):
    """the float64 result rounded ONCE to float32"""
    return f64(x).astype(F32)


def is_f32(x):
    x = f64(x)
    return bool((x.astype(F32).astype(F64) == x).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def hp_sum(x):
    """column sums in extended precision, returned as float64"""
    return np.asarray(np.asarray(x, dtype=np.longdouble).sum(0), dtype=F64)


# ================================================================================================================= restatements
def gemm_tn(A, B, shift=None, rows=None):
    """A^T (B - 1 s^T) over the first `rows` rows"""
    A, B = f64(A)[:rows], f64(B)[:rows]
    if shift is not None:
        B = B - f64(shift)[None, :]
    return A.T @ B


def col_sums(dz, y=None, mean=None, rstd=None, rows=None, live=None):
    """(sum_r dz, sum_r dz * xhat) with xhat = (y - mean) * rstd; y None: (sum_r dz, None). live < 0 drops the entry of dz."""
    dz = f64(dz)[:rows]
    if live is not None:
        dz = np.where(np.asarray(live)[:rows] < 0, 0.0, dz)
    if y is None:
        return hp_sum(dz), None
    return hp_sum(dz), hp_sum(dz * xhat_of(f64(y)[:rows], mean, rstd))


def xhat_of(y, mean, rstd):
    return (f64(y) - f64(mean)[None, :]) * f64(rstd)[None, :]


def du_terms(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, n):
    """the parts of du = gamma rstd (dz - sum_dz / n - xhat sum_dzx / n), each as the kernel forms it (for the exactness check and for
    the float bound)"""
    inv_n = 1.0 / n if n > 0 else 0.0
    t = dict(xh=xhat_of(y, mean, rstd), grs=f64(gamma) * f64(rstd), k0=f64(sum_dz) * inv_n, k1=f64(sum_dzx) * inv_n)
    t["p"] = t["xh"] * t["k1"][None, :]
    t["t1"] = f64(dz) - t["k0"][None, :]
    t["t2"] = t["t1"] - t["p"]
    t["d"] = t["grs"][None, :] * t["t2"]
    return t


def bn_relu_du(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, rows=None, want_sum=False):
    """du = [y > 0] gamma rstd (dz - sum_dz / n - xhat sum_dzx / n) over the first n = `rows` rows (+ its column sums)"""
    dz, y = f64(dz)[:rows], f64(y)[:rows]
    du = np.where(y > 0, du_terms(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, len(dz))["d"], 0.0)
    return (du, hp_sum(du)) if want_sum else du


def du_bound(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, n, c=8):
    """c 2^-24 |gamma rstd| (|dz| + |sum_dz| / n + |xhat| |sum_dzx| / n), (1 + c u) for the second-order terms"""
    t = du_terms(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, n)
    return c * U * (1 + c * U) * np.abs(t["grs"])[None, :] * (np.abs(f64(dz)) + np.abs(t["k0"])[None, :] + np.abs(t["p"]))


def segments_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)).astype(np.int32)


def segmax_affine_arg(Z, rowptr, scale=None, shift=None, first=True):
    """per (segment, column): the largest w = z * scale + shift, the FIRST row that reaches it (first=False: the last, what `>=`
    in the serial walk would give), and that row's raw z. Empty segment: 0, -1, 0. -> (out float64, arg int32, zwin float32)"""
    Z32 = np.asarray(Z, dtype=F32)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n_seg, H = len(rowptr) - 1, Z32.shape[1]
    E = int(rowptr[-1])
    s = np.ones(H) if scale is None else f64(scale)
    sh = np.zeros(H) if shift is None else f64(shift)
    w = f64(Z32[:E]) * s[None, :] + sh[None, :]
    out, arg, zwin = np.zeros((n_seg, H)), np.full((n_seg, H), -1, np.int32), np.zeros((n_seg, H), F32)
    full = np.flatnonzero(np.diff(rowptr) > 0)
    if len(full):
        seg = segments_of(rowptr)
        m = np.full((n_seg, H), -np.inf)
        m[full] = np.maximum.reduceat(w, rowptr[full], axis=0)
        hit = w == m[seg]
        rows = np.arange(E)[:, None]
        if first:
            a = np.minimum.reduceat(np.where(hit, rows, E), rowptr[full], axis=0)
        else:
            a = np.maximum.reduceat(np.where(hit, rows, -1), rowptr[full], axis=0)
        arg[full] = a
        cols = np.arange(H)[None, :]
        out[full] = w[a, cols]                              # (the winner's own w: keeps its sign of zero)
        zwin[full] = Z32[a, cols]
    return out, arg, zwin


def segmax_stats_zwin(dout, arg, zwin, mean, rstd):
    """the two BatchNorm sums of the one-hot row gradient from the kept winners' values"""
    return col_sums(dout, zwin, mean, rstd, live=arg)


def segmax_stats_gather(dout, arg, Z, mean, rstd):
    """the same with the winners' rows gathered from Z"""
    arg = np.asarray(arg)
    zsel = f64(Z)[np.maximum(arg, 0), np.arange(arg.shape[1])[None, :]]
    return col_sums(dout, np.where(arg < 0, 0.0, zsel), mean, rstd, live=arg)


def segmax_bn_relu_du(dout, arg, Z, rowptr, mean, rstd, gamma, sum_dz, sum_dzx, capacity, relu=True):
    """du[e] of every row of every segment from the one-hot gradient dz[arg[v][c]][c] = dout[v][c]; rows [E, capacity) are zero.
    -> (du [capacity, cols], column sums over the live rows)"""
    E = int(np.asarray(rowptr)[-1])
    seg = segments_of(rowptr)
    Zl = f64(Z)[:E]
    dz = np.where(np.asarray(arg)[seg] == np.arange(E)[:, None], f64(dout)[seg], 0.0)
    d = du_terms(dz, Zl, mean, rstd, gamma, sum_dz, sum_dzx, E)["d"]
    if relu:
        d = np.where(Zl > 0, d, 0.0)
    du = np.zeros((capacity, Zl.shape[1]))
    du[:E] = d
    return du, hp_sum(d), dz


def edge_scatter(dG, rowptr, src, n_src):
    """dA[v] = sum of dG over the edges into v, dB[u] = over the edges out of u"""
    E = int(np.asarray(rowptr)[-1])
    g = f64(dG)[:E]
    dA, dB = np.zeros((len(rowptr) - 1, g.shape[1])), np.zeros((n_src, g.shape[1]))
    np.add.at(dA, segments_of(rowptr), g)
    np.add.at(dB, np.asarray(src)[:E], g)
    return dA, dB


def edge_relu_sum(ZA, ZB, rowptr, src):
    """Y[e] = relu(ZA[dst e] + ZB[src e]): a float32 sum of two float32 (what the forward stored), returned as float64"""
    E = int(np.asarray(rowptr)[-1])
    return f64(np.maximum(f64(ZA)[segments_of(rowptr)] + f64(ZB)[np.asarray(src)[:E]], 0.0).astype(F32))


def edge_bn_scatter(dG, rowptr, src, n_src, Y=None, mean=None, rstd=None, gamma=None, sum_dz=None, sum_dzx=None, ZA=None, ZB=None):
    """the three forms: mean None (plain scatter of dG), Y given, Y rebuilt as relu(ZA[dst] + ZB[src]). -> (dA, dB, d per edge)"""
    E = int(np.asarray(rowptr)[-1])
    d = f64(dG)[:E]
    if mean is not None:
        y = edge_relu_sum(ZA, ZB, rowptr, src) if ZA is not None else f64(Y)[:E]
        d = bn_relu_du(d, y, mean, rstd, gamma, sum_dz, sum_dzx)
    dA, dB = edge_scatter(d, rowptr, src, n_src)
    return dA, dB, d


def edge_bn_sums_from_products(M, db2, W2, mean, rstd):
    """sum_e dh = db2 W2 and sum_e dh xhat = rstd (sum_k W2 * M - mean sum_e dh) per column, dh = du2 W2, M = du2^T Z1"""
    a = hp_sum(f64(db2)[:, None] * f64(W2))
    b = hp_sum(f64(W2) * f64(M))
    return a, f64(rstd) * (b - f64(mean) * a)


# ================================================================================================================= dispatch
TN_T, TN_R, TN16_R = 128, 16, 32
GEMM_BRANCHES = ("small16", "small32", "tn16_128", "tn16_256", "f32_128", "reduce32", "reduce8", "small_vec", "small_scalar", "full",
                 "general", "moved_n", "moved_k", "skip_subtile", "vector", "scalar", "stage_tail", "full_stage_tail", "second_chunk")
SEGMAX_BRANCHES = ("long_v4", "long_v1", "short_v4", "short_v1")


def tn_chunks(rows, N, K):
    tiles = cdiv(N, TN_T) * cdiv(K, TN_T)
    chunks = min((512 if 4 < tiles <= 16 else 1024) // tiles, 512, cdiv(max(rows, 1), 128))
    return max(chunks, 1)


def gemm_workspace(rows, N, K):
    return tn_chunks(rows, N, K) * N * K


def gemm_plan(rows, N, K, bwd="default", a_vec=True, b_vec=True, no_small=False, live=None):
    """what morig_gemm_tn_shift launches for `rows` host rows (`live`: the device-side row count) -> dict(kernel, chunks, chunk_rows,
    reduce, branches)"""
    live = rows if live is None else live
    chunks = tn_chunks(rows, N, K)
    split16 = bwd != "f32" and rows >= TN16_R                       # fewer host rows than one stage of the split kernel: the exact kernel
    br = set()
    if N <= 32 and K <= 32 and not no_small:
        kernel = "small16" if (N <= 16 and K <= 16) else "small32"
        chunk_rows = cdiv(cdiv(max(rows, 1), chunks), 64) * 64
        br.add("small_vec" if (a_vec and b_vec and N % 4 == 0 and K % 4 == 0) else "small_scalar")
        stage, TT = 64, None
    else:
        stage = TN16_R if split16 else TN_R
        tiles_big = cdiv(N, 256) * cdiv(K, 256)
        chunks_big = min(chunks, max(1, 256 // tiles_big)) if tiles_big <= 256 else chunks
        if split16 and N >= 256 and K >= 256 and tiles_big * chunks_big >= 200:
            kernel, TT, chunks = "tn16_256", 256, chunks_big
        else:
            kernel, TT = ("tn16_128" if split16 else "f32_128"), 128
        chunk_rows = cdiv(cdiv(max(rows, 1), chunks), stage) * stage
    spans = [max(0, min((c + 1) * chunk_rows, live) - c * chunk_rows) for c in range(chunks)]
    if any(s % stage for s in spans):
        br.add("stage_tail")
    if chunks > 1 and spans[1] > 0:
        br.add("second_chunk")
    if TT is not None:
        br.add("vector" if (a_vec and b_vec) else "scalar")
        for n_own in range(0, N, TT):
            for k_own in range(0, K, TT):
                n0, k0 = n_own, k_own
                if split16:
                    if a_vec and N >= TT and N % 4 == 0 and n_own + TT > N:
                        n0 = N - TT
                        br.add("moved_n")
                    if b_vec and K >= TT and K % 4 == 0 and k_own + TT > K:
                        k0 = K - TT
                        br.add("moved_k")
                full = split16 and a_vec and b_vec and n0 + TT <= N and k0 + TT <= K
                br.add("full" if full else "general")
                if full and any(s % stage for s in spans):
                    br.add("full_stage_tail")
                if not full and (any(n0 + c >= N for c in range(0, TT, 32)) or any(k0 + c >= K for c in range(0, TT, 32))):
                    br.add("skip_subtile")
    br.add(kernel)
    reduce = 32 if chunks >= 64 else 8
    br.add(f"reduce{reduce}")
    return dict(kernel=kernel, chunks=chunks, chunk_rows=chunk_rows, reduce=reduce, branches=br, spans=spans)


def stats_slab_rows(rows_cap, cols):
    groups = cdiv(cols, 64)
    slabs = max(1024 // max(groups, 1), 64)
    r = (cdiv(max(rows_cap, 1), slabs) + 3) & ~3
    return max(r, 256)


def stats_plan(rows, cols):
    """-> (slab_rows, slabs, quads of the last column group)"""
    sr = stats_slab_rows(rows, cols)
    return sr, cdiv(max(rows, 1), sr), min(16, (cols - (cdiv(cols, 64) - 1) * 64 + 3) >> 2)


def segmax_plan(n_seg, H, v4):
    threads = n_seg * (H // (4 if v4 else 1))
    return ("long" if (threads < 32768 and n_seg <= 400) else "short") + ("_v4" if v4 else "_v1")


def window_v4(cols, ld, col0):
    """what vec4_ptr and `cols & 3` decide for a column window of a base that starts 16-byte aligned"""
    return cols % 4 == 0 and ld % 4 == 0 and col0 % 4 == 0


# ================================================================================================================= windows
def window(cols, mode):
    """(ld, col0) of a column window: "vec" 16-byte aligned with ld a multiple of 4, "odd" at an odd offset of a wider base"""
    if mode == "vec":
        return 4 + cdiv(cols, 4) * 4 + 4, 4
    return cols + 1 + GUARD + (cols % 2), 1                         # an odd ld as well


def in_window(a, mode, rows_extra=0, fill=np.nan):
    """`a` [rows, cols] placed in a `fill`-ed base -> (base float32, col0)"""
    a = np.asarray(a, dtype=F32)
    ld, col0 = window(a.shape[1], mode)
    base = np.full((a.shape[0] + rows_extra, ld), fill, dtype=F32)
    base[:a.shape[0], col0:col0 + a.shape[1]] = a
    return base, col0


# ================================================================================================================= GEMM cases
T128 = (33, 64, 65, 96, 97, 127, 128, 129, 130, 132)
R128 = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 128, 129, 257)
GEMM_FAMILIES = ("int", "splitA", "splitB", "float")


def _gcase(name, rows, N, K, want, group):
    return dict(name=name, rows=rows, N=N, K=K, want=want, group=group)


@functools.lru_cache(maxsize=None)
def gemm_cases():
    """every case names the kernel the default path must take (`want`; under MORIG_TRAIN_BWD=f32 the two MFMA split kernels become
    f32_128, and so they do below TN16_R = 32 host rows: the split kernel's tails shorter than a stage are reached through rows_dev) and, for the ones aimed at a branch inside a kernel, the branches (`must`, on 16-byte aligned operands, default path)"""
    cs = []
    for r, n, k in ((1, 1, 1), (63, 16, 16), (64, 16, 16), (65, 13, 16), (129, 16, 12)):
        cs.append(_gcase(f"small16_{r}x{n}x{k}", r, n, k, "small16", "small"))
    for r, n, k in ((200, 17, 16), (200, 16, 17), (200, 32, 32), (200, 29, 32)):
        cs.append(_gcase(f"small32_{r}x{n}x{k}", r, n, k, "small32", "small"))
    for r, n, k in ((200, 33, 32), (200, 32, 33)):
        cs.append(_gcase(f"past_small_{r}x{n}x{k}", r, n, k, "tn16_128", "past"))
    for i, n in enumerate(T128):
        for j, k in enumerate(T128):
            r = R128[(3 * i + j) % len(R128)]
            cs.append(_gcase(f"t128_{r}x{n}x{k}", r, n, k, "tn16_128" if r >= TN16_R else "f32_128", f"t128_N{n}"))
    big = [_gcase("t256_moved_full", 7168, 260, 260, "tn16_256", "big"), _gcase("t256_general", 7168, 258, 262, "tn16_256", "big"),
           _gcase("t256_one_tile", 25600, 256, 256, "tn16_256", "big"), _gcase("stay128_K255", 7168, 256, 255, "tn16_128", "big"),
           _gcase("stay128_32chunks", 4096, 256, 256, "tn16_128", "big"), _gcase("reduce32_64chunks", 8192, 16, 16, "small16", "big"),
           _gcase("reduce8_63chunks", 8064, 16, 16, "small16", "big")]
    big[0]["must"] = {"full", "moved_n", "moved_k", "reduce8"}
    big[1]["must"] = {"general", "skip_subtile"}
    big[2]["must"] = {"full", "reduce32"}
    big[5]["must"] = {"reduce32"}
    big[6]["must"] = {"reduce8"}
    for c in big:
        c["group"] = c["name"]                                          # (a test of its own each: the restated products take a second)
    for c in cs:
        if c["name"] == "small16_129x16x12":
            c["must"] = {"second_chunk", "stage_tail"}
        if c["name"].endswith("x132x132"):
            c["must"] = {"full", "moved_n", "moved_k"}
    return tuple(cs + big)


def gemm_groups():
    return tuple(dict.fromkeys(c["group"] for c in gemm_cases()))


def _split_range(rows):
    """(largest odd numerator k of the k/4 operand, largest integer of the other) with rows * k * b < 2^24 quarter units"""
    for kmax, bmax in ((1023, 7), (1023, 3), (1023, 1), (511, 1)):
        if rows * kmax * bmax < 2 ** 24:
            return kmax, bmax
    raise ValueError(f"{rows} rows: no exact split range")


def _quarters(rng, shape, kmax):
    """+-k/4 with k odd in [257, kmax]: 9-10 significant bits, so bf16(x) != x and the lo half carries the rest exactly"""
    k = 2 * rng.integers(128, (kmax - 1) // 2 + 1, size=shape) + 1
    return (np.where(rng.integers(0, 2, size=shape) == 1, -1.0, 1.0) * k / 4.0).astype(F32)


def gemm_inputs(case, family):
    """-> dict(A [rows, N], B [rows, K], shift [K], centred [rows, K], grid): float32 arrays. A call with b_shift is given B (the
    shift still in it), a call without is given `centred`; in the exact families B - shift == centred bit for bit."""
    rows, N, K = case["rows"], case["N"], case["K"]
    rng = np.random.default_rng([rows, N, K, GEMM_FAMILIES.index(family)])
    if family == "int":
        amax = max(1, min(7, (2 ** 24 - 1) // (rows * 10)))
        A = rng.integers(-amax, amax + 1, size=(rows, N)).astype(F32)
        Bc = rng.integers(-7, 8, size=(rows, K)).astype(F32)
        shift = rng.integers(-3, 4, size=K).astype(F32)
        grid = 1.0
    elif family in ("splitA", "splitB"):
        kmax, bmax = _split_range(rows)
        q = _quarters(rng, (rows, N if family == "splitA" else K), kmax)
        ints = rng.integers(-bmax, bmax + 1, size=(rows, K if family == "splitA" else N)).astype(F32)
        A, Bc = (q, ints) if family == "splitA" else (ints, q)
        shift = rng.integers(-2, 3, size=K).astype(F32)
        grid = 0.25
    else:
        A = (rng.standard_normal((rows, N)) * 10.0 ** np.linspace(-3, 3, N)[None, :]).astype(F32)
        Bc = (rng.standard_normal((rows, K)) * 10.0 ** np.linspace(3, -3, K)[None, :]).astype(F32)
        shift = (0.5 * 10.0 ** np.linspace(3, -3, K)).astype(F32)
        grid = None
    B = (Bc + shift[None, :]).astype(F32)                                  # exact families: B - shift gives Bc back exactly
    if grid is None:
        Bc = (B - shift[None, :]).astype(F32)                              # the float32 difference the kernel forms
    return dict(A=A, B=B, shift=shift, grid=grid, centred=Bc)


def gemm_exact_units(inp, with_shift):
    """max over the output of sum_r |a| |b| in units of the grid: below 2^24 every partial sum of any order is a float32"""
    b = f64(inp["B"]) - f64(inp["shift"])[None, :] if with_shift else f64(inp["centred"])
    return float((np.abs(f64(inp["A"])).T @ np.abs(b)).max()) / inp["grid"]


def bf16_needs_lo(x):
    """True where the nearest bf16 differs from x (8 significant bits are not enough)"""
    b = np.asarray(x, dtype=F32).view(np.uint32)
    return (b & 0xFFFF) != 0


# ================================================================================================================= row-pass cases
ROW_COLS = (1, 3, 4, 35, 63, 64, 65, 68, 130)
ROW_ROWS = (1, 255, 256, 257, 16384, 16385)
POW2 = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def pow2_below(n):
    return 1 << (max(n, 1).bit_length() - 1)


def _quarter(rng, shape, lim):
    """multiples of 1/4 in [-lim, lim]"""
    return (rng.integers(-4 * lim, 4 * lim + 1, size=shape) / 4.0).astype(F32)


def row_inputs(rows, cols, family):
    """operands of bn_backward_stats / bn_relu_backward: dz, y (a ReLU output: a third of it zero), mean, rstd, gamma and the two
    sums as GIVEN inputs of the du pass (`n_exact` rows: multiples of n_exact, so that sum / n is on the grid)"""
    rng = np.random.default_rng(1000 * rows + cols + (7 if family == "float" else 0))
    if family == "exact":
        dz = _quarter(rng, (rows, cols), 4)
        y = np.maximum(_quarter(rng, (rows, cols), 6) - 2.0, 0.0).astype(F32)
        mean = _quarter(rng, cols, 2)
        rstd = np.abs(rng.choice(POW2, size=cols)).astype(F32)
        gamma = (rng.choice(POW2, size=cols) * rng.choice([1.0, 3.0], size=cols)).astype(F32)
        q0, q1 = _quarter(rng, cols, 2), rng.choice(POW2, size=cols).astype(F32)
    else:
        dz = (rng.standard_normal((rows, cols)) * 10.0 ** np.linspace(-3, 3, cols)[None, :]).astype(F32)
        y = np.maximum(rng.standard_normal((rows, cols)) * 3.0 + 0.7, 0.0).astype(F32)
        mean = y.astype(F64).mean(0).astype(F32)
        rstd = (1.0 / np.sqrt(y.astype(F64).var(0) + 1e-5)).astype(F32)
        gamma = (rng.standard_normal(cols) + np.where(rng.integers(0, 2, cols) == 1, 1.5, -1.5)).astype(F32)
        q0 = q1 = None
    return dict(dz=dz, y=y, mean=mean, rstd=rstd, gamma=gamma, q0=q0, q1=q1)


def given_sums(inp, n, cols):
    """the sums handed to an exact du pass over n live rows: n * (grid values) when n is a power of two (1 / n is then exact and
    sum / n is the grid value), zero otherwise (the mean terms vanish identically)"""
    if n > 0 and n & (n - 1) == 0:
        return (n * inp["q0"][:cols]).astype(F32), (n * inp["q1"][:cols]).astype(F32)
    return np.zeros(cols, F32), np.zeros(cols, F32)


def du_is_exact(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, n):
    """every intermediate of the du expression is a float32, and so is 1 / n (unless both sums are zero: 0 * fl(1 / n) is 0)"""
    t = du_terms(dz, y, mean, rstd, gamma, sum_dz, sum_dzx, n)
    no_sums = not (np.any(sum_dz) or np.any(sum_dzx))
    return (no_sums or is_f32(1.0 / n if n else 0.0)) and all(is_f32(t[k]) for k in ("xh", "grs", "k0", "k1", "p", "t1", "t2", "d"))


def live_rows_of(rows):
    """the device-side live row counts a row case runs with (None: the host count)"""
    return tuple(dict.fromkeys([None, pow2_below(rows - 1) if rows > 1 else 0, rows // 3]))


# ---- segmented statistics: n_seg from ROW_ROWS, a table mixing empty, one-row and one long segment
def seg_table(n_seg, family):
    """lengths of n_seg segments: the pattern 1, 0, 1, 2, 0, 1 ... and ONE long segment in the middle; the exact family's total is a
    power of two (1 / E enters du)"""
    pat = np.array([1, 0, 1, 2, 0, 1, 0, 0, 3, 1])
    lens = pat[np.arange(n_seg) % len(pat)].astype(np.int64)
    if n_seg == 1:
        lens[:] = 4 if family == "exact" else 5
        return lens
    mid = n_seg // 2
    lens[mid] = 0
    rest = int(lens.sum())
    if family == "exact":
        total = 1 << (rest + 300).bit_length()
        lens[mid] = total - rest
    else:
        lens[mid] = 301
    return lens


def rowptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def seg_inputs(n_seg, cols, family):
    """Z (capacity rows, NaN behind the live ones), rowptr, seg_of_row, dout, BatchNorm terms; the arg table comes from the restated
    segmax_affine_arg under scale = gamma rstd, shift = -mean gamma rstd (the forward's max of the normalised values)"""
    rng = np.random.default_rng(77 * n_seg + cols + (3 if family == "float" else 0))
    lens = seg_table(n_seg, family)
    rowptr = rowptr_of(lens)
    E = int(rowptr[-1])
    cap = E + (0 if n_seg == 256 else 5)
    if family == "exact":
        Zl = _quarter(rng, (E, cols), 5)
        mean = _quarter(rng, cols, 2)
        rstd = np.abs(rng.choice(POW2, size=cols)).astype(F32)
        gamma = (rng.choice(POW2, size=cols) * rng.choice([1.0, 3.0], size=cols)).astype(F32)
        dout = _quarter(rng, (n_seg, cols), 4)
        sdz, sdzx = (E * _quarter(rng, cols, 2)).astype(F32), (E * rng.choice(POW2, size=cols)).astype(F32)
    else:
        Zl = (rng.standard_normal((E, cols)) * 2.0 + 0.3).astype(F32)
        mean = Zl.astype(F64).mean(0).astype(F32)
        rstd = (1.0 / np.sqrt(Zl.astype(F64).var(0) + 1e-5)).astype(F32)
        gamma = (rng.standard_normal(cols) + np.where(rng.integers(0, 2, cols) == 1, 1.5, -1.5)).astype(F32)
        dout = (rng.standard_normal((n_seg, cols)) * 10.0 ** np.linspace(-3, 3, cols)[None, :]).astype(F32)
        sdz = sdzx = None
    Z = np.full((cap, cols), np.nan, F32)
    Z[:E] = Zl
    grs = (f64(gamma) * f64(rstd))
    _, arg, zwin = segmax_affine_arg(Zl, rowptr, grs, -f64(mean) * grs)
    return dict(Z=Z, rowptr=rowptr, seg=segments_of(rowptr), E=E, cap=cap, dout=dout, mean=mean, rstd=rstd, gamma=gamma, arg=arg, zwin=zwin,
                sdz=sdz, sdzx=sdzx, lens=lens)


# ================================================================================================================= segmax_affine_arg cases
def seg_lengths(RL):
    return (0, 1, 2, RL - 1, RL, RL + 1, 4 * RL - 1, 4 * RL, 4 * RL + 1, 8 * RL + 3)


def _arg_case(name, n_seg, H, mode, lens, want, family="exact", ties=None, scale="pow2"):
    return dict(name=name, n_seg=n_seg, H=H, mode=mode, lens=np.asarray(lens, np.int64), want=want, family=family, ties=ties, scale=scale)


@functools.lru_cache(maxsize=None)
def arg_cases():
    """`mode` is the window of Z and out ("vec": V = 4 when H % 4 == 0; "odd": V = 1). `want` is the kernel the rule must pick."""
    short_pat = lambda n: np.array([0, 1, 2, 3, 1, 5])[np.arange(n) % 6]
    cs = [_arg_case("rule_400x324_long", 400, 324, "vec", short_pat(400), "long_v4"),
          _arg_case("rule_400x328_short", 400, 328, "vec", short_pat(400), "short_v4"),
          _arg_case("rule_401x16_short", 401, 16, "vec", short_pat(401), "short_v4"),
          _arg_case("rule_400x16_long", 400, 16, "vec", short_pat(400), "long_v4"),
          _arg_case("rule_400x81_long_v1", 400, 81, "vec", short_pat(400), "long_v1"),
          _arg_case("rule_400x83_short_v1", 400, 83, "vec", short_pat(400), "short_v1"),
          _arg_case("rule_401x16_short_window", 401, 16, "odd", short_pat(401), "short_v1")]
    for fam in ("exact", "float"):
        for sc in ("pow2", "none"):
            cs.append(_arg_case(f"lengths_RL64_H20_{fam}_{sc}", 10, 20, "vec", seg_lengths(64), "long_v4", fam, scale=sc))
            cs.append(_arg_case(f"lengths_RL16_H19_{fam}_{sc}", 10, 19, "vec", seg_lengths(16), "long_v1", fam, scale=sc))
        cs.append(_arg_case(f"lengths_RL16_H20_window_{fam}", 10, 20, "odd", seg_lengths(16), "long_v1", fam))
        cs.append(_arg_case(f"lengths_short_H20_{fam}", 401, 20, "vec", np.resize(seg_lengths(16), 401), "short_v4", fam))
        cs.append(_arg_case(f"lengths_short_H19_{fam}", 401, 19, "vec", np.resize(seg_lengths(16), 401), "short_v1", fam))
    for name, n_seg, H, mode, RL, want in (("ties_long_v4", 6, 20, "vec", 64, "long_v4"), ("ties_long_v1", 6, 19, "vec", 16, "long_v1"),
                                           ("ties_short_v4", 402, 20, "vec", 64, "short_v4"), ("ties_short_v1", 402, 19, "vec", 16, "short_v1")):
        cs.append(_arg_case(name, n_seg, H, mode, np.resize([4 * RL + 5] * 6, n_seg), want, ties=RL, scale="mixed"))
    return tuple(cs)


TIE_LAYOUTS = ("all_equal", "two_lanes", "one_lane_quad", "signed_zero", "negative_scale", "last_rows")


def arg_inputs(case):
    """float family: the first of eight seeds whose table has no near-tie (arg_margin above 16 float32 ulps)"""
    if case["family"] != "float":
        return _arg_inputs(case["name"], 0)
    for k in range(8):
        inp = _arg_inputs(case["name"], k)
        if arg_margin(inp) > 16 * 2.0 ** -23:
            return inp
    raise ValueError(case["name"])


@functools.lru_cache(maxsize=None)
def _arg_inputs(name, k):
    """Z [E, H], rowptr, scale, shift. Exact family: a quarter grid in [-4, 4] (ties everywhere: 33 values over up to 515 rows);
    scale a power of two of either sign, shift a small integer. Tie cases: segment s takes layout TIE_LAYOUTS[s % 6] around the lane
    count RL = case["ties"]:
      all_equal       every row the same value
      two_lanes       the maximum at rows 5 and RL + 9 of the segment (row lanes 5 and 9), below it elsewhere
      one_lane_quad   the maximum at rows 3 and 3 + 2 RL (the same lane, inside its first unrolled quadruple)
      signed_zero     -0.0 at row 2, +0.0 at row 7, negative elsewhere: w ties, the kept raw value tells which row won
      negative_scale  the MINIMUM of z twice (rows 1 and RL + 1) under a negative scale
      last_rows       the maximum at the last two rows (the tail loop behind the quadruples)"""
    case = next(c for c in arg_cases() if c["name"] == name)
    rng = np.random.default_rng([zlib.crc32(name.encode()), k])
    H, rowptr = case["H"], rowptr_of(case["lens"])
    E = int(rowptr[-1])
    if case["family"] == "float":
        Z = (rng.standard_normal((E, H)) * 3.0).astype(F32)
        scale = (rng.standard_normal(H) + np.where(rng.integers(0, 2, H) == 1, 1.5, -1.5)).astype(F32)
        shift = rng.standard_normal(H).astype(F32)
    else:
        Z = _quarter(rng, (E, H), 4)
        scale = rng.choice(POW2, size=H).astype(F32)
        shift = rng.integers(-3, 4, size=H).astype(F32)
    if case["ties"]:
        RL = case["ties"]
        scale = np.abs(scale)
        for s in range(case["n_seg"]):
            e0, e1 = int(rowptr[s]), int(rowptr[s + 1])
            lay = TIE_LAYOUTS[s % len(TIE_LAYOUTS)]
            seg = np.minimum(Z[e0:e1], 2.0)
            if lay == "all_equal":
                seg[:] = 1.25
            elif lay == "two_lanes":
                seg[[5, RL + 9]] = 3.5
            elif lay == "one_lane_quad":
                seg[[3, 3 + 2 * RL]] = 3.5
            elif lay == "signed_zero":
                seg[:] = -np.abs(seg) - 0.25
                seg[2], seg[7] = -0.0, 0.0
            elif lay == "negative_scale":
                seg[:] = np.maximum(seg, -2.0)
                seg[[1, RL + 1]] = -3.5
            else:
                seg[[-2, -1]] = 3.5
            Z[e0:e1] = seg
        # negative scales on the segments whose tie is a minimum of z: every column of this case walks every segment, so the sign is
        # per CASE column; the layouts that need a positive scale use even columns, negative_scale is checked on odd ones
        scale[1::2] *= -1.0
        shift = np.where(np.arange(H) % 4 < 2, shift, 0.0).astype(F32)
    if case["scale"] == "none":
        scale = shift = None
    return dict(Z=Z, rowptr=rowptr, scale=scale, shift=shift, E=E)


def tie_columns(layout, H):
    """the columns of a tie case on which `layout` is the winner's layout (positive scale: even columns, negative: odd)"""
    return np.arange(1 if layout == "negative_scale" else 0, H, 2)


def arg_margin(inp):
    """float family: the smallest gap between the best and the second best w of any (segment, column) with two rows or more, over
    |best| -- the arg table is decided by the inputs alone, fused multiply-add or not, once this is above a few float32 ulps"""
    Z, rowptr = f64(inp["Z"]), inp["rowptr"]
    s = 1.0 if inp["scale"] is None else f64(inp["scale"])[None, :]
    sh = 0.0 if inp["shift"] is None else f64(inp["shift"])[None, :]
    worst = np.inf
    for v in range(len(rowptr) - 1):
        e0, e1 = int(rowptr[v]), int(rowptr[v + 1])
        if e1 - e0 < 2:
            continue
        w = np.sort(Z[e0:e1] * s + sh, axis=0)
        mag = np.abs(Z[e0:e1] * s).max(0) + np.abs(sh)
        worst = min(worst, float(((w[-1] - w[-2]) / mag).min()))
    return worst


# ================================================================================================================= edge cases
EDGE_GRAPHS = ((1, 1), (64, 64), (65, 40), (40, 65), (300, 1))
EDGE_H = (1, 4, 33, 64)


@functools.lru_cache(maxsize=None)
def edge_graph(n_nodes, n_src, family="exact"):
    """a bipartite CSR by target: one vertex with 300 in-edges, every third vertex without in-edges, every fourth source without
    out-edges (where there is more than one), parallel edges allowed. The exact family has a power of two of edges (1 / E enters d).
    -> dict(rowptr, src, dst, E, cap)"""
    rng = np.random.default_rng(100 * n_nodes + n_src)
    lens = np.zeros(n_nodes, np.int64)
    hub = n_nodes // 2
    lens[hub] = 300
    for v in range(n_nodes):
        if v != hub and v % 3 != 0:
            lens[v] = 1 + (v % 5)
    total = int(lens.sum())
    if family == "exact":
        lens[hub] += (1 << total.bit_length()) - total
    E = int(lens.sum())
    allowed = np.array([u for u in range(n_src) if n_src == 1 or u % 4 != 3])
    src = rng.choice(allowed, size=E).astype(np.int32)
    cap = E + 7
    rowptr = rowptr_of(lens)
    dst = np.zeros(cap, np.int32)
    dst[:E] = segments_of(rowptr)
    srcc = np.zeros(cap, np.int32)
    srcc[:E] = src
    for a in (rowptr, srcc, dst):
        a.flags.writeable = False
    return dict(rowptr=rowptr, src=srcc, dst=dst, E=E, cap=cap, n_nodes=n_nodes, n_src=n_src, lens=lens)


def edge_inputs(n_nodes, n_src, H, family):
    g = edge_graph(n_nodes, n_src, "exact" if family == "exact" else "float")
    rng = np.random.default_rng(31 * n_nodes + 7 * n_src + H + (1 if family == "float" else 0))
    E, cap = g["E"], g["cap"]
    if family == "exact":
        dG = rng.integers(-4, 5, size=(E, H)).astype(F32)
        ZA, ZB = _quarter(rng, (n_nodes, H), 2), _quarter(rng, (n_src, H), 2)
        mean = _quarter(rng, H, 1)
        rstd = np.abs(rng.choice(POW2, size=H)).astype(F32)
        gamma = rng.choice(POW2, size=H).astype(F32)
        sdz, sdzx = (E * _quarter(rng, H, 1)).astype(F32), (E * rng.choice(POW2, size=H)).astype(F32)
    else:
        dG = (rng.standard_normal((E, H)) * 10.0 ** np.linspace(-3, 3, H)[None, :]).astype(F32)
        ZA, ZB = rng.standard_normal((n_nodes, H)).astype(F32), rng.standard_normal((n_src, H)).astype(F32)
        y = edge_relu_sum(ZA, ZB, g["rowptr"], g["src"])
        mean = y.mean(0).astype(F32)
        rstd = (1.0 / np.sqrt(y.var(0) + 1e-5)).astype(F32)
        gamma = (rng.standard_normal(H) + 1.5).astype(F32)
        sdz = (dG.astype(F64).sum(0)).astype(F32)
        sdzx = (dG.astype(F64) * xhat_of(y, mean, rstd)).sum(0).astype(F32)
    Y = np.full((cap, H), np.nan, F32)
    Y[:E] = edge_relu_sum(ZA, ZB, g["rowptr"], g["src"]).astype(F32)          # a float32 sum of two float32: what the forward stored
    G = np.full((cap, H), np.nan, F32)
    G[:E] = dG
    return dict(g=g, dG=G, Y=Y, ZA=ZA, ZB=ZB, mean=mean, rstd=rstd, gamma=gamma, sdz=sdz, sdzx=sdzx)


PRODUCT_SHAPES = ((1, 1), (15, 17), (16, 16), (17, 15), (33, 130))


def product_inputs(h_out, h_in, family):
    rng = np.random.default_rng(1000 * h_out + h_in + (5 if family == "float" else 0))
    if family == "exact":
        return dict(M=_quarter(rng, (h_out, h_in), 8), db2=_quarter(rng, h_out, 4), W2=_quarter(rng, (h_out, h_in), 2), mean=_quarter(rng, h_in, 2),
                    rstd=np.abs(rng.choice(POW2, size=h_in)).astype(F32))
    return dict(M=(rng.standard_normal((h_out, h_in)) * 50).astype(F32), db2=(rng.standard_normal(h_out) * 10).astype(F32),
                W2=(rng.standard_normal((h_out, h_in)) / np.sqrt(h_out)).astype(F32), mean=(rng.standard_normal(h_in) + 2).astype(F32),
                rstd=(np.abs(rng.standard_normal(h_in)) + 0.5).astype(F32))
