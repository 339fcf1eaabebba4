"""csrc/train_bwd.hip on the device at the sizes its kernels and its dispatch branch on: the cases of tests/train_bwd_cases.py (their
conditions are asserted on the CPU by tests/test_train_bwd_cases.py) through ``native.get_ops()``. Inputs sit in NaN-filled bases (a
read outside the window poisons the result), outputs in sentinel-filled bases with guard rows and guard columns that must stay
untouched. Figures are printed before they are asserted (run with -s).

Bars. u = 2^-24.
  exact inputs   bit equality with the float64 restatement rounded once to float32, for every operator and every dispatch branch.
  arg tables     always compared exactly (the float family of segmax_affine_arg has no near-ties: asserted on the CPU).
  repeats        a second run gives the same bits, everywhere except edge_scatter_backward's dB on float inputs (atomics).
  gemm_tn, float the bars of test_gpu_backward.test_gemm_tn: 2e-6 (MORIG_TRAIN_BWD=f32) and 2e-5 (bf16 x 3 split) of |a_n| |b_k| per entry.
                 (The split kernel missed its bar on one-row products, up to 1.17 of it -- 3 * 2^-16 per product with nothing to average
                 over; products of fewer than 32 host rows take the exact kernel since. The split kernel's tails below a stage are
                 reached through rows_dev.)
  column sums    the kernel adds float32 terms in fp64 and rounds once: |err| <= rows 2^-53 sum|term| + u |sum|; a term of sum dz is
                 dz itself (exact), a term of sum dz * xhat is fl(dz * fl(fl(y - mean) * rstd)): three roundings, (1 + u)^3 - 1 of |term|.
  du             du = fl(grs * fl(fl(dz - k0) - fl(xh * k1))) with grs = fl(gamma rstd), k0 = fl(sum_dz * fl(1 / n)), k1 likewise,
                 xh = fl(fl(y - mean) * rstd). Roundings that reach each part of the result: dz 4 (two differences, grs, the product),
                 k0 6 (+ its own two), xh * k1 8 (+ xh two, k1 two, the product one, without the first difference): at most c = 8,
                 |err| <= 8 u |gamma rstd| (|dz| + |sum_dz| / n + |xhat| |sum_dzx| / n); a fused multiply-add only removes roundings.
                 Entries behind a closed ReLU gate are exactly zero: the gate compares an input.
  sums of du     the sum of the entries' bounds + rows 2^-53 sum|du| + u |sum|.
  edge scatter   a float32 chain of m terms: sum of the terms' du bounds + (m - 1) u (1 + m u) sum|d| per vertex.
  segmax out     w = fl(fl(z s) + sh): 2 u (|z s| + |sh|).
  products       fp64 throughout, one rounding to float32 at the end: (h_out + 4) 2^-53 of the terms' magnitudes + u |result|.

Not covered: MORIG_TN_NO_BIG (read once per process), non-finite inputs."""
import numpy as np
import pytest
import torch

import train_bwd_cases as tc
from morig_amd import native
from morig_amd.native import CSR, Mat, _p, _stream, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("vec", "odd")
U = tc.U
U53 = 2.0 ** -53


def OPS():
    return native.get_ops()


def lib_workspace(rows, N, K):
    return int(OPS().lib.morig_gemm_tn_workspace(rows, N, K))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                # a copy: the tables' arrays are read-only


def host(t):
    return t.detach().cpu().numpy()


def scalar_dev(n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=DEV)


def win(a, mode, fill=np.nan):
    """an input window: `a` inside a NaN-filled base with guard rows behind it -> Mat"""
    base, col0 = tc.in_window(a, mode, tc.GUARD, fill)
    return Mat.of(dev(base), col0, a.shape[1], 0, a.shape[0])


def out_win(rows, cols, mode):
    return win(np.full((rows, cols), tc.SENTINEL, np.float32), mode, fill=tc.SENTINEL)


def int_win(a, mode):
    """an int32 table as a column window of a wider one (its row stride is what the operators take)"""
    ld, col0 = tc.window(a.shape[1], mode)
    base = np.full((a.shape[0] + tc.GUARD, ld), -99, np.int32)
    base[:a.shape[0], col0:col0 + a.shape[1]] = a
    return dev(base)[:a.shape[0], col0:col0 + a.shape[1]]


def read(m, what):
    """the window's content, after the check that nothing around it was written"""
    base = host(m.base)
    mask = np.ones(base.shape, bool)
    mask[m.row0:m.row0 + m.rows, m.col0:m.col0 + m.cols] = False
    assert (base[mask] == tc.SENTINEL).all(), f"{what}: written outside the window"
    return base[m.row0:m.row0 + m.rows, m.col0:m.col0 + m.cols].copy()


def bits(got, want, what):
    """bit equality with the float64 restatement rounded once; the message names the first entries that differ"""
    want = tc.once(want) if np.asarray(want).dtype != np.float32 else np.asarray(want)
    got = np.asarray(got)
    if not tc.same_bits(got, want):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32)) if got.shape == want.shape else None
        first = [] if bad is None else [(tuple(int(x) for x in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:5]]
        raise AssertionError(f"{what}: {0 if bad is None else len(bad)} of {got.size} entries differ in bits, first (index, got, want): {first}")


def within(got, want, bound, what, figures):
    """|got - want| <= bound entry by entry; records the worst ratio"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    figures[what] = max(figures.get(what, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3g}"


def show(title, figures):
    print(f"\n[{title}] worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(figures.items())))


def plus_zero(x):
    """a sum that is zero comes out as +0.0 on the device (0.0 + -0.0): the restated sum is normalised the same way"""
    return tc.once(x) + np.float32(0.0)


def set_bwd(monkeypatch, bwd, no_small=False):
    if bwd == "f32":
        monkeypatch.setenv("MORIG_TRAIN_BWD", "f32")
    else:
        monkeypatch.delenv("MORIG_TRAIN_BWD", raising=False)
    if no_small:
        monkeypatch.setenv("MORIG_TN_NO_SMALL", "1")
    else:
        monkeypatch.delenv("MORIG_TN_NO_SMALL", raising=False)


# ------------------------------------------------------------------------------------------------------------------ gemm_tn
def gemm_direct(A, B, shift, live, out):
    """morig_gemm_tn_shift with a device-side row count and a workspace of EXACTLY the pinned size, NaN-filled, guard floats behind it:
    a partial tile that is not written shows in the result, a write past the workspace in the guard"""
    n_ws = lib_workspace(A.rows, A.cols, B.cols)
    ws = torch.full((n_ws + 64,), float("nan"), dtype=torch.float32, device=DEV)
    rd = scalar_dev(live)
    check(OPS().lib.morig_gemm_tn_shift(A.ptr, A.ld, B.ptr, B.ld, _p(shift), A.rows, _p(rd), A.cols, B.cols, _p(ws), n_ws, out.ptr, out.ld,
                                        _stream()), "morig_gemm_tn_shift")
    assert bool(torch.isnan(ws[n_ws:]).all()), "written behind the workspace"


def run_gemm_case(c, bwd, figures):
    """one case in both window modes; the restated results are computed once"""
    rows, N, K = c["rows"], c["N"], c["K"]
    ops = OPS()
    assert lib_workspace(rows, N, K) == tc.gemm_workspace(rows, N, K), (c["name"], "the restated chunk count has drifted from the library")
    for fam in ("int", "splitA", "splitB"):
        inp = tc.gemm_inputs(c, fam)
        want = {n: plus_zero(tc.gemm_tn(inp["A"], inp["centred"], rows=n)) for n in {rows, rows // 3, 1, 0}}
        for mode in MODES:
            tag = f"{c['name']}/{mode}/{bwd}"
            A, B, Bc, sh = win(inp["A"], mode), win(inp["B"], mode), win(inp["centred"], mode), dev(inp["shift"])
            bits(host(ops.gemm_tn(A, Bc)), want[rows], f"{tag}/{fam} plain")
            o = out_win(N, K, mode)                                    # ldo > K inside a sentinel-filled base
            ops.gemm_tn(A, B, out=o, b_shift=sh, rows_dev=scalar_dev(rows // 3))
            bits(read(o, tag), want[rows // 3], f"{tag}/{fam} b_shift, rows_dev = rows // 3, out window")
            if fam == "int":
                bits(host(ops.gemm_tn(A, B, b_shift=sh)), want[rows], f"{tag}/int b_shift")
                for live in (0, 1, rows // 3, rows):
                    o = out_win(N, K, mode)
                    gemm_direct(A, Bc, None, live, o)
                    bits(read(o, tag), want[live], f"{tag}/int rows_dev = {live}, NaN workspace")
    inp = tc.gemm_inputs(c, "float")
    tol = 2e-6 if bwd == "f32" else 2e-5
    for live in dict.fromkeys((rows, max(rows // 3, 1))):
        a64, b64 = inp["A"].astype(np.float64)[:live], inp["B"].astype(np.float64)[:live] - inp["shift"].astype(np.float64)[None, :]
        scale = np.maximum(np.linalg.norm(a64, axis=0)[:, None] * np.linalg.norm(b64, axis=0)[None, :], 1e-300)
        w_shift, w_plain = a64.T @ b64, a64.T @ inp["centred"].astype(np.float64)[:live]
        rd = None if live == rows else scalar_dev(live)
        for mode in MODES:
            A, B, Bc, sh = win(inp["A"], mode), win(inp["B"], mode), win(inp["centred"], mode), dev(inp["shift"])
            got = host(ops.gemm_tn(A, B, b_shift=sh, rows_dev=rd))
            within(got, w_shift, tol * scale, f"float {bwd} b_shift", figures)
            assert tc.same_bits(got, host(ops.gemm_tn(A, B, b_shift=sh, rows_dev=rd))), f"{c['name']}/{mode}/{bwd}: a second run differs"
            within(host(ops.gemm_tn(A, Bc, rows_dev=rd)), w_plain, tol * scale, f"float {bwd} plain", figures)


@pytest.mark.parametrize("bwd", ["default", "f32"])
@pytest.mark.parametrize("group", tc.gemm_groups())
def test_gemm_tn_at_the_dispatch_branches(group, bwd, monkeypatch):
    """every GEMM case, 16-byte aligned windows (vector loaders, FULL, the moved-back tile) and windows at an odd offset (scalar
    loaders): exact families bit for bit (plain, b_shift, an out window with ldo > K, rows_dev in {0, 1, rows // 3, rows} on a
    NaN-filled workspace of exactly morig_gemm_tn_workspace floats), float family to the project's bars, the chunk count pinned"""
    set_bwd(monkeypatch, bwd)
    figures = {}
    for c in (c for c in tc.gemm_cases() if c["group"] == group):
        run_gemm_case(c, bwd, figures)
    show(f"gemm_tn {group} {bwd}", figures)


@pytest.mark.parametrize("bwd", ["default", "f32"])
def test_gemm_tn_small_shapes_through_the_mfma_kernels(bwd, monkeypatch):
    """MORIG_TN_NO_SMALL=1: N, K <= 32 on the 128-tile kernels, whose 32-column sub-tiles wholly past N or K are skipped"""
    set_bwd(monkeypatch, bwd, no_small=True)
    figures = {}
    for c in (c for c in tc.gemm_cases() if c["group"] == "small"):
        run_gemm_case(c, bwd, figures)
    show(f"gemm_tn small shapes, MORIG_TN_NO_SMALL=1, {bwd}", figures)


# ------------------------------------------------------------------------------------------------------------------ statistics and du
def sums_bounds(dz, y, mean, rstd, n, want):
    """(bound of sum dz, bound of sum dz * xhat) from the docstring's count"""
    dz = np.abs(dz.astype(np.float64)[:n])
    b0 = n * U53 * dz.sum(0)
    b0 = b0 + U * (np.abs(want[0]) + b0)
    if y is None:
        return b0, None
    t = (dz * np.abs(tc.xhat_of(y[:n], mean, rstd))).sum(0)
    b1 = ((1 + U) ** 3 - 1) * t + n * U53 * t
    return b0, b1 + U * (np.abs(want[1]) + b1)


@pytest.mark.parametrize("family", ["exact", "float"])
@pytest.mark.parametrize("cols", tc.ROW_COLS)
def test_bn_statistics_and_du_passes(cols, family):
    """bn_backward_stats (with y and with y=None) and bn_relu_backward (flat, want_sum, du aliasing dz) over ROW_ROWS x both windows x
    the live row counts of live_rows_of: the host count and two device-side counts below it"""
    ops, fig = OPS(), {}
    for rows in tc.ROW_ROWS:
        inp = tc.row_inputs(rows, cols, family)
        mean, rstd, gamma = dev(inp["mean"]), dev(inp["rstd"]), dev(inp["gamma"])
        for mode in MODES:
            dzM, yM = win(inp["dz"], mode), win(inp["y"], mode)
            for live in tc.live_rows_of(rows):
                n, rd, tag = rows if live is None else live, scalar_dev(live), f"rows {rows} cols {cols} {mode} live {live}"
                sdz, sdzx = ops.bn_backward_stats(dzM, yM, mean, rstd, rows_dev=rd)
                only, none = ops.bn_backward_stats(dzM, rows_dev=rd)
                again = ops.bn_backward_stats(dzM, yM, mean, rstd, rows_dev=rd)
                assert none is None and torch.equal(only, sdz) and torch.equal(again[0], sdz) and torch.equal(again[1], sdzx), tag
                want = tc.col_sums(inp["dz"], inp["y"], inp["mean"], inp["rstd"], rows=n)
                if family == "exact":
                    bits(host(sdz), plus_zero(want[0]), f"sum dz, {tag}")
                    bits(host(sdzx), plus_zero(want[1]), f"sum dz xhat, {tag}")
                    s0, s1 = tc.given_sums(inp, n, cols)
                else:
                    b0, b1 = sums_bounds(inp["dz"], inp["y"], inp["mean"], inp["rstd"], n, want)
                    within(host(sdz), want[0], b0, "sum dz", fig)
                    within(host(sdzx), want[1], b1, "sum dz xhat", fig)
                    s0, s1 = host(sdz), host(sdzx)                       # the du pass takes the device's own sums: inputs of the restatement
                if n == 0:
                    continue
                s0d, s1d = dev(s0), dev(s1)
                du_a, du_b = out_win(rows, cols, mode), out_win(rows, cols, mode)
                assert ops.bn_relu_backward(dzM, yM, mean, rstd, gamma, s0d, s1d, du_a, rows_dev=rd) is None
                sdu = ops.bn_relu_backward(dzM, yM, mean, rstd, gamma, s0d, s1d, du_b, rows_dev=rd, want_sum=True)
                ga, gb = read(du_a, tag), read(du_b, tag)
                assert (ga[n:] == tc.SENTINEL).all() and (gb[n:] == tc.SENTINEL).all(), f"{tag}: rows behind the live count written"
                wdu, wsum = tc.bn_relu_du(inp["dz"], inp["y"], inp["mean"], inp["rstd"], inp["gamma"], s0, s1, rows=n, want_sum=True)
                if family == "exact":
                    bits(ga[:n], wdu, f"du flat, {tag}")
                    bits(gb[:n], wdu, f"du with sums, {tag}")
                    bits(host(sdu), plus_zero(wsum), f"sum du, {tag}")
                else:
                    bnd = tc.du_bound(inp["dz"][:n], inp["y"][:n], inp["mean"], inp["rstd"], inp["gamma"], s0, s1, n)
                    within(ga[:n], wdu, bnd, "du flat", fig)
                    within(gb[:n], wdu, bnd, "du with sums", fig)
                    closed = inp["y"][:n] <= 0
                    assert (ga[:n][closed] == 0).all() and (gb[:n][closed] == 0).all(), f"{tag}: a closed ReLU gate let a gradient through"
                    bs = bnd.sum(0) + n * U53 * np.abs(wdu).sum(0)
                    within(host(sdu), wsum, bs + U * (np.abs(wsum) + bs), "sum du", fig)
                    bd = n * U53 * np.abs(gb[:n].astype(np.float64)).sum(0)         # against the device's own du: the sum alone
                    within(host(sdu), tc.hp_sum(gb[:n]), bd + U * (np.abs(wsum) + bd), "sum du of the device's du", fig)
                # du aliasing dz: the block runs it in place
                for want_sum, ref in ((False, ga), (True, gb)):
                    io = win(inp["dz"], mode, fill=tc.SENTINEL)
                    ops.bn_relu_backward(io, yM, mean, rstd, gamma, s0d, s1d, io, rows_dev=rd, want_sum=want_sum)
                    got = read(io, tag)
                    assert tc.same_bits(got[:n], ref[:n]) and tc.same_bits(got[n:], inp["dz"][n:]), f"{tag}: in place (want_sum={want_sum}) differs"
    show(f"bn passes cols {cols} {family}", fig)


@pytest.mark.parametrize("family", ["exact", "float"])
@pytest.mark.parametrize("cols", tc.ROW_COLS)
def test_segmax_statistics_and_du(cols, family):
    """segmax_bn_backward_stats in both forms and segmax_bn_relu_backward (relu on and off, with and without the sums) on segment tables
    that mix empty, one-row and one long segment, n_seg from ROW_ROWS, capacity beyond the live rows: the tail of du is zeroed inside
    the window, the sentinel kept outside it; Z behind the live rows is NaN and never read"""
    ops, fig = OPS(), {}
    for n_seg in tc.ROW_ROWS:
        s = tc.seg_inputs(n_seg, cols, family)
        E, cap = s["E"], s["cap"]
        mean, rstd, gamma = dev(s["mean"]), dev(s["rstd"]), dev(s["gamma"])
        rowptr, seg = dev(s["rowptr"]), dev(s["seg"])
        for mode in MODES:
            tag = f"n_seg {n_seg} cols {cols} {mode}"
            doutM, ZM = win(s["dout"], mode), win(s["Z"], mode)
            arg, zwin = int_win(s["arg"], mode), win(s["zwin"], mode).view()
            by_w = ops.segmax_bn_backward_stats(doutM, arg, None, mean, rstd, zwin=zwin)
            by_g = ops.segmax_bn_backward_stats(doutM, arg, ZM, mean, rstd)
            again = ops.segmax_bn_backward_stats(doutM, arg, ZM, mean, rstd)
            assert torch.equal(again[0], by_g[0]) and torch.equal(again[1], by_g[1]), tag
            ww = tc.segmax_stats_zwin(s["dout"], s["arg"], s["zwin"], s["mean"], s["rstd"])
            wg = tc.segmax_stats_gather(s["dout"], s["arg"], s["Z"][:max(E, 1)], s["mean"], s["rstd"])
            if family == "exact":
                for got, want, what in ((by_w, ww, "kept winners"), (by_g, wg, "gathered")):
                    bits(host(got[0]), plus_zero(want[0]), f"sum dz ({what}), {tag}")
                    bits(host(got[1]), plus_zero(want[1]), f"sum dz xhat ({what}), {tag}")
                s0, s1 = s["sdz"], s["sdzx"]
            else:
                dz1 = np.where(s["arg"] < 0, 0.0, s["dout"]).astype(np.float32)
                b0, b1 = sums_bounds(dz1, s["zwin"], s["mean"], s["rstd"], n_seg, ww)
                for got, want, what in ((by_w, ww, "kept winners"), (by_g, wg, "gathered")):
                    within(host(got[0]), want[0], b0, f"sum dz ({what})", fig)
                    within(host(got[1]), want[1], b1, f"sum dz xhat ({what})", fig)
                s0, s1 = host(by_w[0]), host(by_w[1])
            s0d, s1d = dev(s0), dev(s1)
            for relu in (True, False):
                wdu, wsum, dz = tc.segmax_bn_relu_du(s["dout"], s["arg"], s["Z"], s["rowptr"], s["mean"], s["rstd"], s["gamma"], s0, s1, cap, relu=relu)
                du_a, du_b = out_win(cap, cols, mode), out_win(cap, cols, mode)
                assert ops.segmax_bn_relu_backward(doutM, arg, ZM, rowptr, seg, mean, rstd, gamma, s0d, s1d, du_a, relu=relu) is None
                sdu = ops.segmax_bn_relu_backward(doutM, arg, ZM, rowptr, seg, mean, rstd, gamma, s0d, s1d, du_b, relu=relu, want_sum=True)
                ga, gb = read(du_a, tag), read(du_b, tag)
                assert tc.same_bits(ga, gb), f"{tag} relu={relu}: du with and without the sums differ"
                bits(ga[E:], np.zeros((cap - E, cols), np.float32), f"the tail of du, {tag}")
                if family == "exact":
                    bits(ga[:E], wdu[:E], f"du relu={relu}, {tag}")
                    bits(host(sdu), plus_zero(wsum), f"sum du relu={relu}, {tag}")
                else:
                    bnd = tc.du_bound(dz, s["Z"][:E], s["mean"], s["rstd"], s["gamma"], s0, s1, E)
                    within(ga[:E], wdu[:E], bnd, f"du relu={relu}", fig)
                    if relu:
                        assert (ga[:E][s["Z"][:E] <= 0] == 0).all(), f"{tag}: a closed ReLU gate let a gradient through"
                    bs = bnd.sum(0) + E * U53 * np.abs(wdu).sum(0)
                    within(host(sdu), wsum, bs + U * (np.abs(wsum) + bs), f"sum du relu={relu}", fig)
    show(f"segmax passes cols {cols} {family}", fig)


# ------------------------------------------------------------------------------------------------------------------ segmax_affine_arg
@pytest.mark.parametrize("name", [c["name"] for c in tc.arg_cases()])
def test_segmax_affine_arg_on_both_kernels(name):
    """both sides of the long / short rule, V = 4 and V = 1, every listed segment length around the row lanes and the 4-way unroll, the tie
    layouts: arg and the kept raw values exactly, out bit for bit on exact inputs and within 2 u (|z s| + |sh|) on float inputs"""
    ops, fig = OPS(), {}
    c = next(c for c in tc.arg_cases() if c["name"] == name)
    inp = tc.arg_inputs(c)
    n_seg, H = c["n_seg"], c["H"]
    wout, warg, wz = tc.segmax_affine_arg(inp["Z"], inp["rowptr"], inp["scale"], inp["shift"])
    ZM, rowptr = win(inp["Z"] if inp["E"] else np.zeros((1, H), np.float32), c["mode"]), dev(inp["rowptr"])
    sc, sh = (None, None) if inp["scale"] is None else (dev(inp["scale"]), dev(inp["shift"]))
    for want_zwin in (True, False, True):
        o = out_win(n_seg, H, c["mode"])
        got = ops.segmax_affine_arg(ZM, rowptr, n_seg, o, sc, sh, want_zwin=want_zwin)
        arg = host(got[0] if want_zwin else got)
        wrong = np.argwhere(arg != warg)
        assert len(wrong) == 0, f"{name}: {len(wrong)} winners differ, first (segment, column, got, want): " \
                                f"{[(int(v), int(j), int(arg[v, j]), int(warg[v, j])) for v, j in wrong[:5]]}"
        if want_zwin:
            bits(host(got[1]), wz, f"{name}: kept raw values")
        out = read(o, name)
        if c["family"] == "exact":
            bits(out, wout, f"{name}: out")
        else:
            s = 1.0 if inp["scale"] is None else inp["scale"].astype(np.float64)[None, :]
            b = 0.0 if inp["shift"] is None else np.abs(inp["shift"].astype(np.float64))[None, :]
            within(out, wout, 2 * U * (1 + U) * (np.abs(wz.astype(np.float64) * s) + b), "out", fig)
    show(name, fig)


# ------------------------------------------------------------------------------------------------------------------ edge operators
def chain_bound(d, term_bound, g, n_src):
    """the bound of a float32 chain per target and per source: the terms' own bounds + (m - 1) u (1 + m u) sum|d|"""
    outs = []
    for sums, m in zip(zip(tc.edge_scatter(term_bound, g["rowptr"], g["src"], n_src), tc.edge_scatter(np.abs(d), g["rowptr"], g["src"], n_src)),
                       (g["lens"], np.bincount(g["src"][:g["E"]], minlength=n_src))):
        m = m.astype(np.float64)[:, None]
        outs.append(sums[0] + np.maximum(m - 1, 0) * U * (1 + m * U) * sums[1])
    return outs


@pytest.mark.parametrize("family", ["exact", "float"])
@pytest.mark.parametrize("n_nodes,n_src", tc.EDGE_GRAPHS)
def test_edge_scatter_operators_on_bipartite_graphs(n_nodes, n_src, family):
    """edge_bn_scatter_backward in its three forms and edge_scatter_backward with n_src above, below and equal to n_nodes: vertices without
    in-edges, sources without out-edges, one vertex with 300 in-edges, capacity beyond E with NaN behind the live rows"""
    ops, fig = OPS(), {}
    for H in tc.EDGE_H:
        i = tc.edge_inputs(n_nodes, n_src, H, family)
        g = i["g"]
        E = g["E"]
        kw = {k: dev(i[k]) for k in ("mean", "rstd", "gamma")}
        kw.update(sum_dz=dev(i["sdz"]), sum_dzx=dev(i["sdzx"]))
        bn = dict(mean=i["mean"], rstd=i["rstd"], gamma=i["gamma"], sum_dz=i["sdz"], sum_dzx=i["sdzx"])
        want = {"plain": tc.edge_bn_scatter(i["dG"], g["rowptr"], g["src"], n_src),
                "Y given": tc.edge_bn_scatter(i["dG"], g["rowptr"], g["src"], n_src, Y=i["Y"], **bn),
                "Y rebuilt": tc.edge_bn_scatter(i["dG"], g["rowptr"], g["src"], n_src, ZA=i["ZA"], ZB=i["ZB"], **bn)}
        assert np.array_equal(want["Y given"][0], want["Y rebuilt"][0]) and np.array_equal(want["Y given"][1], want["Y rebuilt"][1])
        tb = tc.du_bound(i["dG"][:E], i["Y"][:E], i["mean"], i["rstd"], i["gamma"], i["sdz"], i["sdzx"], E)
        for mode in MODES:
            tag = f"{n_nodes} x {n_src} H {H} {mode}"
            csr = CSR(dev(g["rowptr"]), dev(g["src"]), dev(g["dst"]), n_nodes, g["cap"], torch.zeros(1, dtype=torch.int32, device=DEV))
            GM, YM, ZA, ZB = win(i["dG"], mode), win(i["Y"], mode), win(i["ZA"], mode), win(i["ZB"], mode)
            for form, args in (("plain", dict(Y=None)), ("Y given", dict(Y=YM, **kw)), ("Y rebuilt", dict(Y=None, ZA=ZA, ZB=ZB, **kw))):
                runs = []
                for _ in range(2):
                    dA, dB = out_win(n_nodes, H, mode), out_win(n_src, H, mode)
                    ops.edge_bn_scatter_backward(GM, args["Y"], csr, n_src, dA, dB, **{k: v for k, v in args.items() if k != "Y"})
                    runs.append((read(dA, tag), read(dB, tag)))
                assert tc.same_bits(runs[0][0], runs[1][0]) and tc.same_bits(runs[0][1], runs[1][1]), f"{tag} {form}: a second run differs"
                wa, wb, d = want[form]
                if family == "exact":
                    bits(runs[0][0], plus_zero(wa), f"dA {form}, {tag}")
                    bits(runs[0][1], plus_zero(wb), f"dB {form}, {tag}")
                else:
                    ba, bb = chain_bound(d, np.zeros_like(d) if form == "plain" else np.where(i["Y"][:E] > 0, tb, 0.0), g, n_src)
                    within(runs[0][0], wa, ba, f"dA {form}", fig)
                    within(runs[0][1], wb, bb, f"dB {form}", fig)
            runs = []
            for _ in range(2):
                dA, dB = out_win(n_nodes, H, mode), out_win(n_src, H, mode)
                ops.edge_scatter_backward(GM, csr, n_src, dA, dB)
                runs.append((read(dA, tag), read(dB, tag)))
            assert tc.same_bits(runs[0][0], runs[1][0]), f"{tag}: dA of the atomic scatter differs between runs"
            wa, wb, d = want["plain"]
            if family == "exact":
                bits(runs[0][0], plus_zero(wa), f"dA atomic scatter, {tag}")
                bits(runs[0][1], plus_zero(wb), f"dB atomic scatter, {tag}")
                assert tc.same_bits(runs[0][1], runs[1][1]), f"{tag}: integer gradients add exactly in any order"
            else:
                ba, bb = chain_bound(d, np.zeros_like(d), g, n_src)
                within(runs[0][0], wa, ba, "dA atomic scatter", fig)
                within(runs[0][1], wb, bb, "dB atomic scatter", fig)
    show(f"edge operators {n_nodes} x {n_src} {family}", fig)


@pytest.mark.parametrize("family", ["exact", "float"])
@pytest.mark.parametrize("h_out,h_in", tc.PRODUCT_SHAPES)
def test_edge_bn_sums_from_products(h_out, h_in, family):
    """16 columns x 16 row lanes per workgroup: h_out and h_in below, at and above 16, and more than one column group"""
    ops, fig = OPS(), {}
    i = tc.product_inputs(h_out, h_in, family)
    wa, wb = tc.edge_bn_sums_from_products(i["M"], i["db2"], i["W2"], i["mean"], i["rstd"])
    for mode in MODES:
        M, W2 = win(i["M"], mode).view(), win(i["W2"], mode).view()
        a, b = ops.edge_bn_sums_from_products(M, dev(i["db2"]), W2, dev(i["mean"]), dev(i["rstd"]))
        a2, b2 = ops.edge_bn_sums_from_products(M, dev(i["db2"]), W2, dev(i["mean"]), dev(i["rstd"]))
        assert torch.equal(a, a2) and torch.equal(b, b2)
        if family == "exact":
            bits(host(a), plus_zero(wa), f"sum dz {h_out} x {h_in} {mode}")
            bits(host(b), plus_zero(wb), f"sum dz xhat {h_out} x {h_in} {mode}")
        else:
            w, m = np.abs(i["W2"].astype(np.float64)), np.abs(i["M"].astype(np.float64))
            ta = (np.abs(i["db2"].astype(np.float64))[:, None] * w).sum(0)
            tb_ = np.abs(i["rstd"].astype(np.float64)) * ((w * m).sum(0) + np.abs(i["mean"].astype(np.float64)) * ta)
            within(host(a), wa, (h_out + 4) * U53 * ta + U * np.abs(wa), "sum dz", fig)
            within(host(b), wb, (h_out + 4) * U53 * tb_ + U * np.abs(wb), "sum dz xhat", fig)
    show(f"products {h_out} x {h_in} {family}", fig)
