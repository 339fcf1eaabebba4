"""The conditions of tests/train_bwd_cases.py, on the CPU: every case reaches the dispatch branch it names (on the restated dispatch; the
device file pins that restatement to the library through morig_gemm_tn_workspace), the exact family is exact, the tie layouts are
present, every operand is within the size limit, the branch lists are covered -- and the restatements mean what the reference means:
torch.autograd in float64 through oracle/nets.py modules in training mode gives the same du, dgamma / dbeta, dA / dB and weight
gradients as the restatements composed, within 1e-12 of scale."""
import numpy as np
import pytest
import torch

import train_bwd_cases as tc
from oracle import nets

MODES = ("vec", "odd")


def _vecs(mode):
    return dict(a_vec=mode == "vec", b_vec=mode == "vec")


# ------------------------------------------------------------------------------------------------------------------ GEMM
def test_gemm_cases_reach_the_kernel_they_name():
    for c in tc.gemm_cases():
        assert c["rows"] * max(c["N"], c["K"]) <= tc.MAX_OPERAND, c["name"]
        for mode in MODES:
            for bwd in ("default", "f32"):
                plan = tc.gemm_plan(c["rows"], c["N"], c["K"], bwd, **_vecs(mode))
                want = c["want"] if (bwd == "default" or c["want"].startswith("small")) else "f32_128"
                assert plan["kernel"] == want, (c["name"], mode, bwd, plan)
                assert tc.gemm_workspace(c["rows"], c["N"], c["K"]) >= plan["chunks"] * c["N"] * c["K"]
        plan = tc.gemm_plan(c["rows"], c["N"], c["K"], "default", a_vec=True, b_vec=True)
        assert c.get("must", set()) <= plan["branches"], (c["name"], plan)
        if c["group"] == "small":                                       # MORIG_TN_NO_SMALL=1: through the MFMA kernels' skipped sub-tiles
            for bwd, kernel in (("default", "tn16_128" if c["rows"] >= tc.TN16_R else "f32_128"), ("f32", "f32_128")):
                plan = tc.gemm_plan(c["rows"], c["N"], c["K"], bwd, no_small=True)
                assert plan["kernel"] == kernel and "skip_subtile" in plan["branches"], (c["name"], plan)


def test_gemm_named_cases():
    by = {c["name"]: c for c in tc.gemm_cases()}
    two = tc.gemm_plan(129, 16, 12)
    assert two["chunks"] == 2 and two["spans"] == [128, 1], two                     # one row in the second chunk
    assert tc.gemm_plan(8192, 16, 16)["chunks"] == 64 and tc.gemm_plan(8192, 16, 16)["reduce"] == 32
    assert tc.gemm_plan(8064, 16, 16)["chunks"] == 63 and tc.gemm_plan(8064, 16, 16)["reduce"] == 8
    one = tc.gemm_plan(25600, 256, 256)
    assert one["kernel"] == "tn16_256" and one["chunks"] == 200
    assert tc.gemm_plan(4096, 256, 256)["chunks"] == 32                            # 1 big tile x 32 chunks < 200
    moved = tc.gemm_plan(7168, 260, 260)
    assert moved["kernel"] == "tn16_256" and moved["chunks"] == 56 and "general" not in moved["branches"]
    gen = tc.gemm_plan(7168, 258, 262)["branches"]                                 # (its first tile is whole; the edge tiles are not moved)
    assert gen.isdisjoint({"moved_n", "moved_k"}) and {"general", "skip_subtile"} <= gen
    assert "full" not in tc.gemm_plan(128, 132, 132, a_vec=True, b_vec=False)["branches"]
    assert {"t256_moved_full", "stay128_K255"} <= set(by)
    # the 128-tile table: every extent meets every extent, every row count occurs
    t128 = [c for c in tc.gemm_cases() if c["group"].startswith("t128")]
    assert {(c["N"], c["K"]) for c in t128} == {(n, k) for n in tc.T128 for k in tc.T128}
    assert {c["rows"] for c in t128} == set(tc.R128)
    # below one stage of the split kernel the default path is the exact kernel; the split kernel still sees 0, 1 and rows // 3 live rows
    assert tc.gemm_plan(31, 64, 64)["kernel"] == "f32_128" and tc.gemm_plan(32, 64, 64)["kernel"] == "tn16_128"
    assert all(tc.gemm_plan(r, 64, 64, live=live)["kernel"] == "tn16_128" for r in tc.R128 if r >= 32 for live in (0, 1, r // 3))
    assert {r // 3 for r in tc.R128 if r >= 32} >= {11, 15, 16, 42, 43, 85}


def test_gemm_branch_list_is_covered_by_exact_cases():
    """every case runs the exact families in both window modes and under both settings of MORIG_TRAIN_BWD, the small ones also
    with MORIG_TN_NO_SMALL: together they reach every branch of the list"""
    seen = set()
    for c in tc.gemm_cases():
        for mode in MODES:
            for bwd in ("default", "f32"):
                for live in (None, 0, 1, c["rows"] // 3):
                    seen |= tc.gemm_plan(c["rows"], c["N"], c["K"], bwd, live=live, **_vecs(mode))["branches"]
                if c["group"] == "small":
                    seen |= tc.gemm_plan(c["rows"], c["N"], c["K"], bwd, no_small=True, **_vecs(mode))["branches"]
    assert seen == set(tc.GEMM_BRANCHES), set(tc.GEMM_BRANCHES) ^ seen


@pytest.mark.parametrize("group", tc.gemm_groups())
def test_gemm_exact_families_are_exact(group):
    """sum_r |a||b| in grid units below 2^24 for every output entry, with and without the shift; the split families' k/4 operand needs
    its lo half everywhere, the integer operand nowhere (so lo * lo is identically zero); B - shift is exact in float32"""
    for c in (c for c in tc.gemm_cases() if c["group"] == group):
        for fam in ("int", "splitA", "splitB"):
            inp = tc.gemm_inputs(c, fam)
            for with_shift in (False, True):
                assert tc.gemm_exact_units(inp, with_shift) < 2 ** 24, (c["name"], fam, with_shift)
            assert tc.same_bits(inp["B"] - inp["shift"][None, :], inp["centred"]), (c["name"], fam)
            assert tc.is_f32(inp["centred"].astype(np.float64) + inp["shift"].astype(np.float64)[None, :])
            a_lo, b_lo = tc.bf16_needs_lo(inp["A"]), tc.bf16_needs_lo(inp["centred"])
            if fam == "splitA":
                assert a_lo.all() and not b_lo.any() and not tc.bf16_needs_lo(inp["B"]).any()
            elif fam == "splitB":
                assert b_lo.all() and not a_lo.any()
            else:
                assert not a_lo.any() and not b_lo.any() and not tc.bf16_needs_lo(inp["B"]).any()
            if fam != "int":                                            # hi + lo holds the k/4 operand exactly: at most 16 significant bits
                q = inp["A"] if fam == "splitA" else inp["centred"]
                k = np.abs(q.astype(np.float64)) * 4
                assert (k == np.round(k)).all() and (k % 2 == 1).all() and k.min() >= 257 and k.max() <= 1023
        assert tc.gemm_inputs(c, "float")["A"].dtype == np.float32


# ------------------------------------------------------------------------------------------------------------------ row passes
def test_row_shapes_cross_the_slab_and_quad_branches():
    quads = {tc.stats_plan(256, cols)[2] for cols in tc.ROW_COLS}
    assert {1, 9, 16} <= quads                                          # RL = 256 / quads leaves idle threads at 9
    assert tc.stats_plan(1, 1)[2] == 1 and tc.stats_plan(256, 35)[2] == 9 and tc.stats_plan(256, 130)[2] == 1
    for cols in tc.ROW_COLS:
        slabs = [tc.stats_plan(r, cols)[1] for r in tc.ROW_ROWS]
        assert slabs == [1, 1, 1, 2, 64, 65], (cols, slabs)             # slab_rows = 256; 64 slab lanes in the final pass
        assert all(tc.stats_plan(r, cols)[0] == 256 for r in tc.ROW_ROWS)
    assert max(tc.ROW_ROWS) * max(tc.ROW_COLS) <= tc.MAX_OPERAND
    assert {tc.window_v4(c, *tc.window(c, "vec")) for c in tc.ROW_COLS} == {True, False}
    assert not any(tc.window_v4(c, *tc.window(c, "odd")) for c in tc.ROW_COLS)


@pytest.mark.parametrize("cols", tc.ROW_COLS)
def test_row_exact_inputs_are_exact(cols):
    for rows in tc.ROW_ROWS:
        inp = tc.row_inputs(rows, cols, "exact")
        assert (inp["y"] == 0).any() or rows * cols < 8
        assert tc.is_f32(tc.xhat_of(inp["y"], inp["mean"], inp["rstd"]) * inp["dz"])     # the statistics' term g * xhat
        for live in tc.live_rows_of(rows):
            n = rows if live is None else live
            s0, s1 = tc.given_sums(inp, n, cols)
            assert live is None or live < rows
            assert tc.du_is_exact(inp["dz"][:n], inp["y"][:n], inp["mean"], inp["rstd"], inp["gamma"], s0, s1, n), (rows, live)
            if n and n & (n - 1) == 0:
                assert s0.any() or s1.any()
        assert any(n and (n & (n - 1)) == 0 for n in [rows if v is None else v for v in tc.live_rows_of(rows)]) or rows == 1


@pytest.mark.parametrize("cols", tc.ROW_COLS)
def test_segment_tables_and_exact_inputs(cols):
    for n_seg in tc.ROW_ROWS:
        s = tc.seg_inputs(n_seg, cols, "exact")
        lens, E = s["lens"], s["E"]
        assert E & (E - 1) == 0 and E == int(s["rowptr"][-1]) and s["cap"] * cols <= tc.MAX_OPERAND
        if n_seg >= 255:
            assert (lens == 0).any() and (lens == 1).any() and (lens > 256).sum() == 1 and s["cap"] > E - (n_seg == 256)
        assert ((s["arg"] < 0) == (lens == 0)[:, None]).all()
        seg = s["seg"]
        dz = np.where(s["arg"][seg] == np.arange(E)[:, None], s["dout"].astype(np.float64)[seg], 0.0)
        assert tc.du_is_exact(dz, s["Z"][:E], s["mean"], s["rstd"], s["gamma"], s["sdz"], s["sdzx"], E)
        assert np.isnan(s["Z"][E:]).all()
        f = tc.seg_inputs(n_seg, cols, "float")
        assert f["E"] & (f["E"] - 1) != 0 or n_seg == 1
    assert [tc.stats_plan(n, cols)[1] for n in tc.ROW_ROWS] == [1, 1, 1, 2, 64, 65]
    caps = [tc.seg_inputs(n, cols, "exact")["cap"] for n in tc.ROW_ROWS]
    assert max(tc.stats_plan(c, cols)[1] for c in caps) > 64 and min(tc.stats_plan(c, cols)[1] for c in caps) == 1


# ------------------------------------------------------------------------------------------------------------------ segmax_affine_arg
def test_arg_cases_sit_on_both_sides_of_the_rule():
    seen = set()
    for c in tc.arg_cases():
        ld, col0 = tc.window(c["H"], c["mode"])
        got = tc.segmax_plan(c["n_seg"], c["H"], tc.window_v4(c["H"], ld, col0))
        assert got == c["want"], (c["name"], got)
        assert len(c["lens"]) == c["n_seg"] and int(c["lens"].sum()) * c["H"] <= tc.MAX_OPERAND
        seen.add(got)
    assert seen == set(tc.SEGMAX_BRANCHES)
    assert tc.segmax_plan(400, 324, True) == "long_v4" and tc.segmax_plan(400, 328, True) == "short_v4"
    assert tc.segmax_plan(401, 16, True) == "short_v4" and tc.segmax_plan(400, 16, True) == "long_v4"
    for RL, H in ((64, 20), (16, 19)):                                  # every listed length, and H off the 16-column groups
        want = {0, 1, 2, RL - 1, RL, RL + 1, 4 * RL - 1, 4 * RL, 4 * RL + 1, 8 * RL + 3}
        assert any(set(c["lens"].tolist()) == want and c["H"] == H and c["want"].startswith("long") for c in tc.arg_cases())
        assert H % 16 != 0


def test_arg_tie_layouts_are_present_and_the_restated_break_is_noticed():
    """the layouts are where arg_inputs' docstring puts them, and the restatement with the LAST maximum (`>=` in the serial walk)
    differs from the one with the first on every tie case, on every layout"""
    for c in (c for c in tc.arg_cases() if c["ties"]):
        RL, inp = c["ties"], tc.arg_inputs(c)
        Z, rowptr, s, sh = inp["Z"].astype(np.float64), inp["rowptr"], inp["scale"].astype(np.float64), inp["shift"].astype(np.float64)
        out, arg, zwin = tc.segmax_affine_arg(inp["Z"], rowptr, inp["scale"], inp["shift"])
        _, arg_ge, zwin_ge = tc.segmax_affine_arg(inp["Z"], rowptr, inp["scale"], inp["shift"], first=False)
        assert (s[1::2] < 0).all() and (s[0::2] > 0).all()
        for v in range(min(c["n_seg"], 12)):
            lay = tc.TIE_LAYOUTS[v % len(tc.TIE_LAYOUTS)]
            e0, e1 = int(rowptr[v]), int(rowptr[v + 1])
            cols = tc.tie_columns(lay, c["H"])
            w = Z[e0:e1] * s + sh
            winners = [np.flatnonzero(w[:, j] == w[:, j].max()) for j in cols]
            assert all(len(x) >= 2 for x in winners), (c["name"], lay)
            first = {"all_equal": 0, "two_lanes": 5, "one_lane_quad": 3, "signed_zero": 2, "negative_scale": 1, "last_rows": e1 - e0 - 2}[lay]
            assert all(x[0] == first for x in winners) and (arg[v, cols] == e0 + first).all()
            assert (arg_ge[v, cols] != arg[v, cols]).all(), (c["name"], lay)
            if lay == "two_lanes":
                assert all(x.tolist() == [5, RL + 9] for x in winners) and 5 % RL != (RL + 9) % RL
            if lay == "one_lane_quad":
                assert all(x.tolist() == [3, 3 + 2 * RL] for x in winners) and e1 - e0 >= 4 * RL
            if lay == "signed_zero":
                assert np.signbit(zwin[v, cols]).all() and not np.signbit(zwin_ge[v, cols]).any()
                assert (out[v, cols] == sh[cols]).all() and not (np.signbit(out[v, cols]) & (out[v, cols] == 0)).any()   # the tie is in w
            if lay == "all_equal":
                assert len(winners[0]) == e1 - e0
        assert not tc.same_bits(arg, arg_ge)


def test_arg_float_cases_have_no_near_ties():
    """the float family's arg table is compared exactly on the device: the best and the second best w of every (segment, column) are
    at least 16 float32 ulps of the operands apart, so no rounding of z * scale + shift (fused or not: 2 ulps at most) decides"""
    n = 0
    for c in (c for c in tc.arg_cases() if c["family"] == "float"):
        assert tc.arg_margin(tc.arg_inputs(c)) > 16 * 2.0 ** -23, c["name"]
        n += 1
    assert n >= 6


# ------------------------------------------------------------------------------------------------------------------ edges
def test_edge_graphs_have_the_shapes_the_kernel_branches_on():
    assert {(a > b, a < b, a == b) for a, b in tc.EDGE_GRAPHS} == {(True, False, False), (False, True, False), (False, False, True)}
    for n_nodes, n_src in tc.EDGE_GRAPHS:
        g = tc.edge_graph(n_nodes, n_src)
        E = g["E"]
        assert E & (E - 1) == 0 and g["cap"] > E and int(g["rowptr"][n_nodes]) == E and g["lens"].max() >= 300
        assert (g["src"][:E] < n_src).all() and (g["dst"][:E] == tc.segments_of(g["rowptr"])).all()
        if n_nodes > 1:
            assert (g["lens"] == 0).any()
        if n_src > 1:
            assert len(np.setdiff1d(np.arange(n_src), g["src"][:E])) > 0
        for H in tc.EDGE_H:
            i = tc.edge_inputs(n_nodes, n_src, H, "exact")
            assert np.isnan(i["dG"][E:]).all() and np.isnan(i["Y"][E:]).all()
            assert tc.du_is_exact(i["dG"][:E], i["Y"][:E], i["mean"], i["rstd"], i["gamma"], i["sdz"], i["sdzx"], E)
            assert tc.same_bits(tc.edge_relu_sum(i["ZA"], i["ZB"], g["rowptr"], g["src"]).astype(np.float32), i["Y"][:E])
            assert H < 4 or ((i["Y"][:E] == 0).any() and (i["Y"][:E] > 0).any())
            fl = tc.edge_inputs(n_nodes, n_src, H, "float")
            assert fl["g"]["E"] & (fl["g"]["E"] - 1) != 0


# ------------------------------------------------------------------------------------------------------------------ the reference's meaning
def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), ref.detach().numpy().astype(np.float64)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got - ref).max()) / scale
    assert got.shape == ref.shape and err <= 1e-12, (what, err)


def _bn_terms(bn, y):
    mean, var = y.mean(0), y.var(0)                                     # (biased: what BatchNorm1d normalises with in training)
    return mean, 1.0 / np.sqrt(var + bn.eps), bn.weight.detach().numpy(), bn.bias.detach().numpy()


def _randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.num_features, generator=g, dtype=torch.float64) + 0.5)
                m.weight[::3] *= -1.0
                m.bias.copy_(torch.randn(m.num_features, generator=g, dtype=torch.float64) * 0.2)
    return mod


@pytest.mark.parametrize("n,cin,cout", [(37, 5, 7), (64, 3, 16)])
def test_dense_block_restatements_are_autograd(n, cin, cout):
    """Seq(Linear, ReLU, BatchNorm1d) in training mode: dgamma / dbeta = the two column sums, du = bn_relu_du, dW = du^T x, db = sum du"""
    torch.manual_seed(n)
    with torch.enable_grad():
        blk = _randomise(nets.mlp_stack([cin, cout])[0].double().train(), 3)
        x = torch.randn(n, cin, dtype=torch.float64)
        G = torch.randn(n, cout, dtype=torch.float64)
        u = blk[0](x)
        u.retain_grad()
        (blk[2](blk[1](u)) * G).sum().backward()
    y = np.maximum(u.detach().numpy(), 0.0)
    mean, rstd, gamma, _ = _bn_terms(blk[2], y)
    sdz, sdzx = tc.col_sums(G.numpy(), y, mean, rstd)
    _close(sdz, blk[2].bias.grad, "dbeta")
    _close(sdzx, blk[2].weight.grad, "dgamma")
    du, sdu = tc.bn_relu_du(G.numpy(), y, mean, rstd, gamma, sdz, sdzx, want_sum=True)
    _close(du, u.grad, "du")
    _close(tc.gemm_tn(du, x.numpy()), blk[0].weight.grad, "dW")
    _close(sdu, blk[0].bias.grad, "db")
    _close(tc.col_sums(du)[0], blk[0].bias.grad, "db as a plain column sum")
    # the centred product:  du^T (x - 1 m^T) + colsum(du) (x) m  is the same weight gradient
    m = x.numpy().mean(0)
    _close(tc.gemm_tn(du, x.numpy(), shift=m) + sdu[:, None] * m[None, :], blk[0].weight.grad, "dW from the centred product")


@pytest.mark.parametrize("n,cin,cout,e", [(23, 4, 6, 90), (40, 3, 8, 200)])
def test_edge_block_restatements_are_autograd(n, cin, cout, e):
    """EdgeMaxConv in training mode, restated on the operators of the native path: u1[e] = A[dst] + B[src] with A = x (Wa - Wb)^T + b1,
    B = x Wb^T; max of BatchNorm2 as segmax_affine_arg; the one-hot statistics (both forms), segmax_bn_relu_du, the first
    BatchNorm's sums from the products and from a pass, edge_bn_scatter in its three forms, the plain scatter"""
    torch.manual_seed(e)
    with torch.enable_grad():
        conv = _randomise(nets.EdgeMaxConv(cin, cout).double().train(), 5)
        x = torch.randn(n, cin, dtype=torch.float64, requires_grad=True)
        ei = torch.randint(0, n, (2, e))
        G = torch.randn(n, cout, dtype=torch.float64)
        (conv(x, ei) * G).sum().backward()
    ein = nets._loop_normalised(ei, n).numpy()
    order = np.argsort(ein[1], kind="stable")
    src, dst = ein[0][order].astype(np.int32), ein[1][order].astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int32)
    E = len(src)
    (l1, _, bn1), (l2, _, bn2) = conv.nn_pos[0], conv.nn_pos[1]
    W1, b1, W2, b2 = (t.detach().numpy() for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    Wa, Wb = W1[:, :cin], W1[:, cin:]
    xn = x.detach().numpy()
    ZA, ZB = xn @ (Wa - Wb).T + b1, xn @ Wb.T
    Y1 = np.maximum(ZA[dst] + ZB[src], 0.0)
    m1, r1, g1, be1 = _bn_terms(bn1, Y1)
    z1 = (Y1 - m1) * r1 * g1 + be1
    Y2 = np.maximum(z1 @ W2.T + b2, 0.0)
    m2, r2, g2, be2 = _bn_terms(bn2, Y2)
    # segmax_affine_arg takes float32 rows; the float64 forward is compared on its own evaluation of w
    w2 = (Y2 - m2) * r2 * g2 + be2
    arg = np.full((n, cout), -1, np.int32)
    for v in range(n):
        arg[v] = rowptr[v] + np.argmax(w2[rowptr[v]:rowptr[v + 1]], axis=0)
    o32, a32, zw32 = tc.segmax_affine_arg(Y2.astype(np.float32), rowptr, (g2 * r2).astype(np.float32), (be2 - m2 * g2 * r2).astype(np.float32))
    assert (a32 == arg).mean() > 0.98 and np.abs(o32 - w2[arg, np.arange(cout)[None, :]]).max() < 1e-5
    zwin = Y2[arg, np.arange(cout)[None, :]]
    dout = G.numpy()
    sa = tc.col_sums(dout, zwin, m2, r2, live=arg)
    sb = tc.segmax_stats_gather(dout, arg, Y2, m2, r2)
    for a, b in zip(sa, sb):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    _close(sa[0], bn2.bias.grad, "dbeta2")
    _close(sa[1], bn2.weight.grad, "dgamma2")
    du2, sdu2, _ = tc.segmax_bn_relu_du(dout, arg, Y2, rowptr, m2, r2, g2, sa[0], sa[1], E + 3)
    assert (du2[E:] == 0).all()
    _close(sdu2, l2.bias.grad, "db2")
    _close(tc.gemm_tn(du2[:E], z1), l2.weight.grad, "dW2")
    # the Linear behind the BatchNorm without the ReLU gate: relu=False is du of BatchNorm alone
    lin_only, _, _ = tc.segmax_bn_relu_du(dout, arg, Y2, rowptr, m2, r2, g2, sa[0], sa[1], E, relu=False)
    assert np.abs(np.where(Y2 > 0, lin_only, 0.0) - du2[:E]).max() == 0.0 and (lin_only != du2[:E]).any()
    dh = du2[:E] @ W2
    s1 = tc.col_sums(dh, Y1, m1, r1)
    _close(s1[0], bn1.bias.grad, "dbeta1")
    _close(s1[1], bn1.weight.grad, "dgamma1")
    M = tc.gemm_tn(du2[:E], Y1)
    p = tc.edge_bn_sums_from_products(M, sdu2, W2, m1, r1)
    _close(p[0], bn1.bias.grad, "dbeta1 from the products")
    _close(p[1], bn1.weight.grad, "dgamma1 from the products")
    # (the rebuilt form rounds ZA + ZB to float32, as the forward stores it: compared here on operands that are float32 already)
    dA, dB, _ = tc.edge_bn_scatter(dh, rowptr, src, n, Y=Y1, mean=m1, rstd=r1, gamma=g1, sum_dz=s1[0], sum_dzx=s1[1])
    du1 = tc.bn_relu_du(dh, Y1, m1, r1, g1, s1[0], s1[1])
    pa, pb = tc.edge_scatter(du1, rowptr, src, n)
    pc = tc.edge_bn_scatter(du1, rowptr, src, n)
    assert np.array_equal(pa, dA) and np.array_equal(pb, dB) and np.array_equal(pc[0], dA) and np.array_equal(pc[1], dB)
    _close(dA.sum(0), l1.bias.grad, "db1")
    _close(np.concatenate([tc.gemm_tn(dA, xn), tc.gemm_tn(dB - dA, xn)], axis=1), l1.weight.grad, "dW1")
    _close(dA @ (Wa - Wb) + dB @ Wb, x.grad, "dx")
    za32, zb32 = ZA.astype(np.float32), ZB.astype(np.float32)
    y32 = tc.edge_relu_sum(za32, zb32, rowptr, src)
    r_a = tc.edge_bn_scatter(dh, rowptr, src, n, Y=y32, mean=m1, rstd=r1, gamma=g1, sum_dz=s1[0], sum_dzx=s1[1])
    r_b = tc.edge_bn_scatter(dh, rowptr, src, n, mean=m1, rstd=r1, gamma=g1, sum_dz=s1[0], sum_dzx=s1[1], ZA=za32, ZB=zb32)
    assert np.array_equal(r_a[0], r_b[0]) and np.array_equal(r_a[1], r_b[1])
    assert np.abs(r_a[0] - dA).max() <= 1e-5 * np.abs(dA).max()


@pytest.mark.parametrize("h_out,h_in", tc.PRODUCT_SHAPES)
def test_products_restatement_is_the_pass_over_the_rows(h_out, h_in):
    rng = np.random.default_rng(h_out + h_in)
    rows = 50
    du2, Z1, W2 = rng.standard_normal((rows, h_out)), rng.standard_normal((rows, h_in)) + 1.0, rng.standard_normal((h_out, h_in))
    mean, rstd = Z1.mean(0), 1.0 / np.sqrt(Z1.var(0) + 1e-5)
    a, b = tc.edge_bn_sums_from_products(tc.gemm_tn(du2, Z1), du2.sum(0), W2, mean, rstd)
    wa, wb = tc.col_sums(du2 @ W2, Z1, mean, rstd)
    assert np.abs(a - wa).max() <= 1e-12 * np.abs(du2 @ W2).sum(0).max()
    assert np.abs(b - wb).max() <= 1e-12 * (np.abs(du2 @ W2) * np.abs(tc.xhat_of(Z1, mean, rstd))).sum(0).max() * 10
    for fam in ("exact", "float"):
        i = tc.product_inputs(h_out, h_in, fam)
        assert i["M"].shape == (h_out, h_in) and i["W2"].shape == (h_out, h_in)
