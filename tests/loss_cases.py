"""Generated cases for the loss kernels (csrc/losses.hip, csrc/losses_skin.hip) at the sizes the kernels branch on, their float64 oracle
results, the float32-oracle deviations the bounds are made of, and the run / compare functions that tests/test_loss_cases.py (emulated
op layer, CPU) and tests/test_loss_differential.py (device) share. Not a test file.

Every input comes from a seed: ``np.random.default_rng([TAG, seed, attempt])``, drawn again (at most 50 attempts) until the ORACLE ALONE
confirms the case's conditions, so nothing is excluded afterwards. Inputs are created as float32 and widened for the oracle: device and
oracle see the same values. Bounds: per family and quantity the MAXIMUM over the family's cases of the deviation of the float32 oracle
from the float64 oracle (relative for a loss, relative to max |grad| for a gradient), times FACTOR, floored at one float32 ulp -- the
convention of tests/test_gpu_losses.py with the measured deviation taken per family, because a single generated case lands on
accidentally tiny deviations."""
import contextlib
import functools

import numpy as np
import torch

import loss_oracle as lo
import skin_loss_oracle as so
from morig_amd import losses
from test_gpu_losses import bound, rel_max, report
from test_loss_oracle import CHAMFER_MARGIN
from test_skin_loss_oracle import MIN_DIST

ATTEMPTS = 50
PAD = 4                                                     # columns on either side of a strided view: 16 bytes, the rows stay aligned
TAGS = dict(infonce=0x6E6365, multipos=0x6D706F, chamfer=0x636866, logratio=0x6C7261, frames=0x66726D, skin_ce=0x736365, ce_probs=0x636570)


def redraw(family, seed, draw, ok):
    for attempt in range(ATTEMPTS):
        c = draw(np.random.default_rng([TAGS[family], seed, attempt]))
        if ok(c):
            c["attempts"] = attempt + 1
            return c
    raise AssertionError(f"{family} seed {seed}: no draw met the conditions")


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def loss_dev(got, want):
    got, want = float(got), float(want)
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def grad_dev(got, want):
    return rel_max(np.asarray(got), np.asarray(want))


def npy(t):
    return t.detach().cpu().numpy().copy()


def leaf_of(t, device, view):
    """-> (leaf, what the loss is given): the tensor itself, or the middle columns of a wider leaf, read in place"""
    if not view:
        leaf = t.clone().to(device).requires_grad_(True)               # a leaf of its own: the case is shared and stays as it is
        return leaf, leaf
    w = t.shape[-1]
    wide = torch.full(tuple(t.shape[:-1]) + (w + 2 * PAD,), 7.0)
    wide[..., PAD:PAD + w] = t
    leaf = wide.to(device).requires_grad_(True)
    return leaf, leaf[..., PAD:PAD + w]


def grad_of(leaf, view):
    """the gradient of the columns the loss was given; the other columns of a viewed leaf are exact zeros"""
    g = npy(leaf.grad)
    if not view:
        return g
    w = g.shape[-1] - 2 * PAD
    assert (g[..., :PAD] == 0).all() and (g[..., PAD + w:] == 0).all()
    return np.ascontiguousarray(g[..., PAD:PAD + w])


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def batch_vector(counts):
    return torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(list(counts), dtype=torch.long))


# =================================================================================================================== infoNCE
# (vertices, points, v2p rows, p2v rows, all rows share one anchor). Each side is the key set of one direction: both lists of key
# counts run over {1, 4, 5, 8, 31, 32, 33, 64, 65, 97}; row counts over {1, 31, 32, 33, 127, 128, 129, 257}.
NCE_KEYS = (1, 4, 5, 8, 31, 32, 33, 64, 65, 97)
NCE_ROWS = (1, 31, 32, 33, 127, 128, 129, 257)
NCE_BATCHES = {
    "edges": [(1, 4, 1, 31, False), (5, 8, 32, 33, False), (31, 32, 0, 33, False),           # pair 2: skipped, between live pairs
              (33, 31, 127, 128, False), (64, 65, 129, 0, False),                              # pair 4: no p2v rows
              (97, 33, 257, 1, False), (65, 97, 128, 129, True),                               # pair 6: one anchor for all rows
              (32, 64, 31, 127, False), (8, 1, 33, 32, False), (4, 5, 1, 257, False)],
    "view": [(32, 32, 33, 31, False), (64, 33, 1, 128, False), (31, 1, 32, 257, False), (1, 64, 127, 129, False)],
}
NCE_CASES = {f"{b}_tau{t}": (b, tau, c, b == "view") for b, t, tau, c in
             (("edges", "007", 0.07, 2.5), ("edges", "001", 0.01, 1.0), ("view", "007", 0.07, 1.0), ("view", "001", 0.01, 2.5))}
NCE_SKIPPED, NCE_NO_P2V = 2, 4


def nce_forced_labels(nk):
    """key 0, key nk - 1, and one key in either lane half of the last (partial) tile: in a tile of 32 keys lanes 0..31 hold the rows
    {0-3, 8-11, 16-19, 24-27}, lanes 32..63 the others"""
    base = 32 * ((nk - 1) // 32)
    lower = [k for k in range(base, nk) if (k - base) % 8 < 4]
    upper = [k for k in range(base, nk) if (k - base) % 8 >= 4]
    return [nk - 1, 0, lower[-1]] + ([upper[-1]] if upper else [])


def nce_draw(pairs, tau):
    def draw(rng):
        unit = lambda n: f32((lambda x: x / np.linalg.norm(x, axis=1, keepdims=True))(rng.standard_normal((n, 64))))
        nv, npt = [p[0] for p in pairs], [p[1] for p in pairs]
        c = dict(vtx=unit(sum(nv)), pts=unit(sum(npt)), vtx_batch=batch_vector(nv), pts_batch=batch_vector(npt), tau=tau, B=len(pairs),
                 pairs=pairs)
        for name, na, nk, rows in (("v2p", nv, npt, [p[2] for p in pairs]), ("p2v", npt, nv, [p[3] for p in pairs])):
            corr = []
            for b, r in enumerate(rows):
                anchor = np.full(r, rng.integers(0, na[b])) if pairs[b][4] else rng.integers(0, na[b], size=r)
                label = rng.integers(0, nk[b], size=r)
                forced = nce_forced_labels(nk[b])[:r]
                label[:len(forced)] = forced
                corr.append(np.stack([anchor, label], 1).reshape(r, 2))
            c["corr_" + name], c["cb_" + name] = i64(np.concatenate(corr)), batch_vector(rows)
        c["want"] = [npy(t) for t in lo.infonce(*nce_args(c, torch.float64), tau, c["B"])]
        return c
    return draw


def nce_args(c, dtype):
    return (c["vtx"].to(dtype), c["pts"].to(dtype), c["corr_v2p"], c["corr_p2v"], c["vtx_batch"], c["pts_batch"], c["cb_v2p"], c["cb_p2v"])


def nce_case(name):
    b, tau, upstream, view = NCE_CASES[name]
    c = redraw("infonce", sorted(NCE_CASES).index(name), nce_draw(NCE_BATCHES[b], tau), lambda c: np.isfinite(c["want"][0]) and c["want"][0] != 0)
    got = [npy(t) for t in lo.infonce(*nce_args(c, torch.float32), tau, c["B"])]
    c.update(c=upstream, view=view, dev=dict(loss=loss_dev(got[0], c["want"][0]), grad_vtx=grad_dev(got[1], c["want"][1]),
                                              grad_pts=grad_dev(got[2], c["want"][2])))
    return c


def nce_run(c, device):
    lv, vtx = leaf_of(c["vtx"], device, c["view"])
    lp, pts = leaf_of(c["pts"], device, c["view"])
    idx = [c[k].to(device) for k in ("corr_v2p", "corr_p2v", "vtx_batch", "pts_batch", "cb_v2p", "cb_p2v")]
    loss = losses.infoNCE(vtx, pts, *idx, c["tau"], num_graphs=c["B"])
    (c["c"] * loss).backward()
    return float(loss), grad_of(lv, c["view"]), grad_of(lp, c["view"])


def nce_check(name, c, device, bnd):
    got, again = nce_run(c, device), nce_run(c, device)
    assert same_bits(got, again), "a second run gives other bits"
    loss, gv, gp = got
    ok = report(f"infoNCE {name} loss rel", loss_dev(loss, c["want"][0]), bnd["loss"])
    ok &= report(f"infoNCE {name} grad_vtx rel", grad_dev(gv, c["c"] * c["want"][1]), bnd["grad_vtx"])
    ok &= report(f"infoNCE {name} grad_pts rel", grad_dev(gp, c["c"] * c["want"][2]), bnd["grad_pts"])
    assert ok
    vb, pb = npy(c["vtx_batch"]), npy(c["pts_batch"])
    if len(c["pairs"]) > NCE_NO_P2V:
        assert (gv[vb == NCE_SKIPPED] == 0).all() and (gp[pb == NCE_SKIPPED] == 0).all()            # the skipped pair: exactly zero
        # the pair without p2v rows: its vertices are keys of nothing, those that anchor no row receive exactly zero
        anchors = npy(c["corr_v2p"])[npy(c["cb_v2p"]) == NCE_NO_P2V, 0]
        idle = np.setdiff1d(np.arange((vb == NCE_NO_P2V).sum()), anchors)
        assert len(idle) and (gv[vb == NCE_NO_P2V][idle] == 0).all()
    assert np.isfinite(gv).all() and np.isfinite(gp).all()


# =================================================================================================================== multi-positive
# name: (S, width, n_pos, n_neg, vertices per mesh, upstream, view)
MP_CASES = {
    "s2": (2, 4, 1, 1, (2,), 1.0, False),
    "s3_ragged": (3, 8, 2, 63, (3, 8, 20), 2.5, False),
    "s63": (63, 60, 63, 64, (70,), 1.0, False),
    "s64_ragged": (64, 64, 64, 65, (64, 81, 130), 2.5, False),
    "s65": (65, 124, 2, 255, (77,), 1.0, False),
    "s129_view": (129, 128, 64, 256, (140,), 2.5, True),
    "s257_ragged": (257, 64, 63, 256, (300, 257, 263), 1.0, False),
}
MP_PRODUCT_LIMIT = 4.0


def mp_draw(S, D, n_pos, n_neg, sizes):
    def draw(rng):
        B = len(sizes)
        c = dict(feat=f32(rng.standard_normal((sum(sizes), D)) * (1.4 / np.sqrt(D))), batch=batch_vector(sizes), B=B, S=S, sizes=sizes,
                 sample_ids=i64(np.stack([rng.permutation(n)[:S] for n in sizes])),               # without replacement, not monotone
                 pos_ids=i64(rng.integers(0, S, size=(B, S, n_pos))), neg_ids=i64(rng.integers(0, S, size=(B, S, n_neg))))
        c["want"] = [npy(t) for t in lo.multipos(c["feat"].double(), c["batch"], c["sample_ids"], c["pos_ids"], c["neg_ids"], B)]
        return c
    return draw


def mp_products(c):
    """the largest |product| among the sampled rows of a mesh"""
    f = c["feat"].double()
    rows = so._rows(c["batch"], c["sample_ids"], c["B"])
    return max(float((f[r] @ f[r].T).abs().max()) for r in rows)


def mp_shared_and_repeated(c):
    """some row has a sample that is a positive AND a negative of it, and some row a negative drawn twice"""
    pos, neg = npy(c["pos_ids"]).reshape(-1, c["pos_ids"].shape[2]), npy(c["neg_ids"]).reshape(-1, c["neg_ids"].shape[2])
    shared = any(np.intersect1d(p, n).size for p, n in zip(pos, neg))
    return shared and any(len(np.unique(n)) < len(n) for n in neg)


def mp_ok(c):
    return (np.isfinite(c["want"][0]) and c["want"][0] != 0 and mp_products(c) <= MP_PRODUCT_LIMIT
            and (c["neg_ids"].shape[2] < 2 or mp_shared_and_repeated(c)))


def mp_case(name):
    S, D, n_pos, n_neg, sizes, upstream, view = MP_CASES[name]
    c = redraw("multipos", sorted(MP_CASES).index(name), mp_draw(S, D, n_pos, n_neg, sizes), mp_ok)
    got = [npy(t) for t in lo.multipos(c["feat"], c["batch"], c["sample_ids"], c["pos_ids"], c["neg_ids"], c["B"])]
    c.update(c=upstream, view=view, dev=dict(loss=loss_dev(got[0], c["want"][0]), grad=grad_dev(got[1], c["want"][1])))
    return c


def mp_run(c, device):
    leaf, feat = leaf_of(c["feat"], device, c["view"])
    samples = tuple(c[k].to(device) for k in ("sample_ids", "pos_ids", "neg_ids"))
    loss = losses.multi_pos_infoNCE(feat, None, c["batch"].to(device), samples=samples, num_graphs=c["B"])
    (c["c"] * loss).backward()
    return float(loss), grad_of(leaf, c["view"])


def mp_sampled(c):
    sampled = np.zeros(len(c["feat"]), dtype=bool)
    sampled[npy(so._rows(c["batch"], c["sample_ids"], c["B"])).reshape(-1)] = True
    return sampled


def mp_check(name, c, device, bnd):
    got, again = mp_run(c, device), mp_run(c, device)
    assert same_bits(got, again), "a second run gives other bits"
    loss, grad = got
    ok = report(f"multi-pos {name} loss rel", loss_dev(loss, c["want"][0]), bnd["loss"])
    ok &= report(f"multi-pos {name} grad rel", grad_dev(grad, c["c"] * c["want"][1]), bnd["grad"])
    assert ok
    sampled = mp_sampled(c)
    assert (grad[~sampled] == 0).all() and (~sampled).sum() == sum(c["sizes"]) - c["B"] * c["S"]   # unsampled rows: exactly zero


def mp_no_negative_case():
    """n_neg = 0: log(exp(p)) - p, the loss and every coefficient exactly 0 in the kernel's arithmetic"""
    c = mp_draw(5, 8, 3, 0, (9,))(np.random.default_rng([TAGS["multipos"], 99, 0]))
    assert c["want"][0] == 0 and (c["want"][1] == 0).all()
    return dict(c, c=2.5, view=False)


# =================================================================================================================== chamfer
# (vertices, joints) per mesh; name: (meshes, upstream, view)
CH_CASES = {
    "ragged_a": (((1, 1), (257, 257), (1, 2), (513, 1024)), 2.5, False),
    "ragged_b": (((2, 1), (255, 255), (1025, 1023), (256, 256)), 1.0, False),
    "one_vertex": (((1, 1024),), 2.5, False),
    "coincide_view": (((513, 1024),), 1.0, True),
}
CH_COINCIDE = (300, 700)                                    # vertex 300 IS joint 700 (a slot beyond the first of its thread)
CH_TIE = (5, 530)                                           # joint 530 IS joint 5: an exact tie for every vertex
CH_LARGE = {"ragged_a": [3], "ragged_b": [2], "coincide_view": [0]}


def ch_slots_carry(p, q):
    """joints with index >= 256, >= 512 and >= 768 each the nearest joint of vertices from at least two different 256-vertex blocks:
    the slots 1 .. 3 of chamfer_bwd_q_kernel accumulate over more than one LDS fill"""
    d = (p[:, None, :].double() - q[None, :, :].double()).pow(2).sum(-1)
    a1 = npy(d.argmin(dim=1))
    blocks = np.arange(len(a1)) // 256
    out = []
    for lo_j in (256, 512, 768):
        hit = [j for j in np.unique(a1[(a1 >= lo_j) & (a1 < lo_j + 256)]) if len(np.unique(blocks[a1 == j])) >= 2]
        out.append(len(hit))
    return out


def ch_mesh(seed, n, m, coincide=False):
    def draw(rng):
        p, q = f32(rng.uniform(-0.5, 0.5, size=(n, 3))), f32(rng.uniform(-0.5, 0.5, size=(m, 3)))
        if coincide:
            p[CH_COINCIDE[0]] = q[CH_COINCIDE[1]]
        return dict(p=p, q=q)

    def ok(c):
        # the coincident pair has distance 0 and its runner-up far away: its own gap is clear, no waiver is needed
        if lo.chamfer_margin(c["p"].double(), c["q"].double()) < CHAMFER_MARGIN:
            return False
        return m < 1023 or n < 513 or min(ch_slots_carry(c["p"], c["q"])) >= 1
    return redraw("chamfer", seed, draw, ok)


def ch_oracle(c, dtype):
    return [npy(t) for t in lo.chamfer(c["p"].to(dtype), c["batch"], c["q"].to(dtype), c["q_batch"], c["B"])]


def ch_case(name):
    meshes, upstream, view = CH_CASES[name]
    base = 100 * sorted(CH_CASES).index(name)
    parts = [ch_mesh(base + k, n, m, coincide=name == "coincide_view") for k, (n, m) in enumerate(meshes)]
    c = dict(p=torch.cat([x["p"] for x in parts]), q=torch.cat([x["q"] for x in parts]), batch=batch_vector([n for n, _ in meshes]),
             q_batch=batch_vector([m for _, m in meshes]), B=len(meshes), meshes=meshes, attempts=max(x["attempts"] for x in parts),
             c=upstream, view=view)
    c["want"] = ch_oracle(c, torch.float64)
    got = ch_oracle(c, torch.float32)
    c["dev"] = dict(loss=loss_dev(got[0], c["want"][0]), grad_p=grad_dev(got[1], c["want"][1]), grad_q=grad_dev(got[2], c["want"][2]))
    return c


def chamfer_first_occurrence(p, q):
    """one mesh in numpy in the dtype of its inputs, ties to the FIRST index (np.argmin) -> (loss, d loss / d p, d loss / d q)"""
    n, m = len(p), len(q)
    diff = p[:, None, :] - q[None, :, :]
    d = np.sqrt((diff * diff).sum(-1))
    a1, a2 = d.argmin(axis=1), d.argmin(axis=0)
    ii, jj = np.arange(n), np.arange(m)
    d1, d2 = d[ii, a1], d[a2, jj]
    half = p.dtype.type(0.5)
    unit = lambda v, r: np.where(r[:, None] > 0, v / np.where(r > 0, r, 1)[:, None], 0).astype(p.dtype)
    u1, u2 = unit(diff[ii, a1], d1) * (half / n), unit(diff[a2, jj], d2) * (half / m)
    gp, gq = u1.copy(), -u2
    np.add.at(gq, a1, -u1)
    np.add.at(gp, a2, u2)
    return half * (d1.mean() + d2.mean()), gp, gq


def ch_tie_case():
    """300 vertices, 600 joints, joint 530 a copy of joint 5; every other decision clear by CHAMFER_MARGIN, and joint 5 is somebody's
    nearest joint: the tie decides where that vertex's gradient goes"""
    def draw(rng):
        p, q = f32(rng.uniform(-0.5, 0.5, size=(300, 3))), f32(rng.uniform(-0.5, 0.5, size=(600, 3)))
        q[CH_TIE[1]] = q[CH_TIE[0]]
        return dict(p=p, q=q)

    def ok(c):
        rest = torch.cat([c["q"][:CH_TIE[1]], c["q"][CH_TIE[1] + 1:]]).double()
        d = (c["p"][:, None, :].double() - c["q"][None, :, :].double()).pow(2).sum(-1)
        return lo.chamfer_margin(c["p"].double(), rest) >= CHAMFER_MARGIN and bool((npy(d).argmin(axis=1) == CH_TIE[0]).any())
    c = redraw("chamfer", 900, draw, ok)
    c.update(batch=batch_vector([300]), q_batch=batch_vector([600]), B=1, meshes=((300, 600),), c=2.5, view=False)
    c["want"] = list(chamfer_first_occurrence(npy(c["p"]).astype(np.float64), npy(c["q"]).astype(np.float64)))
    got = chamfer_first_occurrence(npy(c["p"]), npy(c["q"]))
    c["dev"] = dict(loss=loss_dev(got[0], c["want"][0]), grad_p=grad_dev(got[1], c["want"][1]), grad_q=grad_dev(got[2], c["want"][2]))
    return c


def ch_run(c, device):
    lp, p = leaf_of(c["p"], device, c["view"])
    lq, q = leaf_of(c["q"], device, c["view"])
    loss = losses.chamfer_batched(p, c["batch"].to(device), q, c["q_batch"].to(device), num_graphs=c["B"])
    (c["c"] * loss).backward()
    return float(loss), grad_of(lp, c["view"]), grad_of(lq, c["view"])


def ch_swapped_run(c, device):
    """mesh (1025, 1023) of ragged_b through the reference's signature with the LARGER set second: the wrapper has to swap"""
    s, sq = c["batch"] == 2, c["q_batch"] == 2
    p, q = c["p"][s].to(device).requires_grad_(True), c["q"][sq].to(device).requires_grad_(True)
    assert q.shape[0] <= losses.CHAMFER_MAX_JOINTS < p.shape[0]
    loss = losses.chamfer_distance_with_average(q.unsqueeze(0), p.unsqueeze(0))
    (c["c"] * loss).backward()
    return float(loss), npy(p.grad), npy(q.grad)


def ch_compare(name, c, got, bnd, want=None, scale=1.0):
    want = c["want"] if want is None else want
    loss, gp, gq = got
    ok = report(f"chamfer {name} loss rel", loss_dev(loss, want[0]), bnd["loss"])
    ok &= report(f"chamfer {name} grad_p rel", grad_dev(gp, scale * c["c"] * want[1]), bnd["grad_p"])
    ok &= report(f"chamfer {name} grad_q rel", grad_dev(gq, scale * c["c"] * want[2]), bnd["grad_q"])
    assert ok
    assert np.isfinite(loss) and np.isfinite(gp).all() and np.isfinite(gq).all()


def ch_check(name, c, device, bnd):
    got, again = ch_run(c, device), ch_run(c, device)
    assert same_bits(got, again), "a second run gives other bits"
    ch_compare(name, c, got, bnd)
    if name == "coincide_view":                             # nothing through the zero distance: zero exactly where the oracle has zero
        v, j = CH_COINCIDE
        assert np.array_equal(got[1][v] == 0, c["want"][1][v] == 0) and np.array_equal(got[2][j] == 0, c["want"][2][j] == 0)
    if name == "tie":                                       # the later copy receives nothing from the vertices: its own term only
        j = CH_TIE[1]
        assert np.array_equal(got[2][j] == 0, c["want"][2][j] == 0)


# =================================================================================================================== log-ratio
# name: (S, feature width, gt_skin width, extra vertices per mesh (0: every row is sampled), upstream, view)
LR_CASES = {
    "s3": (3, 4, 4, (0,), 1.0, False),
    "s4": (4, 4, 128, (1, 70), 2.5, False),
    "s16": (16, 128, 4, (5, 0, 33, 70), 1.0, False),
    "s17": (17, 124, 60, (9,), 2.5, False),
    "s23_view": (23, 32, 48, (0, 41), 1.0, True),
    "s24": (24, 128, 128, (17,), 2.5, False),
    "s50": (50, 32, 48, (3, 70, 0, 28), 1.0, False),
    "s63": (63, 124, 60, (0, 7), 2.5, False),
    "s64": (64, 128, 128, (70, 0), 1.0, False),
}
# name: (T, S, feature width, gt_skin width, extra vertices per mesh, upstream, view)
FRAME_CASES = {"t1": (1, 17, 32, 48, (4, 0), 1.0, False), "t3_view": (3, 24, 4, 4, (30,), 2.5, True)}


def lr_min_dist(x, batch, samples, B):
    """the smallest off-diagonal squared distance among a mesh's sampled rows, over meshes and sets"""
    out = np.inf
    for s in samples.reshape(-1, *samples.shape[-2:]):
        for r in so._rows(batch, s, B):
            d = so.sq_dist(x[r].double())
            out = min(out, float((d + torch.eye(len(r), dtype=torch.float64) * 1e9).min()))
    return out


def lr_draw(S, D, W, extra, n_sets=None, T=0):
    def draw(rng):
        sizes = [S + e for e in extra]
        n, B = sum(sizes), len(sizes)
        gt = rng.uniform(size=(n, W))
        c = dict(gt=f32(gt / gt.sum(1, keepdims=True)), batch=batch_vector(sizes), B=B, S=S, sizes=sizes)
        if n_sets is None:
            c["feat"] = f32(rng.standard_normal((n, D)) * 0.3)
            c["samples"] = i64(np.stack([rng.permutation(k)[:S] for k in sizes]))
        else:
            c["motion_all"], c["motion_aggr"] = f32(rng.standard_normal((n, T, D)) * 0.3), f32(rng.standard_normal((n, D)) * 0.3)
            c["samples"] = i64(np.stack([np.stack([rng.permutation(k)[:S] for k in sizes]) for _ in range(n_sets)]))
        return c
    return draw


def lr_ok(c):
    sets = [c["feat"]] if "feat" in c else [c["motion_all"][:, t, :] for t in range(c["motion_all"].shape[1])] + [c["motion_aggr"]]
    samples = c["samples"].reshape(len(sets), c["B"], c["S"])
    return (all(lr_min_dist(f, c["batch"], samples[k], c["B"]) >= MIN_DIST for k, f in enumerate(sets))
            and lr_min_dist(c["gt"], c["batch"], samples, c["B"]) >= MIN_DIST)


def lr_case(name):
    S, D, W, extra, upstream, view = LR_CASES[name]
    c = redraw("logratio", sorted(LR_CASES).index(name), lr_draw(S, D, W, extra), lr_ok)
    c["want"] = [npy(t) for t in so.logratio(c["feat"].double(), c["gt"].double(), c["batch"], c["samples"], c["B"])]
    got = [npy(t) for t in so.logratio(c["feat"], c["gt"], c["batch"], c["samples"], c["B"])]
    c.update(c=upstream, view=view, dev=dict(loss=loss_dev(got[0], c["want"][0]), grad=grad_dev(got[1], c["want"][1])))
    return c


def lr_run(c, device, mesh=None):
    """the batch, or mesh ``mesh`` alone as a batch of one"""
    feat, gt, batch, samples, B = c["feat"], c["gt"], c["batch"], c["samples"], c["B"]
    if mesh is not None:
        keep = batch == mesh
        feat, gt, batch, samples, B = feat[keep], gt[keep], batch[keep] * 0, samples[mesh:mesh + 1], 1
    leaf, f = leaf_of(feat, device, c["view"])
    loss = losses.log_ratio_loss(f, gt.to(device), batch.to(device), samples=samples.to(device), num_graphs=B)
    (c["c"] * loss).backward()
    return float(loss), grad_of(leaf, c["view"])


def lr_sampled(c, samples=None):
    sampled = np.zeros(len(c["gt"]), dtype=bool)
    sampled[npy(so._rows(c["batch"], c["samples"] if samples is None else samples, c["B"])).reshape(-1)] = True
    return sampled


def lr_check(name, c, device, bnd):
    got, again = lr_run(c, device), lr_run(c, device)
    assert same_bits(got, again), "a second run gives other bits"
    loss, grad = got
    ok = report(f"log-ratio {name} loss rel", loss_dev(loss, c["want"][0]), bnd["loss"])
    ok &= report(f"log-ratio {name} grad rel", grad_dev(grad, c["c"] * c["want"][1]), bnd["grad"])
    assert ok
    sampled = lr_sampled(c)
    assert (grad[~sampled] == 0).all() and (~sampled).sum() == sum(c["sizes"]) - c["B"] * c["S"] and np.isfinite(grad).all()
    B = c["B"]
    if B > 1:                                               # B is a power of two: the division by it is exact
        assert B & (B - 1) == 0
        alone = np.concatenate([lr_run(c, device, b)[1] for b in range(B)]) / np.float32(B)
        assert alone.dtype == np.float32 and np.array_equal(grad, alone), "a mesh's rows are not the mesh-alone rows divided by B"


def frames_case(name):
    T, S, D, W, extra, upstream, view = FRAME_CASES[name]
    c = redraw("frames", sorted(FRAME_CASES).index(name), lr_draw(S, D, W, extra, n_sets=T + 1, T=T), lr_ok)
    oracle = lambda dt: [npy(t) for t in so.logratio_frames(c["motion_all"].to(dt), c["motion_aggr"].to(dt), c["gt"].to(dt), c["batch"],
                                                            c["samples"], c["B"])]
    c["want"] = oracle(torch.float64)
    got = oracle(torch.float32)
    c.update(c=upstream, view=view, T=T, dev=dict(loss=loss_dev(got[0], c["want"][0]), grad=max(grad_dev(got[1], c["want"][1]),
                                                                                                 grad_dev(got[2], c["want"][2]))))
    return c


def frames_run(c, device):
    l_all, m_all = leaf_of(c["motion_all"], device, c["view"])
    l_aggr, m_aggr = leaf_of(c["motion_aggr"], device, c["view"])
    loss = losses.log_ratio_frames(m_all, m_aggr, c["gt"].to(device), c["batch"].to(device), samples=c["samples"].to(device), num_graphs=c["B"])
    (c["c"] * loss).backward()
    return float(loss), grad_of(l_all, c["view"]), grad_of(l_aggr, c["view"])


def frames_check(name, c, device, bnd):
    got, again = frames_run(c, device), frames_run(c, device)
    assert same_bits(got, again), "a second run gives other bits"
    loss, g_all, g_aggr = got
    ok = report(f"log_ratio_frames {name} loss rel", loss_dev(loss, c["want"][0]), bnd["loss"])
    ok &= report(f"log_ratio_frames {name} grad motion_all rel", grad_dev(g_all, c["c"] * c["want"][1]), bnd["grad"])
    ok &= report(f"log_ratio_frames {name} grad motion_aggr rel", grad_dev(g_aggr, c["c"] * c["want"][2]), bnd["grad"])
    assert ok
    for t in range(c["T"] + 1):
        g = g_all[:, t, :] if t < c["T"] else g_aggr
        sampled = lr_sampled(c, c["samples"][t])
        assert (g[~sampled] == 0).all() and (g[sampled] != 0).any()


# =================================================================================================================== masked soft-label CE
# name: (K, rows, upstream, view); label and mask store K + 2 columns
CE_CASES = {f"k{K}_n{n}": (K, n, c, view) for K, n, c, view in
            ((1, 1, 1.0, False), (2, 255, 2.5, False), (3, 256, 1.0, False), (4, 257, 2.5, True), (5, 513, 1.0, False),
             (6, 255, 2.5, False), (7, 257, 1.0, False), (8, 513, 2.5, True), (8, 1, 1.0, False))}
CE_MIN_LABEL = 2.0 ** -6


def ce_draw(K, n):
    def draw(rng):
        count = rng.integers(0, K + 1, size=n)                                          # 0 .. K non-zero labels per row
        order = np.argsort(rng.uniform(size=(n, K)), axis=1)
        nonzero = order < count[:, None]
        label = np.where(nonzero, rng.uniform(CE_MIN_LABEL, 1.0, size=(n, K)), 0.0)
        mask = (rng.uniform(size=(n, K)) < 0.85).astype(np.int64)
        mask[rng.uniform(size=n) < 0.05] = 0                                            # fully masked rows
        if n == 1:
            label, mask = np.maximum(label, CE_MIN_LABEL), np.ones_like(mask)           # the only row has to survive
        # two more stored columns, never zero: a kernel that read past K would see them
        label = np.concatenate([label, rng.uniform(0.5, 1.0, size=(n, 2))], 1)
        mask = np.concatenate([mask, np.ones((n, 2), dtype=np.int64)], 1)
        return dict(x=f32(rng.standard_normal((n, K)) * 2.0), label=f32(label), mask=i64(mask), K=K)
    return draw


def ce_vert_mask(c):
    return so.vert_mask_sequential(npy(c["label"]), npy(c["mask"]).astype(np.float32), c["K"])


def ce_ok(c):
    K = c["K"]
    label, mask = npy(c["label"])[:, :K], npy(c["mask"])[:, :K]
    nonzero = label[label != 0]
    if nonzero.size and (nonzero.min() < CE_MIN_LABEL or nonzero.max() > 1.0):
        return False
    vm = ce_vert_mask(c)
    if not vm.any():
        return False
    nonempty = (label * mask != 0).any(axis=1)
    return K < 2 or len(label) == 1 or (vm[nonempty].any() and (~vm[nonempty]).any())   # both outcomes among the non-empty rows


def ce_case(name):
    K, n, upstream, view = CE_CASES[name]
    c = redraw("skin_ce", sorted(CE_CASES).index(name), ce_draw(K, n), ce_ok)
    c["vert_mask"] = ce_vert_mask(c)
    # the loss GIVEN the sequential mask: the oracle takes the mask, it does not decide it in its own precision
    oracle = lambda dt: [npy(t) for t in so.skin_ce(c["x"].to(dt), c["label"].to(dt), c["mask"], K, torch.from_numpy(c["vert_mask"]))]
    c["want"] = oracle(torch.float64)
    got = oracle(torch.float32)
    c.update(c=upstream, view=view, dev=dict(loss=loss_dev(got[0], c["want"][0]), grad=grad_dev(got[1], c["want"][1])))
    return c


def ce_run(c, device):
    leaf, x = leaf_of(c["x"], device, c["view"])
    loss, vm = losses.skin_ce_loss(x, c["label"].to(device), c["mask"].to(device), nearest_bone=c["K"], return_vert_mask=True)
    (c["c"] * loss).backward()
    return float(loss), grad_of(leaf, c["view"]), npy(vm)


def ce_check(name, c, device, bnd):
    got, again = ce_run(c, device), ce_run(c, device)
    assert same_bits(got, again), "a second run gives other bits"
    loss, grad, vm = got
    assert np.array_equal(vm > 0, c["vert_mask"]) and np.isin(vm, (0.0, 1.0)).all()        # every generated row, to the bit
    ok = report(f"skin CE {name} loss rel", loss_dev(loss, c["want"][0]), bnd["loss"])
    ok &= report(f"skin CE {name} grad rel", grad_dev(grad, c["c"] * c["want"][1]), bnd["grad"])
    assert ok
    assert (grad[~c["vert_mask"]] == 0).all()                                               # a masked-out vertex: exactly zero


# =================================================================================================================== cross_entropy_with_probs
CEP_WEIGHTS = ("none", "K", "N1", "NK")
CEP_REDUCTIONS = (("none", None), ("mean", 2.5), ("sum", 1.0))
CEP_MAX_PROB = 0.9
CEP_CASES = {f"k{K}_n{n}_w{CEP_WEIGHTS[(i + j) % 4]}": (K, n, CEP_WEIGHTS[(i + j) % 4], (i + j) % 3 == 0)
             for i, K in enumerate((1, 2, 127, 128)) for j, n in enumerate((1, 256, 257))}


def cep_draw(K, n, kind):
    def draw(rng):
        t = rng.uniform(size=(n, K)) ** 3
        shape = dict(none=None, K=(K,), N1=(n, 1), NK=(n, K))[kind]
        return dict(x=f32(rng.standard_normal((n, K)) * 2.0), target=f32(t / t.sum(1, keepdims=True)), up=f32(rng.uniform(0.25, 1.0, size=(n, K))),
                    weight=None if shape is None else f32(rng.uniform(0.1, 1.0, size=shape)))
    return draw


def cep_oracle(c, dt, reduction, scalar):
    w = None if c["weight"] is None else torch.broadcast_to(c["weight"], c["x"].shape).to(dt)
    return [npy(t) for t in so.ce_probs(c["x"].to(dt), c["target"].to(dt), w, reduction, c["up"].to(dt) if reduction == "none" else scalar)]


def cep_case(name):
    K, n, kind, view = CEP_CASES[name]
    # a case of ONE row is judged relative to that row alone, and a saturated row (log_softmax of its class next to 0) is all
    # cancellation in any float32 evaluation: the single rows are drawn until no class holds more than CEP_MAX_PROB
    ok = lambda c: n > 1 or K == 1 or float(torch.softmax(c["x"].double(), dim=1).max()) <= CEP_MAX_PROB
    c = redraw("ce_probs", sorted(CEP_CASES).index(name), cep_draw(K, n, kind), ok)
    c.update(view=view, want={}, dev=dict(value=0.0, grad=0.0))
    for reduction, scalar in CEP_REDUCTIONS:
        c["want"][reduction] = cep_oracle(c, torch.float64, reduction, scalar)
        got = cep_oracle(c, torch.float32, reduction, scalar)
        c["dev"]["value"] = max(c["dev"]["value"], grad_dev(got[0].reshape(-1), c["want"][reduction][0].reshape(-1)))
        c["dev"]["grad"] = max(c["dev"]["grad"], grad_dev(got[1], c["want"][reduction][1]))
    return c


def cep_run(c, device, reduction, scalar):
    leaf, x = leaf_of(c["x"], device, c["view"])
    value = losses.cross_entropy_with_probs(x, c["target"].to(device), None if c["weight"] is None else c["weight"].to(device), reduction)
    ((value * c["up"].to(device)).sum() if reduction == "none" else scalar * value).backward()
    return npy(value).reshape(-1), grad_of(leaf, c["view"])


def cep_check(name, c, device, bnd):
    for reduction, scalar in CEP_REDUCTIONS:
        got, again = cep_run(c, device, reduction, scalar), cep_run(c, device, reduction, scalar)
        assert same_bits(got, again), "a second run gives other bits"
        want = c["want"][reduction]
        assert got[0].shape == want[0].reshape(-1).shape
        ok = report(f"cross_entropy_with_probs {name} {reduction} value rel", grad_dev(got[0], want[0].reshape(-1)), bnd["value"])
        ok &= report(f"cross_entropy_with_probs {name} {reduction} grad rel", grad_dev(got[1], want[1]), bnd["grad"])
        assert ok


# =================================================================================================================== the families
FAMILIES = {
    "infonce": (NCE_CASES, nce_case, nce_check),
    "multipos": (MP_CASES, mp_case, mp_check),
    "chamfer": (list(CH_CASES) + ["tie"], lambda name: ch_tie_case() if name == "tie" else ch_case(name), ch_check),
    "logratio": (LR_CASES, lr_case, lr_check),
    "frames": (FRAME_CASES, frames_case, frames_check),
    "skin_ce": (CE_CASES, ce_case, ce_check),
    "ce_probs": (CEP_CASES, cep_case, cep_check),
}
ALL = [(family, name) for family, (names, _, _) in FAMILIES.items() for name in names]


@contextlib.contextmanager
def fixed_order():
    """the oracles sum with index_put_(accumulate=True), whose order on several CPU threads is not fixed: the float32 deviations -- the
    bounds -- are the same in every run only with the deterministic variants"""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before)


@functools.lru_cache(maxsize=None)
def case(family, name):
    with fixed_order():
        return FAMILIES[family][1](name)


@functools.lru_cache(maxsize=None)
def deviations(family):
    """per quantity the maximum over the family's cases of the float32 oracle's deviation from the float64 oracle"""
    devs = [case(family, name)["dev"] for name in FAMILIES[family][0]]
    return {q: max(d[q] for d in devs) for q in devs[0]}


def bounds(family):
    return {q: bound(d) for q, d in deviations(family).items()}


def check(family, name, device):
    FAMILIES[family][2](name, case(family, name), device, bounds(family))


def table():
    lines = ["family-maximum deviation of the float32 oracle from the float64 oracle (the bound is FACTOR times each, floored at one ulp)"]
    for family in FAMILIES:
        lines.append(f"  {family:9s} " + ", ".join(f"{q} {d:.2e} (bound {bound(d):.2e})" for q, d in deviations(family).items()))
    return "\n".join(lines)
