"""GPU: ``kmeans_kernel``, ``ransac_vote_kernel``, ``ransac_fit_kernel`` and ``ransac_apply_kernel`` (csrc/piecewise.hip) through
morig_amd.piecewise, and through morig_amd.native for the statuses and the tables the kernels refuse, against the oracle
(tests/piecewise_oracle.py) on the generated cases of tests/piecewise_cases.py: vertex counts around the 1 024-thread stride and the
64-wide ballot chunks, embedding widths around the ``lane`` / ``lane + 64`` halves in both input types, cluster counts through every
round of the 16 owning waves, reseeds of clusters 16 and up, the prune at 8 and 9 members, the loop's ends, a ragged batch; handle counts
around the vote kernel's 64 lanes and the fit kernel's 256 threads up to a fourth pass, hypothesis counts that leave workgroups half
empty or spanning problems, the refit share at its boundary, inliers only past position 256, ties, a problem without a fit.
tests/test_piecewise_cases.py proves the case conditions, the packing and this file's comparison code without a device.

Discrete results equal the oracle's. k-means centres are compared BIT FOR BIT (oracle and kernel add the same float64 values in the
same documented order), the fit sum within ``fit_f64_bound``. RANSAC R, t, moved vertices and distance sums (relative) are held to 16
times the family maximum of what the float64 oracle deviates from its own longdouble run, measured against the longdouble run; every
figure is printed next to its yardstick before it is asserted (run with -s). Where the project claims bits -- a mesh alone against its
batch, a second run, a vertex of a segment below 4 handles, a healthy problem next to a refused one -- bits are asserted."""
import numpy as np
import pytest
import torch

import piecewise_cases as pc
import piecewise_oracle as po
from morig_amd import native, piecewise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}
STATE_KEYS = ("seeds", "n_iter", "n_kept", "members", "centres_emb", "centres_euc", "fit")
DETAIL_KEYS = ("handles", "counts", "sums", "R", "t")


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def up(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


# =================================================================================================================== k-means
def km_run(names):
    """the named cases as one batch through piecewise.kernel_kmeans -> [(labels, state)] with host arrays"""
    cases = [pc.km_case(n) for n in names]
    s = cases[0]["spec"]
    labels, states = piecewise.kernel_kmeans([up(c["X"]) for c in cases], [up(c["verts"]) for c in cases], n_clusters=s["K"],
                                             max_iter=s["max_iter"], w_euc=pc.W_EUC, tol=s["tol"], first=[c["first"] for c in cases],
                                             return_state=True)
    assert all(l.is_cuda and l.dtype == torch.int64 for l in labels)
    return [(l.cpu().numpy(), st) for l, st in zip(labels, states)]


def km_alone(name):
    return cached(("km", name), lambda: km_run([name])[0])


def km_ops(cases, vptr=None, first=None):
    """the op layer on its own -> the raw result dict on the host"""
    s = cases[0]["spec"]
    X, pos = torch.cat([up(c["X"]) for c in cases]), torch.cat([up(c["verts"]) for c in cases])
    vptr = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cases])]) if vptr is None else vptr
    first = [c["first"] for c in cases] if first is None else first
    res = native.get_ops().kernel_kmeans(X, pos, up(np.asarray(vptr, dtype=np.int32)), up(np.asarray(first, dtype=np.int32)), s["K"],
                                         s["max_iter"], pc.W_EUC, s["tol"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def same_state(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in STATE_KEYS)


KM_RUNNABLE = tuple(n for n in pc.KM_NAMES if n not in pc.KM_NO_CLUSTER)


@pytest.mark.parametrize("name", KM_RUNNABLE)
def test_kmeans_against_the_oracle(name):
    labels, st = km_alone(name)
    pc.km_compare("device", name, labels, st)


def test_kmeans_batch_is_every_mesh_alone_and_runs_twice_with_the_same_bits():
    """six meshes of 65, 1 025, 9, 257, 129 and 120 vertices: no mesh after the first starts at a multiple of 64 rows"""
    batch, again = km_run(pc.KM_BATCH), km_run(pc.KM_BATCH)
    for name, (labels, st), (labels2, st2) in zip(pc.KM_BATCH, batch, again):
        pc.km_compare("device, in its batch", name, labels, st)
        alone_labels, alone = km_alone(name)
        assert np.array_equal(labels, alone_labels) and same_state(st, alone), name
        assert np.array_equal(labels, labels2) and same_state(st, st2), name


@pytest.mark.parametrize("name", ["rounds_k64_d128", "reseed_coincident_k40", "lanes_d65_float64", "stride_v2049"])
def test_kmeans_runs_twice_with_the_same_bits(name):
    (labels, st), = km_run([name])
    alone_labels, alone = km_alone(name)
    assert np.array_equal(labels, alone_labels) and same_state(st, alone)


@pytest.mark.parametrize("name", pc.KM_NO_CLUSTER)
def test_no_cluster_raises_and_names_the_mesh(name):
    c, ops = pc.km_case(name), native.get_ops()
    _, want = c["want"]
    if c["spec"]["K"] == 1:                                                    # behind a healthy mesh of nine vertices
        cases, at, v0 = [pc.km_case("prune_v9_k1"), c], 1, 9
    else:
        cases, at, v0 = [c], 0, 0
    with pytest.raises(ValueError, match=f"mesh {at}: no cluster keeps"):
        piecewise.kernel_kmeans([up(x["X"]) for x in cases], [up(x["verts"]) for x in cases], n_clusters=c["spec"]["K"],
                                first=[x["first"] for x in cases])
    res = km_ops(cases)
    assert res["info"][at].tolist() == [ops.KMEANS_NO_CLUSTER, want["n_iter"], 0, 0] and np.all(res["labels"][v0:] == -1)
    assert np.array_equal(res["seeds"][at], want["seeds"]) and np.array_equal(res["members"][at], want["members"])
    assert np.array_equal(res["centres_emb"][at], want["centres_emb"]) and np.array_equal(res["centres_euc"][at], want["centres_euc"])
    if at:                                                                     # the healthy mesh in front is untouched
        labels, st = km_alone("prune_v9_k1")
        assert res["info"][0].tolist() == [ops.KMEANS_OK, st["n_iter"], 1, 0] and np.array_equal(res["labels"][:9], labels)


# =================================================================================================================== RANSAC
def rs_run(name, meshes=None):
    """piecewise.piecewise_ransac on a batch (or on the meshes ``meshes`` of it with their sample slices) -> (vertices, details)"""
    c = pc.rs_case(name)
    samples = c["samples"] if meshes is None else np.concatenate([c["mesh_samples"][i] for i in meshes])
    details = []
    out = piecewise.piecewise_ransac(*[[up(a) for a in l] for l in pc.lists(c, meshes)], samples=samples, n_iter=c["n_iter"], details=details)
    assert all(o.is_cuda and o.dtype == torch.float64 for o in out)
    return [o.cpu().numpy() for o in out], details


def rs_batch(name):
    return cached(("rs", name), lambda: rs_run(name))


class OpsRun:
    """a batch through the op layer as piecewise.piecewise_ransac drives it, with the tables open to a corruption"""

    def __init__(self, name):
        c = pc.rs_case(name)
        src, dst, vis, seg = pc.lists(c)
        sizes = [len(s) for s in src]
        self.vptr = np.concatenate([[0], np.cumsum(sizes)])
        self.src = torch.cat([up(a, torch.float64) for a in src]).reshape(-1, 3).contiguous()
        self.dst = torch.cat([up(a, torch.float64) for a in dst]).reshape(-1, 3).contiguous()
        mesh_of = torch.repeat_interleave(torch.arange(len(sizes), device=DEV), torch.tensor(sizes, device=DEV))
        self.plan = piecewise.RansacPlan(torch.cat([up(a, torch.float64) for a in vis]), torch.cat([up(a) for a in seg]), mesh_of, pc.THRESHOLD)
        self.samples = up(c["samples"])
        self.handles, self.hptr = self.plan.handles, self.plan.hptr

    def run(self, handles=None, hptr=None, samples=None):
        ops = native.get_ops()
        handles = self.handles if handles is None else handles
        hptr = self.hptr if hptr is None else hptr
        samples = self.samples if samples is None else samples
        count, dsum = ops.ransac_vote(self.src, self.dst, handles, hptr, samples, pc.INLIER_DIST)
        chosen, best, flag, Rt = ops.ransac_fit(self.src, self.dst, handles, hptr, samples, count, dsum, pc.INLIER_DIST, pc.REFIT_SHARE)
        out = ops.ransac_apply(self.src, self.dst, self.plan.problem_of, flag, Rt)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in dict(count=count, dsum=dsum, chosen=chosen, best=best, flag=flag, Rt=Rt, out=out).items()}

    def details(self, raw):
        """the raw arrays in the shape of piecewise_ransac's ``details`` -> (vertices per mesh, details)"""
        ops, plan = native.get_ops(), self.plan
        handles, hptr = self.handles.cpu().numpy(), self.hptr.cpu().numpy()
        seg_mesh, seg_label = plan.segment_mesh.cpu().numpy(), plan.segment_label.cpu().numpy()
        det = []
        for p, s in enumerate(plan.problem_segment):
            m = int(seg_mesh[s])
            det.append(dict(mesh=m, label=int(seg_label[s]), handles=handles[hptr[p]:hptr[p + 1]].astype(np.int64) - self.vptr[m],
                            by_count=int(raw["chosen"][p, 0]), by_sum=int(raw["chosen"][p, 1]), best_count=int(raw["best"][p]),
                            refit=bool(raw["flag"][p] == ops.RANSAC_REFIT), R=raw["Rt"][p, :9].reshape(3, 3), t=raw["Rt"][p, 9:],
                            counts=raw["count"][p], sums=raw["dsum"][p]))
        return [raw["out"][self.vptr[m]:self.vptr[m + 1]] for m in range(len(self.vptr) - 1)], det


def ops_run(name):
    return cached(("ops", name), lambda: OpsRun(name))


def clean(name):
    return cached(("clean", name), lambda: ops_run(name).run())


RS_RUNNABLE = tuple(n for n in pc.RS_NAMES if n != "nofit")


@pytest.mark.parametrize("name", RS_RUNNABLE)
def test_ransac_against_the_oracle(name):
    out, details = rs_batch(name)
    _cache["dev", name] = pc.rs_compare("device", name, out, details)


def test_the_problem_without_a_fit_raises_and_leaves_the_batch_intact():
    """the wrapper names mesh and label; through the op layer the other five problems of the batch hold their oracle results and the
    unfitted segment's vertices come back unmoved (rs_compare asserts both)"""
    with pytest.raises(ValueError, match="mesh 1, label 9"):
        rs_run("nofit")
    run, raw, ops = ops_run("nofit"), clean("nofit"), native.get_ops()
    out, det = run.details(raw)
    assert raw["flag"].tolist() == [ops.RANSAC_REFIT, ops.RANSAC_SMALLEST_SUM, ops.RANSAC_REFIT, ops.RANSAC_NONE, ops.RANSAC_SMALLEST_SUM,
                                    ops.RANSAC_REFIT]
    assert raw["chosen"][3].tolist() == [-1, -1] and raw["best"][3] == 0 and np.all(raw["dsum"][3] >= 1e10) and np.all(raw["count"][3] == 0)
    assert np.array_equal(raw["Rt"][3], np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]))
    _cache["dev", "nofit"] = pc.rs_compare("device, op layer", "nofit", out, det)
    # the meshes on either side alone, through the wrapper: the bits of the batch
    alone, _ = rs_run("nofit", [0, 2])
    assert np.array_equal(alone[0], out[0]) and np.array_equal(alone[1], out[2])


def test_bounds_in_use():
    for name in pc.RS_NAMES:
        if ("dev", name) not in _cache:
            _cache["dev", name] = pc.rs_deviation(*(rs_batch(name) if name != "nofit" else ops_run(name).details(clean(name))), pc.rs_long(name))
    print("\n" + pc.table(device={n: _cache["dev", n] for n in pc.RS_NAMES}))


def same_details(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for x, y in zip(a, b) for k in DETAIL_KEYS) and all(
        (x["by_count"], x["by_sum"], x["best_count"], x["refit"], x["label"]) == (y["by_count"], y["by_sum"], y["best_count"], y["refit"], y["label"])
        for x, y in zip(a, b))


@pytest.mark.parametrize("name", RS_RUNNABLE)
def test_ransac_runs_twice_with_the_same_bits(name):
    out, details = rs_run(name)
    for a, b in zip(out, rs_batch(name)[0]):
        assert np.array_equal(a, b)
    assert same_details(details, rs_batch(name)[1])


@pytest.mark.parametrize("name", ["shapes", "no_problem"])
def test_a_mesh_alone_is_the_mesh_in_its_batch(name):
    out, details = rs_batch(name)
    for i in range(len(out)):
        alone, det = rs_run(name, [i])
        assert np.array_equal(alone[0], out[i]), (name, i)
        assert same_details(det, [d for d in details if d["mesh"] == i])


def test_meshes_of_several_batches_in_one_launch_keep_their_bits():
    """the n_iter = 20 batches as ONE ragged batch of seven meshes (float32 and float64 inputs side by side): every mesh and every
    problem keeps the bits it has in its own batch"""
    names = ("labels", "shapes", "no_problem", "float32")
    cases = [pc.rs_case(n) for n in names]
    assert {c["n_iter"] for c in cases} == {20}
    lists = [[up(m[k]) for c in cases for m in c["meshes"]] for k in ("src", "dst", "vis", "seg")]
    details = []
    out = piecewise.piecewise_ransac(*lists, samples=np.concatenate([c["samples"] for c in cases]), n_iter=20, details=details)
    own_out = [o for n in names for o in rs_batch(n)[0]]
    own_det = [d for n in names for d in rs_batch(n)[1]]
    assert len(out) == len(own_out) == 7 and len(details) == len(own_det)
    for a, b in zip(out, own_out):
        assert np.array_equal(a.cpu().numpy(), b)
    for a, b in zip(details, own_det):
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in DETAIL_KEYS) and a["label"] == b["label"]


# =================================================================================================================== refused tables
NAME = "iter5"                                                                 # three problems of 20, 70 and 130 handles, five hypotheses


def refused(raw, p):
    ops = native.get_ops()
    return (np.all(raw["count"][p] == 0) and np.all(np.isinf(raw["dsum"][p])) and raw["flag"][p] == ops.RANSAC_NONE
            and raw["chosen"][p].tolist() == [-1, -1] and raw["best"][p] == 0
            and np.array_equal(raw["Rt"][p], np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])))


def untouched(raw, want, p):
    return all(np.array_equal(raw[k][p], want[k][p]) for k in ("count", "dsum", "chosen", "best", "flag", "Rt"))


@pytest.mark.parametrize("what,at,value,bad", [("descending", 2, 10, 1), ("negative", 0, -1, 0), ("past_the_handles", 3, 221, 2)])
def test_a_handle_range_that_is_no_range_is_refused(what, at, value, bad):
    """ONE entry of hptr = [0, 20, 90, 220] is corrupted. ``handle_range`` (piecewise.hip:68-73) reads hptr[p] and hptr[p + 1] -- inside
    the table for every p < n_problems -- and answers false for h0 < 0, h1 > n_handles or h1 < h0 BEFORE ``sample_rows`` or any handle is
    read: the vote kernel writes count 0 and an infinite sum (:98-102), the fit kernel's ``!range_ok ||`` short-circuits (:146-156) to
    MORIG_RANSAC_NONE, the apply kernel leaves the vertices (:232). "descending" also turns problem 2 into the range [10, 220), which is
    a range inside the handle array with 210 >= every sample: it is computed, and not compared. The problems whose two entries are
    untouched keep their bits."""
    run, want = ops_run(NAME), clean(NAME)
    hptr = run.hptr.clone()
    assert hptr.tolist() == [0, 20, 90, 220] and run.handles.numel() == 220
    hptr[at] = value
    raw = run.run(hptr=hptr)
    assert refused(raw, bad), what
    for p in range(3):
        if p != bad and not (what == "descending" and p == 2):
            assert untouched(raw, want, p), (what, p)
    po_ = run.plan.problem_of.cpu().numpy()
    assert np.array_equal(raw["out"][po_ == bad], run.src.cpu().numpy()[po_ == bad])          # unmoved
    keep = (po_ != bad) & ~((what == "descending") & (po_ == 2))
    assert np.array_equal(raw["out"][keep], want["out"][keep])


@pytest.mark.parametrize("value", [-1, "n_rows"])
def test_a_handle_that_is_no_row_is_skipped(value):
    """One handle of problem 1 that no hypothesis samples becomes -1 or n_rows. The vote kernel's handle loop (piecewise.hip:108-109) and the
    three loops of the refit (:163-164, :178-179, :196-197) test ``row < 0 || row >= n_rows`` before the row is used; ``sample_rows``
    (:83-84) does the same for a sampled handle. Count and sum are the oracle's over the remaining 69 handles; problems 0 and 2 keep
    their bits."""
    run, want, c = ops_run(NAME), clean(NAME), pc.rs_case(NAME)
    smp = c["samples"][1]
    pos = max(set(range(70)) - set(smp.reshape(-1).tolist()))
    handles = run.handles.clone()
    handles[20 + pos] = run.src.shape[0] if value == "n_rows" else value
    raw = run.run(handles=handles)
    m = c["meshes"][0]
    h = np.delete(c["want"][0][1][1]["handles"], pos)
    d = po.ransac_segment(m["src"][h], m["dst"][h], np.where(smp > pos, smp - 1, smp), pc.INLIER_DIST, pc.REFIT_SHARE, dtype=pc.LONG)
    bar = pc.rs_bounds("hypothesis counts")["sums"]
    dev = float(np.abs(raw["dsum"][1].astype(pc.LONG) / d["sums"] - 1).max())
    print(f"\nhandle {pos} -> {value}: sums against the longdouble oracle over 69 handles {dev:.2e} (bar {bar:.2e})")
    assert np.array_equal(raw["count"][1], d["counts"]) and dev <= bar
    assert raw["chosen"][1].tolist() == [d["by_count"], d["by_sum"]] and raw["best"][1] == d["best_count"] and not d["refit"]
    assert np.abs(raw["Rt"][1, :9].reshape(3, 3) - d["R"]).max() <= pc.rs_bounds("hypothesis counts")["R"]
    assert untouched(raw, want, 0) and untouched(raw, want, 2)


def test_no_hypothesis_gives_no_fit():
    """n_iter = 0: the vote launches nothing, thread 0 of the fit kernel loops over no hypothesis (piecewise.hip:135), ``use < 0`` (:155)
    comes before ``sample_rows``: MORIG_RANSAC_NONE for every problem, the vertices of the problems unmoved, the others on the target"""
    run = ops_run(NAME)
    raw = run.run(samples=torch.zeros(3, 0, 3, dtype=torch.int32, device=DEV))
    ops = native.get_ops()
    assert raw["count"].shape == (3, 0) and raw["flag"].tolist() == [ops.RANSAC_NONE] * 3 and raw["chosen"].tolist() == [[-1, -1]] * 3
    po_ = run.plan.problem_of.cpu().numpy()
    assert np.array_equal(raw["out"][po_ >= 0], run.src.cpu().numpy()[po_ >= 0])
    assert np.array_equal(raw["out"][po_ < 0], run.dst.cpu().numpy()[po_ < 0])


KM3 = ("batch_v65", "batch_v9_copies", "batch_v129")                             # vptr = [0, 65, 74, 203]


@pytest.mark.parametrize("what,at,value,bad", [("no_vertex", 3, 74, 2), ("negative_start", 0, -5, 0), ("past_the_rows", 3, 204, 2)])
def test_kmeans_refuses_a_mesh_whose_range_is_none(what, at, value, bad):
    """ONE entry of vptr is corrupted, at an end of the table so that only one mesh reads it. The kernel reads vptr[b] and vptr[b + 1]
    and leaves with MORIG_KMEANS_BAD_MESH for ``v0 < 0 || V < 1 || v0 + V > n_rows`` (piecewise.hip:327-332) before it reads ``first``
    or a row. The neighbours give the bits of the clean run."""
    cases, ops = [pc.km_case(n) for n in KM3], native.get_ops()
    want = cached("km3", lambda: km_ops(cases))
    vptr = np.array([0, 65, 74, 203])
    vptr[at] = value
    res = km_ops(cases, vptr=vptr)
    assert res["info"][bad, 0] == ops.KMEANS_BAD_MESH and res["info"][bad, 1:].tolist() == [0, 0, 0], what
    clean_vptr = [0, 65, 74, 203]
    for b in range(3):
        if b != bad:
            assert np.array_equal(res["info"][b], want["info"][b]) and res["info"][b, 0] == ops.KMEANS_OK
            assert np.array_equal(res["labels"][clean_vptr[b]:clean_vptr[b + 1]], want["labels"][clean_vptr[b]:clean_vptr[b + 1]])
            assert all(np.array_equal(res[k][b], want[k][b]) for k in ("seeds", "members", "centres_emb", "centres_euc", "fit")), (what, b)
    for b, name in enumerate(KM3):                                             # and the clean run is the wrapper's
        assert np.array_equal(want["labels"][clean_vptr[b]:clean_vptr[b + 1]], km_alone(name)[0])


@pytest.mark.parametrize("first,start", [(-3, 0), (129, 128), (2 ** 31 - 1, 128)])
def test_kmeans_clamps_the_first_seed(first, start):
    """``cur < 0 ? 0 : (cur >= V ? V - 1 : cur)`` (piecewise.hip:334-335) before ``cur`` indexes anything: the seeds of the clamped start"""
    c = pc.km_case("batch_v129")
    res = km_ops([c], first=[first])
    assert np.array_equal(res["seeds"][0], po.fps(c["verts"], 6, start)) and res["info"][0, 0] == native.get_ops().KMEANS_OK
    labels, st = po.kernel_kmeans(c["X"], c["verts"], 6, 100, pc.W_EUC, pc.TOL, start)
    if st["row_margin"] >= 1e-5 and st["fit_margin"] >= 1e-5:                  # not a generated case: compared where its margins allow
        assert np.array_equal(res["labels"], labels) and np.array_equal(res["centres_euc"][0], st["centres_euc"])


def test_null_pointers_and_negative_sizes_are_invalid():
    """the entry points answer MORIG_E_INVALID before anything is launched"""
    lib, E = native.get_ops().lib, native._K["MORIG_E_INVALID"]
    N = None
    for n_rows, n_handles, n_problems, n_iter in ((-1, 0, 1, 1), (5, -1, 1, 1), (5, 0, -1, 1), (5, 0, 1, -1), (5, 0, 1, 1)):
        assert lib.morig_ransac_vote(N, N, n_rows, N, n_handles, N, n_problems, N, n_iter, 0.05, N, N, N) == E
        assert lib.morig_ransac_fit(N, N, n_rows, N, n_handles, N, n_problems, N, n_iter, N, N, 0.05, 0.35, N, N, N, N, N) == E
    for n_rows, n_problems in ((-1, 0), (5, -1), (5, 0), (5, 2)):
        assert lib.morig_ransac_apply(N, N, n_rows, N, n_problems, N, N, N, N) == E
    for n_rows, D, n_meshes, K, max_iter in ((-1, 8, 1, 6, 10), (9, 0, 1, 6, 10), (9, 8, -1, 6, 10), (9, 8, 1, 0, 10), (9, 8, 1, 6, -1), (9, 8, 1, 6, 10)):
        assert lib.morig_kernel_kmeans(N, 0, N, n_rows, D, N, n_meshes, N, K, max_iter, 0.2, 1e-4, N, N, N, N, N, N, N, N, N, N) == E
    torch.cuda.synchronize()                                                   # nothing was launched that could fault
