"""CPU: tests/piecewise_oracle.py against the reference's recorded results (tests/golden/piecewise_ransac.npz, piecewise_kmeans.npz;
tools/make_piecewise_golden.py). Every discrete result is equal; the continuous ones are MEASURED (printed, run with -s; tabulated in
DESIGN.md section 17) and must stay below ORACLE_TOL for float64 quantities and 4 float32 ulps of 1.0 for the float32 centres -- what the
oracle deviates from the reference is the yardstick of the GPU test (tests/test_gpu_piecewise.py: 16 times these figures), never the code
under test. The fixture conditions, the case set and the size cap are re-checked here.

Measured here (x86-64): RANSAC R 1.4e-15, t 2.0e-15, vertices 1.7e-15, distance sums 7.2e-13 relative; k-means float64 centres 0 (bit
equal), float32 embedding centres 1.5e-7, fit sum of the float64 case 0, of the float32 cases 4 % of their float32 bound."""
import json
import os

import numpy as np
import pytest

import piecewise_oracle as po
from morig_amd import piecewise                                                # noqa: F401  (the feature under test: absent on the parent)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORACLE_TOL = 1e-9
F32_TOL = 4 * float(np.finfo(np.float32).eps)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


R_META, R_ARR = load("piecewise_ransac")
K_META, K_ARR = load("piecewise_kmeans")
MESHES = [dict(m, **{k: R_ARR[f"m{i}_{k}"] for k in ("src", "dst", "vis", "seg", "out")}) for i, m in enumerate(R_META["meshes"])]
PROBLEMS = [dict(p, **{k: R_ARR[f"p{i}_{k}"] for k in ("handles", "counts", "sums", "R", "t")}) for i, p in enumerate(R_META["problems"])]
SAMPLES = R_ARR["samples"]


def kmeans_cases():
    out = []
    names = [c["name"] for c in K_META["cases"]]
    for i, c in enumerate(K_META["cases"]):
        j = names.index(c["shares"]) if c["shares"] else i
        out.append(dict(c, X=K_ARR[f"c{j}_X"], verts=K_ARR[f"c{j}_verts"],
                        **{k: K_ARR[f"c{i}_{k}"] for k in ("labels", "seeds", "members", "centres_emb", "centres_euc", "last_labels")}))
    return out


KCASES = kmeans_cases()
_cache = {}


def ransac_runs():
    """the oracle on every mesh, once -> [(vertices, details)]"""
    if "r" not in _cache:
        runs, at = [], 0
        for m in MESHES:
            n = sum(h >= 4 for h in m["handle_counts"])
            runs.append(po.piecewise_ransac(m["src"], m["dst"], m["vis"], m["seg"], SAMPLES[at:at + n], R_META["threshold"],
                                            R_META["inlier_dist"], R_META["refit_share"]))
            at += n
        _cache["r"] = runs
    return _cache["r"]


def kmeans_runs():
    if "k" not in _cache:
        _cache["k"] = [po.kernel_kmeans(c["X"], c["verts"], c["K"], c["max_iter"], K_META["w_euc"], K_META["tol"], c["first"]) for c in KCASES]
    return _cache["k"]


def ransac_deviation():
    """the largest absolute deviations of the oracle from the reference (sums: relative)"""
    dev = dict(R=0.0, t=0.0, vertices=0.0, sums=0.0)
    flat = [d for _, det in ransac_runs() for d in det]
    for d, p in zip(flat, PROBLEMS):
        dev["R"] = max(dev["R"], float(np.abs(d["R"] - p["R"]).max()))
        dev["t"] = max(dev["t"], float(np.abs(d["t"] - p["t"]).max()))
        dev["sums"] = max(dev["sums"], float(np.abs(d["sums"] / p["sums"] - 1).max()))
    for (out, _), m in zip(ransac_runs(), MESHES):
        dev["vertices"] = max(dev["vertices"], float(np.abs(out - m["out"]).max()))
    return dev


def fit_f32_bound(c):
    """The reference multiplies a float32 X with float32 centres: a product of two unit rows of width D is off by at most D * 2^-24 (the
    standard bound with sum |x_j c_j| <= 1), halved in the distance and summed over V vertices. The fit sum of a float32 case is no
    float64 quantity of the reference; it is held to this bound and not to ORACLE_TOL."""
    return c["V"] * c["D"] * 2.0 ** -24 / 2


def fit_f64_bound(c):
    """The fit sum of a float64 case is a sum of V non-negative terms, each made of D + 8 or so operations: two implementations that add
    in different orders differ by at most 2 (V - 1) u times the sum, their terms by a few (D + 8) u; u = 2^-53."""
    return (2 * c["V"] + 2 * (c["D"] + 8)) * 2.0 ** -53 * c["fit"]


def kmeans_deviation():
    """the largest deviations of the oracle from the reference: the centres absolute, the fit sums as shares of their bounds"""
    dev = dict(centres_f64=0.0, centres_emb_f32=0.0, fit_f64_share=0.0, fit_f32_share=0.0)
    for (_, st), c in zip(kmeans_runs(), KCASES):
        kept = np.nonzero(st["members"] > 8)[0]
        emb = float(np.abs(st["centres_emb"][kept] - c["centres_emb"]).max())
        key = "centres_emb_f32" if c["dtype"] == "float32" else "centres_f64"
        dev[key] = max(dev[key], emb)
        dev["centres_f64"] = max(dev["centres_f64"], float(np.abs(st["centres_euc"][kept] - c["centres_euc"]).max()))
        if c["dtype"] == "float64":
            dev["fit_f64_share"] = max(dev["fit_f64_share"], abs(st["fit"] - c["fit"]) / fit_f64_bound(c))
        else:                                                                  # as a share of what the reference's float32 products may lose
            dev["fit_f32_share"] = max(dev["fit_f32_share"], abs(st["fit"] - c["fit"]) / fit_f32_bound(c))
    return dev


# ------------------------------------------------------------------------------------------------------------------------- RANSAC
def test_ransac_discrete_results_equal_the_reference():
    flat = [(mi, d) for mi, (_, det) in enumerate(ransac_runs()) for d in det]
    assert len(flat) == len(PROBLEMS) == len(SAMPLES)
    for (mi, d), p in zip(flat, PROBLEMS):
        assert (mi, d["label"]) == (p["mesh"], p["label"])
        assert np.array_equal(d["handles"], p["handles"]) and len(d["handles"]) == p["n_handles"]
        assert np.array_equal(d["counts"], p["counts"]), (mi, d["label"])
        assert d["by_count"] == p["by_count"] and d["best_count"] == p["best_count"] and d["refit"] == p["refit"]
        if not p["refit"]:                                                     # only there the smallest-sum hypothesis is used
            assert d["by_sum"] == p["by_sum"]
        else:                                                                  # equal sums up to rounding among repeated triples
            assert abs(d["sums"][d["by_sum"]] / p["sums"][p["by_sum"]] - 1) <= ORACLE_TOL
    for m in MESHES:
        _, handles = po.segment_handles(m["vis"], m["seg"], R_META["threshold"])
        assert [len(h) for h in handles] == m["handle_counts"]


def test_ransac_continuous_results_within_the_bar():
    dev = ransac_deviation()
    print("piecewise RANSAC, oracle vs reference:", {k: f"{v:.2e}" for k, v in dev.items()})
    assert all(v < ORACLE_TOL for v in dev.values()), dev


def test_ransac_fixture_conditions_and_cases():
    cond = R_META["conditions"]
    flat = [d for _, det in ransac_runs() for d in det]
    assert min(d["sigma_ratio"] for d in flat) >= cond["sigma_ratio"] and min(d["sigma_ratio_vote"] for d in flat) >= cond["sigma_ratio_vote"]
    assert cond["sigma_ratio"] == cond["sigma_ratio_vote"] == 1e-3
    assert min(d["dist_margin"] for d in flat) >= cond["dist_margin"] and cond["dist_margin"] >= 1e-9
    assert min(d["sum_gap"] for d in flat if not d["refit"]) > cond["sum_gap"] and cond["sum_gap"] == 1e-9
    for key in ("sigma_ratio", "sigma_ratio_vote", "dist_margin", "sum_gap"):
        assert R_META["margins"][key] >= cond[key]
    # the case set
    sizes, branches, single, one = MESHES
    assert sizes["handle_counts"] == [0, 3, 4, 63, 65, 257] and single["name"] == "single" and len(np.unique(single["seg"])) == 1
    assert one["V"] == 1 and np.array_equal(one["out"], one["dst"])
    assert sorted(np.unique(branches["seg"])) == [2, 7, 40] and list(branches["seg"][:6]) == [7, 2, 40, 7, 2, 40]
    assert np.sum(branches["vis"] == 0.3) == 3 and np.sum(branches["vis"] == np.nextafter(0.3, 0)) == 3
    by = {(p["mesh"], p["label"]): p for p in PROBLEMS}
    assert by[(1, 7)]["refit"] and not by[(1, 2)]["refit"] and by[(1, 2)]["best_count"] > 0
    assert by[(1, 40)]["by_count"] == -1 and by[(1, 40)]["best_count"] == 0 and not by[(1, 40)]["refit"]
    kept = [v for v in np.nonzero(branches["vis"] == 0.3)[0]]                   # 0.3 itself is a handle, its lower neighbour is not
    for v in kept:
        assert v in by[(1, int(branches["seg"][v]))]["handles"]
    for v in np.nonzero(branches["vis"] == np.nextafter(0.3, 0))[0]:
        assert v not in by[(1, int(branches["seg"][v]))]["handles"]
    for m in MESHES:                                                           # a segment below 4 handles copies the target
        rank, handles = po.segment_handles(m["vis"], m["seg"], R_META["threshold"])
        for l, h in enumerate(handles):
            if len(h) < 4:
                assert np.array_equal(m["out"][rank == l], m["dst"][rank == l])


def test_horn_rotation_equals_the_recorded_rotations():
    worst = max(float(np.abs(po.horn(M)[0] - R).max()) for M, R in zip(R_ARR["fit_M"], R_ARR["fit_R"]))
    print(f"Horn + Jacobi vs the reference's SVD rotations on {len(R_ARR['fit_M'])} recorded fits: {worst:.2e}")
    assert worst < ORACLE_TOL


# ------------------------------------------------------------------------------------------------------------------------- k-means
@pytest.mark.parametrize("i", range(len(KCASES)), ids=[c["name"] for c in KCASES])
def test_kmeans_discrete_results_equal_the_reference(i):
    (labels, st), c = kmeans_runs()[i], KCASES[i]
    assert np.array_equal(st["seeds"], c["seeds"])                             # bit-equal distances: the same arg-max everywhere
    assert st["n_iter"] == c["n_iter"] and st["n_kept"] == c["n_kept"]
    assert np.array_equal(st["members"], c["members"]) and np.array_equal(st["last_labels"], c["last_labels"])
    assert np.array_equal(labels, c["labels"])


def test_kmeans_continuous_results_within_the_bar():
    dev = kmeans_deviation()
    print("kernel k-means, oracle vs reference:", {k: f"{v:.2e}" for k, v in dev.items()})
    assert dev["centres_f64"] < ORACLE_TOL and dev["centres_emb_f32"] < F32_TOL, dev
    assert dev["fit_f64_share"] <= 1.0 and dev["fit_f32_share"] <= 1.0, dev


def test_kmeans_fixture_conditions_and_cases():
    cond = K_META["conditions"]
    assert cond == dict(row_margin=1e-5, fit_margin=1e-5)
    for (_, st), c in zip(kmeans_runs(), KCASES):
        assert st["row_margin"] >= cond["row_margin"] and st["fit_margin"] >= cond["fit_margin"], c["name"]
    assert K_META["margins"]["row_margin"] >= cond["row_margin"] and K_META["margins"]["fit_margin"] >= cond["fit_margin"]
    by = {c["name"]: (c, st) for (_, st), c in zip(kmeans_runs(), KCASES)}
    assert (by["v257"][0]["V"], by["v257"][0]["D"], by["v257"][0]["K"]) == (257, 16, 6)
    assert (by["default"][0]["V"], by["default"][0]["D"], by["default"][0]["K"]) == (1000, 64, 20)
    c, st = by["coincident"]
    assert st["reseeds"] > 0 and len(np.unique(c["verts"][c["seeds"]], axis=0)) < c["K"]
    c, st = by["dropped"]
    assert (c["V"], c["K"]) == (70, 8) and st["n_kept"] < 8 and np.any(st["members"] <= 8)
    c, st = by["cut"]
    assert c["max_iter"] == 2 and st["n_iter"] == 2 and c["n_iter_uncut"] > 2
    assert by["f64"][0]["X"].dtype == np.float64 and by["default"][0]["X"].dtype == np.float32


def test_fixture_size_cap():
    size = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("piecewise_"))
    assert size <= 400 * 1000, size
