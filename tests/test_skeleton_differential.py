"""GPU: csrc/skeleton.hip against tests/skeleton_oracle.py on generated inputs: 20 seeds, each drawn again until the oracle ALONE
confirms the fixture conditions (no length / 0.01 within 1e-6 of a half-integer, no voxel coordinate within 1e-9 of a rounding
boundary, every Prim decision clear by 1e-5 with exact ties only between integer costs, the two best root logits 1e-5 apart), so no
case is excluded afterwards. The sizes are the ones the kernels branch on: J around the wavefront and workgroup widths (2, 3, 31 .. 33,
63 .. 65, 128, 256, and 1025 = one above the limit, refused), ragged batches with non-zero offsets, a batch of 64, bones of more than
64 samples, grids with occupied voxels on their border and joints outside them.

Criteria as in tests/test_gpu_skeleton.py: integers equal; the inside share bit-equal, the distance within one float32 ulp; count-derived
cost entries bit-equal, -log entries and keys within 1e-14 relative."""
import numpy as np
import pytest
import torch

import skeleton_oracle as sk
from morig_amd import native, skeleton
from test_skeleton_oracle import bits32, bits64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (2, 3, 31, 32, 33, 63, 64, 65)
LEN_MARGIN, VOX_MARGIN, KEY_MARGIN = 1e-6, 1e-9, 1e-5


class Grid:
    def __init__(self, data, translate, scale):
        self.data, self.translate, self.scale, self.dims = data, [float(x) for x in translate], float(scale), [88, 88, 88]


def random_grid(rng):
    """a few boxes, every face of the grid partly occupied (index 0 and 87 on each axis), its own placement in space"""
    g = np.zeros((88, 88, 88), dtype=bool)
    for _ in range(6):
        lo = rng.integers(0, 70, size=3)
        hi = lo + rng.integers(8, 40, size=3)
        g[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    for axis in range(3):
        for side in (0, 87):
            sl = [slice(int(a), int(a) + 30) for a in rng.integers(0, 58, size=3)]
            sl[axis] = side
            g[tuple(sl)] = True
    return Grid(g, rng.uniform(-0.6, -0.5, size=3), rng.uniform(1.0, 1.2))


def geometry_case(seed, sizes):
    """joints in a box a little larger than the grid (bones of up to ~200 samples, some joints outside); redrawn until the oracle
    reports the margins"""
    for attempt in range(50):
        rng = np.random.default_rng([0x67656F, seed, attempt])
        grids = [random_grid(rng) for _ in sizes]
        joints = [rng.uniform(-0.65, 0.65, size=(n, 3)) for n in sizes]
        want = [sk.pair_attributes(j, g.data, g.translate, g.scale, 88) for j, g in zip(joints, grids)]
        if all(o["length_margin"] >= LEN_MARGIN and o["voxel_margin"] >= VOX_MARGIN for o in want):
            return joints, grids, want
    raise AssertionError("no draw met the conditions")


def check_geometry(joints, grids, want):
    pairs, attr, outside, pptr = skeleton.pair_attributes_batched(joints, grids)
    pairs, attr, outside = pairs.cpu().numpy(), attr.cpu().numpy(), outside.cpu().numpy()
    joff = 0
    for b, o in enumerate(want):
        sl = slice(int(pptr[b]), int(pptr[b + 1]))
        assert np.array_equal(pairs[sl] - joff, o["pairs"]) and np.array_equal(outside[sl], o["outside_count"]), b
        assert np.array_equal(bits32(attr[sl, 1]), bits32(o["pair_attr"][:, 1])) and np.all(attr[sl, 2] == 1.0), b
        ulp = np.abs(bits32(attr[sl, 0]).astype(np.int64) - bits32(o["pair_attr"][:, 0]).astype(np.int64))
        assert int(ulp.max(initial=0)) <= 1, b
        joff += len(joints[b])
    return want


@pytest.mark.parametrize("seed", range(20))
def test_pair_geometry_ragged_batches(seed):
    rng = np.random.default_rng([0x73697A, seed])
    sizes = [int(x) for x in rng.choice(SIZES, size=int(rng.integers(2, 5)))]
    if seed < len(SIZES):
        sizes[-1] = SIZES[seed]                                 # every size at least once, behind a non-zero offset
    want = check_geometry(*geometry_case(seed, sizes))
    assert max(int(o["n_samples"].max()) for o in want if len(o["n_samples"])) > 64 or max(sizes) < 4        # more than one wavefront
    assert any((o["outside_count"] > 0).any() for o in want)


@pytest.mark.parametrize("n", (128, 256))
def test_pair_geometry_wide_meshes(n):
    check_geometry(*geometry_case(100 + n, [5, n]))


def test_pair_geometry_batch_of_64():
    rng = np.random.default_rng(64)
    check_geometry(*geometry_case(64, [int(x) for x in rng.integers(2, 13, size=64)]))


def cost_case(seed, sizes, saturate=True):
    """logits, outside counts (many of them > 1: integer costs, exact ties), joints on and off the plane; redrawn until the oracle's
    Prim reports its decisions clear, or, for a disconnected mesh, nothing: that mesh's status is the result"""
    for attempt in range(200):
        rng = np.random.default_rng([0x707269, seed, attempt])
        meshes, ok = [], True
        for n in sizes:
            n_pairs = n * (n - 1) // 2
            j32 = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)
            on_plane = rng.uniform(size=n) < 0.3
            j32[on_plane, 0] = rng.uniform(-0.0199, 0.0199, size=int(on_plane.sum())).astype(np.float32)
            # about 12 edges per joint, the other probabilities saturate at 1 (cost <= 0, no edge): J keys spread over the whole cost
            # range; on a dense graph they are all minima over hundreds of costs and crowd closer than 1e-5 whatever the draw
            density = min(0.95, 12.0 / n) if saturate else 1.0
            pl = rng.normal(-5.0, 3.0, size=n_pairs).astype(np.float32)
            pl[rng.uniform(size=n_pairs) >= density] = 30.0
            outside = np.where(rng.uniform(size=n_pairs) < 0.3 * density, rng.integers(0, 4, size=n_pairs), 0).astype(np.int32)    # costs 4 and 6
            rl = rng.normal(0.0, 1.0, size=n).astype(np.float32)
            cost, root, from_count = sk.connectivity_cost(pl, rl, j32, outside)
            parent, key, status, info = sk.prim(cost, root)
            if status == 0 and not (info["margin"] >= KEY_MARGIN and info["ties_integer"]):
                ok = False
            if sk.root_margin(rl) < KEY_MARGIN:
                ok = False
            meshes.append(dict(j32=j32, pl=pl, rl=rl, outside=outside, cost=cost, root=root, from_count=from_count, parent=parent, key=key,
                               status=status))
        if ok:
            return meshes
    raise AssertionError("no draw met the conditions")


def check_cost_and_tree(meshes):
    counts = [len(m["j32"]) for m in meshes]
    jb = torch.repeat_interleave(torch.arange(len(meshes)), torch.tensor(counts)).to(DEV)
    cat = lambda k: torch.from_numpy(np.concatenate([m[k] for m in meshes])).to(DEV)
    costs, root = skeleton.connectivity_cost(cat("pl"), cat("rl"), cat("j32"), None, jb, outside_count=cat("outside"))
    assert root.cpu().tolist() == [m["root"] for m in meshes]
    for got, m in zip(costs, meshes):
        got = got.cpu().numpy()
        fc = m["from_count"]
        assert np.array_equal(bits64(got[fc]), bits64(m["cost"][fc]))
        assert np.all(np.abs(got[~fc] - m["cost"][~fc]) <= 1e-14 * np.abs(m["cost"][~fc]))
    want_status = [m["status"] for m in meshes]
    try:
        parents, keys = skeleton.prim_mst(costs, root)
        status = [0] * len(meshes)
    except skeleton.PrimError as e:
        status = e.status
        live = [b for b, s in enumerate(status) if s == 0]
        parents, keys = [None] * len(meshes), [None] * len(meshes)
        if live:
            ps, ks = skeleton.prim_mst([costs[b] for b in live], root[live])
            for b, p, k in zip(live, ps, ks):
                parents[b], keys[b] = p, k
    assert status == want_status
    for b, m in enumerate(meshes):
        if m["status"] == 0:
            assert np.array_equal(parents[b].cpu().numpy(), m["parent"]), b
            k = keys[b].cpu().numpy()
            assert np.all(np.abs(k - m["key"]) <= 1e-14 * np.abs(m["key"])), b
    return want_status


@pytest.mark.parametrize("seed", range(20))
def test_cost_and_tree_ragged_batches(seed):
    rng = np.random.default_rng([0x73697B, seed])
    pool = SIZES + (128, 256)
    sizes = [int(x) for x in rng.choice(pool, size=int(rng.integers(2, 5)))]
    if seed < len(pool):
        sizes[-1] = pool[seed]
    check_cost_and_tree(cost_case(seed, sizes))


def test_cost_and_tree_batch_of_64():
    rng = np.random.default_rng(65)
    check_cost_and_tree(cost_case(64, [int(x) for x in rng.integers(24, 49, size=64)]))


def test_a_disconnected_mesh_sets_its_status_and_leaves_the_others():
    meshes = cost_case(7, [5, 4, 6], saturate=False)
    m = meshes[1]
    m["pl"][:] = 30.0                                               # no edge at all in the middle mesh
    m["outside"][:] = 0
    m["cost"], m["root"], m["from_count"] = sk.connectivity_cost(m["pl"], m["rl"], m["j32"], m["outside"])
    m["parent"], m["key"], m["status"], _ = sk.prim(m["cost"], m["root"])
    assert check_cost_and_tree(meshes) == [0, 1, 0]


def test_more_joints_than_the_limit_is_refused():
    n = skeleton.MAX_JOINTS + 1
    cost = torch.rand(n, n, dtype=torch.float64, device=DEV) + 1.0
    with pytest.raises(native.MorigNativeError, match="unsupported"):
        skeleton.prim_mst(cost + cost.t(), 0)
    parent, _ = skeleton.prim_mst((cost + cost.t())[:skeleton.MAX_JOINTS, :skeleton.MAX_JOINTS].contiguous(), 0)      # the limit itself runs
    assert int(parent[0]) == -1 and int((parent >= 0).sum()) == skeleton.MAX_JOINTS - 1
