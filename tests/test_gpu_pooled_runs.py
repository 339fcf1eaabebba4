"""The pooled LDS-DMA GEMMs (csrc/gemm_dmap.hip POOL launches, csrc/gemm_dma.hip pooled branch; csrc/pool_epilogue.h, csrc/pool_runs.h):
column max per mesh of relu(X W^T + b) * s + t, reduced raw (max AND min per column) over runs of consecutive row tiles and
transformed once per column and flush.

GPU cases: K = 64 and K = 96 on split-layout X, shapes with more than 256 tiles of 256 x 256 (the persistent kernel's rule), segment
layouts that put mesh boundaries on tile edges, on wave-slab edges and inside slabs, a partial last tile over garbage rows, ids without
rows; scale vectors of mixed signs with an exact 0 and columns whose values are all negative, ReLU on and off. Reference: fp64 on the
host, criterion 1e-4 * max(1, max |ref|); every case runs twice, bit-identical. The run length is read once per process
(MORIG_POOL_RUN), so run lengths 1, 2 and 16 come from one child process each, which runs every case; all three must agree bit for
bit with each other and with this process (default run length).

CPU case: the run list's index arithmetic (pool_runs.h) in a stand-alone C++ program under the host sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda"
TILE = 256
KS = (64, 96)
# "wide": 65 row tiles x 4 column blocks = 260 tiles (+ 37 rows: a 66th, partial row tile); "tall": 258 row tiles x 1 column block
SHAPES = {"wide": dict(M=16640, N=1024, extra=37), "tall": dict(M=66000, N=256, extra=0),
          "small": dict(M=1000, N=256, extra=0)}                      # "small": 4 tiles, the one-tile-per-workgroup kernel
LAYOUTS = {"wide": ("tiles", "slabs", "ragged", "one", "partial", "sparse_ids"), "tall": ("ragged", "one"),
           "small": ("slabs", "ragged", "partial")}
GARBAGE = 3.0e4                                                       # rows past M: large, positive, inside the fp16 range
RUN_LENGTHS = (1, 2, 16)


# ------------------------------------------------------------------------------------------------------------------- seeded inputs
def rows_of(shape, layout):
    s = SHAPES[shape]                                                 # ("small": M = 1000 ends inside a tile under every layout)
    return s["M"] + (s["extra"] if layout == "partial" else 0)


def make_problem(shape, K):
    """-> x [alloc, K + 32] fp32 (random rows, then GARBAGE up to the next tile edge), packed layer with the special columns"""
    from morig_amd import packing
    s = SHAPES[shape]
    N, rows = s["N"], s["M"] + s["extra"]
    alloc = (rows + TILE - 1) // TILE * TILE
    g = torch.Generator().manual_seed(7919 * K + N)
    x = torch.zeros(alloc, K + 32)
    x[:, :K] = GARBAGE
    x[:rows, :K] = torch.randn(rows, K, generator=g)
    W = torch.randn(N, K, generator=g) / (K ** 0.5)                   # pre-activations ~ N(0, 1)
    b = torch.randn(N, generator=g) * 0.1
    b[2] = b[3] = -8.0                                                # columns 2, 3: pre-activation + bias < 0 on every row
    lin = packing.pack_linear(W, b)
    Np = lin.W.shape[0]
    scale = torch.randn(Np, generator=g)                              # mixed signs
    shift = torch.randn(Np, generator=g) * 0.2
    scale[0] = 0.0                                                    # exact zero: the column is its shift
    scale[1] = -0.75
    scale[2], shift[2] = 0.25, -1.0                                   # all values negative, non-negative scale
    scale[3], shift[3] = -0.25, -4.0                                  # all values negative, negative scale
    lin.scale, lin.shift = scale, shift
    return x, lin


def make_seg(layout, rows, seed):
    """sorted int32 mesh ids of `rows` rows, and the number of pool rows"""
    if layout in ("tiles", "partial"):                                # boundaries on tile edges (the last mesh of "partial": 37 rows)
        seg = torch.arange(rows) // TILE
    elif layout == "sparse_ids":                                      # even ids only, and three more ids behind the last one
        seg = (torch.arange(rows) // TILE) * 2
    elif layout == "one":
        seg = torch.zeros(rows, dtype=torch.long)
    else:
        g = torch.Generator().manual_seed(seed)
        lens = []
        while sum(lens) < rows:
            if layout == "slabs":                                     # 64 k rows: boundaries on wave-slab edges inside a tile
                lens.append(64 * int(torch.randint(1, 8, (1,), generator=g)))
            else:                                                     # "ragged": 1 .. 700 rows, slabs of two or three meshes
                lens.append(int(torch.randint(1, 701, (1,), generator=g)))
        seg = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))[:rows]
    n_seg = int(seg[-1]) + 1 + (3 if layout == "sparse_ids" else 0)
    return seg.int(), n_seg


def case_list():
    return [(shape, K, layout, relu) for shape in ("wide", "tall") for K in KS for layout in LAYOUTS[shape] for relu in (False, True)]


def case_name(shape, K, layout, relu):
    return f"{shape}-K{K}-{layout}-{'relu' if relu else 'lin'}"


class DeviceProblem:
    """one (shape, K): inputs on the device; the pre-activations in fp64 on the host (computed when first asked for)"""

    def __init__(self, shape, K):
        from morig_amd import packing
        self.shape, self.K = shape, K
        self.x, self.lin = make_problem(shape, K)
        self.xs = packing.split_f16(self.x).to(DEV)
        self.x_dev = self.x.to(DEV)
        self.lin_dev = packing.to_device(self.lin, DEV)
        self._pre = None

    def pre(self):
        if self._pre is None:
            N, K = SHAPES[self.shape]["N"], self.K
            self._pre = self.x[:, :K].double() @ self.lin.W[:N, :K].double().t()
        return self._pre

    def run(self, ops, layout, relu, split=True):
        from morig_amd.native import Mat
        rows = rows_of(self.shape, layout)
        seg, n_seg = make_seg(layout, rows, seed=rows + self.K)
        pool = torch.full((n_seg, self.lin_dev.W.shape[0]), 7.0, device=DEV)
        X = Mat.of(self.xs if split else self.x_dev, 0, self.K, 0, rows)
        ops.gemm(X, self.lin_dev, relu, seg=seg.to(DEV), pool=pool, x_split=split)
        torch.cuda.synchronize()
        return pool[:, :SHAPES[self.shape]["N"]].cpu()

    def reference(self, layout, relu):
        """relu(X W^T + b) * s + t in fp64, column max per mesh; rows of ids without vertices are 0 (torch_scatter's fill)"""
        N = SHAPES[self.shape]["N"]
        rows = rows_of(self.shape, layout)
        seg, n_seg = make_seg(layout, rows, seed=rows + self.K)
        v = self.pre()[:rows] + self.lin.bias[:N].double()
        if relu:
            v = v.clamp_min(0.0)
        v = v * self.lin.scale[:N].double() + self.lin.shift[:N].double()
        ref = torch.full((n_seg, N), float("-inf"), dtype=torch.float64)
        ref.index_reduce_(0, seg.long(), v, "amax", include_self=True)
        present = torch.zeros(n_seg, dtype=torch.bool)
        present[seg.long()] = True
        ref[~present] = 0.0
        return ref, present


def persistent_rule(rows, N, K):
    """csrc/gemm_dma.hip, launch_gemm16_dma: a pooled split-X launch runs gemm16_dmap_kernel<true> when N is a multiple of 256, K > 32
    and it has more than 256 tiles of 256 x 256; with at most 256 tiles it runs the 128 x 128 one-tile kernel"""
    return N % 256 == 0 and K > 32 and ((rows + TILE - 1) // TILE) * (N // TILE) > 256


# ------------------------------------------------------------------------------------------------------------------- fixtures
_problem = []


def get_problem(shape, K):
    """the (shape, K) problem with its fp64 pre-activations, computed once and shared by the cases that follow (one is kept at a time)"""
    if not _problem or (_problem[0].shape, _problem[0].K) != (shape, K):
        _problem[:] = [DeviceProblem(shape, K)]
    return _problem[0]


@pytest.fixture(scope="module", params=["f16x3", "f32"])
def ops(request):
    from morig_amd import native
    o = native.get_ops()
    prev = o.precision
    o.precision = request.param
    yield o
    o.precision = prev


_children = {}


def child_results(tmp_path_factory):
    """{run length: {case name: pooled result}}: one child process per run length, every case in each (started once per module; after a
    child that failed none is started any more)"""
    if _children:
        if "failed" in _children:
            pytest.fail(_children["failed"])
        return _children
    d = tmp_path_factory.mktemp("pooled_runs")
    for R in RUN_LENGTHS:
        out = str(d / f"run{R}.npz")
        env = dict(os.environ)
        env["MORIG_POOL_RUN"] = str(R)
        env.pop("MORIG_DMA_PERSIST", None)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, timeout=300,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            msg = None if r.returncode == 0 else f"MORIG_POOL_RUN={R}: the child exited with {r.returncode}\n{r.stdout[-2000:]}"
        except subprocess.TimeoutExpired:
            msg = f"MORIG_POOL_RUN={R}: the child ran into its time limit"
        if msg:
            _children["failed"] = msg
            pytest.fail(msg)
        z = np.load(out)
        _children[R] = {k: z[k] for k in z.files}
    return _children


def _child(out):
    from morig_amd import native
    ops = native.get_ops()
    ops.precision = "f16x3"
    res, prob = {}, None
    for shape, K, layout, relu in case_list():
        if prob is None or (prob.shape, prob.K) != (shape, K):
            prob = DeviceProblem(shape, K)
        a = prob.run(ops, layout, relu).numpy()
        b = prob.run(ops, layout, relu).numpy()
        assert a.tobytes() == b.tobytes(), case_name(shape, K, layout, relu)
        res[case_name(shape, K, layout, relu)] = a
    np.savez(out, **res)


# ------------------------------------------------------------------------------------------------------------------- GPU cases
def _check(got, ref, present, what):
    tol = 1e-4 * max(1.0, float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    print(f"{what}: max |diff| {err:.3e}, bound {tol:.3e} (max |ref| {float(ref.abs().max()):.4g})")
    assert not torch.isnan(got).any(), what
    if (~present).any():
        assert float(got[~present].abs().max()) == 0.0, what                                # ids without rows pool to exactly 0
    assert err <= tol, (what, err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,K,layout,relu", case_list(), ids=[case_name(*c) for c in case_list()])
def test_pooled_persistent_layouts(ops, shape, K, layout, relu):
    """every layout against the fp64 reference, on both arithmetic paths; the split-fp16 path must have run the persistent kernel"""
    from morig_amd import native
    problem = get_problem(shape, K)
    fast = ops.precision == "f16x3"
    rows, N = rows_of(problem.shape, layout), SHAPES[problem.shape]["N"]
    ref, present = problem.reference(layout, relu)
    assert (ref[present][:, 2] < 0).all() and (ref[present][:, 3] < 0).all()                     # the all-negative columns are
    assert float(problem.lin.scale[0]) == 0.0 and (problem.lin.scale[:N] < 0).any()              # there, so is the zero scale
    native.prof_enable(True)
    native.prof_reset()
    try:
        got = problem.run(ops, layout, relu, split=fast)
        kinds = native.prof_collect()
    finally:
        native.prof_enable(False)
    if fast:
        assert persistent_rule(rows, N, problem.K)
        assert "gemm_f16x3_pool" in kinds and kinds["gemm_f16x3_pool"]["symbol"].startswith("gemm16_dmap_kernel<true>"), kinds
        assert "gemm_f16x3_dma128" not in kinds, kinds
    again = problem.run(ops, layout, relu, split=fast)
    assert got.numpy().tobytes() == again.numpy().tobytes()
    _check(got, ref, present, f"{case_name(problem.shape, problem.K, layout, relu)} [{ops.precision}]")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,K", [(s, K) for s in ("wide", "tall") for K in KS])
def test_pooled_run_lengths_agree_bit_for_bit(shape, K, tmp_path_factory):
    """run lengths 1 (a run is a tile: the former order), 2 and 16, forced in child processes: identical to each other and to this
    process, and each within the criterion of the fp64 reference"""
    from morig_amd import native
    res = child_results(tmp_path_factory)
    problem = get_problem(shape, K)
    ops = native.get_ops()
    prev, ops.precision = ops.precision, "f16x3"
    try:
        mine = {c: problem.run(ops, c[2], c[3]).numpy() for c in case_list() if c[:2] == (shape, K)}
    finally:
        ops.precision = prev
    for (_, _, layout, relu), got in mine.items():
        name = case_name(shape, K, layout, relu)
        base = res[RUN_LENGTHS[0]][name]
        for R in RUN_LENGTHS[1:]:
            assert res[R][name].tobytes() == base.tobytes(), (name, R)
        assert got.tobytes() == base.tobytes(), name
        ref, present = problem.reference(layout, relu)
        _check(torch.from_numpy(res[RUN_LENGTHS[-1]][name]), ref, present, f"{name} [run 16]")


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("layout", LAYOUTS["small"])
def test_pooled_one_tile_kernel(K, layout, relu):
    """M = 1000, N = 256: four tiles of 256 x 256, which the launcher gives to the one-tile-per-workgroup kernel (gemm_dma.hip) -- the
    same pooled epilogue without runs"""
    from morig_amd import native
    ops = native.get_ops()
    prev, ops.precision = ops.precision, "f16x3"
    prob = get_problem("small", K)
    rows = rows_of("small", layout)
    assert not persistent_rule(rows, SHAPES["small"]["N"], K)
    native.prof_enable(True)
    native.prof_reset()
    try:
        got = prob.run(ops, layout, relu)
        kinds = native.prof_collect()
        again = prob.run(ops, layout, relu)
    finally:
        native.prof_enable(False)
        ops.precision = prev
    assert "gemm_f16x3_dma128" in kinds and kinds["gemm_f16x3_dma128"]["symbol"].startswith("gemm16_dma_kernel<128, 128"), kinds
    assert got.numpy().tobytes() == again.numpy().tobytes()
    ref, present = prob.reference(layout, relu)
    _check(got, ref, present, f"{case_name('small', K, layout, relu)} [one tile]")


# ------------------------------------------------------------------------------------------------------------------- the run list, on the host
RUN_LIST_CHECK = r"""
#include "pool_runs.h"
#include <cstdio>
#include <vector>
using namespace morig;
int main() {
    const int TM[] = {1, 15, 16, 17, 1000, 5120}, TN[] = {1, 2, 4}, GRID[] = {8, 32, 248, 256}, RR[] = {1, 2, 16};
    long checked = 0;
    for (int tiles_m : TM) for (int tiles_n : TN) for (int grid : GRID) for (int R : RR) {
        const int T = tiles_m * tiles_n, units = pool_run_units(tiles_m, tiles_n, R);
        std::vector<int> seen(T, 0);
        long total = 0;
        for (int block = 0; block < grid; ++block) {
            int first, end, stride, mine = 0, prev_lin = -1;
            pool_wg_runs(units, grid, block, first, end, stride);
            for (int u = first; u < end; u += stride) {
                const int cb = pool_run_col_block(u, tiles_n), n = pool_run_count(u, tiles_m, tiles_n, R);
                int lin = pool_run_first_tile(u, tiles_n, R);
                if (n < 1 || n > R || cb < 0 || cb >= tiles_n) { std::printf("bad run %d: count %d, column block %d\n", u, n, cb); return 1; }
                for (int k = 0; k < n; ++k, lin += tiles_n) {                       // the kernel's walk: + tiles_n per tile
                    if (lin < 0 || lin >= T) { std::printf("tile %d outside 0..%d\n", lin, T); return 1; }
                    if (lin % tiles_n != cb) { std::printf("run %d leaves its column block\n", u); return 1; }
                    if (k > 0 && lin / tiles_n != prev_lin / tiles_n + 1) { std::printf("run %d skips a row tile\n", u); return 1; }
                    ++seen[lin]; ++mine; prev_lin = lin;
                }
            }
            if (mine != pool_wg_tiles(tiles_m, tiles_n, R, grid, block)) { std::printf("pool_wg_tiles disagrees for block %d\n", block); return 1; }
            if (R == 1) {                                                           // R = 1: the store launches' list
                const int xcd = block & 7, bi = block >> 3, nbx = grid >> 3;
                const int t_lo = (int)((long long)T * xcd / 8), t_hi = (int)((long long)T * (xcd + 1) / 8);
                const int n_my = (t_hi - t_lo - bi + nbx - 1) / nbx;
                if (mine != (n_my > 0 ? n_my : 0) || (mine > 0 && (first != t_lo + bi || stride != nbx || pool_run_first_tile(first, tiles_n, 1) != first))) {
                    std::printf("run length 1 is not the former order (block %d)\n", block); return 1;
                }
            }
            total += mine;
        }
        for (int t = 0; t < T; ++t)
            if (seen[t] != 1) { std::printf("tiles_m %d tiles_n %d grid %d R %d: tile %d visited %d times\n", tiles_m, tiles_n, grid, R, t, seen[t]); return 1; }
        if (total != T) return 1;
        // the launcher's choice: a power of two, and two runs for every workgroup unless it fell to 1
        const int L = pool_run_length(tiles_m, tiles_n, grid, 16);
        if (L < 1 || L > 16 || (L & (L - 1))) { std::printf("run length %d\n", L); return 1; }
        if (L > 1) for (int block = 0; block < grid; ++block) {
            int first, end, stride;
            pool_wg_runs(pool_run_units(tiles_m, tiles_n, L), grid, block, first, end, stride);
            if (first + stride >= end) { std::printf("tiles_m %d tiles_n %d grid %d: block %d has fewer than two runs at %d\n", tiles_m, tiles_n, grid, block, L); return 1; }
        }
        if (pool_run_length(tiles_m, tiles_n, 0, R) != R) return 1;                 // a forced length is taken as it is
        ++checked;
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
"""


def test_run_list_visits_every_tile_once(tmp_path):
    src, exe = str(tmp_path / "pool_runs_check.cpp"), str(tmp_path / "pool_runs_check")
    with open(src, "w") as f:
        f.write(RUN_LIST_CHECK)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "morig_amd", "csrc"), src, "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    assert done.stdout.strip() == f"ok {6 * 3 * 4 * 3}"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: test_gpu_pooled_runs.py child OUT.npz")
