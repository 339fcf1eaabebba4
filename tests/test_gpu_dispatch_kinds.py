"""GPU: which kernel every arm of the GEMM / EdgeConv launch plans (csrc/dispatch_core.h) takes, seen from outside the library: one
smallest launch per arm through the public op layer with the live profiling on, then the kind name and kernel symbol that
``native.prof_collect()`` reports for it -- recorded with no switch set before the plans were written down in one place -- and the result
against a float64 product at the tolerance tests/test_gpu_kernels.py uses for that engine (2e-5 of the scale: another summation order;
3e-6 for the few-rows kernel and the bf16 x 6 split, which are float32-class).
What this resolves: the KIND of a launch. The symbol is morig_prof_symbol(kind), a fixed string per kind and not the kernel that ran (the
pooled tile launch reports the persistent pooled kernel's, the bf16 x 6 arms the fp32 tile's), so a launch that moves to a kernel of
another kind fails here, while arms that share a kind are told apart by their results only: h32_folded_x3 / h32_affine, dma256_store /
dma256_tail, tile_pool / persistent_pool, and the f32 / bf16 x 6 tiles. Which kernel each of those takes is held by
tools/dispatch_host_check.cpp on the plans themselves.
Graphs have 64 vertices and 200 edges, GEMMs 130 rows unless the arm needs more."""
import pytest
import torch

from morig_amd import native, packing
from morig_amd.native import Mat

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = "tile_kernel<%d, %d, %d, %d, %d,"


@pytest.fixture()
def ops():
    o = native.get_ops()
    prev = (o.precision, o.exact_arith)
    native.prof_enable(True)
    yield o
    native.prof_enable(False)
    o.precision, o.exact_arith = prev


def _one_launch(fn):
    """run fn with a clean account -> the (kind name, launches, symbol) it left"""
    torch.cuda.synchronize()
    native.prof_reset()
    fn()
    torch.cuda.synchronize()
    return sorted((k, v["launches"], v["symbol"]) for k, v in native.prof_collect().items())


# ---- morig_gemm ------------------------------------------------------------------------------------------------------------------
def _lin(N, K, seed, bf16=False):
    g = torch.Generator().manual_seed(seed)
    p = packing.pack_linear(torch.randn(N, K, generator=g) / (K ** 0.5), torch.randn(N, generator=g) * 0.1)
    Np = p.W.shape[0]
    p.scale = torch.randn(Np, generator=g) if p.scale is None else p.scale * torch.randn(Np, generator=g)
    p.shift = torch.randn(Np, generator=g) * 0.2
    if bf16:
        p.Wsplit_bf16 = packing.split_bf16(p.W)
    return p


def _gemm_ref(x, lin, relu=True):
    ref = x.double() @ lin.W[:lin.N, :lin.K].double().t() + lin.bias[:lin.N].double()
    if relu:
        ref = ref.clamp_min(0.0)
    return ref * lin.scale[:lin.N].double() + lin.shift[:lin.N].double()


def _close(got, ref, tol):
    err = (got.detach().cpu().double() - ref).abs().max().item()
    assert err <= tol * max(1.0, ref.abs().max().item()), (err, tol)


# arm: (M, N, K, precision, exact_arith, form, kind, symbol, tolerance)
GEMM_ARMS = {
    "few_rows":        (8, 128, 128, "f16x3", "bf16x6", "plain", "misc", None, 3e-6),
    "tile_f16_bn32":   (130, 32, 32, "f16x3", "bf16x6", "plain", "gemm_f16x3_bn32", TILE % (32, 32, 0, 0, 1), 2e-5),
    "tile_f16_bn64":   (130, 64, 32, "f16x3", "bf16x6", "plain", "gemm_f16x3_bn64", TILE % (64, 32, 0, 0, 1), 2e-5),
    "tile_f16_bn128":  (130, 128, 32, "f16x3", "bf16x6", "plain", "gemm_f16x3_bn128", TILE % (128, 32, 0, 0, 1), 2e-5),
    "tile_x6_bn32":    (130, 32, 32, "f32", "bf16x6", "plain", "gemm_f32_bn32", TILE % (32, 32, 0, 0, 0), 3e-6),
    "tile_x6_bn64":    (130, 64, 32, "f32", "bf16x6", "plain", "gemm_f32_bn64", TILE % (64, 32, 0, 0, 0), 3e-6),
    "tile_x6_bn128":   (130, 128, 32, "f32", "bf16x6", "plain", "gemm_f32_bn128", TILE % (128, 32, 0, 0, 0), 3e-6),
    "tile_f32_bn32":   (130, 32, 32, "f32", "f32", "plain", "gemm_f32_bn32", TILE % (32, 32, 0, 0, 0), 2e-5),
    "tile_f32_bn64":   (130, 64, 32, "f32", "f32", "plain", "gemm_f32_bn64", TILE % (64, 32, 0, 0, 0), 2e-5),
    "tile_f32_bn128":  (130, 128, 32, "f32", "f32", "plain", "gemm_f32_bn128", TILE % (128, 32, 0, 0, 0), 2e-5),
    "tile_bf16_image": (130, 64, 32, "f16x3", "bf16x6", "bf16", "misc", None, 2e-5),
    "tile_pool":       (130, 128, 32, "f16x3", "bf16x6", "pool", "gemm_f16x3_pool", "gemm16_dmap_kernel<true>", 2e-5),
    "dma128":          (130, 128, 32, "f16x3", "bf16x6", "split", "gemm_f16x3_dma128", "gemm16_dma_kernel<128, 128, 2, 2", 2e-5),
    "dma128_few_tiles": (256, 256, 32, "f16x3", "bf16x6", "split", "gemm_f16x3_dma128", "gemm16_dma_kernel<128, 128, 2, 2", 2e-5),
    "dma256_store":    (65792, 256, 64, "f16x3", "bf16x6", "split", "gemm_f16x3_dma", "gemm16_dma_kernel<256, 256, 4, 2", 2e-5),
    "dma256_tail":     (65792, 256, 64, "f16x3", "bf16x6", "tail", "gemm_f16x3_dma", "gemm16_dma_kernel<256, 256, 4, 2", 2e-5),
    "persistent_store": (16640, 1024, 768, "f16x3", "bf16x6", "split", "gemm_f16x3_dmap", "gemm16_dmap_kernel<false>", 2e-5),
    "persistent_pool": (65792, 256, 64, "f16x3", "bf16x6", "split_pool", "gemm_f16x3_pool", "gemm16_dmap_kernel<true>", 2e-5),
}


@pytest.mark.parametrize("arm", sorted(GEMM_ARMS))
def test_gemm_arm_runs_the_recorded_kernel(ops, arm):
    M, N, K, precision, exact, form, kind, symbol, tol = GEMM_ARMS[arm]
    ops.precision, ops.exact_arith = precision, exact
    g = torch.Generator().manual_seed(M + N + K)
    lin = _lin(N, K, 3, bf16=form == "bf16")
    ling = packing.to_device(lin, DEV)
    x = torch.randn(M, K, generator=g)
    ref = _gemm_ref(x, lin)
    if form in ("pool", "split_pool"):
        seg = (torch.arange(M) * 3 // M).int()                       # three meshes, sorted
        ref = torch.stack([ref[seg.long() == s].max(dim=0)[0] for s in range(3)])
        got = torch.zeros(3, N, device=DEV)
        xg = (packing.split_f16(x) if form == "split_pool" else x).to(DEV)
        call = lambda: ops.gemm(Mat.of(xg, 0, K), ling, True, seg=seg.to(DEV), pool=got, x_split=form == "split_pool")
    elif form == "tail":
        rows = M // 64                                              # 64 replicas read one copy of the last 32 columns
        xt = torch.randn(rows, 32, generator=g)
        ref = _gemm_ref(torch.cat([x[:, :K - 32], xt.repeat(64, 1)], dim=1), lin)
        xg, tg = packing.split_f16(x[:, :K - 32].contiguous()).to(DEV), packing.split_f16(xt).to(DEV)
        got = torch.zeros(M, N, device=DEV)
        assert ops.gemm_takes_tail(ling, Mat.of(got), 32)
        call = lambda: ops.gemm(Mat.of(xg), ling, True, Y=Mat.of(got), x_split=True, x_tail=Mat.of(tg))
    else:
        xg = (packing.split_f16(x) if form == "split" else x).to(DEV)
        got = torch.zeros(M, N, device=DEV)
        call = lambda: ops.gemm(Mat.of(xg, 0, K), ling, True, Y=Mat.of(got), x_split=form == "split")
    ran = _one_launch(call)
    print(arm, ran)
    assert ran == [(kind, 1, symbol)]
    _close(got, ref, tol)


# ---- the EdgeConv family -----------------------------------------------------------------------------------------------------------
def _graph(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, 64, (200,), generator=g), torch.randint(0, 64, (200,), generator=g)])


def _edge_pack(H, seed, folded):
    g = torch.Generator().manual_seed(seed)
    Hp, Kp = max(H, 32), (H + 31) // 32 * 32
    W2 = torch.zeros(Hp, Kp)
    W2[:H, :H] = torch.randn(H, H, generator=g) / (H ** 0.5)

    def vec(n, fill, v):
        out = torch.full((n,), fill)
        out[:H] = v
        return out
    s1, t1 = vec(Kp, 1.0, torch.randn(H, generator=g)), vec(Kp, 0.0, torch.randn(H, generator=g) * 0.2)
    pe = packing.PackedEdge(H, s1, t1, W2, vec(Hp, 0.0, torch.randn(H, generator=g) * 0.1), vec(Hp, 1.0, torch.randn(H, generator=g)),
                            vec(Hp, 0.0, torch.randn(H, generator=g) * 0.2))
    if folded:
        pe.s1 = pe.t1 = None
    pe.W2split = packing.split_f16(W2) if H >= 32 else None
    return pe


def _hidden_ref(a, b, csr, ec):
    """float64 per-edge rows z = s2 relu(W2 (s1 relu(A[dst] + B[src]) + t1) + b2) + t2 of the CSR's live rows, and their targets"""
    H, E = ec.H, int(csr.rowptr[-1])
    src, dst = csr.src[:E].cpu().long(), csr.dst[:E].cpu().long()
    h = torch.relu(a.double()[dst] + b.double()[src])
    if ec.s1 is not None:
        h = h * ec.s1[:H].double() + ec.t1[:H].double()
    z = torch.relu(h @ ec.W2[:H, :H].double().t() + ec.b2[:H].double()) * ec.s2[:H].double() + ec.t2[:H].double()
    return z, dst


def _segmax(z, dst):
    out = torch.full((64, z.shape[1]), float("-inf"), dtype=torch.float64)
    return out.scatter_reduce(0, dst[:, None].expand(-1, z.shape[1]), z, reduce="amax", include_self=True)


# arm: (H, hidden affine folded, CSR form, output form, kind, symbol)
EDGE_ARMS = {
    "h16":            (16, False, "plain", "rows", "edgeconv_h16", TILE % (32, 16, 1, 2, 0)),
    "h32_folded_x3":  (32, True, "plain", "rows", "edgeconv_f16x3_h32", TILE % (32, 32, 1, 2, 1)),
    "h32_affine":     (32, False, "plain", "rows", "edgeconv_f16x3_h32", TILE % (32, 32, 1, 2, 1)),
    "h64":            (64, True, "plain", "rows", "edgeconv_f16x3_h64", TILE % (64, 32, 1, 2, 1)),
    "h128_pad4_rl":   (128, True, "pad4", "rows", "edgeconv_f16x3_h128_rl", "edge_rl128_kernel"),
    "h128_plain_pp":  (128, True, "plain", "rows", "edgeconv_f16x3_h128", "edge_pp_kernel<128"),
    "h256_pad4_ws":   (256, True, "pad4", "rows", "edgeconv_f16x3_h256", "edge_ws_kernel<256"),
    "h256_min4_mix":  (256, True, "min4", "split", "edgeconv_f16x3_h256", "edge_ws_kernel<256"),
    "h256_plain_pp":  (256, True, "plain", "rows", "edgeconv_f16x3_h256_pp", "edge_pp_kernel<256"),
    "h256_misaligned_pc": (256, True, "plain", "misaligned", "edgeconv_f16x3_pc", "edge_pc_kernel"),
}


@pytest.mark.parametrize("arm", sorted(EDGE_ARMS))
def test_edgeconv_arm_runs_the_recorded_kernel(ops, arm):
    H, folded, form, out_form, kind, symbol = EDGE_ARMS[arm]
    ops.precision = "f16x3"
    g = torch.Generator().manual_seed(H)
    ab = torch.randn(64, 2 * H, generator=g)
    ec = _edge_pack(H, 5, folded)
    csr = ops.csr_build(_graph(H).to(DEV), 64, pad4=form == "pad4", min4=form == "min4")
    z, dst = _hidden_ref(ab[:, :H], ab[:, H:], csr, ec)
    abg, ecg = ab.to(DEV), packing.to_device(ec, DEV)
    col0 = 3 if out_form == "misaligned" else 0
    out = torch.zeros(64, H + 32, device=DEV)
    A, B, O = Mat.of(abg, 0, H), Mat.of(abg, H, H), Mat.of(out, col0, H)
    if out_form == "split":
        assert ops.edgeconv_can_split_out(A, B, csr, ecg, O)
    ran = _one_launch(lambda: ops.edgeconv(A, B, csr, ecg, O, out_split=out_form == "split"))
    print(arm, ran)
    assert ran == [(kind, 1, symbol)]
    got = packing.unsplit_f16(out.cpu(), H) if out_form == "split" else out[:, col0:col0 + H]
    _close(got, _segmax(z, dst), 2e-5)


def test_pointconv_passes_run_the_recorded_kernels(ops):
    """morig_edge_hidden at H = 64, then morig_segmax_gemm at N = 64 on its rows"""
    ops.precision = "f16x3"
    g = torch.Generator().manual_seed(64)
    ab = torch.randn(64, 128, generator=g)
    ec, lin = _edge_pack(64, 6, False), _lin(64, 64, 7)
    csr = ops.csr_build(_graph(9).to(DEV), 64)
    z, dst = _hidden_ref(ab[:, :64], ab[:, 64:], csr, ec)
    abg = ab.to(DEV)
    zg = torch.zeros(csr.capacity, 64, device=DEV)
    ran = _one_launch(lambda: ops.edge_hidden(Mat.of(abg, 0, 64), Mat.of(abg, 64, 64), csr, packing.to_device(ec, DEV), Mat.of(zg)))
    print("edge_hidden", ran)
    assert ran == [("pointconv_f16x3", 1, None)]
    _close(zg[:z.shape[0]], z, 2e-5)
    og = torch.zeros(64, 64, device=DEV)
    ran = _one_launch(lambda: ops.segmax_gemm(Mat.of(zg), packing.to_device(lin, DEV), True, csr, Mat.of(og)))
    print("segmax_gemm", ran)
    assert ran == [("pointconv_f16x3", 1, None)]
    _close(og, _segmax(_gemm_ref(zg[:z.shape[0]].cpu(), lin), dst), 2e-5)


@pytest.mark.parametrize("col0,kind,symbol", [(0, "edgeconv_f16x3_x3_persistent", "edge_x3_kernel"),
                                              (1, "edgeconv_f16x3_x3", TILE % (32, 32, 2, 2, 1))])
def test_edgeconv_x3_arm_runs_the_recorded_kernel(ops, col0, kind, symbol):
    """16-byte aligned output rows: the persistent kernel; a misaligned window: the tile engine"""
    ops.precision = "f16x3"
    g = torch.Generator().manual_seed(3)
    x = torch.zeros(64, 4)
    x[:, :3] = torch.randn(64, 3, generator=g)
    W1a, W1b, b1 = torch.zeros(32, 4), torch.zeros(32, 4), torch.randn(32, generator=g) * 0.2
    W1a[:, :3], W1b[:, :3] = torch.randn(32, 3, generator=g), torch.randn(32, 3, generator=g)
    ec = _edge_pack(32, 8, True)
    csr = ops.csr_build(_graph(4).to(DEV), 64)
    a = x[:, :3].double() @ W1a[:, :3].double().t() + b1.double()
    z, dst = _hidden_ref(a, x[:, :3].double() @ W1b[:, :3].double().t(), csr, ec)
    out = torch.zeros(64, 36, device=DEV)
    ran = _one_launch(lambda: ops.edgeconv_x3(Mat.of(x.to(DEV)), (W1a.to(DEV), W1b.to(DEV), b1.to(DEV)), csr, packing.to_device(ec, DEV),
                                              Mat.of(out, col0, 32)))
    print("edgeconv_x3", col0, ran)
    assert ran == [(kind, 1, symbol)]
    _close(out[:, col0:col0 + 32], _segmax(z, dst), 2e-5)
