"""ctypes binding of libmorig_hip.so (the C ABI in include/morig_hip.h) + the op layer the
network plans are written against.

There is NO fallback: if the shared library is missing, or a tensor is not on a ROCm device, the
product path raises. (tests/ inject a torch emulation of the *same op interface* to check the host
logic on CPU; that emulation lives under tests/ and is never importable from here.)
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import threading
from dataclasses import dataclass
from typing import Optional

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MORIG_HIP_LIB") or os.path.join(_HERE, "lib", "libmorig_hip.so")   # env: A/B builds

# The argument structs, the exports' signatures and the MORIG_* constants are what include/morig_hip.h declares: abi.py reads the header.
_K = abi.CONSTANTS
MorigNativeError = abi.MorigNativeError
GemmArgs = abi.STRUCTS["morig_gemm_args"]
EdgeConvArgs = abi.STRUCTS["morig_edgeconv_args"]
EdgeConvX3Args = abi.STRUCTS["morig_edgeconv_x3_args"]
PointConvArgs = abi.STRUCTS["morig_pointconv_args"]
SegmaxArgs = abi.STRUCTS["morig_segmax_args"]
IkArgs = abi.STRUCTS["morig_ik_args"]
NceArgs = abi.STRUCTS["morig_nce_args"]
LogRatioArgs = abi.STRUCTS["morig_logratio_args"]
EXPORTS = tuple(abi.SIGNATURES)
ABI_VERSION = _K["MORIG_ABI_VERSION"]
_lib = None


def _args(cls):
    """a zeroed argument struct with its struct_size set (ABI 3: the library refuses a struct shorter than its version-3 layout and reads
    members past struct_size as zero, include/morig_hip.h)"""
    a = cls()
    a.struct_size = C.sizeof(cls)
    return a


def load_library(path: str = LIB_PATH):
    """dlopen libmorig_hip.so and type every export. Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise MorigNativeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C morig_amd/csrc`). There is no CPU fallback for the MoRig forward path.")
    lib = C.CDLL(path)
    for name, (res, args) in abi.SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError if the header and the build disagree
        fn.restype, fn.argtypes = res, args
    if lib.morig_abi_version() != ABI_VERSION:
        raise MorigNativeError(f"libmorig_hip.so ABI version {lib.morig_abi_version()}, this binding is written against {ABI_VERSION} "
                               "(argument structs start with struct_size since 3): rebuild with `make -C morig_amd/csrc`")
    _lib = lib
    return lib


def library_path() -> str:
    """the file load_library() maps (MORIG_HIP_LIB selects an A/B build)"""
    return LIB_PATH


def check(status: int, what: str) -> None:
    if status != 0:
        lib = load_library()
        msg = lib.morig_strerror(status).decode()
        if status == _K["MORIG_E_HIP"]:
            msg += f" [hipError_t={lib.morig_last_hip_error()}]"
        raise MorigNativeError(f"{what}: {msg}")


PAIR_PASSES = os.environ.get("MORIG_EDGE_PAIR", "1") != "0"


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------
# the op interface the plans use
# ---------------------------------------------------------------------------------------------
@dataclass
class Mat:
    """A column window of a row-major fp32 2-D tensor: rows [row0, row0+rows), cols [col0, col0+cols)."""
    base: torch.Tensor
    row0: int
    col0: int
    rows: int
    cols: int

    @staticmethod
    def of(t: torch.Tensor, col0: int = 0, cols: Optional[int] = None, row0: int = 0, rows: Optional[int] = None) -> "Mat":
        assert t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1, "need a row-major fp32 matrix"
        cols = t.shape[1] - col0 if cols is None else cols
        rows = t.shape[0] - row0 if rows is None else rows
        assert 0 <= col0 and col0 + cols <= t.shape[1] and 0 <= row0 and row0 + rows <= t.shape[0]
        return Mat(t, row0, col0, rows, cols)

    @property
    def ld(self) -> int:
        return self.base.stride(0)

    @property
    def ptr(self) -> int:
        return self.base.data_ptr() + 4 * (self.row0 * self.ld + self.col0)

    def view(self) -> torch.Tensor:
        return self.base[self.row0:self.row0 + self.rows, self.col0:self.col0 + self.cols]


@dataclass
class CSR:
    rowptr: torch.Tensor      # int32 [n+1]
    src: torch.Tensor         # int32 [cap]
    dst: torch.Tensor         # int32 [cap]
    n_nodes: int
    capacity: int
    status: torch.Tensor      # int32 [1], non-zero = index out of range (read once per forward by NativeOps.guarded)
    edge_count: int = 0       # exact E' when known (accounting only)
    quad: bool = False        # segments padded to multiples of 4 (MORIG_CSR_PAD4)
    min4: bool = False        # segments of at least 4 rows, not aligned (MORIG_CSR_MIN4: the mixed-quad form of the H = 256 EdgeConv kernel)
    _transposed: Optional[tuple] = None

    def transposed(self, n_src: Optional[int] = None):
        """-> (rowptr_t int32 [n_src + 1], perm_t int32 [capacity]): the same edges grouped by SOURCE, perm_t[k] = the row of this CSR
        holding the k-th edge in (source, row) order -- what ``edge_bn_scatter_backward`` walks to sum the gradient of the source
        side in a fixed order. Built once per graph with stream-ordered torch calls (stable sort; no host read: the live row count
        stays on the device, rows past it sort behind every vertex)."""
        n_src = self.n_nodes if n_src is None else n_src
        if self._transposed is None or self._transposed[0] != n_src:
            dev = self.src.device
            live = self.rowptr[self.n_nodes]
            pos = torch.arange(self.capacity, device=dev)
            keys = torch.where(pos < live, self.src.long().clamp(0, n_src), torch.full((), n_src, dtype=torch.int64, device=dev))
            skeys, order = torch.sort(keys, stable=True)
            rowptr_t = torch.searchsorted(skeys, torch.arange(n_src + 1, device=dev)).int()
            self._transposed = (n_src, rowptr_t.contiguous(), order.int().contiguous())
        return self._transposed[1], self._transposed[2]


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def padded_for_pool(lin):
    """A pooled morig_gemm launch always runs the 128-column tile and reads W / bias / scale / shift up to the next multiple of 128
    rows, whatever N is: a packed layer with fewer rows (N <= 64 packs to 32 or 64) gets zero rows appended, once, kept on the layer.
    Without them the launch reads past the end of the weight image."""
    rows = lin.W.shape[0]
    if rows % 128 == 0:
        return lin
    cached = lin.__dict__.get("_pool128")
    if cached is None:
        pad = 128 - rows % 128

        def grow(t, fill=0.0):
            if t is None:
                return None
            return torch.cat([t, torch.full((pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)]).contiguous()
        cached = dataclasses.replace(lin, W=grow(lin.W), bias=grow(lin.bias), scale=grow(lin.scale, 1.0), shift=grow(lin.shift),
                                     Wsplit=grow(lin.Wsplit), Wsplit_bf16=grow(lin.Wsplit_bf16))
        lin.__dict__["_pool128"] = cached
    return cached


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise MorigNativeError("the MoRig native forward path needs ROCm device tensors (no CPU fallback); "
                                   "move the model and data to 'cuda'")


class PendingGuard:
    """What a forward enqueued with ``NativeOps.guarded_async`` leaves behind: ONE small device tensor [range flag, CSR status
    words ...] snapshotted on the stream behind the forward's last launch. ``result()`` is the host read the synchronous guard
    does at the end of every forward -- a serving loop calls it AFTER it has enqueued the next forward, so the GPU never idles
    on it. -> True: results valid; False: an operand left the split-fp16 range (re-run on the fp32 path); raises on a bad index."""

    def __init__(self, snapshot: torch.Tensor):
        self.snapshot = snapshot
        self._done = None

    def result(self) -> bool:
        if self._done is None:
            words = self.snapshot.tolist()
            if any(w != 0 for w in words[1:]):
                raise MorigNativeError("edge_index / neighbour index out of range for the vertex count it was built with "
                                       "(morig_csr_build status %s)" % [w for w in words[1:] if w != 0][:4])
            self._done = words[0] == 0
        return self._done


class NativeOps:
    """Thin, validating wrappers: tensors in, C ABI calls out, everything on the current stream."""

    name = "hip"

    def __init__(self):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise MorigNativeError("no ROCm device visible: the MoRig forward path has no CPU fallback")
        # arithmetic of the MFMA contractions: "f16x3" = split-fp16 fast path with overflow guard
        # (default), "f32" = fp32 MFMA everywhere. MORIG_PRECISION overrides.
        self.precision = os.environ.get("MORIG_PRECISION", "f16x3")
        assert self.precision in ("f16x3", "f32")
        # arithmetic of the EXACT path (precision "f32", the re-run behind the range guard, the train-mode forward): "bf16x6" = both fp32
        # operands split into three bf16 limbs in the kernel, six MFMAs per product (float32-class products, float32's range, 2.7x the
        # fp32-MFMA rate: MORIG_SPLIT_BF16X6); "f32" = v_mfma_f32_32x32x2_f32. MORIG_EXACT_ARITH overrides.
        self.exact_arith = os.environ.get("MORIG_EXACT_ARITH", "bf16x6")
        assert self.exact_arith in ("bf16x6", "f32")
        # guard state is PER THREAD (two threads / streams may run forwards concurrently on the one NativeOps): nesting depth,
        # forced-fp32 switch, the CSR status words of the forward in flight and the overflow flag word of each device
        self._tls = threading.local()
        # accounting only (bench.py): exact self-loop-normalised edge counts E' per input graph, learned during
        # warm-up with one host read each, so the live FLOP counters use ALGORITHMIC edges (no capacity, no padding)
        self.learn_edge_counts = False
        self._edge_counts = {}

    # -- split-fp16 guard -------------------------------------------------------------------------
    @property
    def fast(self) -> bool:
        return self.precision == "f16x3" and not self._force_f32

    @property
    def split_activations(self) -> bool:
        """plans keep GEMM->GEMM activations in the split-fp16 layout while the fast path is active"""
        return self.fast and os.environ.get("MORIG_SPLIT_ACT", "1") != "0"

    def _state(self):
        t = self._tls
        if not hasattr(t, "depth"):
            t.depth, t.force_f32, t.csr_status, t.ovf = 0, False, None, {}
        return t

    @property
    def _depth(self):
        return self._state().depth

    @_depth.setter
    def _depth(self, v):
        self._state().depth = v

    @property
    def _force_f32(self):
        return self._state().force_f32

    @_force_f32.setter
    def _force_f32(self, v):
        self._state().force_f32 = v

    @property
    def _csr_status(self):
        return self._state().csr_status

    @_csr_status.setter
    def _csr_status(self, v):
        self._state().csr_status = v

    def _flag(self, device) -> torch.Tensor:
        ovf = self._state().ovf
        key = (device.type, device.index)
        if key not in ovf:
            ovf[key] = torch.zeros(1, dtype=torch.int32, device=device)
        return ovf[key]

    def guarded(self, device, fn, rerun: bool = True, retry=None):
        """Run ``fn()`` (a whole forward) on the fast path; if any kernel reported an operand outside the
        fp16 range, run it again on the exact path. Nested calls run inside the outer guard.
        retry (optional callable -> bool): asked after a range overflow BEFORE the exact path is taken; True = the caller changed
        something (the rig networks raise their range shift: morig_amd.models.basic_modules.NativeModule.forward) and the fast
        path is worth another attempt, False = give up and run exactly.
        rerun=False (train-mode forward: it has side effects on the BatchNorm running buffers, so it must run ONCE):
        the whole forward runs on the exact fp32 MFMA path."""
        if self._depth > 0:
            return fn()
        if not rerun:
            old = self._force_f32
            self._force_f32 = True
            try:
                return self._run_once(device, fn)
            finally:
                self._force_f32 = old
        if not self.fast:
            return self._run_once(device, fn)          # exact-fp32 mode: no range flag to read, but the CSR status words still are
        flag = self._flag(device)
        while True:
            flag.zero_()
            self._depth += 1
            self._csr_status = []
            try:
                out = fn()
            finally:
                self._depth -= 1
                stats, self._csr_status = self._csr_status, None
            # ONE small D2H read per forward: the split-fp16 range flag and the status word of every CSR built on the way
            # (an out-of-range / negative edge or ball-query index is dropped by the count and fill kernels; the reference would
            # raise an index error, so does this)
            words = torch.cat([flag] + stats).tolist() if stats else [int(flag.item())]
            if any(w != 0 for w in words[1:]):
                raise MorigNativeError("edge_index / neighbour index out of range for the vertex count it was built with "
                                       "(morig_csr_build status %s)" % [w for w in words[1:] if w != 0][:4])
            if words[0] == 0 or retry is None or not retry():
                break
        if words[0] != 0:
            self._force_f32 = True
            try:
                out = fn()
            finally:
                self._force_f32 = False
        return out

    def guarded_async(self, device, fn):
        """``fn()`` (a whole eval forward) on the fast path WITHOUT the host read at its end -> (outputs, PendingGuard).
        The flag and the CSR status words of this forward are copied into a fresh tensor on the stream, so the next forward may
        be enqueued (it clears the shared flag word) before ``PendingGuard.result()`` is called. Also what a HIP-graph capture
        of a forward runs through (no host read inside a capture; every replay refreshes the snapshot)."""
        assert self._depth == 0, "guarded_async is for the outermost forward"
        flag = self._flag(device)
        flag.zero_()
        self._depth += 1
        self._csr_status = []
        try:
            out = fn()
        finally:
            self._depth -= 1
            stats, self._csr_status = self._csr_status, None
        return out, PendingGuard(torch.cat([flag] + stats))

    def _run_once(self, device, fn):
        """one pass with the CSR status words checked (no precision flag: the fp32 path cannot overflow fp16)"""
        self._depth += 1
        self._csr_status = []
        try:
            out = fn()
        finally:
            self._depth -= 1
            stats, self._csr_status = self._csr_status, None
        if stats and any(w != 0 for w in torch.cat(stats).tolist()):
            raise MorigNativeError("edge_index / neighbour index out of range for the vertex count it was built with")
        return out

    # -- allocation (PyTorch owns all device memory) -------------------------------------------
    def empty(self, rows, cols, device, dtype=torch.float32):
        return torch.empty((rows, cols), device=device, dtype=dtype)

    # -- graph --------------------------------------------------------------------------------
    def csr_build(self, edge_index: torch.Tensor, n_nodes: int, n_src: Optional[int] = None,
                  skip_negative: bool = False, pad4: bool = False, min4: bool = False) -> CSR:
        """pad4: pad every target's segment to a multiple of 4 by repeating its self loop (exact for
        max-aggregation); enables the in-register quad reduction of the EdgeConv epilogue.
        min4: fill every segment up to 4 rows instead (MORIG_CSR_MIN4: the mixed-quad form of the H = 256 kernel; not with pad4)."""
        assert not (pad4 and min4)
        _need_gpu(edge_index)
        ei = edge_index if (edge_index.dtype == torch.int64 and edge_index.is_contiguous()) else edge_index.long().contiguous()
        E = ei.shape[1]
        dev = ei.device
        cap = E + (4 if (pad4 or min4) else 1) * n_nodes
        rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        src = torch.empty(cap, dtype=torch.int32, device=dev)
        dst = torch.empty(cap, dtype=torch.int32, device=dev)
        cursor = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        if n_src is None and not skip_negative and not pad4 and not min4:
            check(self.lib.morig_csr_build(_p(ei), E, n_nodes, _p(rowptr), _p(src), _p(dst), _p(cursor), _p(status), _stream()),
                  "morig_csr_build")
        else:
            check(self.lib.morig_csr_build_bipartite(_p(ei), E, n_nodes if n_src is None else n_src, n_nodes,
                                                     (_K["MORIG_CSR_SKIP_NEGATIVE"] if skip_negative else 0) | (_K["MORIG_CSR_PAD4"] if pad4 else 0) |
                                                     (_K["MORIG_CSR_MIN4"] if min4 else 0), _p(rowptr), _p(src),
                                                     _p(dst), _p(cursor), _p(status), _stream()), "morig_csr_build_bipartite")
        csr = CSR(rowptr, src, dst, n_nodes, cap, status, quad=pad4, min4=min4)
        if getattr(self, "_csr_status", None) is not None:
            self._csr_status.append(status)            # read with the precision flag at the end of the guarded forward
        key = (ei.data_ptr(), E, n_nodes)
        if self.learn_edge_counts and not pad4 and not min4 and key not in self._edge_counts:
            self._edge_counts[key] = int(rowptr[-1].item())
        csr.edge_count = self._edge_counts.get(key, 0)
        return csr

    def csr_build_dual(self, edge_index: torch.Tensor, n_nodes: int, min4: Optional[bool] = None):
        """-> (plain CSR, 4-aligned CSR) of one square graph from one pass over the COO (morig_csr_build_dual).
        min4 (default: off; MORIG_EDGE_MIX=1 switches it on): the plain CSR's segments are filled up to 4 rows with copies of the self
        loop -- still a plain CSR for every kernel, and the form the H = 256 EdgeConv kernel takes WITHOUT 4-aligned segments (the
        mixed-quad kernel: correct and tested, measured no faster than the 4-aligned form -- DESIGN.md section 5.2 -- hence opt-in)."""
        if min4 is None:
            min4 = os.environ.get("MORIG_EDGE_MIX", "0") == "1"
        _need_gpu(edge_index)
        ei = edge_index if (edge_index.dtype == torch.int64 and edge_index.is_contiguous()) else edge_index.long().contiguous()
        E = ei.shape[1]
        dev = ei.device
        cap, cap4 = E + (4 if min4 else 1) * n_nodes, E + 4 * n_nodes
        rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        rowptr4 = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        src, dst = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        src4, dst4 = torch.empty(cap4, dtype=torch.int32, device=dev), torch.empty(cap4, dtype=torch.int32, device=dev)
        ws = torch.empty(2 * n_nodes + 1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(self.lib.morig_csr_build_dual(_p(ei), E, n_nodes, _p(rowptr), _p(src), _p(dst), _p(rowptr4), _p(src4), _p(dst4), _p(ws),
                                            _K["MORIG_CSR_MIN4"] if min4 else 0, _p(status), _stream()), "morig_csr_build_dual")
        if getattr(self, "_csr_status", None) is not None:
            self._csr_status.append(status)
        key = (ei.data_ptr(), E, n_nodes)
        a = CSR(rowptr, src, dst, n_nodes, cap, status, min4=bool(min4))
        b = CSR(rowptr4, src4, dst4, n_nodes, cap4, status, quad=True)
        a.edge_count = b.edge_count = self._edge_counts.get(key, 0)
        return a, b

    def csr_from_slots(self, coo: torch.Tensor, n_nodes: int, max_nbrs: int, n_src: int) -> CSR:
        """the bipartite CSR of a ball-query slot table (``ball_query`` output): same result as
        ``csr_build(coo, n_nodes, n_src=n_src, skip_negative=True)``, built per target without atomics."""
        _need_gpu(coo)
        assert coo.dtype == torch.int64 and coo.is_contiguous() and coo.shape == (2, n_nodes * max_nbrs)
        dev = coo.device
        cap = n_nodes * (max_nbrs + 1)
        rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        src = torch.empty(cap, dtype=torch.int32, device=dev)
        dst = torch.empty(cap, dtype=torch.int32, device=dev)
        cursor = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(self.lib.morig_csr_from_slots(_p(coo), n_nodes, max_nbrs, n_src, _p(rowptr), _p(src), _p(dst), _p(cursor),
                                            _p(status), _stream()), "morig_csr_from_slots")
        if getattr(self, "_csr_status", None) is not None:
            self._csr_status.append(status)
        return CSR(rowptr, src, dst, n_nodes, cap, status)

    # -- dense ----------------------------------------------------------------------------------
    def gemm(self, X: Mat, lin, relu: bool, Y: Optional[Mat] = None, rowbias: Optional[Mat] = None,
             seg: Optional[torch.Tensor] = None, pool: Optional[torch.Tensor] = None, affine: bool = True,
             x_split: bool = False, y_split: bool = False, x_tail: Optional[Mat] = None):
        """x_split / y_split: the X window is / the Y window shall be in the split-fp16 activation layout
        (include/morig_hip.h); only meaningful while ``self.fast``.
        x_tail: the last ``x_tail.cols`` columns of the input come from row (row % x_tail.rows) of this split-layout matrix instead of X
        (morig_gemm_args.X_tail: a replica-invariant block read from ONE copy); X then holds the first K - x_tail.cols columns.
        Only where ``gemm_takes_tail`` says so."""
        _need_gpu(X.base, lin.W)
        if x_split or y_split:
            if not self.fast:
                raise MorigNativeError("split-fp16 activations requested on the fp32 path (plan bug)")
            if lin.Wsplit is None:                    # weights outside the fp16 range: force the fp32 redo
                self._flag(X.base.device).fill_(1)
                return
        if pool is not None:
            lin = padded_for_pool(lin)
        a = _args(GemmArgs)
        a.M, a.N, a.K = X.rows, lin.N, lin.K
        if x_tail is not None:
            assert x_split and X.cols + x_tail.cols == lin.K and x_tail.cols % 32 == 0, (X.cols, x_tail.cols, lin.K)
            a.X_tail, a.ld_tail, a.tail_rows, a.tail_cols = x_tail.ptr, x_tail.ld, x_tail.rows, x_tail.cols
        else:
            assert X.cols == lin.K, (X.cols, lin.K)
        a.X, a.ldx = X.ptr, X.ld
        a.W, a.ldw = lin.W.data_ptr(), lin.W.stride(0)
        a.bias = lin.bias.data_ptr() if lin.bias is not None else 0
        a.scale = lin.scale.data_ptr() if (affine and lin.scale is not None) else 0
        a.shift = lin.shift.data_ptr() if (affine and lin.shift is not None) else 0
        a.relu = 1 if relu else 0
        if rowbias is not None:
            a.rowbias, a.ld_rowbias = rowbias.ptr, rowbias.ld
        a.seg = seg.data_ptr() if seg is not None else 0
        if Y is not None:
            assert Y.rows == X.rows and Y.cols == lin.N
            a.Y, a.ldy = Y.ptr, Y.ld
        if pool is not None:
            assert pool.shape[1] >= lin.N and pool.is_contiguous()
            a.pool, a.ld_pool, a.n_seg = pool.data_ptr(), pool.stride(0), pool.shape[0]
        if getattr(lin, "Wsplit_bf16", None) is not None:
            # the bf16 split (no range guard: W_split without an overflow word, include/morig_hip.h): whatever self.precision says
            assert pool is None and not x_split and not y_split
            a.W_split, a.overflow, a.w_split_format = lin.Wsplit_bf16.data_ptr(), 0, _K["MORIG_SPLIT_BF16"]
        elif self.fast and lin.Wsplit is not None:
            a.W_split, a.overflow = lin.Wsplit.data_ptr(), self._flag(X.base.device).data_ptr()
        elif self.exact_arith == "bf16x6" and not x_split and not y_split:
            a.w_split_format = _K["MORIG_SPLIT_BF16X6"]                                     # no image: split in the kernel
        a.x_split, a.y_split = int(x_split), int(y_split)
        check(self.lib.morig_gemm(C.byref(a), _stream()), "morig_gemm")

    def gemm_takes_tail(self, lin, Y: Mat, n_tail_cols: int) -> bool:
        """May ``gemm(..., x_split=True, x_tail=...)`` be used for this layer and output window? Mirrors ``gemm_plan`` in
        csrc/dispatch_core.h (K tails exist on the 256 x 256 LDS-DMA store kernel with the register epilogue only; a row bias that is not
        16-byte aligned is refused there too, which this predicate does not look at: tools/dispatch_host_check.cpp holds the two against
        each other); MORIG_GEMM_TAIL=0 switches the tails off (A/B runs: the block is then copied into every replica's row, the round-5
        plan)."""
        return (self.fast and os.environ.get("MORIG_GEMM_TAIL", "1") != "0" and os.environ.get("MORIG_NO_DMA") is None and
                lin.Wsplit is not None and lin.N % 256 == 0 and lin.K % 32 == 0 and n_tail_cols % 32 == 0 and lin.K > n_tail_cols and
                Y.ptr % 16 == 0 and Y.ld % 4 == 0 and os.environ.get("MORIG_GEMM_TR", "1") != "0" and
                os.environ.get("MORIG_DMA_TILE", "256") == "256")

    def pack_tails(self, src: torch.Tensor, col_a, col_b, wa: int, wb: int) -> torch.Tensor:
        """-> [n_tails, rows, 32] split-fp16 chunks: tail t, row v = [src[v, col_a[t]:+wa] | src[v, col_b[t]:+wb] | 0] (morig_pack_tails),
        ONE launch for every tail of a forward."""
        _need_gpu(src)
        assert src.dim() == 2 and src.dtype == torch.float32 and src.stride(1) == 1 and len(col_a) == len(col_b) <= _K["MORIG_MAX_TAILS"]
        n, rows = len(col_a), src.shape[0]
        out = torch.empty((n, rows, 32), dtype=torch.float32, device=src.device)
        ca, cb = (C.c_int32 * n)(*col_a), (C.c_int32 * n)(*col_b)
        check(self.lib.morig_pack_tails(_p(src), src.stride(0), rows, ca, cb, wa, wb, n, _p(out), rows * 32,
                                        self._flag(src.device).data_ptr(), _stream()), "morig_pack_tails")
        return out

    # -- fused edge conv ----------------------------------------------------------------------------
    def edgeconv(self, A: Mat, B: Mat, csr: CSR, ec, out: Mat, replicas: int = 1,
                 in_rep_stride: int = 0, out_rep_stride: int = 0, out_split: bool = False):
        """out_split: `out` (a chunk-aligned window, H % 32 == 0) is written in the split-fp16 activation layout; only where
        ``edgeconv_can_split_out`` says so for the same arguments (MORIG_E_UNSUPPORTED otherwise)."""
        _need_gpu(A.base, B.base, out.base)
        a = self._edge_args(A, B, csr, ec, out, replicas, in_rep_stride, out_rep_stride)
        a.out_split = 1 if out_split else 0
        check(self.lib.morig_edgeconv(C.byref(a), _stream()), "morig_edgeconv")

    def edgeconv_pair(self, first: dict, second: dict):
        """Two EdgeConv launches that write disjoint column blocks of the same rows and do not read each other's results (the template-
        and the geodesic-graph EdgeConv of a unit): ``first`` / ``second`` are the keyword arguments of ``edgeconv``. Same results as the
        two calls; their boundary passes share launches (morig_edgeconv_args.init_with / split_with: one identity pass in front of both
        kernels, one conversion pass behind both when both store split rows) -- 2 x 2 small launches less per unit.
        MORIG_EDGE_PAIR=0: two plain calls (A/B runs)."""
        if not PAIR_PASSES:
            self.edgeconv(**first)
            self.edgeconv(**second)
            return
        calls = []
        for kw in (first, second):
            kw = dict(kw)
            sp = bool(kw.pop("out_split", False))
            _need_gpu(kw["A"].base, kw["B"].base, kw["out"].base)
            a = self._edge_args(kw["A"], kw["B"], kw["csr"], kw["ec"], kw["out"], kw.get("replicas", 1), kw.get("in_rep_stride", 0),
                                kw.get("out_rep_stride", 0))
            a.out_split = 1 if sp else 0
            calls.append(a)
        a1, a2 = calls
        a1.init_with, a2.skip_init = C.addressof(a2), 1
        if a1.out_split and a2.out_split:
            a1.skip_split, a2.split_with = 1, C.addressof(a1)
        check(self.lib.morig_edgeconv(C.byref(a1), _stream()), "morig_edgeconv")
        check(self.lib.morig_edgeconv(C.byref(a2), _stream()), "morig_edgeconv")

    def edgeconv_x3_pair(self, first: dict, second: dict):
        """the same for two ``edgeconv_x3`` launches (keyword arguments of ``edgeconv_x3``): one identity pass for both"""
        if not PAIR_PASSES:
            self.edgeconv_x3(**first)
            self.edgeconv_x3(**second)
            return
        a1, a2 = (self._x3_args(**kw) for kw in (first, second))
        a1.init_with, a2.skip_init = C.addressof(a2), 1
        check(self.lib.morig_edgeconv_x3(C.byref(a1), _stream()), "morig_edgeconv_x3")
        check(self.lib.morig_edgeconv_x3(C.byref(a2), _stream()), "morig_edgeconv_x3")

    def edgeconv_can_split_out(self, A: Mat, B: Mat, csr: CSR, ec, out: Mat, replicas: int = 1,
                               in_rep_stride: int = 0, out_rep_stride: int = 0) -> bool:
        """Would ``edgeconv(..., out_split=True)`` run for these arguments? (kernel choice, alignment, environment switches: the library
        decides, morig_edgeconv_can_split_out; nothing is launched)"""
        a = self._edge_args(A, B, csr, ec, out, replicas, in_rep_stride, out_rep_stride)
        return bool(self.lib.morig_edgeconv_can_split_out(C.byref(a)))

    def _edge_args(self, A, B, csr, ec, out, replicas, in_rep_stride, out_rep_stride):
        a = _args(EdgeConvArgs)
        a.H = ec.H
        a.n_nodes, a.replicas = csr.n_nodes, replicas
        a.in_rep_stride, a.out_rep_stride = in_rep_stride, out_rep_stride
        a.A, a.lda = A.ptr, A.ld
        a.B, a.ldb = B.ptr, B.ld
        a.rowptr, a.src_sorted, a.dst_sorted = csr.rowptr.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr()
        a.edge_capacity, a.edge_count = csr.capacity, csr.edge_count
        if ec.s1 is not None:
            a.s1, a.t1 = ec.s1.data_ptr(), ec.t1.data_ptr()
        a.W2, a.ldw = ec.W2.data_ptr(), ec.W2.stride(0)
        a.b2, a.s2, a.t2 = ec.b2.data_ptr(), ec.s2.data_ptr(), ec.t2.data_ptr()
        a.out, a.ldo = out.ptr, out.ld
        a.quad_aligned = 1 if csr.quad else 0
        a.seg_min4 = 1 if getattr(csr, "min4", False) else 0
        a.exact_arith = 1 if self.exact_arith == "bf16x6" else 0
        if self.fast and ec.W2split is not None:
            a.W2_split, a.overflow = ec.W2split.data_ptr(), self._flag(A.base.device).data_ptr()
        return a

    def edgeconv_x3(self, X: Mat, first, csr: CSR, ec, out: Mat, replicas: int = 1, in_rep_stride: int = 0, out_rep_stride: int = 0):
        """EdgeConv on a 3-channel vertex input with the first Linear evaluated in the kernel (morig_edgeconv_x3). X: [rows, >= 4]
        window starting at column 0 of 16-byte aligned rows; first = (W1a [32, 4], W1b [32, 4], b1 [32]) from packing.pack_first_x3."""
        a = self._x3_args(X, first, csr, ec, out, replicas, in_rep_stride, out_rep_stride)
        check(self.lib.morig_edgeconv_x3(C.byref(a), _stream()), "morig_edgeconv_x3")

    def _x3_args(self, X: Mat, first, csr: CSR, ec, out: Mat, replicas: int = 1, in_rep_stride: int = 0, out_rep_stride: int = 0):
        _need_gpu(X.base, out.base)
        assert ec.H == 32 and ec.s1 is None and X.col0 % 4 == 0 and X.ld % 4 == 0
        a = _args(EdgeConvX3Args)
        a.H = 32
        a.n_nodes, a.replicas = csr.n_nodes, replicas
        a.in_rep_stride, a.out_rep_stride = in_rep_stride, out_rep_stride
        a.X, a.ldx = X.ptr, X.ld
        a.W1a, a.W1b, a.b1 = first[0].data_ptr(), first[1].data_ptr(), first[2].data_ptr()
        a.rowptr, a.src_sorted, a.dst_sorted = csr.rowptr.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr()
        a.edge_capacity, a.edge_count = csr.capacity, csr.edge_count
        a.W2, a.ldw = ec.W2.data_ptr(), ec.W2.stride(0)
        a.b2, a.s2, a.t2 = ec.b2.data_ptr(), ec.s2.data_ptr(), ec.t2.data_ptr()
        a.out, a.ldo = out.ptr, out.ld
        if self.fast and ec.W2split is not None:
            a.W2_split, a.overflow = ec.W2split.data_ptr(), self._flag(X.base.device).data_ptr()
        return a

    def edge_hidden(self, A: Mat, B: Mat, csr: CSR, ec, Z: Mat):
        """per-edge hidden activations Z [capacity, H] (rows >= E' untouched)."""
        _need_gpu(A.base, B.base, Z.base)
        assert Z.rows == csr.capacity and Z.cols == ec.H
        a = self._edge_args(A, B, csr, ec, Z, 1, 0, 0)
        check(self.lib.morig_edge_hidden(C.byref(a), _stream()), "morig_edge_hidden")

    def segmax_gemm(self, X: Mat, lin, relu: bool, csr: CSR, out: Mat):
        _need_gpu(X.base, out.base)
        assert X.rows == csr.capacity and X.cols == lin.K and out.rows == csr.n_nodes and out.cols == lin.N
        a = _args(SegmaxArgs)
        a.N, a.K = lin.N, lin.K
        a.X, a.ldx = X.ptr, X.ld
        a.W, a.ldw = lin.W.data_ptr(), lin.W.stride(0)
        a.bias = lin.bias.data_ptr() if lin.bias is not None else 0
        a.scale = lin.scale.data_ptr() if lin.scale is not None else 0
        a.shift = lin.shift.data_ptr() if lin.shift is not None else 0
        a.relu = 1 if relu else 0
        a.rowptr, a.dst_sorted, a.n_nodes = csr.rowptr.data_ptr(), csr.dst.data_ptr(), csr.n_nodes
        a.edge_capacity, a.edge_count = csr.capacity, csr.edge_count
        a.out, a.ldo = out.ptr, out.ld
        if self.fast and lin.Wsplit is not None:
            a.W_split, a.overflow = lin.Wsplit.data_ptr(), self._flag(X.base.device).data_ptr()
        check(self.lib.morig_segmax_gemm(C.byref(a), _stream()), "morig_segmax_gemm")

    def pointconv_can_fuse(self, pk, max_nbrs: int) -> bool:
        """the one-launch PointConv (csrc/pointconv_fused.hip) covers this packed local_nn? (split-fp16 arithmetic only)"""
        l3 = pk.get("fused")
        return bool(self.fast and l3 is not None and l3.Wsplit is not None and pk["edge"].W2split is not None and
                    max_nbrs == 64 and pk["edge"].s1 is None and os.environ.get("MORIG_POINTCONV_FUSED", "1") != "0")

    def pointconv_fused(self, A: Mat, B: Mat, coo: torch.Tensor, max_nbrs: int, pk, out: Mat):
        """out[c] = max over the slot table's kept edges + the self loop (c, c) of the 3-layer PointConv message
        (== csr_from_slots -> edge_hidden -> segmax_gemm); coo: the ball_query slot table [2, n_centres * max_nbrs]."""
        _need_gpu(A.base, B.base, out.base, coo)
        ec, l3 = pk["edge"], pk["fused"]
        assert coo.dtype == torch.int64 and coo.is_contiguous() and coo.shape == (2, A.rows * max_nbrs)
        assert A.cols == B.cols == ec.H and out.rows == A.rows and out.cols == l3.N and B.rows >= A.rows
        dev = A.base.device
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        a = _args(PointConvArgs)
        a.A, a.lda, a.B, a.ldb = A.ptr, A.ld, B.ptr, B.ld
        a.slots, a.max_nbrs, a.n_centres, a.n_src = coo.data_ptr(), max_nbrs, A.rows, B.rows
        a.H, a.H3 = ec.H, l3.N
        a.W2_split, a.ldw2, a.b2 = ec.W2split.data_ptr(), ec.W2split.stride(0), ec.b2.data_ptr()
        a.W3_split, a.ldw3, a.b3 = l3.Wsplit.data_ptr(), l3.Wsplit.stride(0), l3.bias.data_ptr()
        a.s3 = l3.scale.data_ptr() if l3.scale is not None else 0
        a.t3 = l3.shift.data_ptr() if l3.shift is not None else 0
        a.relu3 = 1
        a.out, a.ldo = out.ptr, out.ld
        a.overflow, a.status = self._flag(dev).data_ptr(), status.data_ptr()
        check(self.lib.morig_pointconv_fused(C.byref(a), _stream()), "morig_pointconv_fused")
        if getattr(self, "_csr_status", None) is not None:
            self._csr_status.append(status)            # a slot naming a source >= n_src: raised at the end of the guarded forward
        elif int(status.item()) != 0:
            raise MorigNativeError("morig_pointconv_fused: the slot table names a source row outside B")

    # -- point clouds ---------------------------------------------------------------------------------
    def fps(self, pos: Mat, ptr: torch.Tensor, out_ptr: torch.Tensor, start: Optional[torch.Tensor], n_clouds: int,
            max_cloud_points: int, n_samples: int) -> torch.Tensor:
        _need_gpu(pos.base, ptr, out_ptr)
        idx = torch.empty(n_samples, dtype=torch.int32, device=pos.base.device)
        check(self.lib.morig_fps(pos.ptr, pos.ld, _p(ptr), _p(out_ptr), _p(start), n_clouds, max_cloud_points, _p(idx), _stream()),
              "morig_fps")
        return idx

    def ball_query(self, x: Mat, ptr_x: torch.Tensor, y: Mat, ptr_y: torch.Tensor, n_clouds: int, radius: float,
                   max_nbrs: int) -> torch.Tensor:
        _need_gpu(x.base, y.base, ptr_x, ptr_y)
        coo = torch.empty((2, y.rows * max_nbrs), dtype=torch.int64, device=x.base.device)
        check(self.lib.morig_ball_query(x.ptr, x.ld, _p(ptr_x), y.ptr, y.ld, _p(ptr_y), n_clouds, y.rows, float(radius),
                                        max_nbrs, _p(coo), _stream()), "morig_ball_query")
        return coo

    # -- train-mode forward support (csrc/train_ops.hip) ---------------------------------
    def col_stats(self, X: Mat, rows_dev: Optional[torch.Tensor] = None):
        """-> (mean [cols], biased var [cols], count [1]) of the rows of X (rows_dev: int32 [1] on the device = live row count)."""
        _need_gpu(X.base)
        dev = X.base.device
        slabs = (max(X.rows, 1) + 255) // 256
        ws = torch.empty(slabs * 2 * X.cols, dtype=torch.float64, device=dev)
        mean = torch.empty(X.cols, dtype=torch.float32, device=dev)
        var = torch.empty(X.cols, dtype=torch.float32, device=dev)
        cnt = torch.empty(1, dtype=torch.float32, device=dev)
        check(self.lib.morig_col_stats(X.ptr, X.ld, X.rows, _p(rows_dev), X.cols, C.c_void_p(ws.data_ptr()), ws.numel(), _p(mean),
                                       _p(var), _p(cnt), _stream()), "morig_col_stats")
        return mean, var, cnt

    def col_affine(self, X: Mat, scale: torch.Tensor, shift: torch.Tensor, rows_dev: Optional[torch.Tensor] = None,
                   out: Optional[Mat] = None):
        """out = scale * X + shift per column (in place without ``out``)"""
        _need_gpu(X.base, scale, shift)
        assert scale.numel() >= X.cols and shift.numel() >= X.cols and scale.dtype == shift.dtype == torch.float32
        assert out is None or (out.rows == X.rows and out.cols == X.cols)
        check(self.lib.morig_col_affine(X.ptr, X.ld, X.rows, _p(rows_dev), X.cols, _p(scale), _p(shift), out.ptr if out is not None else 0,
                                        out.ld if out is not None else 0, _stream()), "morig_col_affine")

    def bn_finalize(self, bn, mean: torch.Tensor, var: torch.Tensor, count: torch.Tensor):
        """BatchNorm1d ``bn`` in training mode after its column statistics, ONE launch: -> (s, t, rstd); the running buffers and
        num_batches_tracked move in place (``bn.momentum`` must be a number)."""
        _need_gpu(mean, var, count)
        n = mean.numel()
        dev = mean.device
        out = torch.empty((3, n), dtype=torch.float32, device=dev)
        track = bn.track_running_stats and bn.running_mean is not None
        g = bn.weight.detach() if bn.weight is not None else None
        b = bn.bias.detach() if bn.bias is not None else None
        for x in (g, b, bn.running_mean if track else None, bn.running_var if track else None):
            assert x is None or (x.dtype == torch.float32 and x.is_contiguous() and x.device == dev)
        assert mean.dtype == var.dtype == count.dtype == torch.float32 and mean.is_contiguous() and var.is_contiguous()
        check(self.lib.morig_bn_finalize(_p(mean), _p(var), _p(count), _p(g), _p(b), float(bn.eps), float(bn.momentum if track else 0.0),
                                         _p(bn.running_mean) if track else None, _p(bn.running_var) if track else None,
                                         _p(bn.num_batches_tracked) if track else None, _p(out[0]), _p(out[1]), _p(out[2]), n, _stream()),
              "morig_bn_finalize")
        return out[0], out[1], out[2]

    def edge_gather_relu(self, A: Mat, B: Mat, csr: CSR, Z: Mat, want_stats: bool = False):
        """want_stats: -> (mean, biased var, count [1]) of the live rows of Z, as ``col_stats(Z, rows_dev=E')``, from the same pass"""
        _need_gpu(A.base, B.base, Z.base)
        assert Z.rows == csr.capacity and A.cols == B.cols == Z.cols
        ws = st = None
        if want_stats:
            dev = Z.base.device
            ws = torch.empty(((csr.capacity + 255) // 256) * 2 * Z.cols, dtype=torch.float64, device=dev)
            st = torch.empty(2 * Z.cols + 1, dtype=torch.float32, device=dev)
        check(self.lib.morig_edge_gather_relu(A.ptr, A.ld, B.ptr, B.ld, _p(csr.rowptr), csr.n_nodes, _p(csr.src), _p(csr.dst),
                                              csr.capacity, Z.cols, Z.ptr, Z.ld, _p(ws), ws.numel() if want_stats else 0,
                                              _p(st), _p(st[Z.cols:]) if want_stats else _p(None),
                                              _p(st[2 * Z.cols:]) if want_stats else _p(None), _stream()), "morig_edge_gather_relu")
        return (st[:Z.cols], st[Z.cols:2 * Z.cols], st[2 * Z.cols:]) if want_stats else None

    def segmax_affine(self, Z: Mat, rowptr: torch.Tensor, n_segments: int, out: Mat, scale: Optional[torch.Tensor] = None,
                      shift: Optional[torch.Tensor] = None):
        _need_gpu(Z.base, rowptr, out.base)
        assert rowptr.dtype == torch.int32 and out.rows == n_segments and out.cols == Z.cols
        check(self.lib.morig_segmax_affine(Z.ptr, Z.ld, _p(rowptr), n_segments, Z.cols, _p(scale), _p(shift), out.ptr, out.ld,
                                           _stream()), "morig_segmax_affine")

    # -- train-mode backward support (csrc/train_bwd.hip; SURVEY 8 f-4, backward half) --------------------------------
    def bn_backward_stats(self, dz: Mat, y: Optional[Mat] = None, mean: Optional[torch.Tensor] = None,
                          rstd: Optional[torch.Tensor] = None, rows_dev: Optional[torch.Tensor] = None):
        """-> (sum_dz [cols], sum_dz_xhat [cols] or None): dbeta / dgamma of a training-mode BatchNorm1d with input y
        (y None: the plain column sum = dbias)."""
        _need_gpu(dz.base)
        dev = dz.base.device
        slabs = (max(dz.rows, 1) + 255) // 256
        ws = torch.empty(slabs * 2 * dz.cols, dtype=torch.float64, device=dev)
        sdz = torch.empty(dz.cols, dtype=torch.float32, device=dev)
        sdzx = torch.empty(dz.cols, dtype=torch.float32, device=dev) if y is not None else None
        check(self.lib.morig_bn_backward_stats(dz.ptr, dz.ld, y.ptr if y is not None else 0, y.ld if y is not None else 0, dz.rows,
                                               _p(rows_dev), dz.cols, _p(mean), _p(rstd), C.c_void_p(ws.data_ptr()), ws.numel(),
                                               _p(sdz), _p(sdzx), _stream()), "morig_bn_backward_stats")
        return sdz, sdzx

    def bn_relu_backward(self, dz: Mat, y: Mat, mean, rstd, gamma, sum_dz, sum_dzx, du: Mat, rows_dev: Optional[torch.Tensor] = None,
                         want_sum: bool = False):
        """want_sum: -> the column sums of du (float32 [cols], = the bias gradient of the Linear in front), from the same pass"""
        _need_gpu(dz.base, y.base, du.base)
        assert dz.rows == y.rows == du.rows and dz.cols == y.cols == du.cols
        ws = sdu = None
        if want_sum:
            dev = du.base.device
            ws = torch.empty(((max(dz.rows, 1) + 255) // 256) * 2 * dz.cols, dtype=torch.float64, device=dev)
            sdu = torch.empty(dz.cols, dtype=torch.float32, device=dev)
        check(self.lib.morig_bn_relu_backward(dz.ptr, dz.ld, y.ptr, y.ld, dz.rows, _p(rows_dev), dz.cols, _p(mean), _p(rstd), _p(gamma),
                                              _p(sum_dz), _p(sum_dzx), du.ptr, du.ld, _p(ws), ws.numel() if want_sum else 0, _p(sdu),
                                              _stream()), "morig_bn_relu_backward")
        return sdu

    def segmax_affine_arg(self, Z: Mat, rowptr: torch.Tensor, n_segments: int, out: Mat, scale=None, shift=None, want_zwin: bool = False):
        """segmax_affine + the winning row per (segment, column): int32 [n_segments, cols], -1 for empty segments. want_zwin: also the
        winners' values in front of the affine, float32 [n_segments, cols] -> (arg, zwin)."""
        _need_gpu(Z.base, rowptr, out.base)
        assert rowptr.dtype == torch.int32 and out.rows == n_segments and out.cols == Z.cols
        arg = torch.empty((n_segments, Z.cols), dtype=torch.int32, device=Z.base.device)
        zwin = torch.empty((n_segments, Z.cols), dtype=torch.float32, device=Z.base.device) if want_zwin else None
        check(self.lib.morig_segmax_affine_arg(Z.ptr, Z.ld, _p(rowptr), n_segments, Z.cols, _p(scale), _p(shift), out.ptr, out.ld,
                                               _p(arg), arg.stride(0), _p(zwin), zwin.stride(0) if want_zwin else 0, _stream()),
              "morig_segmax_affine_arg")
        return (arg, zwin) if want_zwin else arg

    def segmax_bn_backward_stats(self, dout: Mat, arg: torch.Tensor, Z: Optional[Mat], mean, rstd, zwin: Optional[torch.Tensor] = None):
        """zwin ([n_seg, cols], from segmax_affine_arg): the coalesced kernel; without it the winners' rows are gathered from Z."""
        _need_gpu(dout.base, arg, Z.base if Z is not None else zwin)
        dev = dout.base.device
        n_seg, cols = dout.rows, dout.cols
        assert arg.shape == (n_seg, cols) and (Z is None or Z.cols == cols) and (zwin is None or zwin.shape == (n_seg, cols))
        slabs = (n_seg + 255) // 256
        ws = torch.empty(slabs * 2 * cols, dtype=torch.float64, device=dev)
        sdz = torch.empty(cols, dtype=torch.float32, device=dev)
        sdzx = torch.empty(cols, dtype=torch.float32, device=dev)
        check(self.lib.morig_segmax_bn_backward_stats(dout.ptr, dout.ld, _p(arg), arg.stride(0), Z.ptr if Z is not None else 0,
                                                      Z.ld if Z is not None else 0, _p(zwin), zwin.stride(0) if zwin is not None else 0,
                                                      n_seg, cols, _p(mean), _p(rstd), C.c_void_p(ws.data_ptr()), ws.numel(), _p(sdz),
                                                      _p(sdzx), _stream()), "morig_segmax_bn_backward_stats")
        return sdz, sdzx

    def segmax_bn_relu_backward(self, dout: Mat, arg: torch.Tensor, Z: Mat, rowptr: torch.Tensor, seg_of_row: torch.Tensor, mean, rstd,
                                gamma, sum_dz, sum_dzx, du: Mat, relu: bool = True, want_sum: bool = False):
        """want_sum: -> the column sums of du over the live rows (float32 [cols]), from the same pass."""
        _need_gpu(dout.base, arg, Z.base, du.base, rowptr, seg_of_row)
        assert Z.rows == du.rows and Z.cols == du.cols == dout.cols and seg_of_row.dtype == torch.int32
        ws = sdu = None
        if want_sum:
            dev = du.base.device
            ws = torch.empty(((Z.rows + 255) // 256) * 2 * Z.cols, dtype=torch.float64, device=dev)
            sdu = torch.empty(Z.cols, dtype=torch.float32, device=dev)
        check(self.lib.morig_segmax_bn_relu_backward(dout.ptr, dout.ld, _p(arg), arg.stride(0), Z.ptr, Z.ld, _p(rowptr), dout.rows,
                                                     _p(seg_of_row), Z.rows, Z.cols, _p(mean), _p(rstd), _p(gamma), _p(sum_dz), _p(sum_dzx),
                                                     1 if relu else 0, du.ptr, du.ld, _p(ws), ws.numel() if want_sum else 0, _p(sdu),
                                                     _stream()), "morig_segmax_bn_relu_backward")
        return sdu

    def edge_bn_scatter_backward(self, dG: Mat, Y: Optional[Mat], csr: CSR, n_src: int, dA: Mat, dB: Mat, mean=None, rstd=None, gamma=None,
                                 sum_dz=None, sum_dzx=None, ZA: Optional[Mat] = None, ZB: Optional[Mat] = None):
        """bn_relu_backward + edge_scatter_backward in one pass pair, deterministic (no atomics, the per-edge gradient is not stored):
        dA[v] / dB[u] = sums of d[e] = [Y > 0] gamma rstd (dG - sum_dz / n - xhat sum_dzx / n) into / out of a vertex; mean=None: d = dG."""
        _need_gpu(dG.base, dA.base, dB.base)
        assert dA.rows == csr.n_nodes and dB.rows == n_src and dA.cols == dB.cols == dG.cols
        assert mean is None or ZA is not None or (Y is not None and Y.cols == dG.cols and Y.rows == dG.rows)
        assert (ZA is None) == (ZB is None) and (ZA is None or (ZA.rows == csr.n_nodes and ZB.rows == n_src and ZA.cols == ZB.cols == dG.cols))
        rowptr_t, perm_t = csr.transposed(n_src)
        check(self.lib.morig_edge_bn_scatter_backward(dG.ptr, dG.ld, Y.ptr if Y is not None else 0, Y.ld if Y is not None else 0,
                                                      _p(csr.rowptr), _p(rowptr_t), _p(perm_t), csr.n_nodes, n_src, dG.cols, _p(mean),
                                                      _p(rstd), _p(gamma), _p(sum_dz), _p(sum_dzx), dA.ptr, dA.ld, dB.ptr, dB.ld,
                                                      ZA.ptr if ZA is not None else 0, ZA.ld if ZA is not None else 0,
                                                      ZB.ptr if ZB is not None else 0, ZB.ld if ZB is not None else 0,
                                                      _p(csr.src) if ZA is not None else None, _p(csr.dst) if ZA is not None else None,
                                                      _stream()), "morig_edge_bn_scatter_backward")

    def edge_scatter_backward(self, dG: Mat, csr: CSR, n_src: int, dA: Mat, dB: Mat):
        """backward of Z[e] = A[dst_e] + B[src_e] over the live edges of ``csr``."""
        _need_gpu(dG.base, dA.base, dB.base)
        assert dA.rows == csr.n_nodes and dB.rows == n_src and dA.cols == dB.cols == dG.cols
        check(self.lib.morig_edge_scatter_backward(dG.ptr, dG.ld, _p(csr.rowptr), _p(csr.src), csr.n_nodes, n_src, dG.cols, dA.ptr, dA.ld,
                                                   dB.ptr, dB.ld, _stream()), "morig_edge_scatter_backward")

    def edge_bn_sums_from_products(self, M: torch.Tensor, db2: torch.Tensor, W2: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor):
        """-> (sum_dz, sum_dzx) of the first edge layer's BatchNorm from M = dU2^T Z1, db2 and W2 (no pass over the edges)"""
        _need_gpu(M, db2, W2, mean, rstd)
        h_out, h_in = W2.shape
        assert M.shape == (h_out, h_in) and M.stride(1) == 1 and W2.stride(1) == 1 and db2.numel() >= h_out and db2.is_contiguous()
        assert all(t.dtype == torch.float32 for t in (M, db2, W2, mean, rstd)) and mean.numel() >= h_in and rstd.numel() >= h_in
        out = torch.empty((2, h_in), dtype=torch.float32, device=M.device)
        check(self.lib.morig_edge_bn_sums_from_products(_p(M), M.stride(0), _p(db2), _p(W2), W2.stride(0), _p(mean), _p(rstd), h_out, h_in,
                                                        _p(out[0]), _p(out[1]), _stream()), "morig_edge_bn_sums_from_products")
        return out[0], out[1]

    def gemm_tn(self, A: Mat, B: Mat, out: Optional[Mat] = None, rows_dev: Optional[torch.Tensor] = None,
                b_shift: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A^T B over the rows: [A.cols, B.cols] (the weight gradient dU^T X). b_shift [B.cols]: every row of B is centred on it first,
        A^T (B - 1 b_shift^T)."""
        _need_gpu(A.base, B.base)
        if b_shift is not None:
            assert b_shift.dtype == torch.float32 and b_shift.is_contiguous() and b_shift.numel() >= B.cols
        assert A.rows == B.rows
        dev = A.base.device
        if out is None:
            out = Mat.of(torch.empty((A.cols, B.cols), dtype=torch.float32, device=dev))
        n_ws = int(self.lib.morig_gemm_tn_workspace(A.rows, A.cols, B.cols))
        ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
        check(self.lib.morig_gemm_tn_shift(A.ptr, A.ld, B.ptr, B.ld, _p(b_shift), A.rows, _p(rows_dev), A.cols, B.cols, _p(ws), ws.numel(),
                                           out.ptr, out.ld, _stream()), "morig_gemm_tn_shift")
        return out.base

    def radius_sample(self, x: Mat, y: Mat, radius: float, max_nbrs: int, seed: int):
        """radius_cpu's neighbour table: (slot table int64 [2, ny * max_nbrs] (-1 = unused), hits per row int32 [ny])."""
        _need_gpu(x.base, y.base)
        dev = x.base.device
        coo = torch.empty((2, y.rows * max_nbrs), dtype=torch.int64, device=dev)
        counts = torch.empty(y.rows, dtype=torch.int32, device=dev)
        check(self.lib.morig_radius_sample(x.ptr, x.ld, x.rows, y.ptr, y.ld, y.rows, float(radius), max_nbrs, int(seed) & 0xFFFFFFFF,
                                           _p(coo), _p(counts), _stream()), "morig_radius_sample")
        return coo, counts

    def geo_ball_graph(self, pos: Optional[Mat], mesh_ptr: Optional[torch.Tensor], radius: float, max_nn: int, seed: int,
                       self_loops: bool = False, dist: Optional[torch.Tensor] = None):
        """get_geo_edges (data_proc/common_ops.py:214-226) on the device -> (edge_index int64 [2, E] rows [i, member],
        members int32 [n] uncapped ball sizes). Positions variant: pos [n, >=3] + mesh_ptr int32 [B + 1]; distance variant:
        dist float64 [n, n] of one mesh. ONE host read (the edge count sizes the result)."""
        if dist is not None:
            _need_gpu(dist)
            assert dist.dtype == torch.float64 and dist.dim() == 2 and dist.shape[0] == dist.shape[1] and dist.stride(1) == 1
            n, dev = dist.shape[0], dist.device
        else:
            _need_gpu(pos.base, mesh_ptr)
            assert mesh_ptr.dtype == torch.int32
            n, dev = pos.rows, pos.base.device
        slots = torch.empty((n, max_nn), dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        members = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(1, (n + 2047) // 2048), dtype=torch.int32, device=dev)
        sd = int(seed) & 0xFFFFFFFF
        if dist is not None:
            check(self.lib.morig_geo_ball_graph_dist(_p(dist), dist.stride(0), n, float(radius), max_nn, sd, _p(slots), _p(counts),
                                                     _p(members), _p(offsets), _p(ws), _stream()), "morig_geo_ball_graph_dist")
        else:
            check(self.lib.morig_geo_ball_graph(pos.ptr, pos.ld, _p(mesh_ptr), mesh_ptr.numel() - 1, n, float(radius), max_nn, sd,
                                                _p(slots), _p(counts), _p(members), _p(offsets), _p(ws), _stream()),
                  "morig_geo_ball_graph")
        n_out = int(offsets[n].item()) + (n if self_loops else 0)
        coo = torch.empty((2, n_out), dtype=torch.int64, device=dev)
        if n_out:
            check(self.lib.morig_geo_ball_fill(_p(slots), _p(offsets), n, max_nn, 1 if self_loops else 0, _p(coo), n_out, _stream()),
                  "morig_geo_ball_fill")
        return coo, members

    def knn_interpolate(self, feat: Mat, pos_x: Mat, ptr_x: torch.Tensor, pos_y: Mat, ptr_y: torch.Tensor, n_clouds: int,
                        max_targets_per_cloud: int, k: int, out: Mat):
        _need_gpu(feat.base, pos_x.base, pos_y.base, out.base)
        nt = pos_y.rows
        dev = feat.base.device
        idx = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        wgt = torch.empty((nt, 3), dtype=torch.float32, device=dev)
        assert out.rows == nt and out.cols == feat.cols
        check(self.lib.morig_knn_interpolate(feat.ptr, feat.ld, feat.cols, pos_x.ptr, pos_x.ld, _p(ptr_x), pos_y.ptr, pos_y.ld,
                                             _p(ptr_y), n_clouds, nt, max_targets_per_cloud, k, _p(idx), _p(wgt), out.ptr, out.ld,
                                             _stream()), "morig_knn_interpolate")

    def knn_search(self, pos_x: Mat, ptr_x: torch.Tensor, pos_y: Mat, ptr_y: torch.Tensor, n_clouds: int,
                   max_targets_per_cloud: int, k: int):
        """the geometry half of knn_interpolate: -> (idx [ny, 3] int32, wgt [ny, 3]) for ``knn_apply``."""
        _need_gpu(pos_x.base, pos_y.base)
        nt = pos_y.rows
        dev = pos_x.base.device
        idx = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        wgt = torch.empty((nt, 3), dtype=torch.float32, device=dev)
        check(self.lib.morig_knn_search(pos_x.ptr, pos_x.ld, _p(ptr_x), pos_y.ptr, pos_y.ld, _p(ptr_y), n_clouds, nt,
                                        max_targets_per_cloud, k, _p(idx), _p(wgt), _stream()), "morig_knn_search")
        return idx, wgt

    def knn_apply(self, feat: Mat, nn, out: Mat):
        """out[t] = sum_s w_s feat[idx_s] / sum_s w_s with (idx, wgt) = nn from ``knn_search``."""
        idx, wgt = nn
        _need_gpu(feat.base, out.base, idx, wgt)
        assert out.rows == idx.shape[0] and out.cols == feat.cols
        check(self.lib.morig_knn_apply(feat.ptr, feat.ld, feat.cols, _p(idx), _p(wgt), out.rows, out.ptr, out.ld, _stream()),
              "morig_knn_apply")

    def cosine_nn(self, v: Mat, ptr_v: torch.Tensor, p: Mat, ptr_p: torch.Tensor, n_clouds: int, max_rows_per_cloud: int):
        _need_gpu(v.base, p.base)
        dev = v.base.device
        nn = torch.empty(v.rows, dtype=torch.int32, device=dev)
        sim = torch.empty(v.rows, dtype=torch.float32, device=dev)
        check(self.lib.morig_cosine_nn(v.ptr, v.ld, _p(ptr_v), p.ptr, p.ld, _p(ptr_p), n_clouds, max_rows_per_cloud, v.cols,
                                       _p(nn), _p(sim), _stream()), "morig_cosine_nn")
        return nn, sim

    def reserve_cus(self, n: int):
        """keep n CUs free of persistent EdgeConv workgroups (while FPS runs on a second stream)."""
        check(self.lib.morig_reserve_cus(int(n)), "morig_reserve_cus")

    # -- DeformNet glue (csrc/deform.hip) ----------------------------------------------------------------
    def sigmoid_minmax(self, x: Mat, ptr: torch.Tensor, n_meshes: int, out: Mat):
        """out = per-mesh min-max normalised sigmoid(x) (one column)."""
        _need_gpu(x.base, ptr, out.base)
        assert x.cols == 1 and out.cols == 1 and x.rows == out.rows and ptr.dtype == torch.int32
        check(self.lib.morig_sigmoid_minmax(x.ptr, x.ld, _p(ptr), n_meshes, out.ptr, out.ld, _stream()), "morig_sigmoid_minmax")

    def cosine_knn(self, y: Mat, ptr_y: torch.Tensor, x: Mat, ptr_x: torch.Tensor, n_clouds: int, max_rows_per_cloud: int,
                   k: int, vis: Mat = None, split: bool = False):
        """idx [y.rows, k] int32: the k most similar x rows of the same cloud per y row (-1 padded);
        split: rows with vis < 0.5 query rows with vis >= 0.5 of the same matrix."""
        _need_gpu(y.base, x.base, ptr_y, ptr_x)
        assert ptr_y.dtype == torch.int32 and ptr_x.dtype == torch.int32 and y.cols == x.cols
        idx = torch.empty((y.rows, k), dtype=torch.int32, device=y.base.device)
        if split:
            assert vis is not None and x.ptr == y.ptr
            ptr_x = ptr_y
        check(self.lib.morig_cosine_knn(y.ptr, y.ld, _p(ptr_y), x.ptr, x.ld, _p(ptr_x), n_clouds, max_rows_per_cloud, y.cols, k,
                                        vis.ptr if vis is not None else None, vis.ld if vis is not None else 0, int(split),
                                        _p(idx), _stream()), "morig_cosine_knn")
        return idx

    def flow_vote(self, mode: int, idx: torch.Tensor, feat_q: Mat, feat_s: Mat, pos_q, pos_s, vis: Mat, l1: Mat):
        """similarity-weighted voting into l1 = [flow(3) | vis]; mode 0: from points (pos_s - pos_q), all vertices;
        mode 1: invisible vertices from the flow of their visible neighbours."""
        _need_gpu(idx, feat_q.base, feat_s.base, vis.base, l1.base)
        assert idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == feat_q.rows and l1.cols >= 4
        check(self.lib.morig_flow_vote(mode, _p(idx), idx.shape[1], feat_q.rows, feat_q.ptr, feat_q.ld, feat_s.ptr, feat_s.ld,
                                       feat_q.cols, pos_q.ptr if pos_q is not None else None, pos_q.ld if pos_q is not None else 0,
                                       pos_s.ptr if pos_s is not None else None, pos_s.ld if pos_s is not None else 0,
                                       vis.ptr, vis.ld, l1.ptr, l1.ld, _stream()), "morig_flow_vote")

    # -- joint extraction (csrc/joints.hip): float64 [n, 3] contiguous point sets -----------------------------
    @staticmethod
    def _pts64(pts: torch.Tensor):
        assert pts.dtype == torch.float64 and pts.dim() == 2 and pts.shape[1] == 3 and pts.is_contiguous()

    def inside_mask(self, pts: torch.Tensor, vox88: torch.Tensor, translate, scale: float, dims0: float) -> torch.Tensor:
        _need_gpu(pts, vox88)
        self._pts64(pts)
        assert vox88.dtype == torch.uint8 and vox88.numel() == 88 ** 3 and vox88.is_contiguous()
        keep = torch.empty(pts.shape[0], dtype=torch.uint8, device=pts.device)
        t = (C.c_double * 3)(*[float(v) for v in translate])
        check(self.lib.morig_inside_check(_p(pts), pts.shape[0], _p(vox88), t, float(scale), float(dims0), _p(keep), _stream()),
              "morig_inside_check")
        return keep.bool()

    # -- skinning (csrc/skin.hip) ------------------------------------------------------------------------------------------------
    def vol_geodesic(self, vox: torch.Tensor, vox_tf: torch.Tensor, pos: torch.Tensor, vtx_ptr: torch.Tensor, bones: torch.Tensor,
                     bone_ptr: torch.Tensor, dist_off: torch.Tensor, n_dist: int, n_slots: int) -> tuple:
        """-> (dist int32 [n_dist], status int32 [2]); see include/morig_hip.h."""
        _need_gpu(vox, vox_tf, pos, vtx_ptr, bones, bone_ptr, dist_off)
        nm = vox.shape[0]
        assert vox.dtype == torch.uint8 and vox.is_contiguous() and vox.numel() == nm * 88 ** 3
        assert vox_tf.dtype == torch.float64 and vox_tf.shape == (nm, 5) and vox_tf.is_contiguous()
        self._pts64(pos)
        assert bones.dtype == torch.float64 and bones.dim() == 2 and bones.shape[1] == 6 and bones.is_contiguous()
        assert vtx_ptr.dtype == torch.int32 and bone_ptr.dtype == torch.int32 and dist_off.dtype == torch.int64
        assert vtx_ptr.numel() == nm + 1 and bone_ptr.numel() == nm + 1 and dist_off.numel() == nm + 1
        dev = pos.device
        ws_bytes = int(self.lib.morig_vol_geodesic_workspace(nm, n_slots))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        dist = torch.empty(max(n_dist, 1), dtype=torch.int32, device=dev)
        check(self.lib.morig_vol_geodesic(_p(vox), nm, _p(vox_tf), _p(pos), _p(vtx_ptr), _p(bones), _p(bone_ptr), bones.shape[0],
                                          _p(dist_off), n_slots, _p(ws), ws_bytes, _p(status), _p(dist), _stream()), "morig_vol_geodesic")
        return dist[:n_dist], status

    def skin_bind(self, dist: torch.Tensor, dist_off: torch.Tensor, vtx_ptr: torch.Tensor, bone_ptr: torch.Tensor, n: int, bones: torch.Tensor,
                  is_leaf: torch.Tensor, start_jid: torch.Tensor, skins: Optional[torch.Tensor], k: int) -> dict:
        _need_gpu(dist, dist_off, vtx_ptr, bone_ptr, bones, is_leaf, start_jid, skins)
        assert dist.dtype == torch.int32 and is_leaf.dtype == torch.uint8 and start_jid.dtype == torch.int32
        if skins is not None:
            assert skins.dtype == torch.float64 and skins.dim() == 2 and skins.shape[0] == n and skins.stride(1) == 1
        dev = dist.device
        out = dict(bind_ids=torch.empty((n, k), dtype=torch.int32, device=dev),
                   bind_invd=torch.empty((n, k), dtype=torch.float64, device=dev),
                   labels=None if skins is None else torch.empty((n, k), dtype=torch.float64, device=dev),
                   skin_input=torch.empty((n, 8 * k), dtype=torch.float32, device=dev),
                   skin_nn=torch.empty((n, k), dtype=torch.int64, device=dev),
                   loss_mask=torch.empty((n, k), dtype=torch.int64, device=dev),
                   skin_nnjids=torch.empty((n, k), dtype=torch.int64, device=dev))
        check(self.lib.morig_skin_bind(_p(dist), _p(dist_off), _p(vtx_ptr), _p(bone_ptr), vtx_ptr.numel() - 1, n, _p(bones), _p(is_leaf),
                                       _p(start_jid), _p(skins), 0 if skins is None else skins.stride(0), k, _p(out["bind_ids"]),
                                       _p(out["bind_invd"]), _p(out["labels"]), _p(out["skin_input"]), _p(out["skin_nn"]),
                                       _p(out["loss_mask"]), _p(out["skin_nnjids"]), _stream()), "morig_skin_bind")
        return out

    def skin_scatter(self, logits: torch.Tensor, skin_nn: torch.Tensor, loss_mask: torch.Tensor, batch: torch.Tensor, n_bones: torch.Tensor,
                     mode: int, ldp: int) -> torch.Tensor:
        _need_gpu(logits, skin_nn, loss_mask, batch, n_bones)
        n, k = skin_nn.shape
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[0] == n and logits.shape[1] >= k and logits.stride(1) == 1
        assert skin_nn.dtype == loss_mask.dtype == batch.dtype == torch.int64 and n_bones.dtype == torch.int32
        assert skin_nn.is_contiguous() and loss_mask.is_contiguous() and loss_mask.shape == skin_nn.shape
        P = torch.empty((n, ldp), dtype=torch.float64, device=logits.device)
        check(self.lib.morig_skin_scatter(_p(logits), logits.stride(0), _p(skin_nn), _p(loss_mask), _p(batch), _p(n_bones), n, k, mode,
                                          _p(P), ldp, _stream()), "morig_skin_scatter")
        return P

    def skin_filter(self, P: torch.Tensor, rowptr: torch.Tensor, cols: torch.Tensor, batch: torch.Tensor, n_bones: torch.Tensor,
                    ratio: float) -> torch.Tensor:
        _need_gpu(P, rowptr, cols, batch, n_bones)
        assert P.dtype == torch.float64 and P.is_contiguous() and rowptr.dtype == cols.dtype == n_bones.dtype == torch.int32
        n, ldp = P.shape
        W = torch.empty((n, ldp), dtype=torch.float64, device=P.device)
        check(self.lib.morig_skin_filter(_p(P), ldp, _p(rowptr), _p(cols), _p(batch), _p(n_bones), n, float(ratio), _p(W), ldp, _stream()),
              "morig_skin_filter")
        return W

    # -- surface geodesics and vertex-to-bone distances (csrc/geodesic.hip) -------------------------------------------------------
    def surface_geodesic(self, pts: torch.Tensor, normals: torch.Tensor, s_ptr: torch.Tensor, job_ptr: torch.Tensor, out_off: torch.Tensor,
                         n_out: int, max_samples: int, n_jobs: int, nsrc: int, use_lds: bool, n_slots: int) -> tuple:
        """-> (out float64 [n_out], status int32 [8]); see include/morig_hip.h."""
        _need_gpu(pts, normals, s_ptr, job_ptr, out_off)
        self._pts64(pts)
        self._pts64(normals)
        nm = s_ptr.numel() - 1
        assert normals.shape == pts.shape and s_ptr.dtype == job_ptr.dtype == torch.int32 and out_off.dtype == torch.int64
        assert job_ptr.numel() == nm + 1 and out_off.numel() == nm + 1
        dev = pts.device
        ws_bytes = int(self.lib.morig_surface_geodesic_workspace(pts.shape[0], nm, max_samples, n_slots, int(use_lds)))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        status = torch.empty(8, dtype=torch.int32, device=dev)
        out = torch.empty(n_out, dtype=torch.float64, device=dev)
        check(self.lib.morig_surface_geodesic(_p(pts), _p(normals), _p(s_ptr), _p(job_ptr), nm, pts.shape[0], max_samples, n_jobs, nsrc,
                                              int(use_lds), _p(out_off), n_slots, _p(ws), ws_bytes, _p(status), _p(out), _stream()),
              "morig_surface_geodesic")
        return out, status

    def nearest_point(self, q: torch.Tensor, q_ptr: torch.Tensor, pts: torch.Tensor, p_ptr: torch.Tensor, squared: bool) -> torch.Tensor:
        _need_gpu(q, q_ptr, pts, p_ptr)
        self._pts64(q)
        self._pts64(pts)
        assert q_ptr.dtype == p_ptr.dtype == torch.int32 and q_ptr.numel() == p_ptr.numel()
        out = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        check(self.lib.morig_nearest_point(_p(q), _p(q_ptr), _p(pts), _p(p_ptr), q_ptr.numel() - 1, q.shape[0], int(squared), _p(out), _stream()),
              "morig_nearest_point")
        return out

    def bone_point_distance(self, pos: torch.Tensor, vtx_ptr: torch.Tensor, bones: torch.Tensor, bone_ptr: torch.Tensor, off: torch.Tensor,
                            n_pairs: int) -> tuple:
        _need_gpu(pos, vtx_ptr, bones, bone_ptr, off)
        self._pts64(pos)
        assert bones.dtype == torch.float64 and bones.dim() == 2 and bones.shape[1] == 6 and bones.is_contiguous()
        assert vtx_ptr.dtype == bone_ptr.dtype == torch.int32 and off.dtype == torch.int64
        origins = torch.empty((n_pairs, 3), dtype=torch.float64, device=pos.device)
        dist = torch.empty(n_pairs, dtype=torch.float64, device=pos.device)
        check(self.lib.morig_bone_point_distance(_p(pos), _p(vtx_ptr), _p(bones), _p(bone_ptr), vtx_ptr.numel() - 1, _p(off), n_pairs, _p(origins),
                                                 _p(dist), _stream()), "morig_bone_point_distance")
        return origins, dist

    def bone_visibility(self, pos: torch.Tensor, vtx_ptr: torch.Tensor, bones: torch.Tensor, bone_ptr: torch.Tensor, tri_pos: torch.Tensor,
                        tp_ptr: torch.Tensor, faces: torch.Tensor, f_ptr: torch.Tensor, off: torch.Tensor, blk_ptr: torch.Tensor, n_blocks: int,
                        n_pairs: int) -> torch.Tensor:
        _need_gpu(pos, vtx_ptr, bones, bone_ptr, tri_pos, tp_ptr, faces, f_ptr, off, blk_ptr)
        self._pts64(pos)
        self._pts64(tri_pos)
        assert bones.dtype == torch.float64 and bones.dim() == 2 and bones.shape[1] == 6 and bones.is_contiguous()
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert vtx_ptr.dtype == bone_ptr.dtype == tp_ptr.dtype == f_ptr.dtype == blk_ptr.dtype == torch.int32 and off.dtype == torch.int64
        vis = torch.empty(n_pairs, dtype=torch.uint8, device=pos.device)
        check(self.lib.morig_bone_visibility(_p(pos), _p(vtx_ptr), _p(bones), _p(bone_ptr), _p(tri_pos), _p(tp_ptr), _p(faces), _p(f_ptr), _p(off),
                                             _p(blk_ptr), vtx_ptr.numel() - 1, n_blocks, _p(vis), _stream()), "morig_bone_visibility")
        return vis

    def bone_geodesic(self, dist: torch.Tensor, vis: torch.Tensor, sg: torch.Tensor, sg_off: torch.Tensor, vtx_ptr: torch.Tensor,
                      bone_ptr: torch.Tensor, off: torch.Tensor, n_bones: int) -> dict:
        _need_gpu(dist, vis, sg, sg_off, vtx_ptr, bone_ptr, off)
        assert dist.dtype == sg.dtype == torch.float64 and vis.dtype == torch.uint8 and dist.is_contiguous() and vis.is_contiguous()
        assert sg.is_contiguous() and vis.numel() == dist.numel()
        assert vtx_ptr.dtype == bone_ptr.dtype == torch.int32 and off.dtype == sg_off.dtype == torch.int64
        dev, n = dist.device, dist.numel()
        o = dict(vis_after=torch.empty(n, dtype=torch.uint8, device=dev), n_vis=torch.empty(n_bones, dtype=torch.int32, device=dev),
                 pct=torch.empty(n_bones, dtype=torch.float64, device=dev), out=torch.empty(n, dtype=torch.float64, device=dev),
                 nn=torch.empty(n, dtype=torch.int32, device=dev))
        check(self.lib.morig_bone_geodesic(_p(dist), _p(vis), _p(sg), _p(sg_off), _p(vtx_ptr), _p(bone_ptr), _p(off), vtx_ptr.numel() - 1, n_bones,
                                           n, _p(o["vis_after"]), _p(o["n_vis"]), _p(o["pct"]), _p(o["out"]), _p(o["nn"]), _stream()),
              "morig_bone_geodesic")
        return o

    def skin_bind_geo(self, dist: torch.Tensor, off: torch.Tensor, vtx_ptr: torch.Tensor, bone_ptr: torch.Tensor, n: int, bones: torch.Tensor,
                      is_leaf: torch.Tensor, k: int) -> tuple:
        _need_gpu(dist, off, vtx_ptr, bone_ptr, bones, is_leaf)
        assert dist.dtype == torch.float64 and dist.is_contiguous() and is_leaf.dtype == torch.uint8 and off.dtype == torch.int64
        assert bones.dtype == torch.float64 and bones.is_contiguous() and vtx_ptr.dtype == bone_ptr.dtype == torch.int32
        dev = dist.device
        si = torch.empty((n, 8 * k), dtype=torch.float32, device=dev)
        nn = torch.empty((n, k), dtype=torch.int64, device=dev)
        mask = torch.empty((n, k), dtype=torch.int64, device=dev)
        check(self.lib.morig_skin_bind_geo(_p(dist), _p(off), _p(vtx_ptr), _p(bone_ptr), vtx_ptr.numel() - 1, n, _p(bones), _p(is_leaf), k, _p(si),
                                           _p(nn), _p(mask), _stream()), "morig_skin_bind_geo")
        return si, nn, mask

    # -- skeleton connection (csrc/skeleton.hip) ------------------------------------------------------------------------------------
    @staticmethod
    def _skel_ptrs(joint_ptr: torch.Tensor, pair_ptr: torch.Tensor, nm: int):
        assert joint_ptr.dtype == torch.int32 and pair_ptr.dtype == torch.int32 and joint_ptr.numel() == nm + 1 and pair_ptr.numel() == nm + 1
        assert joint_ptr.is_contiguous() and pair_ptr.is_contiguous()

    def pair_attr(self, joints64: torch.Tensor, joints32: torch.Tensor, joint_ptr: torch.Tensor, pair_ptr: torch.Tensor, n_pairs: int,
                  vox: torch.Tensor, vox_tf: torch.Tensor) -> tuple:
        """-> (pairs int64 [n_pairs, 2], pair_attr float32 [n_pairs, 3], outside_count int32 [n_pairs], status int32 [1])"""
        _need_gpu(joints64, joints32, joint_ptr, pair_ptr, vox, vox_tf)
        nm = vox.shape[0]
        assert vox.dtype == torch.uint8 and vox.is_contiguous() and vox.numel() == nm * 88 ** 3
        assert vox_tf.dtype == torch.float64 and vox_tf.shape == (nm, 5) and vox_tf.is_contiguous()
        self._pts64(joints64)
        assert joints32.dtype == torch.float32 and joints32.shape == joints64.shape and joints32.is_contiguous()
        self._skel_ptrs(joint_ptr, pair_ptr, nm)
        dev = joints64.device
        pairs = torch.empty((n_pairs, 2), dtype=torch.int64, device=dev)
        attr = torch.empty((n_pairs, 3), dtype=torch.float32, device=dev)
        outside = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(self.lib.morig_pair_attr(_p(joints64), _p(joints32), _p(joint_ptr), _p(pair_ptr), nm, n_pairs, _p(vox), _p(vox_tf), _p(pairs),
                                       _p(attr), _p(outside), _p(status), _stream()), "morig_pair_attr")
        return pairs, attr, outside, status

    def skeleton_cost(self, pair_logits: torch.Tensor, root_logits: torch.Tensor, joints32: torch.Tensor, outside_count: torch.Tensor,
                      joint_ptr: torch.Tensor, pair_ptr: torch.Tensor, cost_off: torch.Tensor, n_cost: int, max_joints: int) -> tuple:
        """-> (cost float64 [n_cost], root int32 [n_meshes]); logits are 1-D float32 views of any element stride"""
        _need_gpu(pair_logits, root_logits, joints32, outside_count, joint_ptr, pair_ptr, cost_off)
        nm = joint_ptr.numel() - 1
        self._skel_ptrs(joint_ptr, pair_ptr, nm)
        assert pair_logits.dtype == root_logits.dtype == torch.float32 and pair_logits.dim() == 1 and root_logits.dim() == 1
        assert joints32.dtype == torch.float32 and joints32.dim() == 2 and joints32.shape[1] == 3 and joints32.is_contiguous()
        assert root_logits.numel() == joints32.shape[0] and outside_count.dtype == torch.int32 and outside_count.is_contiguous()
        assert outside_count.numel() == pair_logits.numel() and cost_off.dtype == torch.int64 and cost_off.numel() == nm + 1
        dev = joints32.device
        cost = torch.empty(max(n_cost, 1), dtype=torch.float64, device=dev)
        root = torch.empty(nm, dtype=torch.int32, device=dev)
        ld = lambda t: max(int(t.stride(0)), 1) if t.numel() > 1 else 1
        check(self.lib.morig_skeleton_cost(_p(pair_logits), ld(pair_logits), _p(root_logits), ld(root_logits), _p(joints32), _p(outside_count),
                                           _p(joint_ptr), _p(pair_ptr), _p(cost_off), nm, max_joints, _p(cost), _p(root), _stream()),
              "morig_skeleton_cost")
        return cost[:n_cost], root

    def prim_mst(self, cost: torch.Tensor, cost_off: torch.Tensor, joint_ptr: torch.Tensor, root: torch.Tensor, n_joints: int,
                 max_joints: int) -> tuple:
        """-> (parent int32 [n_joints], key float64 [n_joints], status int32 [n_meshes])"""
        _need_gpu(cost, cost_off, joint_ptr, root)
        nm = joint_ptr.numel() - 1
        assert cost.dtype == torch.float64 and cost.is_contiguous() and cost_off.dtype == torch.int64 and cost_off.numel() == nm + 1
        assert joint_ptr.dtype == torch.int32 and root.dtype == torch.int32 and root.numel() == nm and root.is_contiguous()
        dev = cost.device
        parent = torch.empty(n_joints, dtype=torch.int32, device=dev)
        key = torch.empty(n_joints, dtype=torch.float64, device=dev)
        status = torch.empty(nm, dtype=torch.int32, device=dev)
        check(self.lib.morig_prim_mst(_p(cost), _p(cost_off), _p(joint_ptr), _p(root), nm, max_joints, _p(parent), _p(key), _p(status),
                                      _stream()), "morig_prim_mst")
        return parent, key, status

    IK_FIELDS_I32 = ("joint_ptr", "vert_ptr", "level_off", "parent", "order", "level_ptr", "child_lo", "child_hi", "vptr", "vent_j", "jptr",
                     "jent_v", "root", "iter_time")
    IK_FIELDS_F32 = ("locals_in", "offsets", "vent_xw", "jent_xw", "constraints", "vismask", "w_invis", "thrd")
    IK_FIELDS_F64 = ("lr", "bias1", "bias2_sqrt")

    def ik_solve(self, t: dict, n_problems: int, max_joints: int, max_vertices: int, max_iter: int, with_grad: bool = False) -> dict:
        """morig_ik_solve on the device tensors of ``t`` (the members of morig_ik_args, include/morig_hip.h; morig_amd/tracking.py packs
        them) -> dict(angles, trans, locals, globals, jpos, status[, loss, grad_angles, grad_trans]). Raises where the launch is refused."""
        for names, dt in ((self.IK_FIELDS_I32, torch.int32), (self.IK_FIELDS_F32, torch.float32), (self.IK_FIELDS_F64, torch.float64)):
            for k in names:
                _need_gpu(t[k])
                assert t[k].dtype == dt and t[k].is_contiguous(), k
        nj, nv, ne = t["parent"].numel(), t["vismask"].numel(), t["vent_j"].numel()
        assert t["joint_ptr"].numel() == t["vert_ptr"].numel() == t["level_off"].numel() == n_problems + 1
        assert t["locals_in"].numel() == nj * 9 and t["offsets"].numel() == nj * 3 and t["order"].numel() == nj
        assert t["child_lo"].numel() == t["child_hi"].numel() == nj and t["jptr"].numel() == nj + 1 and t["vptr"].numel() == nv + 1
        assert t["vent_xw"].numel() == ne * 4 and t["jent_xw"].numel() == ne * 4 and t["jent_v"].numel() == ne
        assert t["constraints"].numel() == nv * 3 and t["bias1"].numel() >= max_iter and t["bias2_sqrt"].numel() >= max_iter
        for k in ("root", "iter_time", "lr", "w_invis", "thrd"):
            assert t[k].numel() == n_problems, k
        dev = t["parent"].device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = dict(angles=f32(nj, 3), trans=f32(n_problems, 3), locals=f32(nj, 3, 3), globals=f32(nj, 3, 3), jpos=f32(nj, 3),
                   status=torch.full((n_problems,), -1, dtype=torch.int32, device=dev))
        if with_grad:
            out.update(loss=f32(n_problems), grad_angles=f32(nj, 3), grad_trans=f32(n_problems, 3))
        a = _args(IkArgs)
        a.n_problems, a.max_joints, a.max_vertices, a.max_iter, a.n_entries = n_problems, max_joints, max_vertices, max_iter, ne
        for k in self.IK_FIELDS_I32 + self.IK_FIELDS_F32 + self.IK_FIELDS_F64:
            setattr(a, k, t[k].data_ptr())
        for k, v in out.items():
            setattr(a, k, v.data_ptr())
        check(self.lib.morig_ik_solve(C.byref(a), _stream()), "morig_ik_solve")
        return out

    def ik_solve_lds_bytes(self, max_joints: int, max_vertices: int) -> int:
        return int(self.lib.morig_ik_solve_lds_bytes(max_joints, max_vertices))

    def corr_select(self, nn: torch.Tensor, sim: torch.Tensor, n_pts: int) -> tuple:
        """per point the vertex with the largest similarity among those whose nearest point it is (first vertex on ties, similarity > 0)
        -> (winner int32 [n_pts], -1 where none; winner_sim float32 [n_pts])"""
        _need_gpu(nn, sim)
        assert nn.dtype == torch.int32 and sim.dtype == torch.float32 and nn.is_contiguous() and sim.is_contiguous() and nn.numel() == sim.numel()
        keys = torch.empty(n_pts, dtype=torch.int64, device=nn.device)
        winner = torch.empty(n_pts, dtype=torch.int32, device=nn.device)
        wsim = torch.empty(n_pts, dtype=torch.float32, device=nn.device)
        check(self.lib.morig_corr_select(_p(nn), _p(sim), nn.numel(), n_pts, _p(keys), _p(winner), _p(wsim), _stream()), "morig_corr_select")
        return winner, wsim

    # -- training losses (csrc/losses.hip; morig_amd/losses.py holds the autograd functions) -------------------------------------
    NCE_WIDTH = 64
    MULTIPOS_MAX_WIDTH, MULTIPOS_MAX_POS, MULTIPOS_MAX_NEG = 128, 64, 256
    CHAMFER_MAX_JOINTS = _K["MORIG_CHAMFER_MAX_JOINTS"]

    def loss_status(self, device) -> torch.Tensor:
        """the zeroed status word the loss kernels OR their findings into (MORIG_LOSS_ST_*)"""
        return torch.zeros(1, dtype=torch.int32, device=device)

    def segment_ptr(self, batch: torch.Tensor, n_segments: int, status: torch.Tensor) -> torch.Tensor:
        """int32 [n_segments + 1] row offsets of a sorted int64 batch vector; unsorted / out-of-range values set status bits"""
        _need_gpu(batch, status)
        assert batch.dtype == torch.int64 and batch.is_contiguous() and batch.dim() == 1
        ptr = torch.zeros(n_segments + 1, dtype=torch.int32, device=batch.device)
        check(self.lib.morig_loss_segment_ptr(_p(batch), batch.numel(), n_segments, _p(ptr), _p(status), _stream()), "morig_loss_segment_ptr")
        return ptr

    def _nce_args(self, vtx, pts, corr_v2p, corr_p2v, ptrs, tau, status):
        _need_gpu(vtx, pts, corr_v2p, corr_p2v, status, *ptrs)
        for f in (vtx, pts):
            assert f.dim() == 2 and f.dtype == torch.float32 and f.stride(1) == 1
            if f.shape[1] != self.NCE_WIDTH:
                raise MorigNativeError(f"infoNCE: feature width {f.shape[1]} (MORIG_E_UNSUPPORTED: the kernels are built for width {self.NCE_WIDTH})")
        for c in (corr_v2p, corr_p2v):
            assert c.dtype == torch.int64 and c.is_contiguous() and c.dim() == 2 and c.shape[1] == 2
        a = _args(NceArgs)
        a.n_pairs, a.C, a.tau = ptrs[0].numel() - 1, vtx.shape[1], float(tau)
        a.n_vtx, a.n_pts, a.n_v2p, a.n_p2v = vtx.shape[0], pts.shape[0], corr_v2p.shape[0], corr_p2v.shape[0]
        a.ld_vtx, a.ld_pts = max(vtx.stride(0), self.NCE_WIDTH), max(pts.stride(0), self.NCE_WIDTH)
        a.vtx, a.pts, a.corr_v2p, a.corr_p2v = vtx.data_ptr(), pts.data_ptr(), corr_v2p.data_ptr(), corr_p2v.data_ptr()
        a.ptr_vtx, a.ptr_pts, a.ptr_v2p, a.ptr_p2v = (t.data_ptr() for t in ptrs)
        a.status = status.data_ptr()
        return a

    def infonce_forward(self, vtx, pts, corr_v2p, corr_p2v, ptrs, tau: float, status: torch.Tensor):
        """-> (loss [1], lse [n_v2p + n_p2v]); ptrs = int32 offsets of (vtx, pts, corr_v2p, corr_p2v) per pair"""
        a = self._nce_args(vtx, pts, corr_v2p, corr_p2v, ptrs, tau, status)
        rows = a.n_v2p + a.n_p2v
        lse = torch.zeros(max(rows, 1), dtype=torch.float32, device=vtx.device)
        row_loss = torch.zeros(max(rows, 1), dtype=torch.float32, device=vtx.device)
        loss = torch.empty(1, dtype=torch.float32, device=vtx.device)
        a.lse, a.row_loss, a.loss = lse.data_ptr(), row_loss.data_ptr(), loss.data_ptr()
        check(self.lib.morig_infonce_forward(C.byref(a), _stream()), "morig_infonce_forward")
        return loss, lse

    def infonce_backward(self, vtx, pts, corr_v2p, corr_p2v, ptrs, tau: float, lse, upstream, groups, status: torch.Tensor):
        """-> (grad_vtx, grad_pts); groups = (rowptr_vtx, order_v2p, rowptr_pts, order_p2v): the rows of each direction grouped by their
        global anchor in row order; upstream: float32 [1] on the device"""
        a = self._nce_args(vtx, pts, corr_v2p, corr_p2v, ptrs, tau, status)
        _need_gpu(lse, upstream, *groups)
        dev, W = vtx.device, self.NCE_WIDTH
        rows = a.n_v2p + a.n_p2v
        d_rows = torch.zeros(max(rows, 1), W, dtype=torch.float32, device=dev)
        d_key_pts = torch.zeros(max(a.n_pts, 1), W, dtype=torch.float32, device=dev)
        d_key_vtx = torch.zeros(max(a.n_vtx, 1), W, dtype=torch.float32, device=dev)
        g_vtx = torch.zeros(a.n_vtx, W, dtype=torch.float32, device=dev)
        g_pts = torch.zeros(a.n_pts, W, dtype=torch.float32, device=dev)
        assert upstream.dtype == torch.float32 and upstream.numel() == 1 and lse.dtype == torch.float32 and lse.numel() >= rows
        assert all(t.dtype == torch.int32 and t.is_contiguous() for t in groups)
        a.lse, a.upstream = lse.data_ptr(), upstream.data_ptr()
        a.d_rows, a.d_key_pts, a.d_key_vtx = d_rows.data_ptr(), d_key_pts.data_ptr(), d_key_vtx.data_ptr()
        a.rowptr_vtx, a.order_v2p, a.rowptr_pts, a.order_p2v = (t.data_ptr() for t in groups)
        a.grad_vtx, a.grad_pts, a.ld_gv, a.ld_gp = g_vtx.data_ptr(), g_pts.data_ptr(), W, W
        check(self.lib.morig_infonce_backward(C.byref(a), _stream()), "morig_infonce_backward")
        return g_vtx, g_pts

    def _multipos_check(self, F, pos_ids, neg_ids):
        _need_gpu(F, pos_ids, neg_ids)
        assert F.dim() == 2 and F.dtype == torch.float32 and F.is_contiguous()
        assert pos_ids.dtype == torch.int32 and neg_ids.dtype == torch.int32 and pos_ids.is_contiguous() and neg_ids.is_contiguous()
        D, P, N = F.shape[1], pos_ids.shape[-1], neg_ids.shape[-1]
        if D % 4 or not 4 <= D <= self.MULTIPOS_MAX_WIDTH:
            raise MorigNativeError(f"multi_pos_infoNCE: feature width {D} (MORIG_E_UNSUPPORTED: a multiple of 4 up to {self.MULTIPOS_MAX_WIDTH})")
        if not 1 <= P <= self.MULTIPOS_MAX_POS or N > self.MULTIPOS_MAX_NEG:
            raise MorigNativeError(f"multi_pos_infoNCE: {P} positives / {N} negatives per row (MORIG_E_UNSUPPORTED: at most "
                                   f"{self.MULTIPOS_MAX_POS} / {self.MULTIPOS_MAX_NEG})")
        return D, P, N

    def multipos_forward(self, F, pos_ids, neg_ids, n_meshes: int, n_sample: int, status):
        """F [n_meshes * n_sample][D] sampled rows -> (loss [1], neg_max [rows], neg_sum [rows])"""
        D, P, N = self._multipos_check(F, pos_ids, neg_ids)
        rows = n_meshes * n_sample
        assert F.shape[0] == rows and pos_ids.numel() == rows * P and neg_ids.numel() == rows * N
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=F.device)
        neg_max, neg_sum, row_loss, loss = f32(rows), f32(rows), f32(rows), f32(1)
        check(self.lib.morig_multipos_forward(_p(F), F.stride(0), D, _p(pos_ids), P, _p(neg_ids), N, n_meshes, n_sample, _p(neg_max), _p(neg_sum),
                                              _p(row_loss), _p(loss), _p(status), _stream()), "morig_multipos_forward")
        return loss, neg_max, neg_sum

    def multipos_backward(self, F, pos_ids, neg_ids, n_meshes: int, n_sample: int, neg_max, neg_sum, upstream, rows, n_total: int, status):
        """-> grad [n_total][D]: the sampled rows (rows int32 [n_meshes * n_sample], no duplicates) written, every other row exactly 0"""
        D, P, N = self._multipos_check(F, pos_ids, neg_ids)
        _need_gpu(neg_max, neg_sum, upstream, rows)
        assert rows.dtype == torch.int32 and rows.numel() == n_meshes * n_sample and upstream.dtype == torch.float32 and upstream.numel() == 1
        G = torch.empty(n_meshes * n_sample * n_sample, dtype=torch.float32, device=F.device)
        grad = torch.zeros(n_total, D, dtype=torch.float32, device=F.device)
        check(self.lib.morig_multipos_backward(_p(F), F.stride(0), D, _p(pos_ids), P, _p(neg_ids), N, n_meshes, n_sample, _p(neg_max), _p(neg_sum),
                                               _p(upstream), _p(G), _p(rows), _p(grad), D, _p(status), _stream()), "morig_multipos_backward")
        return grad

    def chamfer_forward(self, p, q, ptr_p, ptr_q, status):
        """p [n_p][3], q [n_q][3] contiguous float32 -> (loss [1], arg1 int32 [n_p], d1 [n_p], key2 int64 [n_q])"""
        _need_gpu(p, q, ptr_p, ptr_q, status)
        assert p.dtype == q.dtype == torch.float32 and p.is_contiguous() and q.is_contiguous() and p.shape[1] == q.shape[1] == 3
        dev, B = p.device, ptr_p.numel() - 1
        arg1 = torch.zeros(p.shape[0], dtype=torch.int32, device=dev)
        d1 = torch.zeros(p.shape[0], dtype=torch.float32, device=dev)
        key2 = torch.empty(q.shape[0], dtype=torch.int64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(self.lib.morig_chamfer_forward(_p(p), _p(q), _p(ptr_p), _p(ptr_q), B, p.shape[0], q.shape[0], _p(arg1), _p(d1), _p(key2), _p(loss),
                                             _p(status), _stream()), "morig_chamfer_forward")
        return loss, arg1, d1, key2

    def chamfer_backward(self, p, q, ptr_p, ptr_q, arg1, d1, key2, upstream, status):
        _need_gpu(p, q, ptr_p, ptr_q, arg1, d1, key2, upstream, status)
        assert upstream.dtype == torch.float32 and upstream.numel() == 1
        gp, gq = torch.zeros_like(p), torch.zeros_like(q)
        check(self.lib.morig_chamfer_backward(_p(p), _p(q), _p(ptr_p), _p(ptr_q), ptr_p.numel() - 1, p.shape[0], q.shape[0], _p(arg1), _p(d1),
                                              _p(key2), _p(upstream), _p(gp), _p(gq), _p(status), _stream()), "morig_chamfer_backward")
        return gp, gq

    # -- the losses of the skin training step (csrc/losses_skin.hip) -----------------------------------------------------------------
    LOGRATIO_MAX_WIDTH, LOGRATIO_MAX_SAMPLE = _K["MORIG_LOGRATIO_MAX_WIDTH"], _K["MORIG_LOGRATIO_MAX_SAMPLE"]
    SKIN_CE_MAX_K, CE_PROBS_MAX_K = _K["MORIG_SKIN_CE_MAX_K"], _K["MORIG_CE_PROBS_MAX_K"]
    CE_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}

    def _logratio_args(self, feat_all, feat_aggr, gt, ptr, samples, status):
        """feat_all: None or an [N, T, D] view with unit channel stride (set t = feat_all[:, t, :]); feat_aggr: None or [N, D] with unit
        channel stride (the last set); gt [N, W]; samples int32 [sets, B, S] contiguous"""
        _need_gpu(feat_all, feat_aggr, gt, ptr, samples, status)
        assert feat_all is not None or feat_aggr is not None
        assert gt.dim() == 2 and gt.dtype == torch.float32 and gt.stride(1) == 1
        assert samples.dtype == torch.int32 and samples.is_contiguous() and samples.dim() == 3 and ptr.dtype == torch.int32
        a = _args(LogRatioArgs)
        a.n_meshes, a.n_rows, a.n_sample, a.W = ptr.numel() - 1, gt.shape[0], samples.shape[2], gt.shape[1]
        a.gt, a.ld_gt = gt.data_ptr(), gt.stride(0)
        if feat_all is not None:
            assert feat_all.dim() == 3 and feat_all.dtype == torch.float32 and feat_all.stride(2) == 1 and feat_all.shape[0] == gt.shape[0]
            a.n_all, a.D = feat_all.shape[1], feat_all.shape[2]
            a.feat_all, a.ld_all, a.set_stride = feat_all.data_ptr(), feat_all.stride(0), feat_all.stride(1)
        if feat_aggr is not None:
            assert feat_aggr.dim() == 2 and feat_aggr.dtype == torch.float32 and feat_aggr.stride(1) == 1 and feat_aggr.shape[0] == gt.shape[0]
            assert feat_all is None or feat_aggr.shape[1] == a.D
            a.D = feat_aggr.shape[1]
            a.feat_aggr, a.ld_aggr = feat_aggr.data_ptr(), feat_aggr.stride(0)
        a.n_sets = a.n_all + (feat_aggr is not None)
        assert samples.shape[0] == a.n_sets and samples.shape[1] == a.n_meshes
        if a.D % 4 or not 4 <= a.D <= self.LOGRATIO_MAX_WIDTH or a.W % 4 or not 4 <= a.W <= self.LOGRATIO_MAX_WIDTH:
            raise MorigNativeError(f"log_ratio_loss: feature width {a.D}, gt_skin width {a.W} (MORIG_E_UNSUPPORTED: multiples of 4 up to "
                                   f"{self.LOGRATIO_MAX_WIDTH})")
        if not 3 <= a.n_sample <= self.LOGRATIO_MAX_SAMPLE:
            raise MorigNativeError(f"log_ratio_loss: {a.n_sample} samples per mesh (MORIG_E_UNSUPPORTED: 3 to {self.LOGRATIO_MAX_SAMPLE})")
        a.ptr, a.samples, a.status = ptr.data_ptr(), samples.data_ptr(), status.data_ptr()
        return a

    def logratio_forward(self, feat_all, feat_aggr, gt, ptr, samples, status):
        """-> (loss [1], tab [sets, B, 2, S, S]: the log-ratio table and the feature distances, kept for the backward)"""
        a = self._logratio_args(feat_all, feat_aggr, gt, ptr, samples, status)
        dev = gt.device
        tab = torch.empty(a.n_sets, a.n_meshes, 2, a.n_sample, a.n_sample, dtype=torch.float32, device=dev)
        wg_loss = torch.empty(a.n_sets * a.n_meshes, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        a.tab, a.wg_loss, a.loss = tab.data_ptr(), wg_loss.data_ptr(), loss.data_ptr()
        check(self.lib.morig_logratio_forward(C.byref(a), _stream()), "morig_logratio_forward")
        return loss, tab

    def logratio_backward(self, feat_all, feat_aggr, gt, ptr, samples, tab, upstream, status):
        """-> (grad_all [N, T, D] or None, grad_aggr [N, D] or None): the sampled rows written, every other row exactly 0"""
        a = self._logratio_args(feat_all, feat_aggr, gt, ptr, samples, status)
        _need_gpu(tab, upstream)
        assert upstream.dtype == torch.float32 and upstream.numel() == 1 and tab.is_contiguous()
        assert tab.numel() == a.n_sets * a.n_meshes * 2 * a.n_sample * a.n_sample
        dev = gt.device
        wg_loss = torch.empty(a.n_sets * a.n_meshes, dtype=torch.float64, device=dev)
        g_all = g_aggr = None
        if feat_all is not None:
            g_all = torch.zeros(feat_all.shape, dtype=torch.float32, device=dev)
            a.grad_all, a.ldg_all, a.gset_stride = g_all.data_ptr(), g_all.stride(0), g_all.stride(1)
        if feat_aggr is not None:
            g_aggr = torch.zeros(feat_aggr.shape, dtype=torch.float32, device=dev)
            a.grad_aggr, a.ldg_aggr = g_aggr.data_ptr(), g_aggr.stride(0)
        a.tab, a.wg_loss, a.upstream = tab.data_ptr(), wg_loss.data_ptr(), upstream.data_ptr()
        check(self.lib.morig_logratio_backward(C.byref(a), _stream()), "morig_logratio_backward")
        return g_all, g_aggr

    def _skin_ce_check(self, x, label, mask, K):
        _need_gpu(x, label, mask)
        if not 1 <= K <= self.SKIN_CE_MAX_K:
            raise MorigNativeError(f"skin_ce_loss: {K} bones per vertex (MORIG_E_UNSUPPORTED: at most {self.SKIN_CE_MAX_K})")
        for t in (x, label, mask):
            assert t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1 and t.shape[0] == x.shape[0] and t.shape[1] >= K

    def skin_ce_forward(self, x, label, mask, K: int):
        """the first K columns of x, label, mask [N, >= K] -> (loss [1], vert_mask [N], sums float64 [2] = numerator, denominator)"""
        self._skin_ce_check(x, label, mask, K)
        n, dev = x.shape[0], x.device
        vert_mask = torch.empty(n, dtype=torch.float32, device=dev)
        part = torch.empty(2 * ((n + 255) // 256), dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(self.lib.morig_skin_ce_forward(_p(x), x.stride(0), _p(label), label.stride(0), _p(mask), mask.stride(0), n, K, _p(vert_mask), _p(part),
                                             _p(sums), _p(loss), _stream()), "morig_skin_ce_forward")
        return loss, vert_mask, sums

    def skin_ce_backward(self, x, label, mask, K: int, sums, upstream):
        self._skin_ce_check(x, label, mask, K)
        _need_gpu(sums, upstream)
        assert sums.dtype == torch.float64 and sums.numel() == 2 and upstream.dtype == torch.float32 and upstream.numel() == 1
        grad = torch.empty(x.shape[0], K, dtype=torch.float32, device=x.device)
        check(self.lib.morig_skin_ce_backward(_p(x), x.stride(0), _p(label), label.stride(0), _p(mask), mask.stride(0), x.shape[0], K, _p(sums),
                                              _p(upstream), _p(grad), _stream()), "morig_skin_ce_backward")
        return grad

    def _ce_probs_check(self, x, target, weight):
        _need_gpu(x, target, weight)
        if not 1 <= x.shape[1] <= self.CE_PROBS_MAX_K:
            raise MorigNativeError(f"cross_entropy_with_probs: {x.shape[1]} classes (MORIG_E_UNSUPPORTED: at most {self.CE_PROBS_MAX_K})")
        for t in (x, target, weight):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape)

    def ce_probs_forward(self, x, target, weight, reduction: str):
        """x, target, weight (or None) [N, K] contiguous -> the [N, K] matrix for "none", the loss [1] for "mean" / "sum" """
        self._ce_probs_check(x, target, weight)
        n, K, dev = x.shape[0], x.shape[1], x.device
        mode = self.CE_REDUCTIONS[reduction]
        if mode == 0:
            cum = torch.empty(n, K, dtype=torch.float32, device=dev)
            check(self.lib.morig_ce_probs_forward(_p(x), _p(target), _p(weight), n, K, 0, _p(cum), None, None, None, _stream()),
                  "morig_ce_probs_forward")
            return cum
        part = torch.empty(2 * ((n + 255) // 256), dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(self.lib.morig_ce_probs_forward(_p(x), _p(target), _p(weight), n, K, mode, None, _p(part), _p(sums), _p(loss), _stream()),
              "morig_ce_probs_forward")
        return loss

    def ce_probs_backward(self, x, target, weight, reduction: str, upstream):
        """upstream: [N, K] contiguous for "none", [1] otherwise -> d x [N, K]"""
        self._ce_probs_check(x, target, weight)
        _need_gpu(upstream)
        mode = self.CE_REDUCTIONS[reduction]
        assert upstream.dtype == torch.float32 and upstream.is_contiguous() and upstream.numel() == (x.numel() if mode == 0 else 1)
        grad = torch.empty_like(x)
        check(self.lib.morig_ce_probs_backward(_p(x), _p(target), _p(weight), x.shape[0], x.shape[1], mode, _p(upstream), _p(grad), _stream()),
              "morig_ce_probs_backward")
        return grad

    # -- rig evaluation metrics (csrc/metrics.hip; morig_amd/metrics.py holds the public functions) -------------------------------
    ASSIGN_MAX_SMALL, ASSIGN_MAX_LARGE = _K["MORIG_ASSIGN_MAX_SMALL"], _K["MORIG_ASSIGN_MAX_LARGE"]
    ASSIGN_ST_SIZE, ASSIGN_ST_PTR, ASSIGN_ST_INFEASIBLE = _K["MORIG_ASSIGN_ST_SIZE"], _K["MORIG_ASSIGN_ST_PTR"], _K["MORIG_ASSIGN_ST_INFEASIBLE"]

    @staticmethod
    def _ptr32(*ptrs):
        for p in ptrs:
            _need_gpu(p)
            assert p.dtype == torch.int32 and p.dim() == 1 and p.is_contiguous() and p.numel() >= 1

    def bone_sample_counts(self, joints: torch.Tensor, bones: torch.Tensor) -> torch.Tensor:
        """joints float64 [J, 3], bones int32 [n, 2] (parent, child) rows of joints -> int64 [n] samples per bone"""
        _need_gpu(bones, joints)
        self._pts64(joints)
        assert bones.dtype == torch.int32 and bones.dim() == 2 and bones.shape[1] == 2 and bones.is_contiguous()
        counts = torch.empty(bones.shape[0], dtype=torch.int64, device=joints.device)
        check(self.lib.morig_bone_sample_counts(_p(joints), joints.shape[0], _p(bones), bones.shape[0], _p(counts), _stream()),
              "morig_bone_sample_counts")
        return counts

    def bone_samples(self, joints: torch.Tensor, bones: torch.Tensor, off: torch.Tensor, n_samples: int) -> torch.Tensor:
        """off int64 [n + 1]: exclusive prefix sum of the counts -> float64 [n_samples, 3]"""
        _need_gpu(bones, off, joints)
        self._pts64(joints)
        assert off.dtype == torch.int64 and off.is_contiguous() and off.numel() == bones.shape[0] + 1
        out = torch.empty(n_samples, 3, dtype=torch.float64, device=joints.device)
        check(self.lib.morig_bone_samples(_p(joints), joints.shape[0], _p(bones), _p(off), bones.shape[0], n_samples, _p(out), _stream()),
              "morig_bone_samples")
        return out

    def nearest_distance(self, a: torch.Tensor, a_ptr: torch.Tensor, b: torch.Tensor, b_ptr: torch.Tensor, squared: bool) -> tuple:
        """-> (float64 [len(a)], int32 [n_meshes] flags: 1 where a mesh has rows in a and none in b)"""
        _need_gpu(a, b)
        self._pts64(a)
        self._pts64(b)
        self._ptr32(a_ptr, b_ptr)
        assert a_ptr.numel() == b_ptr.numel() and a_ptr.numel() >= 2
        nm = a_ptr.numel() - 1
        out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
        flags = torch.zeros(nm, dtype=torch.int32, device=a.device)
        check(self.lib.morig_nearest_distance(_p(a), _p(a_ptr), a.shape[0], _p(b), _p(b_ptr), b.shape[0], nm, int(squared), _p(out), _p(flags),
                                              _stream()), "morig_nearest_distance")
        return out, flags

    def segment_mean(self, x: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
        _need_gpu(x)
        self._ptr32(ptr)
        assert x.dtype == torch.float64 and x.dim() == 1 and x.is_contiguous()
        out = torch.empty(ptr.numel() - 1, dtype=torch.float64, device=x.device)
        check(self.lib.morig_segment_mean(_p(x), _p(ptr), x.numel(), ptr.numel() - 1, _p(out), _stream()), "morig_segment_mean")
        return out

    def assign_joints(self, pred: torch.Tensor, pred_ptr: torch.Tensor, gt: torch.Tensor, gt_ptr: torch.Tensor, match_ptr: torch.Tensor,
                      n_match: int, cost_off: torch.Tensor, n_cost: int) -> tuple:
        """-> (row_ind int32 [n_match], col_ind int32 [n_match], dist float64 [n_match], status int32 [n_meshes])"""
        _need_gpu(pred, gt)
        self._pts64(pred)
        self._pts64(gt)
        self._ptr32(pred_ptr, gt_ptr, match_ptr)
        _need_gpu(cost_off)
        nm = pred_ptr.numel() - 1
        assert gt_ptr.numel() == match_ptr.numel() == cost_off.numel() == nm + 1 and cost_off.dtype == torch.int64 and cost_off.is_contiguous()
        dev = pred.device
        row = torch.empty(n_match, dtype=torch.int32, device=dev)
        col = torch.empty(n_match, dtype=torch.int32, device=dev)
        dist = torch.empty(n_match, dtype=torch.float64, device=dev)
        status = torch.empty(nm, dtype=torch.int32, device=dev)
        cost = torch.empty(n_cost, dtype=torch.float64, device=dev)
        check(self.lib.morig_assign_joints(_p(pred), _p(pred_ptr), pred.shape[0], _p(gt), _p(gt_ptr), gt.shape[0], nm, _p(match_ptr), n_match,
                                           _p(cost), _p(cost_off), n_cost, _p(row), _p(col), _p(dist), _p(status), _stream()),
              "morig_assign_joints")
        return row, col, dist, status

    def joint_scores(self, row_ind: torch.Tensor, dist: torch.Tensor, match_ptr: torch.Tensor, pred_ptr: torch.Tensor, gt_ptr: torch.Tensor,
                     fs: torch.Tensor, fs_ptr: torch.Tensor) -> tuple:
        """-> (hits int32 [n_meshes], float64 [3, n_meshes]: IoU, precision, recall)"""
        _need_gpu(row_ind, dist, fs)
        self._ptr32(match_ptr, pred_ptr, gt_ptr, fs_ptr)
        nm = match_ptr.numel() - 1
        assert pred_ptr.numel() == gt_ptr.numel() == fs_ptr.numel() == nm + 1
        assert row_ind.dtype == torch.int32 and row_ind.is_contiguous() and dist.dtype == torch.float64 and dist.is_contiguous()
        assert row_ind.numel() == dist.numel() and fs.dtype == torch.float64 and fs.dim() == 1 and fs.is_contiguous()
        hits = torch.empty(nm, dtype=torch.int32, device=dist.device)
        out = torch.empty(3, nm, dtype=torch.float64, device=dist.device)
        check(self.lib.morig_joint_scores(_p(row_ind), _p(dist), _p(match_ptr), row_ind.numel(), _p(pred_ptr), _p(gt_ptr), _p(fs), _p(fs_ptr),
                                          fs.numel(), nm, _p(hits), _p(out), _stream()), "morig_joint_scores")
        return hits, out

    def valid_mean(self, x: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
        """x float64 [rows, n], valid int32 [n] -> float64 [rows]: the sum over the valid columns in index order / their number"""
        _need_gpu(x, valid)
        assert x.dtype == torch.float64 and x.dim() == 2 and x.is_contiguous() and valid.dtype == torch.int32 and valid.numel() == x.shape[1]
        out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        check(self.lib.morig_valid_mean(_p(x), _p(valid), x.shape[0], x.shape[1], _p(out), _stream()), "morig_valid_mean")
        return out

    # -- motion-stage evaluation (csrc/motion_metrics.hip; morig_amd/motion_metrics.py holds the public functions) ------------------------
    CURVE_MAX_BINS, MOTION_ST_INDEX = _K["MORIG_CURVE_MAX_BINS"], _K["MORIG_MOTION_ST_INDEX"]

    def corr_hits(self, pts: torch.Tensor, ptr_pts: torch.Tensor, nn: torch.Tensor, ptr_vtx: torch.Tensor, nn_global: bool, corr: torch.Tensor,
                  ptr_corr: torch.Tensor, tol: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
        """pts float32 [P, 3], nn int32 [V], corr int64 [n, 2], tol float32 [n_tol] -> hits int64 [n_pairs, n_tol]; status: the word of
        the segment_ptr calls, gains MOTION_ST_INDEX"""
        _need_gpu(pts, nn, corr, tol, status)
        self._ptr32(ptr_pts, ptr_vtx, ptr_corr)
        B = ptr_corr.numel() - 1
        assert ptr_pts.numel() == ptr_vtx.numel() == B + 1 and B >= 1
        assert pts.dtype == torch.float32 and pts.dim() == 2 and pts.shape[1] == 3 and pts.is_contiguous()
        assert nn.dtype == torch.int32 and nn.dim() == 1 and nn.is_contiguous()
        assert corr.dtype == torch.int64 and corr.dim() == 2 and corr.shape[1] == 2 and corr.is_contiguous()
        assert tol.dtype == torch.float32 and tol.dim() == 1 and tol.is_contiguous() and status.dtype == torch.int32
        hits = torch.empty(B, tol.numel(), dtype=torch.int64, device=pts.device)
        check(self.lib.morig_corr_hits(_p(pts), pts.shape[0], _p(ptr_pts), _p(nn), nn.numel(), _p(ptr_vtx), int(bool(nn_global)), _p(corr),
                                       corr.shape[0], _p(ptr_corr), B, _p(tol), tol.numel(), _p(hits), _p(status), _stream()), "morig_corr_hits")
        return hits

    def pr_counts(self, pred: torch.Tensor, gt: torch.Tensor, ptr: torch.Tensor, thr: torch.Tensor, normalize: bool, status: torch.Tensor) -> tuple:
        """pred float32 [V], gt uint8 [V], thr float32 [n_thr] -> (tp, pp int64 [n_meshes, n_thr], gp int64 [n_meshes])"""
        _need_gpu(pred, gt, thr, status)
        self._ptr32(ptr)
        B = ptr.numel() - 1
        assert pred.dtype == torch.float32 and pred.dim() == 1 and pred.is_contiguous() and gt.dtype == torch.uint8 and gt.is_contiguous()
        assert gt.shape == pred.shape and thr.dtype == torch.float32 and thr.dim() == 1 and thr.is_contiguous() and B >= 1
        tp = torch.empty(B, thr.numel(), dtype=torch.int64, device=pred.device)
        pp, gp = torch.empty_like(tp), torch.empty(B, dtype=torch.int64, device=pred.device)
        check(self.lib.morig_pr_counts(_p(pred), _p(gt), _p(ptr), pred.numel(), B, _p(thr), thr.numel(), int(bool(normalize)), _p(tp), _p(pp),
                                       _p(gp), _p(status), _stream()), "morig_pr_counts")
        return tp, pp, gp

    # -- rig assembly (csrc/rig_assemble.hip; morig_amd/rigging.py holds the public functions) ---------------------------------------
    RIG_RAW = _K["MORIG_RIG_RAW"]

    def rig_assemble(self, W: torch.Tensor, vtx_ptr: torch.Tensor, joint_ptr: torch.Tensor, seg_ptr: torch.Tensor, bone_ptr: torch.Tensor,
                     bones: torch.Tensor, ld_out: int, raw: bool = False) -> torch.Tensor:
        """W float64 [N, n_cols] with any row stride (a view of a wider block is read in place); the int32 tables of
        include/morig_hip.h -> float64 [N, ld_out]"""
        _need_gpu(W, bones)
        self._ptr32(vtx_ptr, joint_ptr, seg_ptr, bone_ptr)
        assert W.dtype == torch.float64 and W.dim() == 2 and (W.shape[1] == 0 or W.stride(1) == 1) and W.stride(0) >= W.shape[1]
        assert bones.dtype == torch.int32 and bones.dim() == 1 and bones.is_contiguous()
        nm = vtx_ptr.numel() - 1
        assert nm >= 1 and joint_ptr.numel() == nm + 1 and ld_out >= 0
        out = torch.empty(W.shape[0], ld_out, dtype=torch.float64, device=W.device)
        check(self.lib.morig_rig_assemble(_p(W), W.stride(0), W.shape[1], W.shape[0], _p(vtx_ptr), _p(joint_ptr), nm, _p(seg_ptr),
                                          seg_ptr.numel() - 1, _p(bone_ptr), bone_ptr.numel() - 1, _p(bones), bones.numel(),
                                          self.RIG_RAW if raw else 0, _p(out), ld_out, _stream()), "morig_rig_assemble")
        return out

    def rig_skin_counts(self, x: torch.Tensor, vtx_ptr: torch.Tensor) -> torch.Tensor:
        """x float64 [N, J] contiguous -> int32 [N]: the entries != 0 of every row"""
        _need_gpu(x)
        self._ptr32(vtx_ptr)
        assert x.dtype == torch.float64 and x.dim() == 2 and x.is_contiguous() and vtx_ptr.numel() >= 2
        counts = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        check(self.lib.morig_rig_skin_entries(_p(x), x.shape[1], x.shape[0], x.shape[1], _p(vtx_ptr), vtx_ptr.numel() - 1, _p(counts), None, 0,
                                              None, None, None, _stream()), "morig_rig_skin_entries")
        return counts

    def rig_skin_fill(self, x: torch.Tensor, vtx_ptr: torch.Tensor, ent_ptr: torch.Tensor, n_entries: int) -> tuple:
        """ent_ptr int32 [N + 1]: exclusive prefix sum of the counts -> (vertex int32, joint int32, weight float64) [n_entries]"""
        _need_gpu(x)
        self._ptr32(vtx_ptr, ent_ptr)
        assert x.dtype == torch.float64 and x.dim() == 2 and x.is_contiguous() and ent_ptr.numel() == x.shape[0] + 1 and n_entries >= 0
        vertex = torch.empty(n_entries, dtype=torch.int32, device=x.device)
        joint = torch.empty(n_entries, dtype=torch.int32, device=x.device)
        weight = torch.empty(n_entries, dtype=torch.float64, device=x.device)
        check(self.lib.morig_rig_skin_entries(_p(x), x.shape[1], x.shape[0], x.shape[1], _p(vtx_ptr), vtx_ptr.numel() - 1, None, _p(ent_ptr),
                                              n_entries, _p(vertex), _p(joint), _p(weight), _stream()), "morig_rig_skin_entries")
        return vertex, joint, weight

    # -- tracking without a rig (csrc/piecewise.hip; morig_amd/piecewise.py holds the public functions) -------------------------------
    RANSAC_SMALLEST_SUM, RANSAC_REFIT, RANSAC_NONE = _K["MORIG_RANSAC_SMALLEST_SUM"], _K["MORIG_RANSAC_REFIT"], _K["MORIG_RANSAC_NONE"]
    KMEANS_OK, KMEANS_BAD_MESH, KMEANS_NO_CLUSTER = _K["MORIG_KMEANS_OK"], _K["MORIG_KMEANS_BAD_MESH"], _K["MORIG_KMEANS_NO_CLUSTER"]
    KMEANS_MAX_CLUSTERS, KMEANS_MAX_DIM = _K["MORIG_KMEANS_MAX_CLUSTERS"], _K["MORIG_KMEANS_MAX_DIM"]

    def _ransac_check(self, src, dst, handles, hptr, samples):
        _need_gpu(src, dst, handles, samples)
        self._pts64(src)
        self._pts64(dst)
        self._ptr32(hptr)
        assert src.shape == dst.shape and handles.dtype == torch.int32 and handles.dim() == 1 and handles.is_contiguous()
        n_problems = hptr.numel() - 1
        assert samples.dtype == torch.int32 and samples.dim() == 3 and samples.shape[0] == n_problems and samples.shape[2] == 3
        assert samples.is_contiguous()
        return n_problems, samples.shape[1]

    def ransac_vote(self, src, dst, handles, hptr, samples, inlier_dist: float) -> tuple:
        """src, dst float64 [N, 3]; handles int32 [H] rows of them in CSR form by hptr int32 [P + 1]; samples int32 [P, n_iter, 3]
        -> (inlier count int32 [P, n_iter], distance sum float64 [P, n_iter])"""
        P, n_iter = self._ransac_check(src, dst, handles, hptr, samples)
        count = torch.empty(P, n_iter, dtype=torch.int32, device=src.device)
        dsum = torch.empty(P, n_iter, dtype=torch.float64, device=src.device)
        check(self.lib.morig_ransac_vote(_p(src), _p(dst), src.shape[0], _p(handles), handles.numel(), _p(hptr), P, _p(samples), n_iter,
                                         float(inlier_dist), _p(count), _p(dsum), _stream()), "morig_ransac_vote")
        return count, dsum

    def ransac_fit(self, src, dst, handles, hptr, samples, count, dsum, inlier_dist: float, refit_share: float) -> tuple:
        """the votes of ransac_vote -> (chosen int32 [P, 2] = hypothesis by count, by sum (-1: none), best count int32 [P], flag int32 [P]
        (RANSAC_*), Rt float64 [P, 12] = R row-major, t)"""
        P, n_iter = self._ransac_check(src, dst, handles, hptr, samples)
        assert count.dtype == torch.int32 and dsum.dtype == torch.float64 and count.shape == dsum.shape == (P, n_iter)
        assert count.is_contiguous() and dsum.is_contiguous()
        dev = src.device
        chosen = torch.empty(P, 2, dtype=torch.int32, device=dev)
        best = torch.empty(P, dtype=torch.int32, device=dev)
        flag = torch.empty(P, dtype=torch.int32, device=dev)
        Rt = torch.empty(P, 12, dtype=torch.float64, device=dev)
        check(self.lib.morig_ransac_fit(_p(src), _p(dst), src.shape[0], _p(handles), handles.numel(), _p(hptr), P, _p(samples), n_iter,
                                        _p(count), _p(dsum), float(inlier_dist), float(refit_share), _p(chosen), _p(best), _p(flag), _p(Rt),
                                        _stream()), "morig_ransac_fit")
        return chosen, best, flag, Rt

    def ransac_apply(self, src, dst, problem_of, flag, Rt) -> torch.Tensor:
        """problem_of int32 [N] (-1: the vertex takes dst) -> float64 [N, 3]"""
        _need_gpu(src, dst, problem_of, flag, Rt)
        self._pts64(src)
        self._pts64(dst)
        assert src.shape == dst.shape and problem_of.dtype == torch.int32 and problem_of.shape == (src.shape[0],) and problem_of.is_contiguous()
        P = flag.numel()
        assert flag.dtype == torch.int32 and flag.is_contiguous() and Rt.dtype == torch.float64 and Rt.shape == (P, 12) and Rt.is_contiguous()
        out = torch.empty_like(src)
        check(self.lib.morig_ransac_apply(_p(src), _p(dst), src.shape[0], _p(problem_of), P, _p(flag), _p(Rt), _p(out), _stream()),
              "morig_ransac_apply")
        return out

    def kernel_kmeans(self, X, pos, vptr, first, n_clusters: int, max_iter: int, w_euc: float, tol: float) -> dict:
        """X float32 or float64 [N, D], pos float64 [N, 3], vptr int32 [B + 1], first int32 [B] -> dict(labels int64 [N], seeds int32
        [B, K], info int32 [B, 4] = (KMEANS_* status, iterations, kept clusters, 0), members int32 [B, K], centres_emb float64 [B, K, D],
        centres_euc float64 [B, K, 3], fit float64 [B]). Sizes beyond KMEANS_MAX_CLUSTERS / KMEANS_MAX_DIM are refused by status."""
        _need_gpu(X, pos, first)
        self._pts64(pos)
        self._ptr32(vptr, first)
        assert X.dtype in (torch.float32, torch.float64) and X.dim() == 2 and X.is_contiguous() and X.shape[0] == pos.shape[0]
        B, N, D, K, dev = vptr.numel() - 1, X.shape[0], X.shape[1], int(n_clusters), X.device
        assert first.numel() == B and K >= 1 and D >= 1
        ok = K <= self.KMEANS_MAX_CLUSTERS and D <= self.KMEANS_MAX_DIM                  # a refused call allocates no result
        i32 = lambda *s: torch.empty(*(s if ok else (1,)), dtype=torch.int32, device=dev)
        f64 = lambda *s: torch.empty(*(s if ok else (1,)), dtype=torch.float64, device=dev)
        res = dict(labels=torch.empty(N if ok else 1, dtype=torch.int64, device=dev), seeds=i32(B, K), info=i32(B, 4), members=i32(B, K),
                   centres_emb=f64(B, K, D), centres_euc=f64(B, K, 3), fit=f64(B))
        label_scratch, dist_scratch = i32(N), f64(N)
        check(self.lib.morig_kernel_kmeans(_p(X), 1 if X.dtype == torch.float64 else 0, _p(pos), N, D, _p(vptr), B, _p(first), K, int(max_iter),
                                           float(w_euc), float(tol), _p(label_scratch), _p(dist_scratch), _p(res["labels"]), _p(res["seeds"]),
                                           _p(res["info"]), _p(res["members"]), _p(res["centres_emb"]), _p(res["centres_euc"]), _p(res["fit"]),
                                           _stream()), "morig_kernel_kmeans")
        return res

    # -- the mesh front end (csrc/meshprep.hip; morig_amd/meshprep.py holds the public functions) -------------------------------------
    MESH_NORMALIZE, MESH_GRID = _K["MORIG_MESH_NORMALIZE"], _K["MORIG_MESH_GRID"]
    VOXEL_ROW_WORDS, VOXEL_MAX_DIMS = _K["MORIG_VOXEL_ROW_WORDS"], _K["MORIG_VOXEL_MAX_DIMS"]
    VOXEL_OK, VOXEL_SWEEP_BOUND = _K["MORIG_VOXEL_OK"], _K["MORIG_VOXEL_SWEEP_BOUND"]

    def _mesh_check(self, verts, vptr, faces=None, fptr=None):
        """verts float64 [N, 3], vptr int32 [B + 1] (host-checked by the caller to rise from 0 to N); faces int32 [F, 3], fptr alike"""
        _need_gpu(verts, vptr, faces, fptr)
        self._pts64(verts)
        self._ptr32(vptr)
        if faces is not None:
            self._ptr32(fptr)
            assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
            assert fptr.numel() == vptr.numel()
        return vptr.numel() - 1

    def mesh_bbox(self, verts, vptr) -> torch.Tensor:
        """-> float64 [B, 6]: minimum x, y, z, maximum x, y, z per mesh"""
        B = self._mesh_check(verts, vptr)
        bbox = torch.empty(B, 6, dtype=torch.float64, device=verts.device)
        check(self.lib.morig_mesh_bbox(_p(verts), _p(vptr), B, _p(bbox), _stream()), "morig_mesh_bbox")
        return bbox

    def mesh_affine(self, verts, vptr, frame, mode: int, mul: float = 1.0) -> torch.Tensor:
        """frame float64 [B, 4] = (t, s) -> (v - t) * s (MESH_NORMALIZE) or (v - t) / s * mul (MESH_GRID), float64 [N, 3]"""
        B = self._mesh_check(verts, vptr)
        _need_gpu(frame)
        assert frame.dtype == torch.float64 and frame.shape == (B, 4) and frame.is_contiguous()
        out = torch.empty_like(verts)
        check(self.lib.morig_mesh_affine(_p(verts), verts.shape[0], _p(vptr), B, _p(frame), int(mode), float(mul), _p(out), _stream()),
              "morig_mesh_affine")
        return out

    def tpl_edge_keys(self, faces, fptr, vptr) -> torch.Tensor:
        """-> int64 [6 F] directed pairs as keys (unsorted; INT64_MAX where a pair is none)"""
        _need_gpu(faces, fptr, vptr)
        self._ptr32(fptr, vptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fptr.numel() == vptr.numel()
        keys = torch.empty(6 * faces.shape[0], dtype=torch.int64, device=faces.device)
        check(self.lib.morig_tpl_edge_keys(_p(faces), faces.shape[0], _p(fptr), _p(vptr), vptr.numel() - 1, _p(keys), _stream()),
              "morig_tpl_edge_keys")
        return keys

    def tpl_edge_flags(self, keys) -> torch.Tensor:
        """sorted keys -> int32 [n]: 1 at the first key of every run"""
        _need_gpu(keys)
        assert keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
        flags = torch.empty(keys.numel(), dtype=torch.int32, device=keys.device)
        check(self.lib.morig_tpl_edge_flags(_p(keys), keys.numel(), _p(flags), _stream()), "morig_tpl_edge_flags")
        return flags

    def tpl_edge_compact(self, keys, flags, rank, vptr, n_edges: int) -> torch.Tensor:
        """-> int64 [2, n_edges]: (vertex, neighbour) of every flagged key, local to the mesh"""
        _need_gpu(keys, flags, rank, vptr)
        self._ptr32(vptr)
        n = keys.numel()
        assert keys.dtype == rank.dtype == torch.int64 and flags.dtype == torch.int32 and flags.numel() == rank.numel() == n
        assert keys.is_contiguous() and flags.is_contiguous() and rank.is_contiguous() and 0 <= n_edges <= n
        out = torch.empty(2, n_edges, dtype=torch.int64, device=keys.device)
        check(self.lib.morig_tpl_edge_compact(_p(keys), _p(flags), _p(rank), n, _p(vptr), vptr.numel() - 1, int(n_edges), _p(out), _stream()),
              "morig_tpl_edge_compact")
        return out

    def voxel_surface(self, grid, faces, fptr, vptr, dims: int) -> torch.Tensor:
        """grid float64 [N, 3] grid coordinates -> uint32-as-int32 [B, dims * dims, VOXEL_ROW_WORDS] surface bitset"""
        B = self._mesh_check(grid, vptr, faces, fptr)
        surface = torch.empty(B, max(int(dims), 0) ** 2, self.VOXEL_ROW_WORDS, dtype=torch.int32, device=grid.device)
        check(self.lib.morig_voxel_surface(_p(grid), _p(faces), faces.shape[0], _p(fptr), _p(vptr), B, int(dims), _p(surface), _stream()),
              "morig_voxel_surface")
        return surface

    def voxel_fill(self, surface, dims: int) -> tuple:
        """-> (solid uint8 [B, dims, dims, dims] indexed [x][y][z], info int32 [B, 2] = (VOXEL_* status, sweeps))"""
        _need_gpu(surface)
        dims = int(dims)
        assert surface.dtype == torch.int32 and surface.dim() == 3 and surface.is_contiguous()
        assert surface.shape[1:] == (max(dims, 0) ** 2, self.VOXEL_ROW_WORDS)
        B = surface.shape[0]
        ok = 1 <= dims <= self.VOXEL_MAX_DIMS                                         # a refused call allocates no result
        solid = torch.empty((B, dims, dims, dims) if ok else (1,), dtype=torch.uint8, device=surface.device)
        info = torch.empty(B, 2, dtype=torch.int32, device=surface.device)
        check(self.lib.morig_voxel_fill(_p(surface), B, dims, _p(solid), _p(info), _stream()), "morig_voxel_fill")
        return solid, info

    def tri_area_cdf(self, verts, vptr, faces, fptr) -> torch.Tensor:
        """-> float64 [F]: per mesh the running sum of its triangle areas in face order"""
        B = self._mesh_check(verts, vptr, faces, fptr)
        cum = torch.empty(faces.shape[0], dtype=torch.float64, device=verts.device)
        check(self.lib.morig_tri_area_cdf(_p(verts), _p(faces), _p(fptr), _p(vptr), B, _p(cum), _stream()), "morig_tri_area_cdf")
        return cum

    def surface_samples(self, verts, vptr, faces, fptr, cum, uniforms, cptr) -> tuple:
        """uniforms float64 [C, 3], cptr int32 [B + 1] -> (pts float64 [C, 3], normals float64 [C, 3], face int32 [C] local to the mesh)"""
        B = self._mesh_check(verts, vptr, faces, fptr)
        _need_gpu(cum, uniforms, cptr)
        self._pts64(uniforms)
        self._ptr32(cptr)
        assert cum.dtype == torch.float64 and cum.shape == (faces.shape[0],) and cum.is_contiguous() and cptr.numel() == B + 1
        n = uniforms.shape[0]
        pts, normals = torch.empty_like(uniforms), torch.empty_like(uniforms)
        tri = torch.empty(n, dtype=torch.int32, device=verts.device)
        check(self.lib.morig_surface_samples(_p(verts), _p(faces), _p(fptr), _p(vptr), B, _p(cum), _p(uniforms), _p(cptr), n, _p(pts), _p(normals),
                                             _p(tri), _stream()), "morig_surface_samples")
        return pts, normals, tri

    # -- mesh simplification (csrc/simplify.hip; morig_amd/meshprep.py simplify) -------------------------------------------------------
    SIMPLIFY_MAX_RES, SIMPLIFY_INDEX_BITS = _K["MORIG_SIMPLIFY_MAX_RES"], _K["MORIG_SIMPLIFY_INDEX_BITS"]
    SIMPLIFY_MAX_INDEX, SIMPLIFY_MESH_SHIFT = _K["MORIG_SIMPLIFY_MAX_INDEX"], _K["MORIG_SIMPLIFY_MESH_SHIFT"]

    def _simplify_frame(self, frame, res, B):
        _need_gpu(frame, res)
        assert frame.dtype == torch.float64 and frame.shape == (B, 4) and frame.is_contiguous()
        assert res.dtype == torch.int32 and res.shape == (B,) and res.is_contiguous()

    def simplify_cell_keys(self, verts, vptr, frame, res, min_res: int, max_res: int) -> torch.Tensor:
        """frame float64 [B, 4] = (bounding-box minimum, largest extent), res int32 [B] -> int64 [N]: mesh << 30 | cell key"""
        B = self._mesh_check(verts, vptr)
        self._simplify_frame(frame, res, B)
        keys = torch.empty(verts.shape[0], dtype=torch.int64, device=verts.device)
        check(self.lib.morig_simplify_cell_keys(_p(verts), verts.shape[0], _p(vptr), B, _p(frame), _p(res), int(min_res), int(max_res), _p(keys),
                                                _stream()), "morig_simplify_cell_keys")
        return keys

    def simplify_face_keys(self, faces, fptr, vptr, cell, n_cells: int) -> tuple:
        """cell int32 [N] -> (corner_cell int32 [3 F], keys int64 [F]: the sorted cell triple, INT64_MAX where two corners share a cell)"""
        _need_gpu(faces, fptr, vptr, cell)
        self._ptr32(fptr, vptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fptr.numel() == vptr.numel()
        assert cell.dtype == torch.int32 and cell.dim() == 1 and cell.is_contiguous()
        F = faces.shape[0]
        corner_cell = torch.empty(3 * F, dtype=torch.int32, device=faces.device)
        keys = torch.empty(F, dtype=torch.int64, device=faces.device)
        check(self.lib.morig_simplify_face_keys(_p(faces), F, _p(fptr), _p(vptr), vptr.numel() - 1, _p(cell), cell.numel(), int(n_cells),
                                                _p(corner_cell), _p(keys), _stream()), "morig_simplify_face_keys")
        return corner_cell, keys

    def simplify_face_compact(self, faces, fptr, vptr, cell, cptr, order, flags, rank, n_out: int) -> torch.Tensor:
        """-> int64 [n_out, 3]: the marked faces as cells local to their mesh, input orientation, smallest first"""
        _need_gpu(faces, fptr, vptr, cell, cptr, order, flags, rank)
        self._ptr32(fptr, vptr, cptr)
        F = faces.shape[0]
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert fptr.numel() == vptr.numel() == cptr.numel() and cell.dtype == torch.int32 and cell.is_contiguous()
        assert order.dtype == rank.dtype == torch.int64 and flags.dtype == torch.int32 and order.numel() == flags.numel() == rank.numel() == F
        assert order.is_contiguous() and flags.is_contiguous() and rank.is_contiguous() and 0 <= n_out <= F
        out = torch.empty(int(n_out), 3, dtype=torch.int64, device=faces.device)
        check(self.lib.morig_simplify_face_compact(_p(faces), F, _p(fptr), _p(vptr), vptr.numel() - 1, _p(cell), _p(cptr), _p(order), _p(flags),
                                                   _p(rank), int(n_out), _p(out), _stream()), "morig_simplify_face_compact")
        return out

    def simplify_quadrics(self, verts, vptr, faces, fptr, frame, res, min_res: int, max_res: int, cell_key, mptr, members, kptr, corners):
        """cell_key int64 [C]; mptr / kptr int64 [C + 1] the runs of every cell in members int64 [N] (vertex rows) and corners int64 [3 F]
        (3 face + corner) -> float64 [C, 3] the output vertices"""
        B = self._mesh_check(verts, vptr, faces, fptr)
        self._simplify_frame(frame, res, B)
        _need_gpu(cell_key, mptr, members, kptr, corners)
        n = cell_key.numel()
        for t in (cell_key, mptr, members, kptr, corners):
            assert t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous()
        assert mptr.numel() == kptr.numel() == n + 1 and members.numel() == verts.shape[0] and corners.numel() == 3 * faces.shape[0]
        out = torch.empty(n, 3, dtype=torch.float64, device=verts.device)
        check(self.lib.morig_simplify_quadrics(_p(verts), verts.shape[0], _p(vptr), _p(faces), faces.shape[0], _p(fptr), B, _p(frame), _p(res),
                                               int(min_res), int(max_res), _p(cell_key), _p(mptr), _p(members), _p(kptr), _p(corners), n, _p(out),
                                               _stream()), "morig_simplify_quadrics")
        return out

    # -- mesh diagnosis and cleaning (csrc/meshcheck.hip; morig_amd/meshprep.py diagnose / clean) ----------------------------------------
    MESHCHECK_BAD_FACE, MESHCHECK_ROUND_GUARD = _K["MORIG_MESHCHECK_BAD_FACE"], _K["MORIG_MESHCHECK_ROUND_GUARD"]
    EDGE_MANIFOLD, EDGE_BOUNDARY = _K["MORIG_EDGE_MANIFOLD"], _K["MORIG_EDGE_BOUNDARY"]
    EDGE_NONMANIFOLD, EDGE_CONFLICT = _K["MORIG_EDGE_NONMANIFOLD"], _K["MORIG_EDGE_CONFLICT"]

    @staticmethod
    def _vec(dtype, n, *ts):
        _need_gpu(*ts)
        for t in ts:
            assert t.dtype == dtype and t.dim() == 1 and t.numel() == n and t.is_contiguous(), (t.dtype, tuple(t.shape), dtype, n)

    def meshcheck_coord_keys(self, verts) -> tuple:
        """verts float64 [N, 3] -> (keys int64 [3, N]: an order-preserving key per coordinate, nonfinite int32 [N])"""
        _need_gpu(verts)
        self._pts64(verts)
        n = verts.shape[0]
        keys = torch.empty(3, n, dtype=torch.int64, device=verts.device)
        nonfinite = torch.empty(n, dtype=torch.int32, device=verts.device)
        check(self.lib.morig_meshcheck_coord_keys(_p(verts), n, _p(keys), _p(nonfinite), _stream()), "morig_meshcheck_coord_keys")
        return keys, nonfinite

    def meshcheck_weld_mark(self, keys, nonfinite, order, vptr) -> torch.Tensor:
        """order int64 [N]: the rows sorted stably by z, y, x -> flags int32 [N]: 1 at the first row of every run of equal rows of one mesh"""
        n = nonfinite.numel()
        self._vec(torch.int32, n, nonfinite)
        self._vec(torch.int64, n, order)
        self._ptr32(vptr)
        _need_gpu(keys)
        assert keys.dtype == torch.int64 and tuple(keys.shape) == (3, n) and keys.is_contiguous()
        flags = torch.empty(n, dtype=torch.int32, device=order.device)
        check(self.lib.morig_meshcheck_weld_mark(_p(keys), _p(nonfinite), _p(order), n, _p(vptr), vptr.numel() - 1, _p(flags), _stream()),
              "morig_meshcheck_weld_mark")
        return flags

    def meshcheck_run_rep(self, order, flags, rank, dead=None) -> torch.Tensor:
        """-> int32 [n]: for every item the first item of its run in ``order`` (-1 where ``dead``)"""
        n = order.numel()
        self._vec(torch.int64, n, order, rank)
        self._vec(torch.int32, n, flags, *(() if dead is None else (dead,)))
        start = torch.empty(n, dtype=torch.int32, device=order.device)
        rep = torch.empty(n, dtype=torch.int32, device=order.device)
        check(self.lib.morig_meshcheck_run_rep(_p(order), _p(flags), _p(rank), _p(dead), n, _p(start), _p(rep), _stream()), "morig_meshcheck_run_rep")
        return rep

    def meshcheck_face_keys(self, faces, fptr, vptr, rep, status) -> tuple:
        """rep int32 [N] -> (tri int32 [F, 3] the representatives of the corners, major, minor int64 [F], degenerate int32 [F])"""
        _need_gpu(faces, status)
        self._ptr32(fptr, vptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fptr.numel() == vptr.numel()
        self._vec(torch.int32, rep.numel(), rep)
        assert status.dtype == torch.int32 and status.numel() >= 1
        F, dev = faces.shape[0], faces.device
        tri = torch.empty(F, 3, dtype=torch.int32, device=dev)
        major, minor = torch.empty(F, dtype=torch.int64, device=dev), torch.empty(F, dtype=torch.int64, device=dev)
        degenerate = torch.empty(F, dtype=torch.int32, device=dev)
        check(self.lib.morig_meshcheck_face_keys(_p(faces), F, _p(fptr), _p(vptr), vptr.numel() - 1, _p(rep), rep.numel(), _p(tri), _p(major),
                                                 _p(minor), _p(degenerate), _p(status), _stream()), "morig_meshcheck_face_keys")
        return tri, major, minor, degenerate

    def meshcheck_face_mark(self, major, minor, order) -> torch.Tensor:
        """order int64 [F]: the faces sorted stably by minor, then major -> flags int32 [F]: 1 at the first face of every vertex set"""
        F = order.numel()
        self._vec(torch.int64, F, major, minor, order)
        flags = torch.empty(F, dtype=torch.int32, device=order.device)
        check(self.lib.morig_meshcheck_face_mark(_p(major), _p(minor), _p(order), F, _p(flags), _stream()), "morig_meshcheck_face_mark")
        return flags

    def _tri(self, tri, surv):
        _need_gpu(tri)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.is_contiguous()
        self._vec(torch.int32, tri.shape[0], surv)
        return tri.shape[0]

    def meshcheck_face_edges(self, verts, tri, surv) -> tuple:
        """-> (referenced int32 [N], zero_area int32 [F], ekeys int64 [3 F]: lo << 32 | hi << 1 | dir of the kept faces, else INT64_MAX)"""
        _need_gpu(verts)
        self._pts64(verts)
        F, n, dev = self._tri(tri, surv), verts.shape[0], verts.device
        referenced = torch.empty(n, dtype=torch.int32, device=dev)
        zero_area = torch.empty(F, dtype=torch.int32, device=dev)
        ekeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        check(self.lib.morig_meshcheck_face_edges(_p(verts), n, _p(tri), _p(surv), F, _p(referenced), _p(zero_area), _p(ekeys), _stream()),
              "morig_meshcheck_face_edges")
        return referenced, zero_area, ekeys

    def meshcheck_cc_round(self, cur, nxt, ekeys, vptr, changed) -> None:
        """one round of the component rule: reads ``cur``, writes ``nxt`` and ``changed`` int32 [B] (1: the labels of that mesh moved)"""
        n = cur.numel()
        self._vec(torch.int32, n, cur, nxt)
        self._vec(torch.int64, ekeys.numel(), ekeys)
        self._ptr32(vptr)
        self._vec(torch.int32, vptr.numel() - 1, changed)
        assert cur.data_ptr() != nxt.data_ptr() or n == 0
        check(self.lib.morig_meshcheck_cc_round(_p(cur), _p(nxt), n, _p(ekeys), ekeys.numel(), _p(vptr), vptr.numel() - 1, _p(changed), _stream()),
              "morig_meshcheck_cc_round")

    def meshcheck_edge_classify(self, keys, label) -> tuple:
        """keys: the sorted edge keys -> (eclass int32 [3 F]: EDGE_* at the first key of every run, root_boundary int32 [N])"""
        self._vec(torch.int64, keys.numel(), keys)
        self._vec(torch.int32, label.numel(), label)
        eclass = torch.empty(keys.numel(), dtype=torch.int32, device=keys.device)
        root_boundary = torch.empty(label.numel(), dtype=torch.int32, device=keys.device)
        check(self.lib.morig_meshcheck_edge_classify(_p(keys), keys.numel(), _p(label), label.numel(), _p(eclass), _p(root_boundary), _stream()),
              "morig_meshcheck_edge_classify")
        return eclass, root_boundary

    def meshcheck_comp_counts(self, tri, surv, referenced, label) -> tuple:
        """-> (root_verts, root_faces int32 [N] per label, face_root int64 [F])"""
        F, n, dev = self._tri(tri, surv), label.numel(), tri.device
        self._vec(torch.int32, n, referenced, label)
        root_verts, root_faces = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        face_root = torch.empty(F, dtype=torch.int64, device=dev)
        check(self.lib.morig_meshcheck_comp_counts(_p(tri), _p(surv), F, _p(referenced), _p(label), n, _p(root_verts), _p(root_faces), _p(face_root),
                                                   _stream()), "morig_meshcheck_comp_counts")
        return root_verts, root_faces, face_root

    def meshcheck_comp_area(self, verts, tri, order, kptr) -> torch.Tensor:
        """order int64 [F]: the faces sorted stably by root, kptr int64 [C + 1] -> area float64 [C]"""
        _need_gpu(verts, tri)
        self._pts64(verts)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.is_contiguous()
        self._vec(torch.int64, tri.shape[0], order)
        self._vec(torch.int64, kptr.numel(), kptr)
        C = kptr.numel() - 1
        area = torch.empty(C, dtype=torch.float64, device=verts.device)
        check(self.lib.morig_meshcheck_comp_area(_p(verts), verts.shape[0], _p(tri), tri.shape[0], _p(order), _p(kptr), C, _p(area), _stream()),
              "morig_meshcheck_comp_area")
        return area

    def meshcheck_keep_flags(self, rep, referenced, label, keep_root, drop_unreferenced: bool, tri, surv) -> tuple:
        """-> (vkeep int32 [N], fkeep int32 [F]): the rows and faces that leave"""
        F, n, dev = self._tri(tri, surv), rep.numel(), rep.device
        self._vec(torch.int32, n, rep, referenced, label, keep_root)
        vkeep, fkeep = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
        check(self.lib.morig_meshcheck_keep_flags(_p(rep), _p(referenced), _p(label), _p(keep_root), int(bool(drop_unreferenced)), n, _p(tri), _p(surv),
                                                  F, _p(vkeep), _p(fkeep), _stream()), "morig_meshcheck_keep_flags")
        return vkeep, fkeep

    def meshcheck_compact(self, verts, rep, vkeep, vrank, vptr, ovptr, tri, surv, fkeep, frank, fptr, ofptr, n_out_v: int, n_out_f: int) -> tuple:
        """-> (out_verts float64 [n_out_v, 3], out_faces int64 [n_out_f, 3], vertex_map int64 [N], face_map int64 [F])"""
        _need_gpu(verts)
        self._pts64(verts)
        F, n, dev = self._tri(tri, surv), verts.shape[0], verts.device
        self._ptr32(vptr, fptr)
        B = vptr.numel() - 1
        self._vec(torch.int32, n, rep, vkeep)
        self._vec(torch.int32, F, fkeep)
        self._vec(torch.int64, n, vrank)
        self._vec(torch.int64, F, frank)
        self._vec(torch.int64, B + 1, ovptr, ofptr)
        assert fptr.numel() == B + 1 and 0 <= n_out_v <= n and 0 <= n_out_f <= F
        out_verts = torch.empty(int(n_out_v), 3, dtype=torch.float64, device=dev)
        out_faces = torch.empty(int(n_out_f), 3, dtype=torch.int64, device=dev)
        vertex_map, face_map = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(F, dtype=torch.int64, device=dev)
        check(self.lib.morig_meshcheck_compact(_p(verts), _p(rep), _p(vkeep), _p(vrank), _p(vptr), _p(ovptr), n, B, _p(tri), _p(surv), _p(fkeep),
                                               _p(frank), _p(fptr), _p(ofptr), F, int(n_out_v), int(n_out_f), _p(out_verts), _p(out_faces),
                                               _p(vertex_map), _p(face_map), _stream()), "morig_meshcheck_compact")
        return out_verts, out_faces, vertex_map, face_map

    # -- mesh repair (csrc/meshfix.hip; morig_amd/meshprep.py repair) --------------------------------------------------------------------
    MESHFIX_ORIENTABLE, MESHFIX_NONORIENTABLE = _K["MORIG_MESHFIX_ORIENTABLE"], _K["MORIG_MESHFIX_NONORIENTABLE"]
    MESHFIX_CLOSED, MESHFIX_INVERTED = _K["MORIG_MESHFIX_CLOSED"], _K["MORIG_MESHFIX_INVERTED"]
    MESHFIX_REGULAR, MESHFIX_TANGLED = _K["MORIG_MESHFIX_REGULAR"], _K["MORIG_MESHFIX_TANGLED"]

    @staticmethod
    def _new(device, dtype, *shape):
        return torch.empty(*shape, dtype=dtype, device=device)

    def meshfix_edge_records(self, faces, fptr, vptr, n_rows: int, status) -> tuple:
        """-> (tri int32 [F, 3] the corners as rows, keys int64 [3 F] = lo << 32 | hi, vals int32 [3 F] = face << 1 | dir), face-major"""
        _need_gpu(faces, status)
        self._ptr32(fptr, vptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fptr.numel() == vptr.numel()
        assert status.dtype == torch.int32 and status.numel() >= 1
        F, dev = faces.shape[0], faces.device
        tri, keys, vals = self._new(dev, torch.int32, F, 3), self._new(dev, torch.int64, 3 * F), self._new(dev, torch.int32, 3 * F)
        check(self.lib.morig_meshfix_edge_records(_p(faces), F, _p(fptr), _p(vptr), vptr.numel() - 1, int(n_rows), _p(tri), _p(keys), _p(vals),
                                                  _p(status), _stream()), "morig_meshfix_edge_records")
        return tri, keys, vals

    def meshfix_links(self, keys, vals, n_faces: int) -> tuple:
        """keys / vals: the records sorted stably by key -> (cover int64 [3 F]: the double cover's edges, face_open int32 [F], bflag int32 [3 F])"""
        n = keys.numel()
        self._vec(torch.int64, n, keys)
        self._vec(torch.int32, n, vals)
        dev = keys.device
        cover, face_open, bflag = self._new(dev, torch.int64, n), self._new(dev, torch.int32, int(n_faces)), self._new(dev, torch.int32, n)
        check(self.lib.morig_meshfix_links(_p(keys), _p(vals), n, int(n_faces), _p(cover), _p(face_open), _p(bflag), _stream()), "morig_meshfix_links")
        return cover, face_open, bflag

    def meshfix_orient_stats(self, lab, face_open) -> tuple:
        """lab int32 [2 F]: the cover's labels -> (root, parity int32 [F], face_root int64 [F], root_open int32 [F])"""
        F, dev = face_open.numel(), face_open.device
        self._vec(torch.int32, 2 * F, lab)
        self._vec(torch.int32, F, face_open)
        root, parity, root_open = (self._new(dev, torch.int32, F) for _ in range(3))
        face_root = self._new(dev, torch.int64, F)
        check(self.lib.morig_meshfix_orient_stats(_p(lab), _p(face_open), F, _p(root), _p(parity), _p(face_root), _p(root_open), _stream()),
              "morig_meshfix_orient_stats")
        return root, parity, face_root, root_open

    def meshfix_signed_volume(self, verts, tri, parity, order, kptr, roots) -> tuple:
        """order int64 [F]: the faces sorted stably by root, kptr int64 [C + 1], roots int64 [C] -> (vol float64, cnt, cnt1 int32) [F], at the roots"""
        _need_gpu(verts, tri)
        self._pts64(verts)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.is_contiguous()
        F, C_, dev = tri.shape[0], roots.numel(), verts.device
        self._vec(torch.int32, F, parity)
        self._vec(torch.int64, F, order)
        self._vec(torch.int64, C_ + 1, kptr)
        self._vec(torch.int64, C_, roots)
        vol, cnt, cnt1 = self._new(dev, torch.float64, F), self._new(dev, torch.int32, F), self._new(dev, torch.int32, F)
        check(self.lib.morig_meshfix_signed_volume(_p(verts), verts.shape[0], _p(tri), _p(parity), F, _p(order), _p(kptr), _p(roots), C_, _p(vol),
                                                   _p(cnt), _p(cnt1), _stream()), "morig_meshfix_signed_volume")
        return vol, cnt, cnt1

    def meshfix_orient_apply(self, tri, fptr, vptr, lab, root, parity, root_open, vol, cnt, cnt1) -> tuple:
        """-> (faces int64 [F, 3] local to their mesh, corners 1 and 2 exchanged where flipped int32 [F], rootinfo int32 [F]: MESHFIX_* bits at the roots)"""
        _need_gpu(tri, vol)
        self._ptr32(fptr, vptr)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.is_contiguous() and fptr.numel() == vptr.numel()
        F, dev = tri.shape[0], tri.device
        self._vec(torch.int32, 2 * F, lab)
        self._vec(torch.int32, F, root, parity, root_open, cnt, cnt1)
        self._vec(torch.float64, F, vol)
        out, flipped, info = self._new(dev, torch.int64, F, 3), self._new(dev, torch.int32, F), self._new(dev, torch.int32, F)
        check(self.lib.morig_meshfix_orient_apply(_p(tri), F, _p(fptr), _p(vptr), vptr.numel() - 1, _p(lab), _p(root), _p(parity), _p(root_open), _p(vol),
                                                  _p(cnt), _p(cnt1), _p(out), _p(flipped), _p(info), _stream()), "morig_meshfix_orient_apply")
        return out, flipped, info

    def meshfix_boundary_init(self, keys, vals, bflag, flipped, n_rows: int) -> tuple:
        """-> (hfrom, hto int32 [3 F]: the boundary half-edges after the flips, nxt, lab, vclass int32 [N]: the state in front of the doubling)"""
        n, F, N, dev = keys.numel(), flipped.numel(), int(n_rows), keys.device
        self._vec(torch.int64, n, keys)
        self._vec(torch.int32, n, vals, bflag)
        self._vec(torch.int32, F, flipped)
        hfrom, hto = self._new(dev, torch.int32, n), self._new(dev, torch.int32, n)
        outdeg, indeg, nxt, lab, vclass = (self._new(dev, torch.int32, N) for _ in range(5))
        check(self.lib.morig_meshfix_boundary_init(_p(keys), _p(vals), _p(bflag), n, _p(flipped), F, N, _p(hfrom), _p(hto), _p(outdeg), _p(indeg), _p(nxt),
                                                   _p(lab), _p(vclass), _stream()), "morig_meshfix_boundary_init")
        return hfrom, hto, nxt, lab, vclass

    def meshfix_loop_round(self, lab, nxt, lab2, nxt2) -> None:
        """one round of pointer doubling: lab2 = min(lab, lab[nxt]), nxt2 = nxt[nxt]; reads (lab, nxt), writes (lab2, nxt2)"""
        n = lab.numel()
        self._vec(torch.int32, n, lab, nxt, lab2, nxt2)
        assert n == 0 or (lab.data_ptr() != lab2.data_ptr() and nxt.data_ptr() != nxt2.data_ptr())
        check(self.lib.morig_meshfix_loop_round(_p(lab), _p(nxt), n, _p(lab2), _p(nxt2), _stream()), "morig_meshfix_loop_round")

    def meshfix_loop_centroid(self, verts, order, lptr, sel) -> torch.Tensor:
        """order int64 [N]: the rows sorted stably by loop label, lptr int64 [L + 1], sel int64 [S] loops -> float64 [S, 3]"""
        _need_gpu(verts)
        self._pts64(verts)
        N, L, S = verts.shape[0], lptr.numel() - 1, sel.numel()
        self._vec(torch.int64, N, order)
        self._vec(torch.int64, L + 1, lptr)
        self._vec(torch.int64, S, sel)
        out = self._new(verts.device, torch.float64, S, 3)
        check(self.lib.morig_meshfix_loop_centroid(_p(verts), N, _p(order), _p(lptr), L, _p(sel), S, _p(out), _stream()), "morig_meshfix_loop_centroid")
        return out

    def meshfix_fill_mark(self, vclass, lab, slot) -> torch.Tensor:
        """slot int32 [N]: the rank of a selected loop at its label, else -1 -> emit int32 [N]: the rows that begin a fan face"""
        n = vclass.numel()
        self._vec(torch.int32, n, vclass, lab, slot)
        emit = self._new(vclass.device, torch.int32, n)
        check(self.lib.morig_meshfix_fill_mark(_p(vclass), _p(lab), _p(slot), n, _p(emit), _stream()), "morig_meshfix_fill_mark")
        return emit

    def meshfix_fill_emit(self, nxt0, emit, erank, lab, slot, vptr, sptr, n_out: int) -> torch.Tensor:
        """-> int64 [n_out, 3]: per marked row v the face (nxt0[v], v, the loop's new vertex), local to the mesh, in ascending v"""
        n = nxt0.numel()
        self._vec(torch.int32, n, nxt0, emit, lab, slot)
        self._vec(torch.int64, n, erank)
        self._ptr32(vptr)
        self._vec(torch.int64, vptr.numel(), sptr)
        assert 0 <= n_out <= n
        out = self._new(nxt0.device, torch.int64, int(n_out), 3)
        check(self.lib.morig_meshfix_fill_emit(_p(nxt0), _p(emit), _p(erank), _p(lab), _p(slot), _p(vptr), _p(sptr), n, vptr.numel() - 1, int(n_out),
                                               _p(out), _stream()), "morig_meshfix_fill_emit")
        return out

    # -- mesh refinement (csrc/refine.hip; morig_amd/meshprep.py refine / interpolate) -----------------------------------------------------
    REFINE_IDLE, REFINE_LENGTH, REFINE_LONGEST = _K["MORIG_REFINE_IDLE"], _K["MORIG_REFINE_LENGTH"], _K["MORIG_REFINE_LONGEST"]

    def _faces32(self, faces, fptr, vptr):
        _need_gpu(faces)
        self._ptr32(fptr, vptr)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fptr.numel() == vptr.numel()
        return faces.shape[0], vptr.numel() - 1

    def refine_edge_records(self, verts, faces, fptr, vptr, status) -> tuple:
        """-> (keys int64 [3 F] = lo << 32 | hi, len2 float64 [3 F], maxbits int64 [B]: the bits of the largest finite len2 of every mesh,
        degenerate int32 [F]); face-major records, INT64_MAX at a face that is not followed"""
        _need_gpu(verts, status)
        self._pts64(verts)
        F, B = self._faces32(faces, fptr, vptr)
        assert status.dtype == torch.int32 and status.numel() >= 1
        dev = faces.device
        keys, len2 = self._new(dev, torch.int64, 3 * F), self._new(dev, torch.float64, 3 * F)
        maxbits, degenerate = self._new(dev, torch.int64, B), self._new(dev, torch.int32, F)
        check(self.lib.morig_refine_edge_records(_p(verts), verts.shape[0], _p(faces), F, _p(fptr), _p(vptr), B, _p(keys), _p(len2), _p(maxbits),
                                                 _p(degenerate), _p(status), _stream()), "morig_refine_edge_records")
        return keys, len2, maxbits, degenerate

    def refine_mark(self, keys, order, flags, len2, vptr, mode, limit2: float, maxbits) -> tuple:
        """keys sorted, order the record at every sorted position, flags the run starts, mode int32 [B] (REFINE_*) -> (mark int32 [n] at the
        run starts, image int64 [n]: the bits of a marked length, else -1)"""
        n = keys.numel()
        self._vec(torch.int64, n, keys, order)
        self._vec(torch.int32, n, flags)
        self._vec(torch.float64, n, len2)
        self._ptr32(vptr)
        B = vptr.numel() - 1
        self._vec(torch.int32, B, mode)
        self._vec(torch.int64, B, maxbits)
        mark, image = self._new(keys.device, torch.int32, n), self._new(keys.device, torch.int64, n)
        check(self.lib.morig_refine_mark(_p(keys), _p(order), _p(flags), _p(len2), n, _p(vptr), B, _p(mode), float(limit2), _p(maxbits), _p(mark),
                                         _p(image), _stream()), "morig_refine_mark")
        return mark, image

    def refine_budget(self, perm, rptr, budget, mark) -> None:
        """perm int64 [n]: the sorted positions by (mesh, image descending, position); clears mark behind budget int64 [B] per mesh, in place"""
        n, B = perm.numel(), budget.numel()
        self._vec(torch.int64, n, perm)
        self._vec(torch.int64, B + 1, rptr)
        self._vec(torch.int64, B, budget)
        self._vec(torch.int32, n, mark)
        check(self.lib.morig_refine_budget(_p(perm), n, _p(rptr), _p(budget), B, _p(mark), _stream()), "morig_refine_budget")

    def refine_number(self, keys, order, mark, erank, vptr, mptr) -> torch.Tensor:
        """-> edge_mid int32 [n] in record order: the new vertex of the record's edge, local to the mesh, or -1"""
        n = keys.numel()
        self._vec(torch.int64, n, keys, order, erank)
        self._vec(torch.int32, n, mark)
        self._ptr32(vptr)
        self._vec(torch.int64, vptr.numel(), mptr)
        edge_mid = self._new(keys.device, torch.int32, n)
        check(self.lib.morig_refine_number(_p(keys), _p(order), _p(mark), _p(erank), n, _p(vptr), _p(mptr), vptr.numel() - 1, _p(edge_mid), _stream()),
              "morig_refine_number")
        return edge_mid

    def refine_pattern(self, edge_mid, degenerate) -> tuple:
        """-> (nchild, pattern int32 [F]): the children of every face and its number of marked edges"""
        F = degenerate.numel()
        self._vec(torch.int32, 3 * F, edge_mid)
        self._vec(torch.int32, F, degenerate)
        nchild, pattern = self._new(edge_mid.device, torch.int32, F), self._new(edge_mid.device, torch.int32, F)
        check(self.lib.morig_refine_pattern(_p(edge_mid), _p(degenerate), F, _p(nchild), _p(pattern), _stream()), "morig_refine_pattern")
        return nchild, pattern

    def refine_emit(self, verts, parents, faces, face_map, edge_mid, crank, fptr, vptr, mptr, keys, mark, erank, n_out_rows: int, n_out_faces: int) -> tuple:
        """-> (verts float64 [n_out_rows, 3], parents int64 [n_out_rows, 2], faces int32 [n_out_faces, 3], face_map int64 [n_out_faces])"""
        _need_gpu(verts, parents, face_map)
        self._pts64(verts)
        F, B = self._faces32(faces, fptr, vptr)
        N, dev = verts.shape[0], verts.device
        assert parents.dtype == torch.int64 and tuple(parents.shape) == (N, 2) and parents.is_contiguous()
        self._vec(torch.int64, F, face_map, crank)
        self._vec(torch.int32, 3 * F, edge_mid, mark)
        self._vec(torch.int64, 3 * F, keys, erank)
        self._vec(torch.int64, B + 1, mptr)
        out_v, out_p = self._new(dev, torch.float64, int(n_out_rows), 3), self._new(dev, torch.int64, int(n_out_rows), 2)
        out_f, out_m = self._new(dev, torch.int32, int(n_out_faces), 3), self._new(dev, torch.int64, int(n_out_faces))
        check(self.lib.morig_refine_emit(_p(verts), _p(parents), N, _p(faces), _p(face_map), _p(edge_mid), _p(crank), F, _p(fptr), _p(vptr), _p(mptr), B,
                                         _p(keys), _p(mark), _p(erank), 3 * F, int(n_out_rows), int(n_out_faces), _p(out_v), _p(out_p), _p(out_f),
                                         _p(out_m), _stream()), "morig_refine_emit")
        return out_v, out_p, out_f, out_m

    def refine_interpolate(self, values, parents, row0: int, row1: int) -> None:
        """values float32 / float64 [V', C], in place: rows [row0, row1) = 0.5 * (values[p0] + values[p1]); both parents lie below row0"""
        _need_gpu(values, parents)
        assert values.dtype in (torch.float32, torch.float64) and values.dim() == 2 and values.is_contiguous()
        n = values.shape[0]
        assert parents.dtype == torch.int64 and tuple(parents.shape) == (n, 2) and parents.is_contiguous() and 0 <= row0 <= row1 <= n
        check(self.lib.morig_refine_interpolate(_p(values), values.element_size(), values.shape[1], _p(parents), int(row0), int(row1), n, _stream()),
              "morig_refine_interpolate")

    # -- the tolerance weld (csrc/proxweld.hip; morig_amd/meshprep.py diagnose / clean / repair with weld_tol) -----------------------------
    def proxweld_cell_keys(self, verts, nonfinite, rep, vptr, eps) -> tuple:
        """rep int32 [N] of the exact weld, eps float64 [B] -> (keys int64 [N]: the packed grid cell of every node -- a finite row that is
        its own representative --, INT64_MAX elsewhere; frame float64 [B, 4]: the low corner and the cell side of every mesh)"""
        _need_gpu(verts, eps)
        self._pts64(verts)
        n, dev = verts.shape[0], verts.device
        self._vec(torch.int32, n, nonfinite, rep)
        self._ptr32(vptr)
        B = vptr.numel() - 1
        self._vec(torch.float64, B, eps)
        box, frame, keys = self._new(dev, torch.int64, B, 6), self._new(dev, torch.float64, B, 4), self._new(dev, torch.int64, n)
        check(self.lib.morig_proxweld_cell_keys(_p(verts), _p(nonfinite), _p(rep), n, _p(vptr), B, _p(eps), _p(box), _p(frame), _p(keys), _stream()),
              "morig_proxweld_cell_keys")
        return keys, frame

    def _sorted_nodes(self, keys, order, pos, vptr, eps2):
        _need_gpu(pos)
        self._pts64(pos)
        n = pos.shape[0]
        self._vec(torch.int64, n, keys, order)
        self._ptr32(vptr)
        self._vec(torch.float64, vptr.numel() - 1, eps2)
        return n, vptr.numel() - 1

    def proxweld_count_links(self, keys, order, pos, vptr, eps2) -> torch.Tensor:
        """keys the cell keys sorted by (mesh, key, row), order int64 [N] the row and pos float64 [N, 3] the coordinates at every sorted
        position, eps2 float64 [B] -> count int32 [N]: the linked nodes with a higher row of every sorted position"""
        n, B = self._sorted_nodes(keys, order, pos, vptr, eps2)
        count = self._new(pos.device, torch.int32, n)
        check(self.lib.morig_proxweld_count_links(_p(keys), _p(order), _p(pos), n, _p(vptr), B, _p(eps2), _p(count), _stream()),
              "morig_proxweld_count_links")
        return count

    def proxweld_emit_links(self, keys, order, pos, vptr, eps2, count, lrank, n_links: int) -> torch.Tensor:
        """lrank int64 [N] the inclusive prefix sum of count -> links int64 [n_links]: row << 32 | other << 1 | 1, the keys ``meshcheck_cc_round`` reads"""
        n, B = self._sorted_nodes(keys, order, pos, vptr, eps2)
        self._vec(torch.int32, n, count)
        self._vec(torch.int64, n, lrank)
        assert n_links >= 0
        links = self._new(pos.device, torch.int64, int(n_links))
        check(self.lib.morig_proxweld_emit_links(_p(keys), _p(order), _p(pos), n, _p(vptr), B, _p(eps2), _p(count), _p(lrank), int(n_links), _p(links),
                                                 _stream()), "morig_proxweld_emit_links")
        return links

    def proxweld_spread(self, verts, rep, nonfinite, vptr) -> torch.Tensor:
        """rep int32 [N] the final representatives -> int64 [B]: the bits of the largest squared distance from a finite row to its representative"""
        _need_gpu(verts)
        self._pts64(verts)
        n = verts.shape[0]
        self._vec(torch.int32, n, rep, nonfinite)
        self._ptr32(vptr)
        maxbits = self._new(verts.device, torch.int64, vptr.numel() - 1)
        check(self.lib.morig_proxweld_spread(_p(verts), _p(rep), _p(nonfinite), n, _p(vptr), vptr.numel() - 1, _p(maxbits), _stream()),
              "morig_proxweld_spread")
        return maxbits

    # -- splitting non-manifold edges and pinched vertices (csrc/meshsplit.hip; morig_amd/meshprep.py split_nonmanifold) --------------------
    def meshsplit_links(self, keys, vals, order, n_faces: int) -> tuple:
        """keys / vals: the records sorted stably by key, order: the sort's permutation -> (links int64 [3 F]: the corner links in the
        component round's key layout, nm int32 [3 F]: 1 at the first record of a run of three or more)"""
        n = keys.numel()
        self._vec(torch.int64, n, keys, order)
        self._vec(torch.int32, n, vals)
        dev = keys.device
        links, nm = self._new(dev, torch.int64, n), self._new(dev, torch.int32, n)
        check(self.lib.morig_meshsplit_links(_p(keys), _p(vals), _p(order), n, int(n_faces), _p(links), _p(nm), _stream()), "morig_meshsplit_links")
        return links, nm

    def meshsplit_fans(self, lab, tri, n_rows: int) -> tuple:
        """lab int32 [3 F]: the converged corner labels -> (first int32 [N]: the lowest fan of every row, INT32_MAX where it has none,
        nfans int32 [N]: its fans)"""
        _need_gpu(tri)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.is_contiguous()
        F, dev = tri.shape[0], tri.device
        self._vec(torch.int32, 3 * F, lab)
        first, nfans = self._new(dev, torch.int32, int(n_rows)), self._new(dev, torch.int32, int(n_rows))
        check(self.lib.morig_meshsplit_fans(_p(lab), _p(tri), F, int(n_rows), _p(first), _p(nfans), _stream()), "morig_meshsplit_fans")
        return first, nfans

    def meshsplit_apply(self, lab, tri, first, rank, fptr, vptr, aptr, verts, n_out_rows: int) -> tuple:
        """rank int64 [3 F]: the inclusive prefix sum of the new-fan flags, aptr int64 [B + 1]: the new fans in front of every mesh ->
        (faces int64 [F, 3] local to their mesh, source int64 [n_out_rows] local to its mesh, verts float64 [n_out_rows, 3])"""
        _need_gpu(verts, tri)
        self._pts64(verts)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.is_contiguous()
        F, n, dev = tri.shape[0], verts.shape[0], verts.device
        self._ptr32(fptr, vptr)
        B = vptr.numel() - 1
        self._vec(torch.int32, 3 * F, lab)
        self._vec(torch.int32, n, first)
        self._vec(torch.int64, 3 * F, rank)
        self._vec(torch.int64, B + 1, aptr)
        assert fptr.numel() == B + 1 and n <= int(n_out_rows) <= n + 3 * F
        out_faces = self._new(dev, torch.int64, F, 3)
        source, out_verts = self._new(dev, torch.int64, int(n_out_rows)), self._new(dev, torch.float64, int(n_out_rows), 3)
        check(self.lib.morig_meshsplit_apply(_p(lab), _p(tri), _p(first), _p(rank), F, _p(fptr), _p(vptr), _p(aptr), B, _p(verts), n, int(n_out_rows),
                                             _p(out_faces), _p(source), _p(out_verts), _stream()), "morig_meshsplit_apply")
        return out_faces, source, out_verts

    # -- motion playback (csrc/playback.hip; morig_amd/playback.py holds the public functions) ------------------------------------------
    POSE_BAD_QUAT, POSE_BAD_INDEX, POSE_FRAME_TILE = _K["MORIG_POSE_BAD_QUAT"], _K["MORIG_POSE_BAD_INDEX"], _K["MORIG_POSE_FRAME_TILE"]

    @staticmethod
    def _f64(t, *shape):
        assert t.dtype == torch.float64 and tuple(t.shape) == shape and t.is_contiguous(), (t.dtype, tuple(t.shape), shape)

    def pose_validate(self, jptr, parent, order, vptr, eptr, ent_joint, status) -> None:
        """ORs POSE_BAD_INDEX into status int32 [B] for every mesh with a parent, order entry, entry offset or entry joint outside it;
        order and (vptr, eptr, ent_joint) may be None"""
        _need_gpu(jptr, parent, order, vptr, eptr, ent_joint, status)
        self._ptr32(jptr, status)
        B, nj = jptr.numel() - 1, parent.numel()
        assert parent.dtype == torch.int32 and parent.is_contiguous() and status.numel() == B
        assert order is None or (order.dtype == torch.int32 and order.numel() == nj and order.is_contiguous())
        rows = entries = 0
        if eptr is not None:
            self._ptr32(vptr, eptr)
            rows, entries = eptr.numel() - 1, ent_joint.numel()
            assert vptr.numel() == B + 1 and ent_joint.dtype == torch.int32 and ent_joint.is_contiguous()
        check(self.lib.morig_pose_validate(_p(jptr), _p(parent), _p(order), _p(vptr), _p(eptr), _p(ent_joint), B, nj, rows, entries, _p(status),
                                           _stream()), "morig_pose_validate")

    def pose_quats(self, quats, jptr, passes: int, align_signs: bool, status, matrices: bool = True) -> tuple:
        """quats float64 [NJ, T, 4] -> (aligned and smoothed copy [NJ, T, 4], R float64 [NJ, 9, T] or None); ORs POSE_BAD_QUAT into status"""
        _need_gpu(quats, jptr, status)
        self._ptr32(jptr, status)
        nj, T = quats.shape[0], quats.shape[1]
        self._f64(quats, nj, T, 4)
        out = torch.empty_like(quats)
        R = torch.empty(nj, 9, T, dtype=torch.float64, device=quats.device) if matrices else None
        check(self.lib.morig_pose_quats(_p(quats), _p(jptr), jptr.numel() - 1, nj, T, int(passes), int(bool(align_signs)), _p(out), _p(R),
                                        _p(status), _stream()), "morig_pose_quats")
        return out, R

    def pose_fk(self, R, jptr, parent, order, offsets, root_pos, pos_f32, status) -> torch.Tensor:
        """R [NJ, 9, T], offsets [NJ, 3], root_pos [B, T, 3], pos_f32 int32 [B] -> xf float64 [NJ, 12, T] (global matrix, position)"""
        _need_gpu(R, jptr, parent, order, offsets, root_pos, pos_f32, status)
        self._ptr32(jptr, status, pos_f32)
        nj, T, B = R.shape[0], R.shape[2], jptr.numel() - 1
        self._f64(R, nj, 9, T)
        self._f64(offsets, nj, 3)
        self._f64(root_pos, B, T, 3)
        assert parent.dtype == order.dtype == torch.int32 and parent.numel() == order.numel() == nj and parent.is_contiguous() and order.is_contiguous()
        assert pos_f32.numel() == status.numel() == B
        xf = torch.empty(nj, 12, T, dtype=torch.float64, device=R.device)
        check(self.lib.morig_pose_fk(_p(R), _p(jptr), _p(parent), _p(order), _p(offsets), _p(root_pos), _p(pos_f32), B, T, _p(status), _p(xf),
                                     _stream()), "morig_pose_fk")
        return xf

    def pose_local(self, bind, vtx, vptr, jptr, eptr, ent_joint, status) -> torch.Tensor:
        """bind [NJ, 12], vtx [N, 3] -> local float64 [E, 3]: inverse(bind[joint]) [v; 1] per entry"""
        _need_gpu(bind, vtx, vptr, jptr, eptr, ent_joint, status)
        self._ptr32(vptr, jptr, eptr, status)
        self._pts64(vtx)
        self._f64(bind, bind.shape[0], 12)
        n = vtx.shape[0]
        assert eptr.numel() == n + 1 and ent_joint.dtype == torch.int32 and ent_joint.is_contiguous()
        local = torch.empty(ent_joint.numel(), 3, dtype=torch.float64, device=vtx.device)
        check(self.lib.morig_pose_local(_p(bind), _p(vtx), _p(vptr), _p(jptr), _p(eptr), _p(ent_joint), vptr.numel() - 1, n, _p(status), _p(local),
                                        _stream()), "morig_pose_local")
        return local

    def pose_skin(self, xf, jptr, vptr, eptr, ent_joint, ent_weight, local, status) -> torch.Tensor:
        """-> float64 [N, T, 3]: per vertex row and frame the weighted sum of its entries' posed local coordinates"""
        _need_gpu(xf, jptr, vptr, eptr, ent_joint, ent_weight, local, status)
        self._ptr32(jptr, vptr, eptr, status)
        n, T, E = eptr.numel() - 1, xf.shape[2], ent_joint.numel()
        self._f64(xf, xf.shape[0], 12, T)
        self._f64(local, E, 3)
        self._f64(ent_weight, E)
        assert ent_joint.dtype == torch.int32 and ent_joint.is_contiguous()
        out = torch.empty(n, T, 3, dtype=torch.float64, device=xf.device)
        check(self.lib.morig_pose_skin(_p(xf), _p(jptr), _p(vptr), _p(eptr), _p(ent_joint), _p(ent_weight), _p(local), vptr.numel() - 1, n, T,
                                       _p(status), _p(out), _stream()), "morig_pose_skin")
        return out

    def pose_traj_errors(self, pred, gt, vis, vptr) -> tuple:
        """pred, gt float64 [N, T, 3], vis uint8 [N, T] -> (full, visible) float64 [B, T]"""
        _need_gpu(pred, gt, vis, vptr)
        self._ptr32(vptr)
        n, T, B = pred.shape[0], pred.shape[1], vptr.numel() - 1
        self._f64(pred, n, T, 3)
        self._f64(gt, n, T, 3)
        assert vis.dtype == torch.uint8 and tuple(vis.shape) == (n, T) and vis.is_contiguous()
        full = torch.empty(B, T, dtype=torch.float64, device=pred.device)
        visible = torch.empty(B, T, dtype=torch.float64, device=pred.device)
        check(self.lib.morig_pose_traj_errors(_p(pred), _p(gt), _p(vis), _p(vptr), B, T, _p(full), _p(visible), _stream()),
              "morig_pose_traj_errors")
        return full, visible

    # -- depth scans (csrc/scan.hip; morig_amd/scan.py holds the public functions) ------------------------------------------------------
    SCAN_MAX_SIDE, SCAN_ORTHOGRAPHIC, SCAN_PINHOLE = _K["MORIG_SCAN_MAX_SIDE"], _K["MORIG_SCAN_ORTHOGRAPHIC"], _K["MORIG_SCAN_PINHOLE"]
    SCAN_CAM_DOUBLES, SCAN_VIEW_INTS, SCAN_BAD_FACE = _K["MORIG_SCAN_CAM_DOUBLES"], _K["MORIG_SCAN_VIEW_INTS"], _K["MORIG_SCAN_BAD_FACE"]
    SCAN_BLOCK = 256                                                               # vertices / query rows per workgroup of blk_ptr

    def _scan_check(self, verts, vptr, faces, fptr, cams, views, kptr=None):
        """verts float64 [N, 3], vptr int32 [NV + 1], faces int32 [F, 3], fptr int32 [M + 1], cams float64 [NV, 16], views int32 [NV, 4],
        kptr int64 [NV + 1] -> (NV, M)"""
        _need_gpu(verts, vptr, faces, fptr, cams, views, kptr)
        self._pts64(verts)
        self._ptr32(vptr, fptr)
        nv, m = vptr.numel() - 1, fptr.numel() - 1
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert cams.dtype == torch.float64 and tuple(cams.shape) == (nv, self.SCAN_CAM_DOUBLES) and cams.is_contiguous()
        assert views.dtype == torch.int32 and tuple(views.shape) == (nv, self.SCAN_VIEW_INTS) and views.is_contiguous()
        assert kptr is None or (kptr.dtype == torch.int64 and kptr.numel() == nv + 1 and kptr.is_contiguous())
        return nv, m

    def scan_raster(self, verts, vptr, faces, fptr, mesh_nv, cams, views, kptr, wptr, min_side: int, max_side: int, n_pixels: int,
                    n_work: int) -> tuple:
        """-> (keys int64 [n_pixels] holding the uint64 key image, status int32 [1]); wptr int64 [NV + 1], mesh_nv int32 [M]"""
        nv, m = self._scan_check(verts, vptr, faces, fptr, cams, views, kptr)
        _need_gpu(mesh_nv, wptr)
        assert mesh_nv.dtype == torch.int32 and mesh_nv.numel() == m and wptr.dtype == torch.int64 and wptr.numel() == nv + 1
        ok = nv == 0 or (1 <= int(min_side) and int(max_side) <= self.SCAN_MAX_SIDE)      # a refused call allocates no result
        keys = torch.empty(int(n_pixels) if ok else 1, dtype=torch.int64, device=verts.device)
        status = torch.empty(1, dtype=torch.int32, device=verts.device)
        check(self.lib.morig_scan_raster(_p(verts), _p(vptr), _p(faces), faces.shape[0], _p(fptr), _p(mesh_nv), _p(cams), _p(views), _p(kptr),
                                         _p(wptr), nv, m, int(min_side), int(max_side), int(n_pixels), int(n_work), _p(keys), _p(status),
                                         _stream()), "morig_scan_raster")
        return keys, status

    def scan_resolve(self, verts, vptr, faces, fptr, cams, views, kptr, keys) -> tuple:
        """-> (depth float64 [NP], face int32 [NP], point float64 [NP, 3], flags int32 [NP])"""
        nv, m = self._scan_check(verts, vptr, faces, fptr, cams, views, kptr)
        _need_gpu(keys)
        assert keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
        n, dev = keys.numel(), verts.device
        depth, point = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, 3, dtype=torch.float64, device=dev)
        face, flags = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        check(self.lib.morig_scan_resolve(_p(verts), _p(vptr), _p(faces), _p(fptr), _p(cams), _p(views), _p(kptr), nv, m, n, _p(keys), _p(depth),
                                          _p(face), _p(point), _p(flags), _stream()), "morig_scan_resolve")
        return depth, face, point, flags

    def scan_compact(self, point, face, flags, rank, kptr, n_hits: int) -> tuple:
        """-> (pts float64 [n_hits, 3], pixel int32 [n_hits] inside the view, face int32 [n_hits]) in pixel order"""
        _need_gpu(point, face, flags, rank, kptr)
        self._pts64(point)
        n, dev = point.shape[0], point.device
        assert face.dtype == flags.dtype == torch.int32 and rank.dtype == kptr.dtype == torch.int64 and face.numel() == flags.numel() == rank.numel() == n
        assert face.is_contiguous() and flags.is_contiguous() and rank.is_contiguous() and kptr.is_contiguous() and 0 <= n_hits <= n
        pts = torch.empty(n_hits, 3, dtype=torch.float64, device=dev)
        pixel, hit_face = torch.empty(n_hits, dtype=torch.int32, device=dev), torch.empty(n_hits, dtype=torch.int32, device=dev)
        check(self.lib.morig_scan_compact(_p(point), _p(face), _p(flags), _p(rank), _p(kptr), kptr.numel() - 1, n, int(n_hits), _p(pts), _p(pixel),
                                          _p(hit_face), _stream()), "morig_scan_compact")
        return pts, pixel, hit_face

    def scan_visibility(self, verts, vptr, faces, fptr, cams, views, blk_ptr, n_blocks: int, vis_eps: float) -> torch.Tensor:
        """blk_ptr int32 [NV + 1]: the prefix sum of ceil(vertices / SCAN_BLOCK) per view -> uint8 [N]"""
        nv, m = self._scan_check(verts, vptr, faces, fptr, cams, views)
        self._ptr32(blk_ptr)
        assert blk_ptr.numel() == nv + 1
        vis = torch.empty(verts.shape[0], dtype=torch.uint8, device=verts.device)
        check(self.lib.morig_scan_visibility(_p(verts), _p(vptr), _p(faces), _p(fptr), _p(cams), _p(views), _p(blk_ptr), nv, m, int(n_blocks),
                                             float(vis_eps), _p(vis), _stream()), "morig_scan_visibility")
        return vis

    def scan_nearest(self, q, qptr, t, tptr, mask, blk_ptr, n_blocks: int) -> tuple:
        """q, t float64 [., 3] with their int32 prefix sums, mask uint8 per target row or None -> (idx int32 [NQ] local to the segment
        or -1, d2 float64 [NQ])"""
        _need_gpu(q, qptr, t, tptr, mask, blk_ptr)
        self._pts64(q)
        self._pts64(t)
        self._ptr32(qptr, tptr, blk_ptr)
        assert qptr.numel() == tptr.numel() == blk_ptr.numel()
        assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == t.shape[0] and mask.is_contiguous())
        idx = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        d2 = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
        check(self.lib.morig_scan_nearest(_p(q), _p(qptr), _p(t), _p(tptr), _p(mask), _p(blk_ptr), qptr.numel() - 1, int(n_blocks), _p(idx), _p(d2),
                                          _stream()), "morig_scan_nearest")
        return idx, d2

    # -- bone rays (csrc/labels.hip; morig_amd/labels.py holds the public functions) -----------------------------------------------------
    RAY_MAX_PER_JOINT, RAY_BAD_FACE, RAY_BAD_TABLE, RAY_STATS = (_K["MORIG_RAY_MAX_PER_JOINT"], _K["MORIG_RAY_BAD_FACE"],
                                                                  _K["MORIG_RAY_BAD_TABLE"], _K["MORIG_RAY_STATS"])
    RAY_BLOCK = 256                                                                # vertices per workgroup of ray_attention's blk_ptr

    def ray_cast(self, origins, dirs, ray_ptr, verts, vptr, faces, fptr, orientation: int) -> tuple:
        """origins, dirs float64 [R, 3], ray_ptr int32 [B + 1] -> (t float64 [R] (+inf), face int32 [R] (-1), point float64 [R, 3] (NaN),
        status int32 [1])"""
        B = self._mesh_check(verts, vptr, faces, fptr)
        _need_gpu(origins, dirs)
        self._pts64(origins)
        self._pts64(dirs)
        self._ptr32(ray_ptr)
        n, dev = origins.shape[0], origins.device
        assert dirs.shape[0] == n and ray_ptr.numel() == B + 1
        t, point = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, 3, dtype=torch.float64, device=dev)
        face, status = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        check(self.lib.morig_ray_cast(_p(origins), _p(dirs), _p(ray_ptr), n, _p(verts), _p(vptr), _p(faces), _p(fptr), B, int(orientation), _p(t),
                                      _p(face), _p(point), _p(status), _stream()), "morig_ray_cast")
        return t, face, point, status

    def ray_select(self, t, joint_ptr, max_rays: int, keep_factor: float, fill: float) -> tuple:
        """t float64 [R], joint_ptr int32 [J + 1] -> (kept uint8 [R], stats float64 [J, 4] = n_hit, n_kept, p20, featuresize)"""
        _need_gpu(t)
        self._ptr32(joint_ptr)
        assert t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous()
        J = joint_ptr.numel() - 1
        ok = int(max_rays) <= self.RAY_MAX_PER_JOINT                                   # a refused call allocates no result
        kept = torch.empty(t.numel() if ok else 1, dtype=torch.uint8, device=t.device)
        stats = torch.empty(J if ok else 1, self.RAY_STATS, dtype=torch.float64, device=t.device)
        check(self.lib.morig_ray_select(_p(t), _p(joint_ptr), J, int(max_rays), float(keep_factor), float(fill), _p(kept), _p(stats), _stream()),
              "morig_ray_select")
        return kept, stats

    def ray_attention(self, verts, vptr, blk_ptr, n_blocks: int, point, kept, ray_ptr, radius: float) -> torch.Tensor:
        """blk_ptr int32 [B + 1]: the prefix sum of ceil(vertices / RAY_BLOCK) per mesh; point float64 [R, 3], kept uint8 [R] -> float32 [N]"""
        B = self._mesh_check(verts, vptr)
        _need_gpu(point, kept)
        self._pts64(point)
        self._ptr32(blk_ptr, ray_ptr)
        assert blk_ptr.numel() == ray_ptr.numel() == B + 1
        assert kept.dtype == torch.uint8 and kept.numel() == point.shape[0] and kept.is_contiguous()
        attn = torch.empty(verts.shape[0], dtype=torch.float32, device=verts.device)
        check(self.lib.morig_ray_attention(_p(verts), _p(vptr), _p(blk_ptr), B, int(n_blocks), _p(point), _p(kept), _p(ray_ptr), float(radius),
                                           _p(attn), _stream()), "morig_ray_attention")
        return attn

    # -- rig transfer between meshes (csrc/transfer.hip; morig_amd/transfer.py holds the public functions) ---------------------------------
    TRANSFER_BLOCK, TRANSFER_MAX_FLOOD = _K["MORIG_TRANSFER_BLOCK"], _K["MORIG_TRANSFER_MAX_FLOOD"]
    TRANSFER_BAD_FACE, TRANSFER_BAD_COORD, TRANSFER_NO_FACES = (_K["MORIG_TRANSFER_BAD_FACE"], _K["MORIG_TRANSFER_BAD_COORD"],
                                                                 _K["MORIG_TRANSFER_NO_FACES"])

    @staticmethod
    def _status32(status):
        _need_gpu(status)
        assert status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous()

    def transfer_keys(self, faces, fptr, vptr, per_face: int, status) -> torch.Tensor:
        """faces int32 [F, 3] -> int64 [F * per_face] neighbour keys, unsorted (per_face 6: "faces", 15: "reference"); status int32
        [1 + B], zeroed by the caller"""
        _need_gpu(faces, fptr, vptr)
        self._ptr32(fptr, vptr)
        self._status32(status)
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous() and fptr.numel() == vptr.numel()
        assert status.numel() == vptr.numel()
        keys = torch.empty(faces.shape[0] * int(per_face), dtype=torch.int64, device=faces.device)
        check(self.lib.morig_transfer_keys(_p(faces), faces.shape[0], _p(fptr), _p(vptr), vptr.numel() - 1, int(per_face), _p(keys), _p(status),
                                           _stream()), "morig_transfer_keys")
        return keys

    def transfer_coincide(self, verts, vptr, blk_ptr, n_blocks: int, ori, optr, status) -> tuple:
        """-> (coincident int32 [N'], nearest int32 [N']) original vertex per remeshed vertex, -1: none"""
        B = self._mesh_check(verts, vptr)
        assert self._mesh_check(ori, optr) == B and blk_ptr.numel() == B + 1 and status.numel() == B + 1
        self._ptr32(blk_ptr)
        self._status32(status)
        coin = torch.empty(verts.shape[0], dtype=torch.int32, device=verts.device)
        near = torch.empty(verts.shape[0], dtype=torch.int32, device=verts.device)
        check(self.lib.morig_transfer_coincide(_p(verts), _p(vptr), _p(blk_ptr), B, int(n_blocks), _p(ori), _p(optr), _p(coin), _p(near),
                                               _p(status), _stream()), "morig_transfer_coincide")
        return coin, near

    def transfer_flood(self, verts, vptr, max_verts: int, rowptr, keys, coin, near, use_nearest: bool, status) -> tuple:
        """keys int64 sorted, rowptr int32 [N' + 1] -> (source int32 [N'], sweep int32 [N']); status[1 + b] += the vertices without a source"""
        B = self._mesh_check(verts, vptr)
        n = verts.shape[0]
        self._ptr32(rowptr)
        self._status32(status)
        _need_gpu(keys, coin, near)
        assert rowptr.numel() == n + 1 and status.numel() == B + 1 and keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
        assert coin.dtype == near.dtype == torch.int32 and coin.numel() == near.numel() == n and coin.is_contiguous() and near.is_contiguous()
        ok = int(max_verts) <= self.TRANSFER_MAX_FLOOD                                 # a refused call allocates no result
        source = torch.empty(n if ok else 1, dtype=torch.int32, device=verts.device)
        sweep = torch.empty(n if ok else 1, dtype=torch.int32, device=verts.device)
        check(self.lib.morig_transfer_flood(_p(verts), _p(vptr), B, int(max_verts), _p(rowptr), _p(keys), _p(coin), _p(near), int(bool(use_nearest)),
                                            _p(source), _p(sweep), _p(status), _stream()), "morig_transfer_flood")
        return source, sweep

    def transfer_closest(self, dst, dptr, blk_ptr, n_blocks: int, verts, vptr, faces, fptr, status) -> tuple:
        """-> (face int32 [N] (-1), bary float64 [N, 3] (NaN), distance float64 [N] (NaN)) per destination vertex"""
        B = self._mesh_check(verts, vptr, faces, fptr)
        assert self._mesh_check(dst, dptr) == B and blk_ptr.numel() == B + 1 and status.numel() >= 1
        self._ptr32(blk_ptr)
        self._status32(status)
        n, dev = dst.shape[0], dst.device
        face = torch.empty(n, dtype=torch.int32, device=dev)
        bary, dist = torch.empty(n, 3, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        check(self.lib.morig_transfer_closest(_p(dst), _p(dptr), _p(blk_ptr), B, int(n_blocks), _p(verts), _p(vptr), _p(faces), _p(fptr), _p(face),
                                              _p(bary), _p(dist), _p(status), _stream()), "morig_transfer_closest")
        return face, bary, dist

    def transfer_rows(self, skins, skin_ptr, joints, src_vptr, vptr, blk_ptr, n_blocks: int, pick, out_ptr, n_out: int, faces=None, fptr=None,
                      bary=None) -> torch.Tensor:
        """skins float64 flat, mesh b a row-major [V_src, joints[b]] block at skin_ptr[b] -> float64 [n_out] flat, mesh b a [V_dst, joints[b]]
        block at out_ptr[b]: the gathered row (pick = source) or, with faces / fptr / bary, the blend over the corners of face pick; then
        row / (ascending sum + 1e-8)"""
        _need_gpu(skins, pick, faces, bary)
        self._ptr32(skin_ptr, src_vptr, vptr, blk_ptr, out_ptr)
        B = vptr.numel() - 1
        assert skins.dtype == torch.float64 and skins.dim() == 1 and skins.is_contiguous()
        assert joints.dtype == torch.int32 and joints.numel() == B and joints.is_cuda and joints.is_contiguous()
        assert skin_ptr.numel() == src_vptr.numel() == blk_ptr.numel() == out_ptr.numel() == B + 1
        assert pick.dtype == torch.int32 and pick.dim() == 1 and pick.is_contiguous()
        if bary is not None:
            self._ptr32(fptr)
            assert bary.dtype == torch.float64 and bary.shape == (pick.numel(), 3) and bary.is_contiguous() and fptr.numel() == B + 1
            assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        out = torch.empty(int(n_out), dtype=torch.float64, device=pick.device)
        check(self.lib.morig_transfer_rows(_p(skins), _p(skin_ptr), _p(joints), _p(src_vptr), _p(faces if bary is not None else None),
                                           _p(fptr if bary is not None else None), _p(vptr), _p(blk_ptr), B, int(n_blocks), _p(pick), _p(bary), _p(out),
                                           _p(out_ptr), _stream()), "morig_transfer_rows")
        return out

    # -- local rigid motion (csrc/local_motion.hip; morig_amd/local_motion.py holds the public functions) -----------------------------------
    LOCAL_MAX_VERTS = _K["MORIG_LOCAL_MAX_VERTS"]
    LOCAL_BAD_FACE, LOCAL_BAD_COORD, LOCAL_BAD_ID = _K["MORIG_LOCAL_BAD_FACE"], _K["MORIG_LOCAL_BAD_COORD"], _K["MORIG_LOCAL_BAD_ID"]

    def local_patches(self, verts, vptr, max_verts: int, rowptr, keys, rungs, status, ptr=None, rung=None, n_ids: int = 0) -> tuple:
        """keys int64 sorted (transfer_keys with per_face 6), rowptr int32 [N + 1], rungs three floats, status int32 [3]. First pass (ptr
        None) -> (counts int32 [N], rung int32 [N]); second pass (ptr int32 [N + 1] the exclusive scan of counts, rung, n_ids = ptr[-1])
        -> ids int32 [n_ids], local to their mesh, ascending per vertex"""
        self._mesh_check(verts, vptr)
        n = verts.shape[0]
        self._ptr32(rowptr)
        self._status32(status)
        _need_gpu(keys)
        assert rowptr.numel() == n + 1 and status.numel() == 3 and keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
        r0, r1, r2 = (float(r) for r in rungs)
        ok = int(max_verts) <= self.LOCAL_MAX_VERTS                                    # a refused call allocates no result
        if ptr is None:
            counts = torch.empty(n if ok else 1, dtype=torch.int32, device=verts.device)
            rung = torch.empty(n if ok else 1, dtype=torch.int32, device=verts.device)
            ids = None
        else:
            self._ptr32(ptr)
            _need_gpu(rung)
            assert ptr.numel() == n + 1 and rung.dtype == torch.int32 and rung.numel() == n and rung.is_contiguous()
            counts, ids = ptr, torch.empty(max(int(n_ids), 1), dtype=torch.int32, device=verts.device)
        check(self.lib.morig_local_patches(_p(verts), _p(vptr), vptr.numel() - 1, n, int(max_verts), _p(rowptr), _p(keys), r0, r1, r2, _p(counts),
                                           _p(rung), _p(ids), _p(status), _stream()), "morig_local_patches")
        return (counts, rung) if ptr is None else ids[:int(n_ids)]

    def local_fit(self, verts0, traj, vptr, patch_ptr, ids, status) -> tuple:
        """verts0 float64 [N, 3], traj float64 or float32 [N, T, 3], patch_ptr int32 [N + 1], ids int32 [E] -> (rot6d float64 [N, T, 6],
        trans [N, T, 3], gap [N, T], residual [N, T]); status int32 [3]"""
        self._mesh_check(verts0, vptr)
        self._ptr32(patch_ptr)
        self._status32(status)
        _need_gpu(traj, ids)
        n = verts0.shape[0]
        assert traj.dtype in (torch.float64, torch.float32) and traj.dim() == 3 and traj.shape[0] == n and traj.shape[2] == 3 and traj.is_contiguous()
        assert patch_ptr.numel() == n + 1 and status.numel() == 3 and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()
        T, dev = int(traj.shape[1]), verts0.device
        rot6d, trans = torch.empty(n, T, 6, dtype=torch.float64, device=dev), torch.empty(n, T, 3, dtype=torch.float64, device=dev)
        gap, residual = torch.empty(n, T, dtype=torch.float64, device=dev), torch.empty(n, T, dtype=torch.float64, device=dev)
        check(self.lib.morig_local_fit(_p(verts0), _p(traj), int(traj.dtype == torch.float32), _p(vptr), vptr.numel() - 1, n, T, _p(patch_ptr),
                                       _p(ids) if ids.numel() else None, ids.numel(), _p(rot6d), _p(trans), _p(gap), _p(residual), _p(status),
                                       _stream()), "morig_local_fit")
        return rot6d, trans, gap, residual

    # -- mesh BVH (csrc/bvh.hip; morig_amd/spatial.py holds the public functions) ---------------------------------------------------------
    BVH_MAX_FACES, BVH_BAD_FACE, BVH_LEVELS = _K["MORIG_BVH_MAX_FACES"], _K["MORIG_BVH_BAD_FACE"], 4

    def bvh_build_keys(self, verts, vptr, faces, fptr, bbox) -> torch.Tensor:
        """bbox float64 [B, 6] of ``mesh_bbox`` -> int64 [F] = mesh << 30 | Morton code of the face's centroid, unsorted"""
        B = self._mesh_check(verts, vptr, faces, fptr)
        _need_gpu(bbox)
        assert bbox.dtype == torch.float64 and bbox.shape == (B, 6) and bbox.is_contiguous()
        keys = torch.empty(faces.shape[0], dtype=torch.int64, device=faces.device)
        check(self.lib.morig_bvh_build_keys(_p(verts), _p(vptr), _p(faces), faces.shape[0], _p(fptr), B, _p(bbox), _p(keys), _stream()),
              "morig_bvh_build_keys")
        return keys

    def _bvh_check(self, verts, vptr, faces, fptr, order, node_ptr) -> int:
        B = self._mesh_check(verts, vptr, faces, fptr)
        _need_gpu(order, node_ptr)
        assert order.dtype == torch.int32 and order.dim() == 1 and order.numel() == faces.shape[0] and order.is_contiguous()
        assert node_ptr.dtype == torch.int32 and node_ptr.shape == (self.BVH_LEVELS, B + 1) and node_ptr.is_contiguous()
        return B

    def bvh_boxes(self, verts, vptr, faces, fptr, order, node_ptr, level_nodes, max_faces: int) -> tuple:
        """order int32 [F]: the face row at every sorted position; node_ptr int32 [4, B + 1]; level_nodes: the four node totals ->
        (boxes float64 [sum(level_nodes), 6], flags int32 [B])"""
        B = self._bvh_check(verts, vptr, faces, fptr, order, node_ptr)
        n = [int(x) for x in level_nodes]
        assert len(n) == self.BVH_LEVELS
        ok = int(max_faces) <= self.BVH_MAX_FACES                                      # a refused call allocates no result
        boxes = torch.empty(sum(n) if ok else 1, 6, dtype=torch.float64, device=verts.device)
        flags = torch.empty(max(B, 1), dtype=torch.int32, device=verts.device)
        check(self.lib.morig_bvh_boxes(_p(verts), _p(vptr), _p(faces), _p(fptr), B, int(max_faces), _p(order), _p(node_ptr), n[0], n[1], n[2], n[3],
                                       _p(boxes), _p(flags), _stream()), "morig_bvh_boxes")
        return boxes, flags[:B]

    def bvh_ray_cast(self, origins, dirs, ray_ptr, verts, vptr, faces, fptr, order, boxes, node_ptr, flags, orientation: int,
                     want_visits: bool = False) -> tuple:
        """``ray_cast`` through the tree -> (t, face, point, status, visits int32 [R] or None)"""
        B = self._bvh_check(verts, vptr, faces, fptr, order, node_ptr)
        _need_gpu(origins, dirs, boxes, flags)
        self._pts64(origins)
        self._pts64(dirs)
        self._ptr32(ray_ptr)
        n, dev = origins.shape[0], origins.device
        assert dirs.shape[0] == n and ray_ptr.numel() == B + 1 and flags.dtype == torch.int32 and flags.numel() == B
        assert boxes.dtype == torch.float64 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous()
        t, point = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, 3, dtype=torch.float64, device=dev)
        face, status = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        visits = torch.empty(n, dtype=torch.int32, device=dev) if want_visits else None
        check(self.lib.morig_bvh_ray_cast(_p(origins), _p(dirs), _p(ray_ptr), n, _p(verts), _p(vptr), _p(faces), _p(fptr), B, _p(order), _p(boxes),
                                          _p(node_ptr), _p(flags), int(orientation), _p(t), _p(face), _p(point), _p(visits), _p(status), _stream()),
              "morig_bvh_ray_cast")
        return t, face, point, status, visits

    def bvh_blocked(self, a, b, seg_ptr, skip_vertex, t_max, verts, vptr, faces, fptr, order, boxes, node_ptr, flags,
                    want_visits: bool = False) -> tuple:
        """a, b float64 [S, 3], seg_ptr int32 [B + 1], skip_vertex int32 [S] or None, t_max float64 [S] or None -> (blocked uint8 [S],
        status int32 [1], visits int32 [S] or None)"""
        B = self._bvh_check(verts, vptr, faces, fptr, order, node_ptr)
        _need_gpu(a, b, boxes, flags, skip_vertex, t_max)
        self._pts64(a)
        self._pts64(b)
        self._ptr32(seg_ptr)
        n, dev = a.shape[0], a.device
        assert b.shape[0] == n and seg_ptr.numel() == B + 1 and flags.dtype == torch.int32 and flags.numel() == B
        assert boxes.dtype == torch.float64 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous()
        assert skip_vertex is None or (skip_vertex.dtype == torch.int32 and skip_vertex.shape == (n,) and skip_vertex.is_contiguous())
        assert t_max is None or (t_max.dtype == torch.float64 and t_max.shape == (n,) and t_max.is_contiguous())
        blocked, status = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        visits = torch.empty(n, dtype=torch.int32, device=dev) if want_visits else None
        check(self.lib.morig_bvh_blocked(_p(a), _p(b), _p(seg_ptr), n, _p(skip_vertex), _p(t_max), _p(verts), _p(vptr), _p(faces), _p(fptr), B,
                                         _p(order), _p(boxes), _p(node_ptr), _p(flags), _p(blocked), _p(visits), _p(status), _stream()),
              "morig_bvh_blocked")
        return blocked, status, visits

    def bvh_closest(self, points, pptr, verts, vptr, faces, fptr, order, boxes, node_ptr, flags, status, want_visits: bool = False) -> tuple:
        """``transfer_closest`` through the tree -> (face, bary, distance, visits int32 [N] or None); status zeroed by the caller"""
        B = self._bvh_check(verts, vptr, faces, fptr, order, node_ptr)
        assert self._mesh_check(points, pptr) == B and flags.dtype == torch.int32 and flags.numel() == B
        _need_gpu(boxes, flags)
        self._status32(status)
        assert boxes.dtype == torch.float64 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous()
        n, dev = points.shape[0], points.device
        face = torch.empty(n, dtype=torch.int32, device=dev)
        bary, dist = torch.empty(n, 3, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        visits = torch.empty(n, dtype=torch.int32, device=dev) if want_visits else None
        check(self.lib.morig_bvh_closest(_p(points), _p(pptr), n, _p(verts), _p(vptr), _p(faces), _p(fptr), B, _p(order), _p(boxes), _p(node_ptr),
                                         _p(flags), _p(face), _p(bary), _p(dist), _p(visits), _p(status), _stream()), "morig_bvh_closest")
        return face, bary, dist, visits

    def _bvh_tree_check(self, n: int, order, boxes, node_ptr, flags, n_faces: int) -> None:
        _need_gpu(order, boxes, node_ptr, flags)
        assert order.dtype == torch.int32 and order.dim() == 1 and order.numel() == n_faces and order.is_contiguous()
        assert node_ptr.dtype == torch.int32 and node_ptr.shape == (self.BVH_LEVELS, n + 1) and node_ptr.is_contiguous()
        assert boxes.dtype == torch.float64 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous()
        assert flags.dtype == torch.int32 and flags.numel() == n and flags.is_contiguous()

    def bvh_view_boxes(self, verts, vptr, view_mesh, faces, fptr, order, node_ptr, level_nodes, max_faces: int) -> tuple:
        """the boxes of one tree per view: verts float64 [N, 3] and vptr int32 [NV + 1] of the views, view_mesh int32 [NV], faces / fptr
        and order int32 [F] of the meshes, node_ptr int32 [4, NV + 1] -> (boxes float64 [sum(level_nodes), 6], flags int32 [NV])"""
        _need_gpu(verts, vptr, view_mesh, faces, fptr, order, node_ptr)
        self._pts64(verts)
        self._ptr32(vptr, fptr)
        nv, m = vptr.numel() - 1, fptr.numel() - 1
        assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and faces.is_contiguous()
        assert view_mesh.dtype == torch.int32 and view_mesh.shape == (nv,) and view_mesh.is_contiguous()
        assert order.dtype == torch.int32 and order.dim() == 1 and order.numel() == faces.shape[0] and order.is_contiguous()
        assert node_ptr.dtype == torch.int32 and node_ptr.shape == (self.BVH_LEVELS, nv + 1) and node_ptr.is_contiguous()
        n = [int(x) for x in level_nodes]
        assert len(n) == self.BVH_LEVELS
        ok = int(max_faces) <= self.BVH_MAX_FACES                                      # a refused call allocates no result
        boxes = torch.empty(sum(n) if ok else 1, 6, dtype=torch.float64, device=verts.device)
        flags = torch.empty(max(nv, 1), dtype=torch.int32, device=verts.device)
        check(self.lib.morig_bvh_view_boxes(_p(verts), _p(vptr), _p(view_mesh), nv, _p(faces), _p(fptr), m, int(max_faces), _p(order), _p(node_ptr),
                                            n[0], n[1], n[2], n[3], _p(boxes), _p(flags), _stream()), "morig_bvh_view_boxes")
        return boxes, flags[:nv]

    def bvh_scan_visibility(self, verts, vptr, faces, fptr, cams, views, vis_eps: float, order, boxes, node_ptr, flags,
                            want_visits: bool = False) -> tuple:
        """``scan_visibility`` through the view trees -> (vis uint8 [N], status int32 [1], visits int32 [N] or None)"""
        nv, m = self._scan_check(verts, vptr, faces, fptr, cams, views)
        self._bvh_tree_check(nv, order, boxes, node_ptr, flags, faces.shape[0])
        n, dev = verts.shape[0], verts.device
        vis, status = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        visits = torch.empty(n, dtype=torch.int32, device=dev) if want_visits else None
        check(self.lib.morig_bvh_scan_visibility(_p(verts), _p(vptr), _p(faces), _p(fptr), _p(cams), _p(views), nv, m, n, float(vis_eps), _p(order),
                                                 _p(boxes), _p(node_ptr), _p(flags), _p(vis), _p(visits), _p(status), _stream()),
              "morig_bvh_scan_visibility")
        return vis, status, visits

    def bvh_bone_visibility(self, pos, vtx_ptr, bones, bone_ptr, tri_pos, tp_ptr, faces, f_ptr, off, n_pairs: int, order, boxes, node_ptr, flags,
                            want_visits: bool = False) -> tuple:
        """``bone_visibility`` through the occluders' tree -> (vis uint8 [n_pairs], status int32 [1], visits int32 [n_pairs] or None)"""
        _need_gpu(pos, vtx_ptr, bones, bone_ptr, off)
        self._pts64(pos)
        B = self._mesh_check(tri_pos, tp_ptr, faces, f_ptr)
        self._ptr32(vtx_ptr, bone_ptr)
        self._bvh_tree_check(B, order, boxes, node_ptr, flags, faces.shape[0])
        assert bones.dtype == torch.float64 and bones.dim() == 2 and bones.shape[1] == 6 and bones.is_contiguous()
        assert vtx_ptr.numel() == bone_ptr.numel() == B + 1 and off.dtype == torch.int64 and off.numel() == B + 1 and off.is_contiguous()
        dev = pos.device
        vis, status = torch.empty(int(n_pairs), dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        visits = torch.empty(int(n_pairs), dtype=torch.int32, device=dev) if want_visits else None
        check(self.lib.morig_bvh_bone_visibility(_p(pos), _p(vtx_ptr), _p(bones), _p(bone_ptr), _p(tri_pos), _p(tp_ptr), _p(faces), _p(f_ptr), _p(off),
                                                 B, int(n_pairs), _p(order), _p(boxes), _p(node_ptr), _p(flags), _p(vis), _p(visits), _p(status),
                                                 _stream()), "morig_bvh_bone_visibility")
        return vis, status, visits

    def knn_bandwidth(self, pts: torch.Tensor, k: int) -> torch.Tensor:
        """device tensor [1] float64: mean distance to the k-th nearest neighbour (self included)."""
        _need_gpu(pts)
        self._pts64(pts)
        n = pts.shape[0]
        ws = torch.empty(n, dtype=torch.float64, device=pts.device)
        bw = torch.empty(1, dtype=torch.float64, device=pts.device)
        check(self.lib.morig_knn_bandwidth(_p(pts), n, k, _p(ws), _p(bw), _stream()), "morig_knn_bandwidth")
        return bw

    def meanshift(self, pts: torch.Tensor, weights: Optional[torch.Tensor], bandwidth: torch.Tensor, max_iter: int) -> torch.Tensor:
        _need_gpu(pts, bandwidth)
        self._pts64(pts)
        n = pts.shape[0]
        if weights is not None:
            assert weights.dtype == torch.float32 and weights.numel() == n and weights.is_contiguous()
        a, b = torch.empty_like(pts), torch.empty_like(pts)
        state = torch.empty(max(max_iter, 1), dtype=torch.float64, device=pts.device)
        in_a = C.c_int32(0)
        check(self.lib.morig_meanshift(_p(pts), _p(weights), n, _p(bandwidth), max_iter, _p(a), _p(b), _p(state), C.byref(in_a),
                                       _stream()), "morig_meanshift")
        return a if in_a.value else b

    def nms_counts(self, pts: torch.Tensor, bandwidth: torch.Tensor) -> torch.Tensor:
        _need_gpu(pts, bandwidth)
        self._pts64(pts)
        counts = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
        check(self.lib.morig_nms_counts(_p(pts), pts.shape[0], _p(bandwidth), _p(counts), _stream()), "morig_nms_counts")
        return counts

    def nms_greedy(self, pts: torch.Tensor, attn: torch.Tensor, bandwidth: torch.Tensor, order: torch.Tensor, thrd_density: float,
                   thrd_attn: float) -> torch.Tensor:
        _need_gpu(pts, attn, bandwidth, order)
        self._pts64(pts)
        n = pts.shape[0]
        assert attn.dtype == torch.float32 and attn.numel() == n and order.dtype == torch.int32 and order.numel() == n
        alive = torch.empty(n, dtype=torch.uint8, device=pts.device)
        check(self.lib.morig_nms_greedy(_p(pts), _p(attn), n, _p(bandwidth), _p(order), float(thrd_density), float(thrd_attn),
                                        _p(alive), _stream()), "morig_nms_greedy")
        return alive.bool()

    # -- the same stages over the point sets of several meshes (ptr: int32 [B + 1] row offsets on the device) ----------------
    def knn_bandwidth_batched(self, pts: torch.Tensor, ptr: torch.Tensor, max_n: int, quantile: float) -> torch.Tensor:
        _need_gpu(pts, ptr)
        self._pts64(pts)
        B = ptr.numel() - 1
        ws = torch.empty(pts.shape[0], dtype=torch.float64, device=pts.device)
        bw = torch.empty(B, dtype=torch.float64, device=pts.device)
        check(self.lib.morig_knn_bandwidth_batched(_p(pts), _p(ptr), B, pts.shape[0], max_n, float(quantile), _p(ws), _p(bw), _stream()),
              "morig_knn_bandwidth_batched")
        return bw

    def meanshift_batched(self, pts: torch.Tensor, weights: Optional[torch.Tensor], ptr: torch.Tensor, max_n: int,
                          bandwidth: torch.Tensor, max_iter: int) -> torch.Tensor:
        _need_gpu(pts, ptr, bandwidth)
        self._pts64(pts)
        B, n = ptr.numel() - 1, pts.shape[0]
        if weights is not None:
            assert weights.dtype == torch.float32 and weights.numel() == n and weights.is_contiguous()
        a, b = torch.empty_like(pts), torch.empty_like(pts)
        state = torch.empty(max(max_iter, 1) * B, dtype=torch.float64, device=pts.device)
        in_a = C.c_int32(0)
        check(self.lib.morig_meanshift_batched(_p(pts), _p(weights), _p(ptr), B, n, max_n, _p(bandwidth), max_iter, _p(a), _p(b),
                                               _p(state), C.byref(in_a), _stream()), "morig_meanshift_batched")
        return a if in_a.value else b

    def meanshift_batched_sorted(self, pts: torch.Tensor, weights: Optional[torch.Tensor], ptr: torch.Tensor, max_n: int,
                                 bandwidth: torch.Tensor, max_iter: int, with_counts: bool = False):
        """meanshift_batched on Morton-sorted points with bounding-box culling of source boxes (csrc/joints.hip); the result is
        returned in the caller's point order. Same sums up to the order of the additions (skipped pairs contribute exactly 0).
        with_counts: also the neighbour counts of the modes within the bandwidth (nms_counts_batched's integers), taken in the sorted
        order with the same culling -> (modes, counts)."""
        _need_gpu(pts, ptr, bandwidth)
        self._pts64(pts)
        B, n = ptr.numel() - 1, pts.shape[0]
        keys = torch.empty(n, dtype=torch.int64, device=pts.device)
        check(self.lib.morig_morton_keys(_p(pts), _p(ptr), B, n, _p(keys), _stream()), "morig_morton_keys")
        perm = torch.argsort(keys, stable=True)       # mirrored points on the x = 0 plane share a Morton key: a stable order keeps the fp64 summation order, and with it the modes' last bits, the same from run to run
        ps = pts[perm].contiguous()
        ws = None if weights is None else weights[perm].contiguous()
        a, b = torch.empty_like(ps), torch.empty_like(ps)
        state = torch.empty(max(max_iter, 1) * B, dtype=torch.float64, device=pts.device)
        bbox = torch.empty(2 * B * ((max_n + 31) // 32) * 6, dtype=torch.float64, device=pts.device)
        in_a = C.c_int32(0)
        check(self.lib.morig_meanshift_sorted(_p(ps), _p(ws), _p(ptr), B, n, max_n, _p(bandwidth), max_iter, _p(a), _p(b), _p(state),
                                              _p(bbox), C.byref(in_a), _stream()), "morig_meanshift_sorted")
        modes_sorted = a if in_a.value else b
        out = torch.empty_like(pts)
        out[perm] = modes_sorted
        if not with_counts:
            return out
        cs = torch.empty(n, dtype=torch.int32, device=pts.device)
        check(self.lib.morig_nms_counts_sorted(_p(modes_sorted), _p(ptr), B, n, max_n, _p(bandwidth), _p(bbox), _p(cs), _stream()),
              "morig_nms_counts_sorted")
        counts = torch.empty_like(cs)
        counts[perm] = cs
        return out, counts

    def nms_counts_batched(self, pts: torch.Tensor, ptr: torch.Tensor, max_n: int, bandwidth: torch.Tensor) -> torch.Tensor:
        _need_gpu(pts, ptr, bandwidth)
        self._pts64(pts)
        counts = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
        check(self.lib.morig_nms_counts_batched(_p(pts), _p(ptr), ptr.numel() - 1, pts.shape[0], max_n, _p(bandwidth), _p(counts),
                                                _stream()), "morig_nms_counts_batched")
        return counts

    def nms_greedy_batched(self, pts: torch.Tensor, attn: torch.Tensor, ptr: torch.Tensor, bandwidth: torch.Tensor,
                           order_local: torch.Tensor, thrd_density: float, thrd_attn: float) -> torch.Tensor:
        _need_gpu(pts, attn, ptr, bandwidth, order_local)
        self._pts64(pts)
        n = pts.shape[0]
        assert attn.dtype == torch.float32 and attn.numel() == n and order_local.dtype == torch.int32 and order_local.numel() == n
        alive = torch.empty(n, dtype=torch.uint8, device=pts.device)
        check(self.lib.morig_nms_greedy_batched(_p(pts), _p(attn), _p(ptr), ptr.numel() - 1, n, _p(bandwidth), _p(order_local),
                                                float(thrd_density), float(thrd_attn), _p(alive), _stream()), "morig_nms_greedy_batched")
        return alive.bool()

    def gather_rows(self, src: Mat, idx: torch.Tensor, dst: Mat):
        _need_gpu(src.base, idx, dst.base)
        assert idx.dtype == torch.int32 and dst.rows == idx.numel() and dst.cols == src.cols
        check(self.lib.morig_gather_rows(src.ptr, src.ld, _p(idx), idx.numel(), src.cols, dst.ptr, dst.ld, _stream()),
              "morig_gather_rows")

    # -- small ops ------------------------------------------------------------------------------------
    def copy2d(self, src: Mat, dst: Mat):
        _need_gpu(src.base, dst.base)
        assert src.rows == dst.rows and src.cols == dst.cols
        check(self.lib.morig_copy2d(src.ptr, src.ld, dst.ptr, dst.ld, src.rows, src.cols, _stream()), "morig_copy2d")

    def copy2d_pad(self, src: Mat, dst: Mat, split: bool = False):
        """dst window (wider than src) = [src | zeros]; split: written in the split-fp16 activation layout."""
        _need_gpu(src.base, dst.base)
        assert src.rows == dst.rows and dst.cols >= src.cols
        if split and not self.fast:
            raise MorigNativeError("split-fp16 activations requested on the fp32 path (plan bug)")
        check(self.lib.morig_copy2d_pad(src.ptr, src.ld, src.rows, src.cols, dst.ptr, dst.ld, dst.cols, int(split),
                                        _p(self._flag(src.base.device)), _stream()), "morig_copy2d_pad")

    def copy2d_rep(self, src: Mat, dst: Mat, replicas: int, dst_row_step: int, src_col_step: int = 0, split: bool = False):
        """`replicas` copies in one launch: copy r = [src window shifted r * src_col_step columns | zeros] into the dst
        window shifted r * dst_row_step rows (dst describes replica 0)."""
        _need_gpu(src.base, dst.base)
        assert src.rows == dst.rows and dst.cols >= src.cols and replicas >= 1
        assert dst.row0 + dst.rows + (replicas - 1) * dst_row_step <= dst.base.shape[0]
        assert src.col0 + src.cols + (replicas - 1) * src_col_step <= src.base.shape[1]
        if split and not self.fast:
            raise MorigNativeError("split-fp16 activations requested on the fp32 path (plan bug)")
        check(self.lib.morig_copy2d_pad_rep(src.ptr, src.ld, src.rows, src.cols, src_col_step, dst.ptr, dst.ld, dst.cols, replicas,
                                            dst_row_step, int(split), _p(self._flag(src.base.device)), _stream()), "morig_copy2d_pad_rep")

    def gather_cols(self, src: Mat, cols: torch.Tensor, dst: Mat):
        _need_gpu(src.base, cols, dst.base)
        assert cols.dtype == torch.int32 and dst.cols == cols.numel() and src.rows == dst.rows
        check(self.lib.morig_gather_cols(src.ptr, src.ld, _p(cols), cols.numel(), dst.ptr, dst.ld, src.rows, _stream()),
              "morig_gather_cols")

    def make_seg(self, batch: torch.Tensor, n_graphs: int, replicas: int) -> torch.Tensor:
        _need_gpu(batch)
        b = batch if (batch.dtype == torch.int64 and batch.is_contiguous()) else batch.long().contiguous()
        n = b.numel()
        seg = torch.empty(n * replicas, dtype=torch.int32, device=b.device)
        check(self.lib.morig_make_seg(_p(b), n, n_graphs, replicas, _p(seg), _stream()), "morig_make_seg")
        return seg

    def rownorm(self, x: Mat, rows_per_rep: int, replicas: int, y: torch.Tensor, ld_row: int, ld_rep: int):
        _need_gpu(x.base, y)
        assert x.rows == rows_per_rep * replicas
        check(self.lib.morig_rownorm(x.ptr, x.ld, rows_per_rep, replicas, x.cols, _p(y), ld_row, ld_rep, _stream()),
              "morig_rownorm")

    def cls_attention(self, x: torch.Tensor, g: torch.Tensor, cls: torch.Tensor, y: Mat):
        _need_gpu(x, g, cls, y.base)
        n, T, Cc = x.shape
        assert x.is_contiguous() and g.is_contiguous() and cls.is_contiguous()
        heads = g.shape[0]
        check(self.lib.morig_cls_attention(_p(x), n, T, Cc, heads, _p(g), _p(cls), y.ptr, y.ld, _stream()),
              "morig_cls_attention")

    def frame_reduce(self, x: torch.Tensor, mode: str, y: Mat):
        _need_gpu(x, y.base)
        n, T, Cc = x.shape
        assert x.is_contiguous()
        check(self.lib.morig_frame_reduce(_p(x), n, T, Cc, 0 if mode == "mean" else 1, y.ptr, y.ld, _stream()),
              "morig_frame_reduce")


_ops: Optional[NativeOps] = None


def get_ops() -> NativeOps:
    """The process-wide op layer. Raises (loudly) when the HIP library or a GPU is missing."""
    global _ops
    if _ops is None:
        _ops = NativeOps()
    return _ops


# ---------------------------------------------------------------------------------------------
# profiling helpers for bench.py
# ---------------------------------------------------------------------------------------------
def prof_enable(on: bool) -> None:
    load_library().morig_prof_enable(1 if on else 0)


def prof_reset() -> None:
    load_library().morig_prof_reset()


def prof_collect():
    """-> {kernel name: dict(launches, ms, flops, bytes)} for kinds that ran."""
    lib = load_library()
    out = {}
    k = 0
    while True:
        nm = lib.morig_prof_name(k)
        if nm is None:
            break
        n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        check(lib.morig_prof_collect(k, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "morig_prof_collect")
        if n.value:
            sym = lib.morig_prof_symbol(k)
            out[nm.decode()] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value,
                                    symbol=sym.decode() if sym else None)
        k += 1
    return out


def device_info():
    lib = load_library()
    cu, lds, clk = C.c_int(), C.c_int(), C.c_int()
    arch = C.create_string_buffer(64)
    st = lib.morig_device_info(C.byref(cu), C.byref(lds), C.byref(clk), arch, 64)
    return dict(status=st, cu_count=cu.value, lds_bytes_per_cu=lds.value, clock_khz=clk.value, arch=arch.value.decode())
