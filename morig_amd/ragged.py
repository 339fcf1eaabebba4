"""The host side of a ragged batch: meshes concatenated row-wise and delimited by a prefix sum ``ptr`` [B + 1]
that ascends from 0. What every staged module needs around its kernels -- the prefix sum, the device a call runs on, the int32 upload
with its range check, the validation of a caller's ``ptr``, the workgroup table ``blk_ptr`` -- stated once. The device side is
``segment_of`` and ``block_row`` in csrc/ragged_core.h; the packing of a list of meshes is morig_amd/meshbatch.py.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import runtime


def ptr_of(counts) -> np.ndarray:
    """the prefix sum of ``counts`` [B] -> int64 [B + 1], starting at 0"""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)


def device_of(*items, device=None) -> torch.device:
    """The device a call runs on: an explicit ``device``; else that of the first CUDA tensor among ``items``; else ``cpu`` when the test
    seam ``runtime._test_ops`` is installed; else the current CUDA device."""
    if device is not None:
        return torch.device(device)
    for t in items:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if runtime._test_ops is not None:
        return torch.device("cpu")
    return torch.device("cuda", torch.cuda.current_device())


def int32_table(values, device, what: str) -> torch.Tensor:
    """``values`` as an int32 tensor on ``device``. The kernels index with int32: a value of 2^31 or more raises ValueError naming
    ``what`` instead of wrapping."""
    a = np.asarray(values, dtype=np.int64)
    if a.size and a.max() >= 2 ** 31:
        raise ValueError(f"{what}: more than 2^31 - 1 rows or entries in one call")
    return torch.from_numpy(a.astype(np.int32)).to(device)


def blocks(counts, block: int, device, what: str) -> tuple:
    """The workgroup table of a kernel that gives segment b ceil(counts[b] / block) workgroups of ``block`` rows -> (blk_ptr int32
    [B + 1] on ``device``, the number of workgroups). ``block`` is the kernel's own constant; ``block_row`` (csrc/ragged_core.h) reads it."""
    host = ptr_of((np.asarray(counts, dtype=np.int64) + block - 1) // block)
    return int32_table(host, device, what), int(host[-1])


def check_ptr(ptr, n: int, what: str) -> np.ndarray:
    """A caller's ``ptr`` (anything numpy reads) -> int64 [B + 1], or ValueError naming ``what``: an integer vector of at least two
    entries that starts at 0, ends at ``n`` and never descends."""
    p = np.asarray(ptr)
    if p.ndim != 1 or p.size < 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"{what} is an integer array [B + 1] with B >= 1")
    p = p.astype(np.int64)
    if p[0] != 0 or p[-1] != n or np.any(np.diff(p) < 0):
        raise ValueError(f"{what} must ascend from 0 to the number of rows ({n})")
    return p


def as_tensor(a) -> torch.Tensor:
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


def cat_to(items: Sequence, device, dtype=None) -> torch.Tensor:
    """the items (tensors or arrays) moved to ``device`` (and ``dtype``) and concatenated along their rows"""
    ts = [as_tensor(a) for a in items]
    ts = [t.to(device=device, dtype=dtype) if dtype is not None else t.to(device) for t in ts]
    return torch.cat(ts, 0).contiguous()


def n_slots(device) -> int:
    """the number of compute units: how many persistent workgroups the job-queue kernels start"""
    return torch.cuda.get_device_properties(device).multi_processor_count
