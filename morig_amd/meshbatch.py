"""The meshes of a call as one ragged batch: ``verts`` float64 [N, 3] and ``faces`` int32 [F, 3] local to their
mesh, concatenated and delimited by ``vptr`` / ``fptr``; every stage that takes a list of meshes packs it here, and lays its workgroups
out over the meshes by ``blocks`` with its own block constant. Host reads: none, but ONE in ``MeshBatch(check_faces="host")``.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from . import ragged
from .ragged import as_tensor, device_of, int32_table, ptr_of


def bad_face(what: str) -> ValueError:
    return ValueError(f"{what}: a face names a vertex outside its mesh")


def pack_faces(what: str, faces: Sequence, device):
    """``faces[b]`` integer [F_b, 3] -> (faces int32 [F, 3] on ``device``, nf int64 ndarray, fptr_host, fptr). Values are clamped to the
    int32 limits before they are narrowed, so an index out of range stays out of range."""
    fs = [as_tensor(f) for f in faces]
    if any(f.dim() != 2 or f.shape[1] != 3 or f.is_floating_point() for f in fs):
        raise ValueError(f"{what}: faces are integer [F, 3] per mesh")
    nf = np.array([f.shape[0] for f in fs], dtype=np.int64)
    fptr_host = ptr_of(nf)
    fptr = int32_table(fptr_host, device, what)
    big = torch.iinfo(torch.int32)
    packed = (torch.cat([f.to(device=device, dtype=torch.int64) for f in fs], 0).clamp(big.min, big.max).to(torch.int32).contiguous() if fs
              else torch.zeros(0, 3, dtype=torch.int32, device=device))
    return packed, nf, fptr_host, fptr


class MeshBatch:
    """``what``, ``n``, ``device`` (that of the first CUDA tensor among verts, faces and ``like``), ``nv`` / ``nf`` int64 ndarrays,
    ``vptr_host`` / ``fptr_host`` and ``vptr`` / ``fptr`` as int32 on the device, ``verts`` (None when only ``n_verts`` is given) and
    ``faces`` (None when not given). ``check_faces``: "device" reads nothing back, the stage's kernel clamps and flags an index outside
    its mesh; "host" checks here with one read and raises ``bad_face`` before anything is launched."""

    def __init__(self, what: str, verts=None, faces=None, n_verts=None, like=(), check_faces: str = "device"):
        verts, faces = (None if x is None else list(x) for x in (verts, faces))
        self.what, self.n = what, len(verts if verts is not None else faces)
        self.device = dev = device_of(*(verts or []), *(faces or []), *like)
        self.verts = self.faces = None
        if verts is not None:
            vs = [as_tensor(v) for v in verts]
            if any(v.dim() != 2 or v.shape[1] != 3 for v in vs):
                raise ValueError(f"{what}: verts are [V, 3] per mesh")
            n_verts = [v.shape[0] for v in vs]
            self.verts = (torch.cat([v.to(device=dev, dtype=torch.float64) for v in vs], 0).contiguous() if vs
                          else torch.zeros(0, 3, dtype=torch.float64, device=dev))
        self.nv = np.array([int(n) for n in n_verts], dtype=np.int64)
        if len(self.nv) != self.n or (self.nv < 0).any():
            raise ValueError(f"{what}: one vertex count per mesh")
        self.vptr_host = ptr_of(self.nv)
        self.vptr = int32_table(self.vptr_host, dev, what)
        if faces is not None:
            if len(faces) != self.n:
                raise ValueError(f"{what}: one faces array per mesh")
            self.faces, self.nf, self.fptr_host, self.fptr = pack_faces(what, faces, dev)
            if check_faces == "host" and self.faces.numel():
                limit = torch.repeat_interleave(int32_table(self.nv, dev, what), torch.from_numpy(self.nf).to(dev))
                if bool(((self.faces < 0) | (self.faces >= limit[:, None])).any()):                # the index check: one host read
                    raise bad_face(what)

    def blocks(self, block: int) -> tuple:
        return ragged.blocks(self.nv, block, self.device, self.what)

    def split_v(self, t: torch.Tensor) -> List[torch.Tensor]:
        return [t[self.vptr_host[b]:self.vptr_host[b + 1]] for b in range(self.n)]

    def take(self, ids: Sequence[int], what: str) -> "MeshBatch":
        """the meshes ``ids`` of a batch with vertices and faces as a batch of their own (nothing is checked again or read back)"""
        sub = object.__new__(MeshBatch)
        sub.what, sub.n, sub.device = what, len(ids), self.device
        sub.nv, sub.nf = self.nv[list(ids)], self.nf[list(ids)]
        sub.vptr_host, sub.fptr_host = ptr_of(sub.nv), ptr_of(sub.nf)
        sub.vptr, sub.fptr = int32_table(sub.vptr_host, self.device, what), int32_table(sub.fptr_host, self.device, what)
        sub.verts = torch.cat([self.verts[self.vptr_host[b]:self.vptr_host[b + 1]] for b in ids], 0).contiguous()
        sub.faces = torch.cat([self.faces[self.fptr_host[b]:self.fptr_host[b + 1]] for b in ids], 0).contiguous()
        return sub


def vertex_adjacency(ops, mesh: MeshBatch, per_face: int, status: torch.Tensor):
    """The directed (vertex, neighbour) keys of ``transfer_keys`` -> (keys int64 sorted, rowptr int32 [N + 1]: global vertex v has
    keys[rowptr[v]:rowptr[v + 1]], their low 32 bits its neighbours). ``status``: int32 [n + 1], word 0 takes the bad-face bit. No host read."""
    keys = torch.sort(ops.transfer_keys(mesh.faces, mesh.fptr, mesh.vptr, per_face, status)).values.contiguous()
    rows = torch.arange(int(mesh.vptr_host[-1]) + 1, dtype=torch.int64, device=mesh.device) << 32
    return keys, torch.searchsorted(keys, rows).to(torch.int32).contiguous()
