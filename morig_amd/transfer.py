"""Rig transfer between meshes of the same shape: moving a rig's skin weights from one mesh to another, on the device (csrc/transfer.hip,
csrc/pointtri_core.h).

    transfer_to_remesh   the reference's ``transfer_rig_to_remesh`` (data_proc/common_ops.py:229-259) for a ragged batch: an artist's rig
                         on the original mesh -> the remeshed mesh the networks train on
    transfer_skins       per destination vertex the skin rows of the closest source triangle, blended by the barycentrics of the closest
                         point: a rig made on a simplified mesh -> the asset it was simplified from
    transfer_rigs        ``transfer_skins`` wrapped into ``formats.Rig`` objects

``transfer_to_remesh`` follows the reference, quirks included. (1) Coincidence: a remeshed vertex takes the row of the LOWEST original
vertex o with (dx^2 + dy^2) + dz^2 == 0 in float64 (np.argmin of a distance row whose minimum is 0): differences that underflow count,
-0.0 equals 0.0. (2) Flood: sweeps until every vertex is filled; a sweep visits the vertices unfilled at its start in ascending index, a
vertex filled earlier in the same sweep counts as filled; a visited vertex with a filled neighbour copies the row of the filled neighbour
at the smallest correctly rounded root distance, strict ``<`` from 1e8 over the ascending neighbours (ties, also of roots whose squares
differ, go to the lowest index). (3) The neighbours of v under ``neighbours="reference"`` are what ``faces[np.argwhere(faces == v)]``
yields: the vertices of the faces that contain v AND, for every corner position c in {0, 1, 2} at which v stands, the vertices of face
NUMBER c (argwhere's column is used as a row index too), minus v; a mesh without a face c adds nothing there (the reference raises
IndexError). ``neighbours="faces"`` is this product's own option: the faces that contain v only, what ``find_tpl_neighbors`` computes.
(4) skins = skins_ori[source] / (row sum + 1e-8), the sum in ascending joint order (numpy adds pairwise: equal up to 2 J 2^-53 relative).
Where the reference hangs or misbehaves, this refuses: a vertex no sweep reaches (in no face, or in a component without a coincident
vertex: the reference's ``while`` never ends) raises ``TransferError`` naming the mesh, or under ``unreachable="nearest"``, this
product's own option, takes the original vertex at the smallest squared distance (lowest index); coordinates that are no finite numbers
of magnitude <= 1e7 (above, the 1e8 start can leave ``closest_nn = -1``, which copies the LAST vertex's row) and face indices outside
the mesh raise ValueError. The flood runs in one workgroup per mesh with its state in LDS: at most ``MAX_FLOOD_VERTS`` = 8 192 remeshed
vertices per mesh.

``transfer_skins`` IS THIS PRODUCT'S OWN RULE: no parity with any DCC tool's weight transfer exists or is claimed, and nobody has measured
what it does to deformation quality. Per destination vertex: the closest point of every source triangle by Ericson's seven regions
(pointtri_core.h: comparisons decide the region, divisions give the barycentrics only, every dot product (x + y) + z); the winner has
the smallest squared distance, then the lowest face; row[j] = (b0 S[f0][j] + b1 S[f1][j]) + b2 S[f2][j], then row / (ascending row sum +
1e-8). A zero-area triangle falls into its vertex and edge regions by the same comparisons. A mesh without faces gives face -1, NaN
barycentrics and distance, zero rows (``transfer_skins``; ``transfer_rigs`` raises). Brute force over all faces by default;
``accel="bvh"`` finds the same face through the mesh BVH of ``spatial``, which is what a source of hundreds of
thousands of faces needs.

Everything is float64 in a fixed order without floating-point atomics: two runs give the same bits, a mesh alone the bits it gives in a
batch. Host reads: ONE status read per call, and ``Rig.skins`` being a host array, one copy of the skin block where rigs are returned.
"""
from __future__ import annotations

import copy
from typing import List, Sequence

import numpy as np
import torch

from .meshbatch import MeshBatch, bad_face, vertex_adjacency
from .ragged import int32_table, ptr_of
from .runtime import get_ops

MAX_FLOOD_VERTS = 8192           # MORIG_TRANSFER_MAX_FLOOD of include/morig_hip.h
COORD_LIMIT = 1e7


class TransferError(RuntimeError):
    """a remeshed vertex that no sweep of the flood can reach"""


class _Skins:
    """the skin matrices of a call, flat on the device: mesh b a row-major [rows[b], J_b] block at ptr[b]"""

    def __init__(self, what: str, skins: Sequence, rows: np.ndarray, dst_rows: np.ndarray, device):
        mats = []
        for b, s in enumerate(skins):
            s = s.detach() if isinstance(s, torch.Tensor) else torch.as_tensor(np.asarray(s, dtype=np.float64))
            if s.numel() == 0 and s.dim() != 2:
                s = s.reshape(int(rows[b]), 0)
            if s.dim() != 2 or s.shape[0] != rows[b]:
                raise ValueError(f"{what}: mesh {b}: skins are [V, J] with one row per source vertex ({int(rows[b])})")
            mats.append(s.to(device=device, dtype=torch.float64))
        self.J = np.array([m.shape[1] for m in mats], dtype=np.int64)
        self.ptr_host, self.out_ptr_host = ptr_of(rows * self.J), ptr_of(dst_rows * self.J)
        self.flat = torch.cat([m.reshape(-1) for m in mats]).contiguous() if mats else torch.zeros(0, dtype=torch.float64, device=device)
        self.ptr, self.out_ptr = int32_table(self.ptr_host, device, what), int32_table(self.out_ptr_host, device, what)
        self.joints = int32_table(self.J, device, what)

    def split(self, out: torch.Tensor, dst_rows: np.ndarray) -> List[torch.Tensor]:
        return [out[self.out_ptr_host[b]:self.out_ptr_host[b + 1]].reshape(int(dst_rows[b]), int(self.J[b])) for b in range(len(self.J))]


def _with_skins(rig, skins_host: np.ndarray, skins_dev: torch.Tensor):
    out = copy.copy(rig)
    for k, v in vars(rig).items():
        if k not in ("skins", "skins_device", "skin_entries_device"):
            setattr(out, k, copy.deepcopy(v))
    out.skins, out.skins_device = skins_host, skins_dev
    if hasattr(out, "skin_entries_device"):
        del out.skin_entries_device                                                 # entries of the OLD skins
    return out


def transfer_to_remesh(verts_ori: Sequence, verts_remesh: Sequence, faces_remesh: Sequence, rigs: Sequence, neighbours: str = "reference",
                       unreachable: str = "raise", return_info: bool = False) -> List[tuple]:
    """``transfer_rig_to_remesh(mesh_ori, mesh_remesh, rig_ori)`` for a list of meshes: ``verts_ori[b]`` [V, 3], ``verts_remesh[b]``
    [V', 3], ``faces_remesh[b]`` integer [F, 3], ``rigs[b]`` a ``formats.Rig`` (anything with ``skins`` [V, J]) on the original mesh.
    -> per mesh (rig, source_vertex): a copy of the rig with ``skins`` float64 [V', J] replaced (``skins_device`` the same on the device),
    joints and hierarchy unchanged; source_vertex int64 [V'] on the device, the original vertex whose row every remeshed vertex received.
    ``return_info`` appends a dict(sweep int32 [V']: 0 coincident, k filled in the reference's k-th sweep; coincident, nearest int32 [V']).
    The rule, the two options and the refusals: the module docstring. At most 8 192 remeshed vertices per mesh."""
    what = "transfer_to_remesh"
    if neighbours not in ("reference", "faces"):
        raise ValueError(f'{what}: neighbours is "reference" or "faces"')
    if unreachable not in ("raise", "nearest"):
        raise ValueError(f'{what}: unreachable is "raise" or "nearest"')
    rigs = list(rigs)
    mesh = MeshBatch(what, verts_remesh, faces_remesh, like=tuple(verts_ori))
    ori = MeshBatch(what, verts_ori, like=(mesh.verts,))
    if ori.n != mesh.n or len(rigs) != mesh.n:
        raise ValueError(f"{what}: one original mesh, one remeshed mesh and one rig per entry")
    if mesh.n == 0:
        return []
    most = int(mesh.nv.max())
    if most > MAX_FLOOD_VERTS:
        raise ValueError(f"{what}: mesh {int(mesh.nv.argmax())} has {most} remeshed vertices: the flood supports at most {MAX_FLOOD_VERTS} per mesh")
    dev, ops = mesh.device, get_ops()
    skins = _Skins(what, [r.skins for r in rigs], ori.nv, mesh.nv, dev)
    status = torch.zeros(mesh.n + 1, dtype=torch.int32, device=dev)
    keys, rowptr = vertex_adjacency(ops, mesh, 15 if neighbours == "reference" else 6, status)
    blk, n_blk = mesh.blocks(ops.TRANSFER_BLOCK)
    coin, near = ops.transfer_coincide(mesh.verts, mesh.vptr, blk, n_blk, ori.verts, ori.vptr, status)
    source, sweep = ops.transfer_flood(mesh.verts, mesh.vptr, most, rowptr, keys, coin, near, unreachable == "nearest", status)
    out = ops.transfer_rows(skins.flat, skins.ptr, skins.joints, ori.vptr, mesh.vptr, blk, n_blk, source, skins.out_ptr, int(skins.out_ptr_host[-1]))
    host = status.cpu().numpy()                                                                         # the status read
    if host[0] & ops.TRANSFER_BAD_FACE:
        raise bad_face(what)
    if host[0] & ops.TRANSFER_BAD_COORD:
        raise ValueError(f"{what}: a coordinate is no finite number of magnitude <= {COORD_LIMIT:g}")
    lost = np.nonzero(host[1:])[0]
    if len(lost):
        b = int(lost[0])
        why = "the mesh has no original vertex" if ori.nv[b] == 0 else "they share no face with a filled vertex, directly or through others"
        raise TransferError(f"{what}: mesh {b}: {int(host[1 + b])} of {int(mesh.nv[b])} remeshed vertices can never be filled ({why}); the "
                            'reference loops forever here. unreachable="nearest" gives them the nearest original vertex')
    host_skins = out.cpu().numpy()                                                                      # Rig.skins is a host array
    res = []
    for b, (rig, dev_skins) in enumerate(zip(rigs, skins.split(out, mesh.nv))):
        hs = host_skins[skins.out_ptr_host[b]:skins.out_ptr_host[b + 1]].reshape(int(mesh.nv[b]), int(skins.J[b]))
        vs = slice(mesh.vptr_host[b], mesh.vptr_host[b + 1])
        item = (_with_skins(rig, hs, dev_skins), source[vs].long())
        res.append(item + (dict(sweep=sweep[vs], coincident=coin[vs], nearest=near[vs]),) if return_info else item)
    return res


def _closest(what: str, src_verts, src_faces, src_skins, dst_verts, accel=None):
    if accel not in (None, "bvh"):
        raise ValueError(f'{what}: accel is None or "bvh"')
    src = MeshBatch(what, src_verts, src_faces, like=tuple(dst_verts))
    dst = MeshBatch(what, dst_verts, like=(src.verts,))
    src_skins = list(src_skins)
    if dst.n != src.n or len(src_skins) != src.n:
        raise ValueError(f"{what}: one source mesh, one skin matrix and one destination per entry")
    if src.n == 0:
        return src, dst, None, None
    dev, ops = src.device, get_ops()
    skins = _Skins(what, src_skins, src.nv, dst.nv, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    blk, n_blk = dst.blocks(ops.TRANSFER_BLOCK)
    if accel == "bvh":
        from . import spatial
        face, bary, dist, _ = spatial._closest(ops, spatial.MeshBVH(src, what), dst, status)
    else:
        face, bary, dist = ops.transfer_closest(dst.verts, dst.vptr, blk, n_blk, src.verts, src.vptr, src.faces, src.fptr, status)
    out = ops.transfer_rows(skins.flat, skins.ptr, skins.joints, src.vptr, dst.vptr, blk, n_blk, face, skins.out_ptr, int(skins.out_ptr_host[-1]),
                            faces=src.faces, fptr=src.fptr, bary=bary)
    word = int(status.cpu()[0])                                                                         # the status read
    if word & ops.TRANSFER_BAD_FACE:
        raise bad_face(what)
    return src, dst, skins, (out, face, bary, dist, word)


def transfer_skins(src_verts: Sequence, src_faces: Sequence, src_skins: Sequence, dst_verts: Sequence, accel=None) -> List[tuple]:
    """Skin rows carried from a source surface to arbitrary points by the closest surface point, this product's own rule (module
    docstring). ``src_verts[b]`` [V, 3], ``src_faces[b]`` integer [F, 3], ``src_skins[b]`` [V, J], ``dst_verts[b]`` [V_dst, 3].
    -> per mesh (skins float64 [V_dst, J], face int32 [V_dst], bary float64 [V_dst, 3], distance float64 [V_dst]) on the device: the
    winning source face, the barycentrics of the closest point on it and its distance. A source without faces gives face -1, NaN
    barycentrics and distance and zero rows. One thread per destination vertex over all faces of its mesh; ``accel="bvh"`` builds the
    source's BVH and walks it, one wave per destination vertex, for the same results. Host reads: one status word."""
    src, dst, skins, res = _closest("transfer_skins", src_verts, src_faces, src_skins, dst_verts, accel)
    if res is None:
        return []
    out, face, bary, dist, _ = res
    return [(s, face[dst.vptr_host[b]:dst.vptr_host[b + 1]], bary[dst.vptr_host[b]:dst.vptr_host[b + 1]], dist[dst.vptr_host[b]:dst.vptr_host[b + 1]])
            for b, s in enumerate(skins.split(out, dst.nv))]


def transfer_rigs(rigs: Sequence, src_meshes: Sequence, dst_verts: Sequence, accel=None) -> List:
    """``transfer_skins`` for rigs: ``rigs[b]`` with ``skins`` [V, J] on the mesh ``src_meshes[b]`` = (verts, faces) -> a copy of every
    rig whose ``skins`` float64 [V_dst, J] (host; ``skins_device`` on the device) belong to ``dst_verts[b]``, joints and hierarchy
    unchanged: what ``playback.skin_trajectory``, ``scan`` and ``Rig.save`` take for the destination mesh. A source without faces and a
    destination with vertices is a ValueError: a rig of zero rows would pose nothing. ``accel``: as in ``transfer_skins``."""
    rigs, src_meshes = list(rigs), list(src_meshes)
    if len(src_meshes) != len(rigs):
        raise ValueError("transfer_rigs: one (verts, faces) pair per rig")
    src, dst, skins, res = _closest("transfer_rigs", [m[0] for m in src_meshes], [m[1] for m in src_meshes], [r.skins for r in rigs], dst_verts,
                                   accel)
    if res is None:
        return []
    out, _, _, _, word = res
    if word & get_ops().TRANSFER_NO_FACES:
        raise ValueError("transfer_rigs: a source mesh without faces")
    host = out.cpu().numpy()                                                                            # Rig.skins is a host array
    return [_with_skins(rig, host[skins.out_ptr_host[b]:skins.out_ptr_host[b + 1]].reshape(int(dst.nv[b]), int(skins.J[b])), s)
            for b, (rig, s) in enumerate(zip(rigs, skins.split(out, dst.nv)))]
