"""Local rigid motion of a deforming mesh: per vertex a small surface patch, and per (vertex, frame) the rotation and translation that
carry the patch from the rest pose to the frame, on the device (csrc/local_motion.hip, csrc/localfit_core.h).

    patches              the reference's ``nnids`` (``get_gt_rotation_icp`` with ``nnids=None``, data_proc/common_ops.py:47-65, and
                         ``find_tpl_neighbors``, :35-44) for a ragged batch
    local_rigid_motion   the reference's ``icp`` (:155-172) on every patch for every frame of a clip, with the conditioning of every fit
                         and its root-mean-square residual, which are this product's own outputs
    gt_rotation_icp      the single-mesh drop-in with the reference's signature shape
    rotation_matrices    6-D representation -> 3 x 3 matrices, in plain torch

``patches`` follows the reference rule by rule. (1) One-ring: the vertices that share a face with v, v removed. (2) Ring growth: two
rounds of "the union of my members' lists". That is the set of end points of the walks of exactly four edges from v, and that is what
the kernel computes; on a mesh whose every edge lies in a proper triangle it equals breadth-first depth <= 4 with v itself included; on
the edge of a degenerate face (a, a, b) that lies in no other face it does not (a's list is {a}), and the walks are what the reference
yields. (3) Distance: float64 sqrt((d0^2 + d1^2) + d2^2) without fused multiply-add, the correctly rounded root, compared by strict
``<``: a candidate at a distance that rounds to the radius is out. (4) Threshold ladder: the radius 0.04; while fewer than 5 candidates
pass, times 1.25, and the loop breaks only AFTER a multiplication passes 0.06 -- so the rungs are ``RUNGS`` = 0.04, 0.04 * 1.25 and
0.04 * 1.25 * 1.25 (float64, computed that way on the host), the first rung with >= 5 candidates is used, and otherwise the third, which
exceeds 0.06, with however few candidates it has. (5) Order: members in ascending index.
Where the reference fails, this does not: a vertex in no face (the reference raises inside ``np.concatenate``) has the patch {v}, rung
2, and is counted in ``Patches.n_isolated``; coordinates that are no finite numbers and face indices outside the mesh raise ValueError;
so does a mesh of more than ``MAX_VERTS`` = 32 768 vertices (two bitsets of the mesh per wave live in LDS).

``local_rigid_motion``: per (vertex, frame) centre both sides by their means (ascending patch order), M = tar_c^T src_c, R the proper
rotation that maximises trace(R^T M) -- Horn's quaternion form (csrc/kabsch_core.h), which is the reference's ``U Vh`` with its
determinant rule wherever that is unique -- and t = mean(tar) - R mean(src). A patch of one point gives the identity exactly and
t = q - p. Patches of rank <= 1 (collinear or coincident points) have no unique answer: one maximiser is returned, not necessarily the
reference's, and ``gap`` = 0 says so. An empty patch (only ``Patches.from_lists`` can make one) gives NaN and is counted.

Everything is float64 in a fixed order without floating-point atomics: two runs give the same bits, a mesh alone the bits it gives in a
batch. There is no CPU fallback. Host reads: ONE per ``patches`` call (the status words and the entry total that sizes ``ids``) and ONE
status read per ``local_rigid_motion`` call; ``Patches.split`` copies the patches to the host when asked.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from .meshbatch import MeshBatch, bad_face, vertex_adjacency
from .ragged import as_tensor, device_of, int32_table, ptr_of
from .runtime import get_ops

MAX_VERTS = 32768                                    # MORIG_LOCAL_MAX_VERTS of include/morig_hip.h
MIN_CANDIDATES = 5
RUNGS = (0.04, 0.04 * 1.25, 0.04 * 1.25 * 1.25)      # thd = 0.04; thd *= 1.25; thd *= 1.25 -- in float64, as the reference's loop does


class Patches:
    """The patches of a ragged batch on the device. ``ptr`` int32 [N + 1] over all vertices of the call, ``ids`` int32 [ptr[-1]] the
    members of every patch, local to their mesh, ascending; ``rung`` int32 [N] the rung of the ladder every vertex used (0 / 1 / 2; -1
    for a caller's own lists); ``vptr_host`` int64 [B + 1] the mesh offsets; ``n_isolated`` the vertices in no face, ``n_empty`` the
    empty rows of a caller's lists."""

    def __init__(self, ptr: torch.Tensor, ids: torch.Tensor, rung: torch.Tensor, vptr_host: np.ndarray, n_isolated: int = 0, n_empty: int = 0):
        self.ptr, self.ids, self.rung, self.vptr_host = ptr, ids, rung, np.asarray(vptr_host, dtype=np.int64)
        self.n_isolated, self.n_empty = int(n_isolated), int(n_empty)

    @property
    def n(self) -> int:
        return len(self.vptr_host) - 1

    @property
    def nv(self) -> np.ndarray:
        return np.diff(self.vptr_host)

    @property
    def device(self):
        return self.ptr.device

    def split(self) -> List[List[np.ndarray]]:
        """per mesh the list the reference returns: one int64 array of ascending vertex indices per vertex (one host copy)"""
        ptr, ids = self.ptr.cpu().numpy().astype(np.int64), self.ids.cpu().numpy().astype(np.int64)
        return [[ids[ptr[v]:ptr[v + 1]] for v in range(self.vptr_host[b], self.vptr_host[b + 1])] for b in range(self.n)]

    @classmethod
    def from_lists(cls, lists: Sequence, device=None) -> "Patches":
        """A caller's own ``nnids``: ``lists[b]`` holds one integer sequence per vertex of mesh b, in the order the fit shall walk it (the
        reference accepts any). An index outside the mesh is a ValueError; an empty row is allowed, gives NaN fits and is counted."""
        lists = [list(rows) for rows in lists]
        dev = device_of(device=device)
        rows, nv = [], []
        for b, mesh_rows in enumerate(lists):
            nv.append(len(mesh_rows))
            for v, row in enumerate(mesh_rows):
                r = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row)
                if r.size and (r.ndim != 1 or not np.issubdtype(r.dtype, np.integer)):
                    raise ValueError(f"Patches.from_lists: mesh {b}, vertex {v}: a patch is a vector of integers")
                r = r.reshape(-1).astype(np.int64)
                if r.size and (r.min() < 0 or r.max() >= len(mesh_rows)):
                    raise ValueError(f"Patches.from_lists: mesh {b}, vertex {v}: a patch names a vertex outside its mesh")
                rows.append(r)
        counts = np.array([len(r) for r in rows], dtype=np.int64)
        ptr_host = ptr_of(counts)
        ids = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        what = "Patches.from_lists"
        return cls(int32_table(ptr_host, dev, what), int32_table(ids, dev, what), torch.full((len(rows),), -1, dtype=torch.int32, device=dev),
                   ptr_of(nv), 0, int((counts == 0).sum()))


class LocalMotion:
    """``rot6d`` float64 [N, T, 6] the first then the second COLUMN of R, ``trans`` [N, T, 3], ``gap`` [N, T] = (l1 - l2) / l1 of Horn's
    matrix = 2 (s2 + d s3) / (s1 + s2 + d s3) (the conditioning of the fit: the error of R is about machine epsilon / gap; 0: no unique
    answer), ``residual`` [N, T] the root-mean-square of |R p + t - q| over the patch (the rigidity score), over all vertices of the call;
    ``n_empty`` the vertices whose patch is empty (NaN rows)."""

    def __init__(self, rot6d, trans, gap, residual, vptr_host, n_empty: int):
        self.rot6d, self.trans, self.gap, self.residual = rot6d, trans, gap, residual
        self.vptr_host, self.n_empty = np.asarray(vptr_host, dtype=np.int64), int(n_empty)

    def split(self) -> List[tuple]:
        """per mesh (rot6d, trans, gap, residual)"""
        p = self.vptr_host
        return [tuple(t[p[b]:p[b + 1]] for t in (self.rot6d, self.trans, self.gap, self.residual)) for b in range(len(p) - 1)]


def patches(verts0: Sequence, faces: Sequence) -> Patches:
    """The reference's ``nnids`` for a list of meshes: ``verts0[b]`` [V, 3] the rest pose, ``faces[b]`` integer [F, 3]. The five rules and
    the refusals: the module docstring. At most ``MAX_VERTS`` = 32 768 vertices per mesh. One wave per vertex, launched twice (count,
    fill) around a scan. Host reads: one (status and the entry total)."""
    what = "patches"
    mesh = MeshBatch(what, verts0, faces)
    dev = mesh.device
    n = int(mesh.vptr_host[-1])
    if n == 0:
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        return Patches(torch.zeros(1, dtype=torch.int32, device=dev), empty, empty.clone(), mesh.vptr_host)
    most = int(mesh.nv.max())
    if most > MAX_VERTS:
        raise ValueError(f"{what}: mesh {int(mesh.nv.argmax())} has {most} vertices: the patch kernel supports at most {MAX_VERTS} per mesh")
    ops = get_ops()
    words = torch.zeros(mesh.n + 1 + 3, dtype=torch.int32, device=dev)
    key_status, status = words[:mesh.n + 1], words[mesh.n + 1:]
    keys, rowptr = vertex_adjacency(ops, mesh, 6, key_status)
    counts, rung = ops.local_patches(mesh.verts, mesh.vptr, most, rowptr, keys, RUNGS, status)
    scan = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0, dtype=torch.int64)])
    host = torch.cat([words.long(), scan[-1:]]).cpu().numpy()                                            # the host read
    if host[0] & ops.TRANSFER_BAD_FACE:
        raise bad_face(what)
    if host[mesh.n + 1] & ops.LOCAL_BAD_COORD:
        raise ValueError(f"{what}: a coordinate is no finite number")
    total = int(host[-1])
    if total >= 2 ** 31:
        raise ValueError(f"{what}: more than 2^31 - 1 patch entries in one call")
    ptr = scan.to(torch.int32).contiguous()
    ids = ops.local_patches(mesh.verts, mesh.vptr, most, rowptr, keys, RUNGS, status, ptr=ptr, rung=rung, n_ids=total)
    return Patches(ptr, ids, rung, mesh.vptr_host, n_isolated=int(host[mesh.n + 2]))


def local_rigid_motion(verts0: Sequence, traj: Sequence, patches: Patches) -> LocalMotion:
    """``verts0[b]`` [V, 3] the rest pose, ``traj[b]`` [V, T, 3] the clip as ``playback.skin_trajectory`` returns it (float32 or float64,
    one T per call), ``patches`` from ``patches()`` or ``Patches.from_lists``. -> ``LocalMotion`` over all vertices of the call; the
    rule: the module docstring. One lane per (vertex, frame). Host reads: one status read."""
    what = "local_rigid_motion"
    traj = [as_tensor(t).detach() for t in traj]
    mesh = MeshBatch(what, verts0, like=(patches.ptr, *traj))
    if len(traj) != mesh.n or patches.n != mesh.n:
        raise ValueError(f"{what}: one rest pose, one trajectory and one set of patches per mesh")
    if not np.array_equal(patches.nv, mesh.nv):
        raise ValueError(f"{what}: the patches were made for meshes of other vertex counts")
    for b, t in enumerate(traj):
        if t.dim() != 3 or t.shape[0] != mesh.nv[b] or t.shape[2] != 3 or not t.is_floating_point():
            raise ValueError(f"{what}: mesh {b}: traj is floating point [V, T, 3] with one row per vertex ({int(mesh.nv[b])})")
    frames = {int(t.shape[1]) for t in traj}
    if len(frames) > 1:
        raise ValueError(f"{what}: one number of frames per call, got {sorted(frames)}")
    dev = mesh.device
    T = frames.pop() if frames else 0
    n = int(mesh.vptr_host[-1])
    dtype = torch.float32 if traj and all(t.dtype == torch.float32 for t in traj) else torch.float64
    if n == 0 or T == 0:
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        return LocalMotion(z(n, T, 6), z(n, T, 3), z(n, T), z(n, T), mesh.vptr_host, 0)
    if n * T > (2 ** 31 - 1) // 6:
        raise ValueError(f"{what}: more than (2^31 - 1) / 6 fits in one call")
    flat = torch.cat([t.to(device=dev, dtype=dtype) for t in traj], 0).contiguous()
    ops = get_ops()
    status = torch.zeros(3, dtype=torch.int32, device=dev)
    rot6d, trans, gap, residual = ops.local_fit(mesh.verts, flat, mesh.vptr, patches.ptr.to(dev), patches.ids.to(dev), status)
    host = status.cpu().numpy()                                                                          # the status read
    if host[0] & ops.LOCAL_BAD_ID:
        raise ValueError(f"{what}: a patch names a vertex outside its mesh")
    return LocalMotion(rot6d, trans, gap, residual, mesh.vptr_host, int(host[2]))


def gt_rotation_icp(verts0, faces, verts_t, nnids=None) -> tuple:
    """``get_gt_rotation_icp(mesh_0, vtx_0, vtx_t, nnids)`` for one mesh: ``verts0`` [V, 3] with ``faces`` [F, 3] in place of the mesh
    object, ``verts_t`` [V, 3] one frame, ``nnids`` None or the list a former call returned. -> (R_all float64 [V, 6], T_all [V, 3]) on
    the device and nnids, the list of V ascending int64 arrays (host), to pass to the next frame's call."""
    pat = patches([verts0], [faces]) if nnids is None else Patches.from_lists([nnids], device=device_of(verts0, verts_t))
    vt = as_tensor(verts_t)
    if vt.dim() != 2 or vt.shape[1] != 3:
        raise ValueError("gt_rotation_icp: verts_t is [V, 3]")
    out = local_rigid_motion([verts0], [vt.reshape(vt.shape[0], 1, 3)], pat)
    return out.rot6d[:, 0], out.trans[:, 0], (pat.split()[0] if nnids is None else nnids)


def rotation_matrices(rot6d: torch.Tensor) -> torch.Tensor:
    """[..., 6] the first and second column of a rotation -> [..., 3, 3]: the third column is their cross product (plain torch)"""
    a, b = rot6d[..., 0:3], rot6d[..., 3:6]
    return torch.stack([a, b, torch.cross(a, b, dim=-1)], dim=-1)
