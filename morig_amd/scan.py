"""Depth scans: from posed vertices, faces and cameras to what the tracking half and the CorrNet / DeformNet training samples take -- the
partial point cloud, the visibility mask of the vertices and the vertex / point correspondences -- on the device (csrc/scan.hip,
csrc/raytri_core.h). The reference only LOADS these (``_pts_traj.npy``, ``_vismask.npy``, ``_corr_v2p.npy``,
``_corr_p2v.npy``; datasets/dataset_pose.py:48-98); its generator was never published, so every rule here is this product's own.

    Camera             orthographic or pinhole, the basis and the pixel sizes computed on the host in float64
    render             depth, face and hit point per pixel
    scan_meshes        per view a ``Scan``: pts / pixel / face, vismask, corr_v2p, corr_p2v
    scan_trajectory    ``[V, T, 3]`` trajectories (playback.skin_trajectory, playback.replay) -> pts_traj, vismask and the correspondences
                       with the frame as last column, the shapes tracking.track, tracking.flow_errors and playback.trajectory_errors take

A VIEW is one (mesh, frame, camera). Inputs are lists with one entry per view (vertices, cameras) or per mesh (faces); ``view_mesh`` names
the mesh of every view, so the views of one mesh share its face table. Arithmetic is float64 in a fixed order, the only atomic is an
integer minimum: two runs give the same bits, and a view alone gives the bits it gives inside a batch.

The pixel ray. Pixel (row i, column j) of a W x H image has a = ((2 j + 1) - W) px and b = (H - (2 i + 1)) py with px = sx / W and
py = sy / H. Orthographic: origin eye + a r + b u, direction f. Pinhole: origin eye, direction f + a r + b u, not normalised, so the depth
t is measured along the optical axis. A ray hits a closed triangle by the division-free Moeller-Trumbore test of raytri_core.h (touching
counts, a zero determinant misses) at t > near; near is 0 for orthographic cameras. The winner of a pixel is the face with the smallest
(bits of float32(t), face index); depth and point are then recomputed in float64 from the winner.

A vertex p is visible when it projects into the closed image rectangle, its depth along f is above near (for both cameras: an
orthographic image does not show what lies behind its plane either), and no face that does not name the vertex meets the segment from its
camera point c (pinhole: eye; orthographic: p - ((p - eye) . f) f) to p at 0 < t < 1 with t |d| < |d| - vis_eps. This does not depend on
the image's resolution and has no depth-map bias.

``corr_radius``, ``vis_eps`` and the thinning of the hits by farthest-point sampling are this product's own choices: nobody has measured
what they do to the networks' accuracy. Sensor noise, lens distortion and parity with any renderer are out of scope.

Host reads: per chunk of views ONE read of (status word, hit counts per view). The correspondence lists of ``scan_meshes`` /
``scan_trajectory`` have lengths that depend on the data: they cost two ``torch.nonzero`` and one read of their per-view counts on top.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import spatial
from .labels import _accel
from .meshbatch import bad_face, pack_faces
from .native import Mat
from .ragged import as_tensor, blocks, device_of, int32_table, ptr_of
from .runtime import get_ops

MAX_SIDE = 1024                  # MORIG_SCAN_MAX_SIDE of include/morig_hip.h
MAX_HITS = 32768                 # morig_fps takes clouds of at most this many points
KEY_BUDGET = 256 << 20           # bytes of key images per chunk of views (chosen, not measured)
ORTHOGRAPHIC, PINHOLE = 0, 1


def _unit(x: np.ndarray) -> np.ndarray:
    n = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError("Camera: eye, target and up do not span a basis")
    return x / n


def _cross(a, b) -> np.ndarray:
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=np.float64)


class Camera:
    """A camera of a view: ``kind``, ``eye``, the basis ``f`` (forward), ``r`` (right), ``u`` (up), the half-pixel sizes ``px`` / ``py``,
    ``near``, ``width`` and ``height``. Built by ``Camera.orthographic`` or ``Camera.pinhole``."""

    def __init__(self, kind: int, eye, target, up, sx: float, sy: float, width: int, height: int, near: float):
        width, height = int(width), int(height)
        if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
            raise ValueError(f"Camera: image {width} x {height}: supported are 1 .. {MAX_SIDE} per side")
        if not (sx > 0.0 and sy > 0.0 and math.isfinite(sx) and math.isfinite(sy)) or not (near >= 0.0 and math.isfinite(near)):
            raise ValueError("Camera: the image extent is positive and finite, near is at least 0")
        eye, target, up = (np.asarray(a, dtype=np.float64).reshape(3) for a in (eye, target, up))
        self.kind, self.eye, self.width, self.height, self.near = kind, eye.copy(), width, height, float(near)
        self.f = _unit(target - eye)
        self.r = _unit(_cross(self.f, up))
        self.u = _cross(self.r, self.f)
        self.px, self.py = sx / width, sy / height

    @classmethod
    def orthographic(cls, eye, target, up, half_width: float, half_height: float, width: int, height: int) -> "Camera":
        return cls(ORTHOGRAPHIC, eye, target, up, float(half_width), float(half_height), width, height, 0.0)

    @classmethod
    def pinhole(cls, eye, target, up, fov_y_deg: float, width: int, height: int, near: float = 1e-3) -> "Camera":
        sy = math.tan(math.radians(float(fov_y_deg)) / 2)
        return cls(PINHOLE, eye, target, up, sy * int(width) / max(int(height), 1), sy, width, height, float(near))

    def row(self) -> np.ndarray:
        """the 16 doubles of csrc/raytri_core.h: eye, f, r, u, px, py, near, 0"""
        return np.concatenate([self.eye, self.f, self.r, self.u, [self.px, self.py, self.near, 0.0]])


class Scan(NamedTuple):
    """What one view gives: pts float64 [P, 3] in row-major pixel order (or the order of the farthest-point thinning), pixel int64 [P]
    (row W + column), face int64 [P], vismask uint8 [V], corr_v2p int64 [K, 2] = (vertex, point), corr_p2v int64 [K', 2] = (point, vertex)"""
    pts: torch.Tensor
    pixel: torch.Tensor
    face: torch.Tensor
    vismask: torch.Tensor
    corr_v2p: torch.Tensor
    corr_p2v: torch.Tensor


class _Job:
    """The views of a call: ``verts`` float64 [V, 3] per view on the device, ``cams``, ``view_mesh``; the meshes' faces concatenated
    (int32 [F, 3], fptr) and the vertex count every mesh's faces are checked against."""

    def __init__(self, what: str, verts: Sequence, faces: Sequence, cameras: Sequence, view_mesh=None):
        self.what = what
        verts, faces, cameras = list(verts), list(faces), list(cameras)
        self.n, self.n_meshes = len(verts), len(faces)
        self.device = dev = device_of(*verts, *faces)
        if len(cameras) != self.n or any(not isinstance(c, Camera) for c in cameras):
            raise ValueError(f"{what}: one Camera per view")
        self.cams = cameras
        self.view_mesh = np.arange(self.n, dtype=np.int64) if view_mesh is None else np.asarray(view_mesh, dtype=np.int64).reshape(-1)
        if self.view_mesh.size != self.n or (self.n and (self.view_mesh.min() < 0 or self.view_mesh.max() >= self.n_meshes)):
            raise ValueError(f"{what}: view_mesh names one mesh of the face list per view")
        vs = [as_tensor(v) for v in verts]
        if any(v.dim() != 2 or v.shape[1] != 3 for v in vs):
            raise ValueError(f"{what}: verts are [V, 3] per view")
        self.verts = [v.to(device=dev, dtype=torch.float64) for v in vs]
        self.nv = np.array([v.shape[0] for v in vs], dtype=np.int64)
        self.faces, self.nf, _, self.fptr = pack_faces(what, faces, dev)
        mesh_nv = np.full(self.n_meshes, 2 ** 31 - 1, dtype=np.int64)                     # a mesh without a view: nothing to check against
        for v in range(self.n):
            m = self.view_mesh[v]
            if mesh_nv[m] != 2 ** 31 - 1 and mesh_nv[m] != self.nv[v]:
                raise ValueError(f"{what}: view {v} has {self.nv[v]} vertices, an earlier view of mesh {m} has {mesh_nv[m]}")
            mesh_nv[m] = self.nv[v]
        self.mesh_nv = int32_table(mesh_nv, dev, what)
        self._order = None

    def order(self, ops) -> torch.Tensor:
        """the faces of every mesh ordered on the vertices of its first view in the job (``spatial.view_order``): taken per job, not per
        chunk, so that the walks do not depend on the chunking"""
        if self._order is None:
            first = [None] * self.n_meshes
            for v in range(self.n - 1, -1, -1):
                first[self.view_mesh[v]] = self.verts[v]
            self._order = spatial.view_order(ops, first, self.faces, self.fptr, self.device)
        return self._order

    def chunks(self, budget: int):
        """view ranges [lo, hi) whose key images (8 bytes per pixel) stay under ``budget`` bytes; a view larger than it goes alone"""
        lo, used = 0, 0
        for v, c in enumerate(self.cams):
            size = 8 * c.width * c.height
            if v > lo and used + size > budget:
                yield lo, v
                lo, used = v, 0
            used += size
        if self.n > lo:
            yield lo, self.n


class _Chunk:
    """the device tables of the views [lo, hi) of a job and their images"""

    def __init__(self, ops, job: _Job, lo: int, hi: int):
        dev, what = job.device, job.what
        self.job, self.lo, self.n = job, lo, hi - lo
        cams = job.cams[lo:hi]
        self.nv = job.nv[lo:hi]
        self.vptr_host = ptr_of(self.nv)
        self.vptr = int32_table(self.vptr_host, dev, what)
        self.verts = torch.cat(job.verts[lo:hi], 0).contiguous()
        self.sizes = np.array([[c.width, c.height] for c in cams], dtype=np.int64).reshape(-1, 2)
        self.kptr_host = ptr_of(self.sizes[:, 0] * self.sizes[:, 1])
        self.kptr = torch.from_numpy(self.kptr_host).to(dev)
        mesh = job.view_mesh[lo:hi]
        self.wptr_host = ptr_of(job.nf[mesh])
        views = np.stack([mesh, self.sizes[:, 0], self.sizes[:, 1], np.array([c.kind for c in cams], dtype=np.int64)], 1).astype(np.int32)
        self.views = torch.from_numpy(np.ascontiguousarray(views)).to(dev)
        self.cams = torch.from_numpy(np.stack([c.row() for c in cams])).to(dev)
        self.tables = (self.verts, self.vptr, job.faces, job.fptr, self.cams, self.views)
        self.keys, self.status = ops.scan_raster(self.verts, self.vptr, job.faces, job.fptr, job.mesh_nv, self.cams, self.views, self.kptr,
                                                 torch.from_numpy(self.wptr_host).to(dev), int(self.sizes.min()), int(self.sizes.max()),
                                                 int(self.kptr_host[-1]), int(self.wptr_host[-1]))
        self.depth, self.face, self.point, self.flags = ops.scan_resolve(*self.tables, self.kptr, self.keys)

    def raise_on(self, status: int, ops) -> None:
        if status == ops.SCAN_BAD_FACE:
            raise bad_face(self.job.what)
        if status != 0:
            raise RuntimeError(f"{self.job.what}: status {status}")



# ------------------------------------------------------------------------------------------------------------------------- render
def render(verts: Sequence, faces: Sequence, cameras: Sequence[Camera], view_mesh=None, key_budget: int = KEY_BUDGET) -> List[tuple]:
    """The depth image of every view: ``verts[v]`` [V, 3] the vertices of view v, ``faces[m]`` integer [F, 3] the faces of mesh m,
    ``view_mesh[v]`` the mesh of view v (None: view v draws mesh v). -> per view (depth float64 [H, W], +inf where nothing is hit; face
    int32 [H, W], -1 there; point float64 [H, W, 3], +inf there) on the device. One triangle per wave over its clamped pixel box; see the
    module docstring for the rules. A face index outside its mesh is a ValueError (checked on the device, read with the chunk's status)."""
    job = _Job("render", verts, faces, cameras, view_mesh)
    ops, out = get_ops(), []
    for lo, hi in job.chunks(int(key_budget)):
        ch = _Chunk(ops, job, lo, hi)
        ch.raise_on(int(ch.status.cpu()[0]), ops)                                                     # the status read
        for v in range(ch.n):
            k0, k1, w, h = int(ch.kptr_host[v]), int(ch.kptr_host[v + 1]), int(ch.sizes[v, 0]), int(ch.sizes[v, 1])
            out.append((ch.depth[k0:k1].view(h, w), ch.face[k0:k1].view(h, w), ch.point[k0:k1].view(h, w, 3)))
    return out


# ------------------------------------------------------------------------------------------------------------------------- scans
def _split_pairs(rows: torch.Tensor, ptr_dev: torch.Tensor, n: int):
    """rows: global row indices of a ragged batch delimited by ptr_dev [n + 1] -> (segment of every row, row local to its segment)"""
    seg = torch.searchsorted(ptr_dev[1:].long().contiguous(), rows, right=True).clamp(max=max(n - 1, 0))
    return seg, rows - ptr_dev.long()[seg]


def _scan_chunk(ops, ch: _Chunk, n_pts: Optional[int], corr_radius: float, vis_eps: float, bvh: bool = False) -> List[Scan]:
    dev, what = ch.job.device, ch.job.what
    rank = torch.cumsum(ch.flags, 0, dtype=torch.int64)
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), rank])[ch.kptr]                # hits in front of every view
    host = torch.cat([ch.status.to(torch.int64), before]).cpu().numpy()                               # THE read: status, hit counts
    ch.raise_on(int(host[0]), ops)
    hptr = host[1:]
    hits = np.diff(hptr)
    pts, pixel, face = ops.scan_compact(ch.point, ch.face, ch.flags, rank, ch.kptr, int(hptr[-1]))
    pptr_host = hptr
    if n_pts is not None:
        for v in range(ch.n):
            if hits[v] > MAX_HITS:
                raise ValueError(f"{what}: view {ch.lo + v} has {hits[v]} hits: thinning to n_pts takes at most {MAX_HITS}")
            if hits[v] < n_pts:
                raise ValueError(f"{what}: view {ch.lo + v} has {hits[v]} hits, fewer than n_pts = {n_pts}")
        p4 = torch.zeros(pts.shape[0], 4, dtype=torch.float32, device=dev)
        p4[:, :3] = pts.float()
        pptr_host = ptr_of([n_pts] * ch.n)
        idx = ops.fps(Mat.of(p4, 0, 3), int32_table(hptr, dev, what), int32_table(pptr_host, dev, what), None, ch.n, int(hits.max()),
                      n_pts * ch.n).long()
        pts, pixel, face = pts[idx].contiguous(), pixel[idx], face[idx]
    pptr = int32_table(pptr_host, dev, what)
    vblk, n_vblk = blocks(ch.nv, ops.SCAN_BLOCK, dev, what)
    if bvh:                                                                                           # the same mask through the chunk's view trees
        job = ch.job
        tree = spatial.ViewBVH(ch.verts, ch.vptr, job.view_mesh[ch.lo:ch.lo + ch.n], job.faces, job.fptr, job.nf, job.order(ops), what)
        vis = ops.bvh_scan_visibility(*ch.tables, float(vis_eps), tree.order, tree.boxes, tree.node_ptr, tree.flags)[0]
    else:
        vis = ops.scan_visibility(*ch.tables, vblk, n_vblk, float(vis_eps))
    pblk, n_pblk = blocks(np.diff(pptr_host), ops.SCAN_BLOCK, dev, what)
    r2 = float(corr_radius) * float(corr_radius)
    v_idx, v_d2 = ops.scan_nearest(ch.verts, ch.vptr, pts, pptr, None, vblk, n_vblk)
    p_idx, p_d2 = ops.scan_nearest(pts, pptr, ch.verts, ch.vptr, vis, pblk, n_pblk)
    v_rows = torch.nonzero((vis != 0) & (v_idx >= 0) & (v_d2 <= r2))[:, 0]
    p_rows = torch.nonzero((p_idx >= 0) & (p_d2 <= r2))[:, 0]
    v_seg, v_loc = _split_pairs(v_rows, ch.vptr, ch.n)
    p_seg, p_loc = _split_pairs(p_rows, pptr, ch.n)
    counts = torch.cat([torch.bincount(v_seg, minlength=ch.n), torch.bincount(p_seg, minlength=ch.n)]).cpu().numpy()   # the sizes read
    cv, cp = ptr_of(counts[:ch.n]), ptr_of(counts[ch.n:])
    v2p = torch.stack([v_loc, v_idx[v_rows].long()], 1)
    p2v = torch.stack([p_loc, p_idx[p_rows].long()], 1)
    out = []
    for v in range(ch.n):
        ps = slice(pptr_host[v], pptr_host[v + 1])
        out.append(Scan(pts[ps], pixel[ps].long(), face[ps].long(), vis[ch.vptr_host[v]:ch.vptr_host[v + 1]], v2p[cv[v]:cv[v + 1]],
                        p2v[cp[v]:cp[v + 1]]))
    return out


def _check_options(what: str, n_pts, corr_radius, vis_eps) -> Optional[int]:
    if n_pts is not None:
        n_pts = int(n_pts)
        if not 1 <= n_pts <= MAX_HITS:
            raise ValueError(f"{what}: n_pts {n_pts}: supported are 1 .. {MAX_HITS}")
    if not (corr_radius >= 0.0 and math.isfinite(corr_radius)) or not (vis_eps >= 0.0 and math.isfinite(vis_eps)):
        raise ValueError(f"{what}: corr_radius and vis_eps are finite and at least 0")
    return n_pts


def scan_meshes(verts: Sequence, faces: Sequence, cameras: Sequence[Camera], n_pts: Optional[int] = None, corr_radius: float = 0.02,
                vis_eps: float = 1e-4, view_mesh=None, key_budget: int = KEY_BUDGET, accel=None) -> List[Scan]:
    """One ``Scan`` per view (arguments as ``render``). ``pts``: the hit points of the depth image in row-major pixel order, with their
    ``pixel`` and ``face``; ``n_pts=None`` keeps all of them (ragged), an integer thins them by farthest-point sampling (morig_fps:
    float32 positions, started at the view's first hit) -- more than 32 768 hits with ``n_pts`` set, or fewer hits than ``n_pts``, is a
    ValueError naming the view. ``vismask`` by the segment rule of the module docstring. ``corr_v2p``: every visible vertex whose nearest
    point of ``pts`` is within ``corr_radius``, ascending by vertex; ``corr_p2v``: every point whose nearest VISIBLE vertex is within
    ``corr_radius``, ascending by point -- the column orders customized_losses.infoNCE:118-131 indexes. Distances are
    (dx^2 + dy^2) + dz^2 in float64 against corr_radius^2, ties go to the lowest index. ``corr_radius``, ``vis_eps`` and the sampler are
    this product's own; their effect on the networks' accuracy is unmeasured. ``accel="bvh"`` takes ``vismask`` from one tree per view
    (``spatial.ViewBVH``: the faces ordered once per mesh of the call, boxes per view) instead of from all faces, for the same bits
    (DESIGN.md section 28); everything else is as without it. A face index out of range is the chunk's status either way."""
    n_pts = _check_options("scan_meshes", n_pts, corr_radius, vis_eps)
    bvh = _accel("scan_meshes", accel)
    job = _Job("scan_meshes", verts, faces, cameras, view_mesh)
    ops, out = get_ops(), []
    for lo, hi in job.chunks(int(key_budget)):
        out += _scan_chunk(ops, _Chunk(ops, job, lo, hi), n_pts, corr_radius, vis_eps, bvh)
    return out


def scan_trajectory(vtx_traj: Sequence, faces: Sequence, cameras: Sequence, n_pts: int, corr_radius: float = 0.02, vis_eps: float = 1e-4,
                    key_budget: int = KEY_BUDGET, accel=None) -> List[tuple]:
    """Scans of animated meshes: ``vtx_traj[m]`` is [V, T, 3] (what playback.skin_trajectory and playback.replay return), ``faces[m]``
    the faces of mesh m, ``cameras[m]`` one Camera for every frame or a sequence of T of them; ``n_pts`` is required, so that the frames
    stack. -> per mesh (pts_traj float64 [n_pts, T, 3], vismask uint8 [V, T], corr_v2p int64 [K, 3] = (vertex, point, frame), corr_p2v
    int64 [K', 3] = (point, vertex, frame)): the frame is the last column, as in datasets/dataset_pose.py:70-79, and the shapes are
    those tracking.track, tracking.flow_errors and playback.trajectory_errors take. Every (mesh, frame) is a view of ``scan_meshes``;
    the views run in chunks whose key images stay under ``key_budget`` bytes (the default is a choice, not a measurement). ``accel``
    as in ``scan_meshes``: the faces of a mesh are ordered on its first frame and boxed again for every frame."""
    _accel("scan_trajectory", accel)
    if n_pts is None:
        raise ValueError("scan_trajectory: n_pts is required")
    n_pts = _check_options("scan_trajectory", n_pts, corr_radius, vis_eps)
    trajs, cameras = [as_tensor(t) for t in vtx_traj], list(cameras)
    if any(t.dim() != 3 or t.shape[2] != 3 for t in trajs):
        raise ValueError("scan_trajectory: vtx_traj are [V, T, 3] per mesh")
    if len(cameras) != len(trajs) or len(faces) != len(trajs):
        raise ValueError("scan_trajectory: one faces array and one camera (or T cameras) per mesh")
    dev = device_of(*trajs, *faces)
    verts, cams, view_mesh, frames = [], [], [], []
    for m, t in enumerate(trajs):
        T = int(t.shape[1])
        cm = [cameras[m]] * T if isinstance(cameras[m], Camera) else list(cameras[m])
        if len(cm) != T:
            raise ValueError(f"scan_trajectory: mesh {m} has {T} frames and {len(cm)} cameras")
        per_frame = t.to(device=dev, dtype=torch.float64).permute(1, 0, 2).contiguous()               # [T, V, 3]: a view owns its rows
        verts += [per_frame[k] for k in range(T)]
        cams += cm
        view_mesh += [m] * T
        frames.append(T)
    scans = scan_meshes(verts, faces, cams, n_pts=n_pts, corr_radius=corr_radius, vis_eps=vis_eps, view_mesh=view_mesh, key_budget=key_budget,
                        accel=accel)
    out, at = [], 0
    for m, T in enumerate(frames):
        mine = scans[at:at + T]
        at += T
        V = int(trajs[m].shape[0])
        with_frame = lambda pairs: (torch.cat([torch.cat([c, torch.full((c.shape[0], 1), k, dtype=torch.int64, device=dev)], 1)
                                               for k, c in enumerate(pairs)], 0) if pairs else torch.zeros(0, 3, dtype=torch.int64, device=dev))
        out.append((torch.stack([s.pts for s in mine], 1) if T else torch.zeros(n_pts, 0, 3, dtype=torch.float64, device=dev),
                    torch.stack([s.vismask for s in mine], 1) if T else torch.zeros(V, 0, dtype=torch.uint8, device=dev),
                    with_frame([s.corr_v2p for s in mine]), with_frame([s.corr_p2v for s in mine])))
    return out
