"""Spatial queries on the meshes of a ragged batch: one acceleration structure, a 64-wide implicit BVH per mesh built on the device
(csrc/bvh.hip, csrc/bvh_core.h), and the queries on it. Every query is DEFINED by the brute-force kernel it must
equal, bit for bit: the tree only decides which faces are looked at.

    build            the tree of a list of meshes (or of a ``MeshBatch``): ``MeshBVH``
    MeshBVH.refit    the boxes again for moved vertices, same topology and same order: no sort
    cast_rays        the nearest hit of arbitrary rays: what ``labels.cast_rays`` returns (``morig_ray_cast``)
    closest_points   the closest surface point: face, barycentrics, distance as ``transfer.transfer_skins`` returns them
                     (``morig_transfer_closest``)
    segments_blocked whether anything of the mesh lies on a segment (any hit; the form a visibility test needs)
    build_views      one tree per view of a scan, the faces ordered once per mesh: ``ViewBVH``, what ``scan.scan_meshes(accel="bvh")``
                     walks with the scan's own visibility rule (``morig_scan_visibility``); ``geodesic.bone_visibility(accel="bvh")``
                     walks a ``MeshBVH`` of the occluders with the vertex-to-bone rule (``morig_bone_visibility``); DESIGN.md section 28

The tree. Faces are ordered per mesh by the 30-bit Morton code of their centroid in the mesh's cubic frame (bounding-box minimum, largest
extent: the frame of ``simplify``), ties in ascending face order (a stable sort of ``mesh << 30 | code``). A level-1 node is the exact
float64 box of 64 consecutive sorted faces, a level-k node the box of 64 consecutive nodes below; levels are added until a mesh has one
node, four at the most (64^4 faces per mesh; more is a ValueError before anything is launched). The node ranges are prefix sums the host
computes from the face counts: the build reads nothing back. Minimum and maximum do not round, so the tree is a function of the data alone.

The queries. One wave per query; at a node every lane tests one child box, at a leaf one face through the header the brute-force kernel
uses, and the running best is the lexicographic minimum of (value, face): ties go to the lowest face whatever the visiting order. A node
is skipped only by a strict comparison against the best, padded by 2^-40 of the query's scale (bvh_core.h). The result equals brute force
whenever every face's computed t (its hit point) or squared distance lies within that padding of its true value; a query with a
component that is no finite number walks the whole tree. ``visits`` counts the box and face tests of a query.

Host reads: none in ``build`` / ``refit``; ONE status word per query call.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from .labels import _orientation, _raise_on, _rays, _split
from .meshbatch import MeshBatch, bad_face, pack_faces
from .ragged import as_tensor, int32_table, ptr_of
from .runtime import get_ops

WIDTH, MAX_LEVELS = 64, 4
MAX_FACES = WIDTH ** MAX_LEVELS            # MORIG_BVH_MAX_FACES of include/morig_hip.h


def level_table(nf) -> np.ndarray:
    """face counts [B] -> int64 [4, B]: the nodes of every mesh at levels 1 .. 4 (0 above the mesh's top level, the first with one node)"""
    n = np.asarray(nf, dtype=np.int64)
    out = np.zeros((MAX_LEVELS, len(n)), dtype=np.int64)
    live = n > 0
    for k in range(MAX_LEVELS):
        n = (n + WIDTH - 1) // WIDTH
        out[k] = np.where(live, n, 0)
        live = live & (n > 1)
    return out


def node_table(nf) -> tuple:
    """-> (node_ptr int64 [4, B + 1]: mesh b owns the box rows [node_ptr[k - 1, b], node_ptr[k - 1, b + 1]) at level k, the levels one
    after another; the node total of every level [4])"""
    counts = level_table(nf)
    totals = counts.sum(1)
    base = ptr_of(totals)[:-1]
    return np.stack([base[k] + ptr_of(counts[k]) for k in range(MAX_LEVELS)]), totals


class MeshBVH:
    """``mesh`` the ``MeshBatch``; ``order`` int32 [F]: the row of ``mesh.faces`` at every sorted position; ``boxes`` float64 [N, 6];
    ``node_ptr`` int32 [4, B + 1] on the device (``node_ptr_host``, ``level_nodes`` on the host); ``flags`` int32 [B]"""

    def __init__(self, mesh: MeshBatch, what: str = "spatial.build"):
        if mesh.verts is None or mesh.faces is None:
            raise ValueError(f"{what}: a mesh batch with vertices and faces")
        most = int(mesh.nf.max()) if mesh.n else 0
        if most > MAX_FACES:
            raise ValueError(f"{what}: mesh {int(mesh.nf.argmax())} has {most} faces: the tree supports at most {MAX_FACES} per mesh")
        self.mesh, self.what, self.max_faces = mesh, what, most
        self.node_ptr_host, self.level_nodes = node_table(mesh.nf)
        self.node_ptr = int32_table(self.node_ptr_host, mesh.device, what).contiguous()
        ops = get_ops()
        if mesh.n and mesh.faces.shape[0]:
            keys = ops.bvh_build_keys(mesh.verts, mesh.vptr, mesh.faces, mesh.fptr, ops.mesh_bbox(mesh.verts, mesh.vptr))
            self.order = torch.sort(keys, stable=True).indices.to(torch.int32).contiguous()
        else:
            self.order = torch.zeros(0, dtype=torch.int32, device=mesh.device)
        self._boxes(ops)

    def _boxes(self, ops) -> None:
        m = self.mesh
        if m.n == 0:
            self.boxes = torch.zeros(0, 6, dtype=torch.float64, device=m.device)
            self.flags = torch.zeros(0, dtype=torch.int32, device=m.device)
            return
        self.boxes, self.flags = ops.bvh_boxes(m.verts, m.vptr, m.faces, m.fptr, self.order, self.node_ptr, self.level_nodes, self.max_faces)

    def refit(self, verts: Sequence) -> "MeshBVH":
        """The same tree over moved vertices: ``verts[b]`` [V_b, 3] with the vertex counts of the build. The faces, their order and the
        node ranges are kept, only the boxes are computed again; queries then equal those of a fresh build's brute force. No host read."""
        moved = MeshBatch(self.what, verts, like=(self.mesh.verts,))
        if moved.n != self.mesh.n or not np.array_equal(moved.nv, self.mesh.nv):
            raise ValueError(f"{self.what}: refit takes the vertex counts the tree was built with")
        out = object.__new__(MeshBVH)
        out.__dict__.update(self.__dict__)
        out.mesh = object.__new__(MeshBatch)
        out.mesh.__dict__.update(self.mesh.__dict__)
        out.mesh.verts = moved.verts
        out._boxes(get_ops())
        return out


def build(verts: Sequence = None, faces: Sequence = None, mesh: MeshBatch = None) -> MeshBVH:
    """The tree of ``verts[b]`` [V, 3], ``faces[b]`` integer [F, 3] (or of a packed ``mesh``). Launches the key kernel, one stable sort
    and one box kernel per level; nothing is read back. A face index outside its mesh is clamped as the brute-force kernels clamp it and
    reported by the queries (ValueError)."""
    return MeshBVH(mesh if mesh is not None else MeshBatch("spatial.build", verts, faces))


class ViewBVH:
    """One tree per VIEW of a scan (``scan.scan_meshes``): view v owns the rows [vptr[v], vptr[v + 1]) of ``verts`` and draws the faces
    of mesh ``view_mesh[v]`` in that mesh's ``order``. ``order`` int32 [F]; ``boxes`` float64 [N, 6], exact for the view's own vertices;
    ``node_ptr`` int32 [4, NV + 1] on the device (``node_ptr_host``, ``level_nodes`` on the host); ``flags`` int32 [NV]; the tables
    ``verts``, ``vptr``, ``view_mesh`` (int32, device; ``view_mesh_host``), ``faces``, ``fptr``."""

    def __init__(self, verts, vptr, view_mesh_host, faces, fptr, nf, order, what: str = "spatial.build_views"):
        ops, dev = get_ops(), verts.device
        view_mesh_host = np.asarray(view_mesh_host, dtype=np.int64).reshape(-1)
        per_view = np.asarray(nf, dtype=np.int64)[view_mesh_host]
        most = int(per_view.max()) if len(per_view) else 0
        if most > MAX_FACES:
            raise ValueError(f"{what}: view {int(per_view.argmax())} draws {most} faces: the tree supports at most {MAX_FACES} per mesh")
        self.what, self.max_faces = what, most
        self.verts, self.vptr, self.faces, self.fptr, self.order, self.view_mesh_host = verts, vptr, faces, fptr, order, view_mesh_host
        self.view_mesh = int32_table(view_mesh_host, dev, what)
        self.node_ptr_host, self.level_nodes = node_table(per_view)
        self.node_ptr = int32_table(self.node_ptr_host, dev, what).contiguous()
        self.boxes, self.flags = ops.bvh_view_boxes(verts, vptr, self.view_mesh, faces, fptr, order, self.node_ptr, self.level_nodes, most)


def view_order(ops, first_verts: Sequence, faces, fptr, device) -> torch.Tensor:
    """The order of every mesh's faces from the vertices it is first seen with: ``first_verts[m]`` float64 [V_m, 3] on the device, or
    None for a mesh that no view draws (its faces keep their rows: nothing reads them). -> int32 [F]. One key kernel, one stable sort."""
    if faces.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int32, device=device)
    none = torch.zeros(0, 3, dtype=torch.float64, device=device)
    vs = [none if v is None else v for v in first_verts]
    vptr = int32_table(ptr_of([v.shape[0] for v in vs]), device, "spatial.build_views")
    verts = torch.cat(vs, 0).contiguous() if vs else none
    keys = ops.bvh_build_keys(verts, vptr, faces, fptr, ops.mesh_bbox(verts, vptr))
    return torch.sort(keys, stable=True).indices.to(torch.int32).contiguous()


def build_views(verts: Sequence, faces: Sequence, view_mesh=None) -> ViewBVH:
    """The trees of the views of a scan: ``verts[v]`` [V, 3] the vertices of view v, ``faces[m]`` integer [F, 3] the faces of mesh m,
    ``view_mesh[v]`` the mesh of view v (None: view v draws mesh v). Every mesh's faces are ordered ONCE, on the vertices of its first
    view; every view gets boxes of its own vertices, so a query equals brute force whatever pose ordered the faces -- only the pruning
    depends on it. Launches the key kernel, one stable sort and one box kernel per level; nothing is read back."""
    what = "spatial.build_views"
    verts, faces = list(verts), list(faces)
    view_mesh = np.arange(len(verts), dtype=np.int64) if view_mesh is None else np.asarray(view_mesh, dtype=np.int64).reshape(-1)
    if view_mesh.size != len(verts) or (len(verts) and (view_mesh.min() < 0 or view_mesh.max() >= len(faces))):
        raise ValueError(f"{what}: view_mesh names one mesh of the face list per view")
    views = MeshBatch(what, verts)
    dev = views.device
    packed, nf, _, fptr = pack_faces(what, faces, dev)
    first = [None] * len(faces)
    for v in range(len(verts) - 1, -1, -1):
        first[view_mesh[v]] = views.verts[views.vptr_host[v]:views.vptr_host[v + 1]]
    order = view_order(get_ops(), first, packed, fptr, dev)
    return ViewBVH(views.verts, views.vptr, view_mesh, packed, fptr, nf, order, what)


def _ray_cast(ops, bvh: MeshBVH, o, d, rp_dev, orientation: int, visits: bool):
    m = bvh.mesh
    return ops.bvh_ray_cast(o, d, rp_dev, m.verts, m.vptr, m.faces, m.fptr, bvh.order, bvh.boxes, bvh.node_ptr, bvh.flags, orientation, visits)


def cast_rays(bvh: MeshBVH, origins, dirs, ray_ptr, orientation: int = 0, return_visits: bool = False):
    """``labels.cast_rays`` through the tree: ``origins``, ``dirs`` [R, 3] with mesh b owning the rows [ray_ptr[b], ray_ptr[b + 1]).
    -> (t, face, point), each a list with one device tensor per mesh: the smallest t > 0 (+inf: a miss), the lowest face among equals
    (-1), point = o + t d (NaN); ``orientation`` filters the winner only. ``return_visits`` appends int32 [R_b] per mesh. Host reads: one
    status word."""
    orientation = _orientation("spatial.cast_rays", orientation)
    o, d, rp, rp_dev = _rays("spatial.cast_rays", origins, dirs, ray_ptr, bvh.mesh.n, bvh.mesh.device)
    if bvh.mesh.n == 0:
        return ([], [], [], []) if return_visits else ([], [], [])
    ops = get_ops()
    t, face, point, status, visits = _ray_cast(ops, bvh, o, d, rp_dev, orientation, return_visits)
    _raise_on("spatial.cast_rays", int(status.cpu()[0]), ops)                                           # the status read
    out = (_split(t, rp), _split(face, rp), _split(point, rp))
    return out + (_split(visits, rp),) if return_visits else out


def _closest(ops, bvh: MeshBVH, pts: MeshBatch, status: torch.Tensor, visits: bool = False):
    m = bvh.mesh
    return ops.bvh_closest(pts.verts, pts.vptr, m.verts, m.vptr, m.faces, m.fptr, bvh.order, bvh.boxes, bvh.node_ptr, bvh.flags, status, visits)


def closest_points(bvh: MeshBVH, points: Sequence, return_visits: bool = False) -> List[tuple]:
    """``points[b]`` [P_b, 3] against mesh b -> per mesh (face int32 [P_b], bary float64 [P_b, 3], distance float64 [P_b]) on the device:
    the face with the smallest squared distance (pointtri_core.h), the lowest among equals, the barycentrics of the closest point and
    its distance. A mesh without faces gives face -1 and NaN. ``return_visits`` appends int32 [P_b]. Host reads: one status word."""
    what = "spatial.closest_points"
    pts = MeshBatch(what, points, like=(bvh.mesh.verts,))
    if pts.n != bvh.mesh.n:
        raise ValueError(f"{what}: one point set per mesh")
    if pts.n == 0:
        return []
    ops = get_ops()
    status = torch.zeros(1, dtype=torch.int32, device=bvh.mesh.device)
    face, bary, dist, visits = _closest(ops, bvh, pts, status, return_visits)
    if int(status.cpu()[0]) & ops.TRANSFER_BAD_FACE:                                                    # the status read
        raise bad_face(what)
    cols = (face, bary, dist) + ((visits,) if return_visits else ())
    return [tuple(c[pts.vptr_host[b]:pts.vptr_host[b + 1]] for c in cols) for b in range(pts.n)]


def segments_blocked(bvh: MeshBVH, a, b, seg_ptr, skip_vertex=None, t_max=None, return_visits: bool = False):
    """Whether the segment from ``a[q]`` to ``b[q]`` ([S, 3] each, mesh m owning the rows [seg_ptr[m], seg_ptr[m + 1])) meets its mesh:
    -> per mesh uint8 [S_m] on the device, 1 when some face that does not name vertex ``skip_vertex[q]`` (integer [S], local to the mesh;
    negative or None: no face is left out) is hit by the ray a + t (b - a) under raytri_core.h (touching counts, t > 0) at
    t < ``t_max[q]`` (float [S]; None: 1, the segment's end excluded). Any hit, no order: the walk ends with the first leaf that holds one.
    ``return_visits`` -> (blocked, visits). Host reads: one status word."""
    what = "spatial.segments_blocked"
    m = bvh.mesh
    pa, pb, sp, sp_dev = _rays(what, a, b, seg_ptr, m.n, m.device)
    if m.n == 0:
        return ([], []) if return_visits else []

    def column(x, dtype, name):
        if x is None:
            return None
        x = as_tensor(x).reshape(-1)
        if x.numel() != pa.shape[0] or (dtype == torch.int32 and x.is_floating_point()):
            raise ValueError(f"{what}: {name} has one {'integer' if dtype == torch.int32 else 'value'} per segment")
        if dtype == torch.int32:
            x = x.to(torch.int64).clamp(-1, torch.iinfo(torch.int32).max)
        return x.to(device=m.device, dtype=dtype).contiguous()

    ops = get_ops()
    blocked, status, visits = ops.bvh_blocked(pa, pb, sp_dev, column(skip_vertex, torch.int32, "skip_vertex"), column(t_max, torch.float64, "t_max"),
                                              m.verts, m.vptr, m.faces, m.fptr, bvh.order, bvh.boxes, bvh.node_ptr, bvh.flags, return_visits)
    _raise_on(what, int(status.cpu()[0]), ops)                                                          # the status read
    return (_split(blocked, sp), _split(visits, sp)) if return_visits else _split(blocked, sp)
