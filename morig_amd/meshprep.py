"""The mesh front end: from ``(vertices, faces)`` to everything the other stages take, on the device and with no dependency beyond
this package (csrc/meshprep.hip, csrc/tribox_core.h).

    normalize        data_proc/common_ops.py:123-138, bit-equal in float64
    tpl_edges        the edge SET of get_tpl_edges (common_ops.py:15-32), grouped by ascending vertex, then ascending neighbour (the
                     reference's order inside one vertex is CPython's set iteration order and is not reproduced)
    voxelize         the solid voxel grid the reference gets from the external ``binvox`` program -> formats.Voxels
    sample_surface   surface samples and normals for morig_amd.geodesic, where the reference calls open3d's Poisson-disk sampler
    simplify         a mesh of at most a target number of faces, where the reference calls open3d's simplify_quadric_decimation: vertex
                     clustering with a regularised quadric representative (csrc/simplify.hip, csrc/quadric_core.h)
    repair           ``clean``, then a consistent orientation per component (outward where the component is closed) and a centroid fan
                     over every simple boundary loop; what cannot be repaired is counted and left alone (csrc/meshfix.hip,
                     csrc/orient_core.h)
    refine           a COARSE mesh brought up to a density by edge splits, to a longest edge or to a vertex count; ``interpolate`` carries
                     per-vertex values up along the parents, ``[:V]`` carries results down: the reference never meets a coarse mesh
                     (csrc/refine.hip, csrc/split_core.h)
    diagnose, clean  a topology report (weld classes, degenerate and duplicate faces, boundary / non-manifold / conflicting edges,
                     components, Euler number) and the lossless cleaning pass that goes with it: the reference has neither, it starts
                     from pre-processed meshes (csrc/meshcheck.hip, csrc/topo_core.h). ``weld_tol``: vertices
                     within a tolerance weld too, by single linkage (csrc/proxweld.hip, csrc/proxweld_core.h)
    split_nonmanifold  ``clean``, then every FAN of faces around a vertex gets its own copy of that vertex: an edge with three or more faces
                     and a pinched ("bow-tie") vertex come apart, nothing moves; ``repair(split=True)`` runs it in front of the orientation
                     (csrc/meshsplit.hip, csrc/fan_core.h)
    prepare_mesh     all of it, then geodesic.surface_geodesic_batched and graph_build's geodesic ball graph

Every function takes lists with one entry per mesh (numpy arrays or tensors, on any device) and runs the whole batch in one launch per
stage; results are device tensors unless said otherwise. Arithmetic is float64 in a fixed order, the only atomics are integer ones whose
result does not depend on order (ORs on bitsets; OR, add and min in the diagnosis; a max in the refinement): two runs give the same bits, and a mesh alone gives
the bits it gives inside a batch.

The voxel rule and the sampler are this product's own. ``binvox`` cannot be matched (neither its binary nor its source is available) and
no parity with open3d's Poisson-disk samples or estimated normals exists or is claimed; nobody has measured what this sampler does to the
networks' accuracy.

Voxel rule. Frame: ``translate`` = bounding-box minimum, ``scale`` = largest extent, grid coordinate g = (p - translate) / scale * dims,
computed once per vertex in that order. Voxel (i, j, k) is the closed cube [i, i + 1] x [j, j + 1] x [k, k + 1], its centre at i + 0.5
(the binvox file format's convention). SURFACE: a voxel is set when a triangle, as a closed set, overlaps the closed cube (13-axis
separating-axis test; a zero axis separates nothing, so a degenerate triangle is decided by its box and edge axes). Touching counts: a
face lying exactly in a grid plane sets BOTH neighbouring layers. INTERIOR: a voxel is set when it is no surface voxel and cannot be
reached from outside the grid through 6-connected non-surface voxels. Watertight shells come out solid; overlapping or
self-intersecting components stay solid where a parity rule would hollow them; a hole wider than a voxel leaks and leaves the shell only.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import formats
from .meshbatch import MeshBatch, bad_face
from .native import Mat
from .ragged import as_tensor, device_of, int32_table, ptr_of
from .runtime import get_ops

MAX_DIMS = 96                    # MORIG_VOXEL_MAX_DIMS of include/morig_hip.h: the fill keeps dims^2 rows of 96 bits in LDS
MAX_CANDIDATES = 32768           # morig_fps takes clouds of at most this many points
SIMPLIFY_MAX_RES = 1024          # MORIG_SIMPLIFY_MAX_RES: a cell key takes 30 bits
SIMPLIFY_MAX_INDEX = 1 << 21     # MORIG_SIMPLIFY_MAX_INDEX: a face key packs three output vertices of a launch at 21 bits each


def _bbox(ops, batch: MeshBatch, what: str) -> np.ndarray:
    """float64 [B, 6] on the host (the frame of every stage is a host value: it is returned to the caller)"""
    if any(n < 1 for n in batch.nv):
        raise ValueError(f"{what}: a mesh without vertices")
    box = ops.mesh_bbox(batch.verts, batch.vptr).cpu().numpy()
    if not np.isfinite(box).all():
        raise ValueError(f"{what}: a vertex coordinate is not finite")
    return box


# ------------------------------------------------------------------------------------------------------------------------- normalize
def normalize(verts: Sequence, pivot: Optional[Sequence] = None, scale: Optional[Sequence] = None):
    """``common_ops.normalize`` for a list of meshes: pivot = (mid x, min y, mid z) of the bounding box, scale = 1 / largest extent,
    then (v - pivot) * scale in float64, bit-equal to the reference. ``pivot`` / ``scale``: one entry per mesh (an entry may be None) to
    apply a given frame, as the reference's optional arguments do. -> one (verts float64 [V, 3] on the device, pivot float64 numpy [3],
    scale float) per mesh."""
    batch = MeshBatch("normalize", verts=verts)
    if batch.n == 0:
        return []
    pivot = [None] * batch.n if pivot is None else list(pivot)
    scale = [None] * batch.n if scale is None else list(scale)
    if len(pivot) != batch.n or len(scale) != batch.n:
        raise ValueError("normalize: one pivot / scale per mesh")
    ops = get_ops()
    box = _bbox(ops, batch, "normalize")
    lo, hi = box[:, :3], box[:, 3:]
    frame = np.zeros((batch.n, 4), dtype=np.float64)
    for b in range(batch.n):
        if scale[b] is None:
            extent = max(hi[b] - lo[b])
            if not extent > 0.0:
                raise ValueError(f"normalize: mesh {b} has no extent")
            frame[b, 3] = 1.0 / extent
        else:
            frame[b, 3] = float(scale[b])
        frame[b, :3] = ([(lo[b, 0] + hi[b, 0]) / 2, lo[b, 1], (lo[b, 2] + hi[b, 2]) / 2] if pivot[b] is None
                        else np.asarray(pivot[b], dtype=np.float64).reshape(3))
    out = ops.mesh_affine(batch.verts, batch.vptr, torch.from_numpy(frame).to(batch.device), ops.MESH_NORMALIZE)
    return [(v, frame[b, :3].copy(), float(frame[b, 3])) for b, v in enumerate(batch.split_v(out))]


# ------------------------------------------------------------------------------------------------------------------------- 1-ring edges
def tpl_edges(faces: Sequence, n_verts: Sequence[int], self_loops: bool = False) -> List[torch.Tensor]:
    """The edge set of ``get_tpl_edges`` for a list of meshes: for every vertex that occurs in a face one column [v, n] per distinct
    n != v sharing a face with it. A face with a repeated index contributes its distinct pairs only, a vertex in no face nothing, a
    duplicate face nothing new. -> int64 [2, E] per mesh on the device (row 0 = v, row 1 = n: the orientation formats.load_rig_sample
    gives tpl_edge_index before its self loops), grouped by ascending v, then ascending n. ``self_loops`` appends one (i, i) per vertex
    as formats._with_self_loops does. Six directed 64-bit keys per face are emitted by a kernel, sorted by torch.sort, and the first key
    of every run is kept by two more kernels; valence is unbounded."""
    batch = MeshBatch("tpl_edges", faces=faces, n_verts=n_verts, check_faces="host")
    if batch.n == 0:
        return []
    ops, dev = get_ops(), batch.device
    keys = torch.sort(ops.tpl_edge_keys(batch.faces, batch.fptr, batch.vptr)).values.contiguous()
    flags = ops.tpl_edge_flags(keys)
    rank = torch.cumsum(flags, 0, dtype=torch.int64)
    bounds = torch.searchsorted(keys, torch.from_numpy(batch.vptr_host << 32).to(dev))             # the first key of every mesh
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), rank])[bounds]              # flagged keys in front of it
    eptr = before.cpu().numpy()                                                                    # the size read
    out = ops.tpl_edge_compact(keys, flags, rank, batch.vptr, int(eptr[-1]))
    res = [out[:, eptr[b]:eptr[b + 1]] for b in range(batch.n)]
    if self_loops:
        res = [torch.cat([e, torch.arange(n, dtype=torch.int64, device=dev).unsqueeze(0).repeat(2, 1)], dim=1) for e, n in zip(res, batch.nv)]
    return res


# ------------------------------------------------------------------------------------------------------------------------- voxels
def voxelize(verts: Sequence, faces: Sequence, dims: int = 88, return_info: bool = False):
    """The solid voxel grid of every mesh by the rule in this module's docstring -> one ``formats.Voxels`` per mesh: ``data`` bool
    [dims]^3 numpy array indexed [x][y][z], ``translate`` = the bounding-box minimum, ``scale`` = the largest extent, ``dims`` [d, d, d].
    Surface: one wave per triangle over the voxels of its clamped bounding box (one triangle spanning the grid is slow but correct),
    integer ORs into a bitset. Interior: one workgroup per mesh floods the outside from the six grid faces in LDS until a sweep changes
    nothing. ``dims`` from 1 to 96; anything else is a ValueError. ``return_info``: also int32 numpy [B, 2] = (status, sweeps)."""
    dims = int(dims)
    if not 1 <= dims <= MAX_DIMS:
        raise ValueError(f"voxelize: dims {dims}: supported are 1 .. {MAX_DIMS}")
    batch = MeshBatch("voxelize", verts=verts, faces=faces, check_faces="host")
    if batch.n == 0:
        return ([], np.zeros((0, 2), dtype=np.int32)) if return_info else []
    ops = get_ops()
    box = _bbox(ops, batch, "voxelize")
    frame = np.zeros((batch.n, 4), dtype=np.float64)
    frame[:, :3] = box[:, :3]
    frame[:, 3] = (box[:, 3:] - box[:, :3]).max(axis=1)
    if not (frame[:, 3] > 0.0).all():
        raise ValueError(f"voxelize: mesh {int(np.argmin(frame[:, 3] > 0.0))} has no extent")
    grid = ops.mesh_affine(batch.verts, batch.vptr, torch.from_numpy(frame).to(batch.device), ops.MESH_GRID, float(dims))
    surface = ops.voxel_surface(grid, batch.faces, batch.fptr, batch.vptr, dims)
    solid, info = ops.voxel_fill(surface, dims)
    info = info.cpu().numpy()                                                                      # the status read
    if (info[:, 0] != ops.VOXEL_OK).any():
        raise RuntimeError(f"voxelize: mesh {int(np.argmax(info[:, 0] != ops.VOXEL_OK))}: the fill passed its bound of dims^3 sweeps")
    data = solid.cpu().numpy().astype(bool)
    out = [formats.Voxels(data[b], [dims] * 3, frame[b, :3].tolist(), float(frame[b, 3])) for b in range(batch.n)]
    return (out, info) if return_info else out


# ------------------------------------------------------------------------------------------------------------------------- samples
def draw_uniforms(n_candidates: int, seed: int) -> np.ndarray:
    """The uniforms of one mesh, float64 [n_candidates, 3] = (triangle, u, v) per candidate, from numpy's PCG64 seeded with ``seed``: a
    host array, reproducible from the seed alone (every mesh has a generator of its own, so a mesh draws the same inside any batch)."""
    return np.random.Generator(np.random.PCG64(int(seed))).random((int(n_candidates), 3))


def sample_surface(verts: Sequence, faces: Sequence, n_samples: int = 4000, oversample: int = 5, seed=0, return_faces: bool = False):
    """Surface samples and normals for morig_amd.geodesic, by this product's own rule: ``oversample * n_samples`` candidates per mesh --
    the triangle by inverse CDF over the float64 cumulative areas (searchsorted, side "right"), the point by the barycentrics
    (1 - sqrt u, sqrt u (1 - v), sqrt u v) -- thinned to ``n_samples`` by farthest-point sampling (morig_fps, float32 positions) from
    candidate 0. The normal of a sample is the unit normal (B - A) x (C - A) of its triangle. ``seed``: an int for every mesh, or one
    per mesh. -> (pts, normals): lists of float64 [n_samples, 3] on the device; ``return_faces``: also the triangle of every sample
    (int64) . Raises ValueError on a mesh of zero total area. No parity with open3d's Poisson-disk samples is claimed."""
    n_samples, oversample = int(n_samples), int(oversample)
    if n_samples < 1 or oversample < 1:
        raise ValueError("sample_surface: n_samples and oversample are at least 1")
    n_cand = n_samples * oversample
    if n_cand > MAX_CANDIDATES:
        raise ValueError(f"sample_surface: {n_cand} candidates per mesh: supported are at most {MAX_CANDIDATES}")
    batch = MeshBatch("sample_surface", verts=verts, faces=faces, check_faces="host")
    if batch.n == 0:
        return ([], [], []) if return_faces else ([], [])
    seeds = [int(seed)] * batch.n if np.ndim(seed) == 0 else [int(s) for s in seed]
    if len(seeds) != batch.n:
        raise ValueError("sample_surface: one seed per mesh")
    ops, dev = get_ops(), batch.device
    cum = ops.tri_area_cdf(batch.verts, batch.vptr, batch.faces, batch.fptr)
    last = torch.from_numpy(np.maximum(batch.fptr_host[1:] - 1, 0)).to(dev)
    total = cum[last].cpu().numpy() if cum.numel() else np.zeros(batch.n)                         # the zero-area read
    for b in range(batch.n):
        if batch.nf[b] == 0 or not (total[b] > 0.0 and np.isfinite(total[b])):
            raise ValueError(f"sample_surface: mesh {b} has no surface area")
    uniforms = torch.from_numpy(np.concatenate([draw_uniforms(n_cand, s) for s in seeds], 0)).to(dev)
    cptr = int32_table(ptr_of([n_cand] * batch.n), dev, "sample_surface")
    pts, normals, tri = ops.surface_samples(batch.verts, batch.vptr, batch.faces, batch.fptr, cum, uniforms, cptr)
    p4 = torch.zeros(pts.shape[0], 4, dtype=torch.float32, device=dev)
    p4[:, :3] = pts.float()
    optr = int32_table(ptr_of([n_samples] * batch.n), dev, "sample_surface")
    idx = ops.fps(Mat.of(p4, 0, 3), cptr, optr, None, batch.n, n_cand, n_samples * batch.n).long()
    sp, sn, st = pts[idx], normals[idx], tri[idx].long()
    cut = lambda t: [t[b * n_samples:(b + 1) * n_samples] for b in range(batch.n)]
    return (cut(sp), cut(sn), cut(st)) if return_faces else (cut(sp), cut(sn))


# ------------------------------------------------------------------------------------------------------------------------- simplify
def _simplify_pass(ops, batch: MeshBatch, frame: torch.Tensor, res: np.ndarray) -> dict:
    """One clustering of a launch group at the resolutions ``res`` (one per mesh), up to the marked faces. Two sorts, no host read:
    ``cptr`` / ``optr`` (the cells and the output faces in front of every mesh) stay on the device."""
    dev, n_rows = batch.device, batch.verts.shape[0]
    res_t = torch.from_numpy(res.astype(np.int32)).to(dev)
    lo, hi = int(res.min()), int(res.max())
    keys = ops.simplify_cell_keys(batch.verts, batch.vptr, frame, res_t, lo, hi)
    skeys, vorder = torch.sort(keys, stable=True)                                                 # members stay in ascending vertex order
    skeys = skeys.contiguous()
    vflags = ops.tpl_edge_flags(skeys)
    vrank = torch.cumsum(vflags, 0, dtype=torch.int64)
    cell = torch.empty(n_rows, dtype=torch.int32, device=dev)
    cell[vorder] = (vrank - 1).to(torch.int32)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    first = torch.searchsorted(skeys, torch.arange(batch.n + 1, dtype=torch.int64, device=dev) << ops.SIMPLIFY_MESH_SHIFT)
    cptr = torch.cat([zero, vrank])[first]                                                         # cells in front of every mesh
    corner_cell, fkeys = ops.simplify_face_keys(batch.faces, batch.fptr, batch.vptr, cell, n_rows)
    sfkeys, forder = torch.sort(fkeys, stable=True)                                               # the lowest input face first among equals
    fflags = ops.tpl_edge_flags(sfkeys.contiguous())
    frank = torch.cumsum(fflags, 0, dtype=torch.int64)
    optr = torch.cat([zero, frank])[torch.searchsorted(sfkeys, cptr << (2 * ops.SIMPLIFY_INDEX_BITS))]
    return dict(res=res_t, lo=lo, hi=hi, skeys=skeys, vorder=vorder, vflags=vflags, vrank=vrank, cell=cell, cptr=cptr,
                corner_cell=corner_cell, forder=forder.contiguous(), fflags=fflags, frank=frank, optr=optr)


def _simplify_group(ops, batch: MeshBatch, target: int, given: List[Optional[int]], what: str):
    """one launch group -> (per mesh (verts, faces, vertex_map, resolution), per mesh the trace [(r, n(r)), ...])"""
    dev = batch.device
    box = _bbox(ops, batch, what)
    frame = np.zeros((batch.n, 4), dtype=np.float64)
    frame[:, :3] = box[:, :3]
    frame[:, 3] = (box[:, 3:] - box[:, :3]).max(axis=1)
    if not (frame[:, 3] > 0.0).all():
        raise ValueError(f"{what}: mesh {int(np.argmin(frame[:, 3] > 0.0))} of the launch has no extent")
    frame_t = torch.from_numpy(frame).to(dev)
    auto = np.array([g is None for g in given])
    res = np.array([SIMPLIFY_MAX_RES if g is None else g for g in given], dtype=np.int64)
    trace = [[] for _ in range(batch.n)]

    def counts(r, asked):
        st = _simplify_pass(ops, batch, frame_t, r)
        n = np.diff(st["optr"].cpu().numpy())                                                      # the one host read of a step
        for b in np.nonzero(asked)[0]:
            trace[b].append((int(r[b]), int(n[b])))
        return st, n

    st = None
    if auto.any():                                                                                 # the bisection of every mesh, together
        st, n = counts(res, auto)
        lo, hi = np.ones(batch.n, dtype=np.int64), np.full(batch.n, SIMPLIFY_MAX_RES, dtype=np.int64)
        open_ = auto & (n > target)
        lo[~open_], hi[~open_] = res[~open_], res[~open_] + 1
        while (hi - lo > 1).any():
            live = hi - lo > 1
            res = np.where(live, (lo + hi) // 2, lo)
            st, n = counts(res, live)
            fits = n <= target
            lo = np.where(live & fits, res, lo)
            hi = np.where(live & ~fits, res, hi)
        if not np.array_equal(res, lo):
            res, st = lo, None
    if st is None:
        st = _simplify_pass(ops, batch, frame_t, res)
    cptr, optr = st["cptr"].cpu().numpy(), st["optr"].cpu().numpy()
    n_cells = int(cptr[-1])
    faces_out = ops.simplify_face_compact(batch.faces, batch.fptr, batch.vptr, st["cell"], int32_table(cptr, dev, what), st["forder"],
                                          st["fflags"], st["frank"], int(optr[-1]))
    runs = torch.arange(n_cells + 1, dtype=torch.int64, device=dev)
    mptr = torch.searchsorted(st["vrank"], runs + 1)
    scc, corder = torch.sort(st["corner_cell"].long(), stable=True)                                # corners by (cell, face, corner)
    kptr = torch.searchsorted(scc, runs)
    cell_key = st["skeys"][mptr[:-1]] if n_cells else st["skeys"][:0]
    pos = ops.simplify_quadrics(batch.verts, batch.vptr, batch.faces, batch.fptr, frame_t, st["res"], st["lo"], st["hi"], cell_key.contiguous(),
                                mptr.contiguous(), st["vorder"].contiguous(), kptr.contiguous(), corder.contiguous())
    vmap = st["cell"].long()
    out = [(pos[cptr[b]:cptr[b + 1]], faces_out[optr[b]:optr[b + 1]], vmap[batch.vptr_host[b]:batch.vptr_host[b + 1]] - int(cptr[b]), int(res[b]))
           for b in range(batch.n)]
    return out, trace


def simplify(verts: Sequence, faces: Sequence, target_faces: int = 3000, resolution=None, return_info: bool = False):
    """Every mesh brought down to at most ``target_faces`` faces by vertex clustering with a regularised quadric representative, where the
    reference calls open3d's ``simplify_quadric_decimation`` (joint2rig.py:317-324). The rule is this product's own (DESIGN.md section
    22); it does NOT reproduce the library's edge collapses, and nobody has measured what its choices -- the regularisation 1e-3, the
    clamp to the cell -- do to skin weights or to the networks' accuracy.

    Per mesh, float64 in a fixed order: the frame is the bounding-box minimum ``lo`` and the largest extent ``ext``; at resolution r a
    vertex lies in cell c = min(floor((p - lo) / ext * r), r - 1) per axis (a vertex on an interior cell plane belongs to the upper
    cell); there is one output vertex per occupied cell, in ascending order of (cx r + cy) r + cz; a face is mapped through the cells
    of its corners, dropped when two corners share a cell, and kept once per vertex SET -- the lowest input face survives, with its
    orientation, rotated so that its smallest index comes first -- in ascending order of the sorted triple. The output vertex is
    cen + solve(M + 1e-3 trace(M) I, b) clamped to the closed cell, cen the mean of the cell's vertices and M = sum n n^T,
    b = sum n (n . (A - cen)) over the corners (face, corner) in the cell, n = (B - A) x (C - A); cen itself where trace(M) is not > 0.

    ``resolution`` None: the r of a mesh is found from ``target_faces``. With n(r) the number of output faces: 1024 if n(1024) <= target,
    else the bisection lo = 1, hi = 1024, mid = (lo + hi) // 2, lo = mid if n(mid) <= target else hi = mid, until hi - lo == 1 -> lo
    (n is not monotone: this procedure is the definition). All meshes of a launch bisect together, one host read per step. A mesh with
    at most ``target_faces`` faces is returned as it is (its vertices and faces, the identity map, resolution 0), as the library call
    does. ``resolution`` an int, or one entry per mesh (None: from the target): that r, 1 .. 1024, whatever the face count.

    -> per mesh (verts float64 [V', 3], faces int64 [F', 3], vertex_map int64 [V], resolution), tensors on the device. ``vertex_map[v]``
    is the output vertex of input vertex v, so per-vertex attributes can be carried across. EVERY occupied cell is an output vertex: an
    input vertex in no face, or one whose faces all collapsed, leaves an output vertex that no output face names -- callers that need a
    vertex list without such vertices filter on ``faces``. ``return_info``: also, per mesh, the bisection trace [(r, n(r)), ...].
    Output vertices are numbered in 21 bits across a launch: the meshes of a call are grouped into launches of at most 2^21 vertices,
    and one mesh above that is a ValueError."""
    target = int(target_faces)
    if target < 0:
        raise ValueError("simplify: target_faces is at least 0")
    given = list(resolution) if isinstance(resolution, (list, tuple, np.ndarray)) else [resolution] * len(verts)
    if len(given) != len(verts):
        raise ValueError("simplify: one resolution per mesh")
    given = [None if g is None else int(g) for g in given]
    for g in given:
        if g is not None and not 1 <= g <= SIMPLIFY_MAX_RES:
            raise ValueError(f"simplify: resolution {g}: supported are 1 .. {SIMPLIFY_MAX_RES}")
    batch = MeshBatch("simplify", verts=verts, faces=faces, check_faces="host")
    out, info = [None] * batch.n, [[] for _ in range(batch.n)]
    groups, size = [], 0
    for b in range(batch.n):
        if given[b] is None and batch.nf[b] <= target:                                             # pass-through
            v0, f0 = int(batch.vptr_host[b]), int(batch.fptr_host[b])
            out[b] = (batch.verts[v0:v0 + batch.nv[b]], batch.faces[f0:f0 + batch.nf[b]].long(),
                      torch.arange(batch.nv[b], dtype=torch.int64, device=batch.device), 0)
            continue
        if batch.nv[b] > SIMPLIFY_MAX_INDEX:
            raise ValueError(f"simplify: mesh {b} has {batch.nv[b]} vertices: output vertices are numbered in 21 bits, "
                             f"at most {SIMPLIFY_MAX_INDEX} vertices per mesh")
        if not groups or size + batch.nv[b] > SIMPLIFY_MAX_INDEX:
            groups.append([])
            size = 0
        groups[-1].append(b)
        size += batch.nv[b]
    ops = get_ops()
    for ids in groups:
        res, trace = _simplify_group(ops, batch.take(ids, "simplify"), target, [given[b] for b in ids], "simplify")
        for b, r, t in zip(ids, res, trace):
            out[b], info[b] = r, t
    return (out, info) if return_info else out


# ------------------------------------------------------------------------------------------------------------------------- diagnosis
REPORT_FIELDS = ("input_verts", "input_faces", "nonfinite_verts", "duplicate_verts", "degenerate_faces", "duplicate_faces", "faces",
                 "zero_area_faces", "verts", "unreferenced_verts", "edges", "boundary_edges", "nonmanifold_edges", "orientation_conflicts",
                 "components", "euler")
ROOT_NONE = (1 << 31) - 1        # morig_meshcheck_comp_counts: the root of a face that is not kept


def _seg_sum(x: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """the sums of the integer (or bool) column ``x`` over the segments of ``ptr`` int64 [B + 1] -> int64 [B], on the device"""
    c = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(x, 0, dtype=torch.int64)])[ptr]
    return c[1:] - c[:-1]


def _component_rounds(ops, rows: torch.Tensor, keys: torch.Tensor, ptr: torch.Tensor, guard: int, what: str):
    """The component rule on the nodes ``rows`` (int32 arange) under the edge ``keys``, ``ptr`` int32 [B + 1] the nodes in front of every
    mesh: all meshes iterate together, one read of the per-mesh ``changed`` words per round -> (labels int32, per mesh the last round
    that moved a label)."""
    B = ptr.numel() - 1
    cur, nxt = rows.clone(), torch.empty_like(rows)
    changed = torch.zeros(B, dtype=torch.int32, device=rows.device)
    last, done = np.zeros(B, dtype=np.int64), 0
    while True:
        ops.meshcheck_cc_round(cur, nxt, keys, ptr, changed)
        done += 1
        moved = changed.cpu().numpy() != 0                                                         # the read of a round
        if rows.numel():
            cur, nxt = nxt, cur
        if not moved.any():
            break
        last[moved] = done
        if done >= guard:
            raise RuntimeError(f"{what}: the component loop passed its bound of {guard} rounds (status {ops.MESHCHECK_ROUND_GUARD})")
    return cur, last


WELD_FIELDS = ("near_verts", "weld_links", "weld_tol", "weld_spread")     # what a report gains with a tolerance


def _weld_tolerance(what: str, n: int, weld: bool, weld_tol, weld_tol_rel, max_links) -> Optional[dict]:
    """The tolerance arguments of ``diagnose`` / ``clean`` / ``repair``, checked before any launch -> None without a tolerance, else
    dict(tol float64 [n], rel, max_links)."""
    if weld_tol is None:
        if weld_tol_rel:
            raise ValueError(f"{what}: weld_tol_rel needs a weld_tol")
        if max_links is not None:
            raise ValueError(f"{what}: max_links needs a weld_tol")
        return None
    if not weld:
        raise ValueError(f"{what}: weld_tol needs weld=True")
    given = list(weld_tol) if isinstance(weld_tol, (list, tuple, np.ndarray)) and np.ndim(weld_tol) else [weld_tol] * n
    if len(given) != n:
        raise ValueError(f"{what}: weld_tol: one tolerance, or one per mesh ({n}), not {len(given)}")
    for b, t in enumerate(given):
        if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not (np.isfinite(t) and t >= 0):
            raise ValueError(f"{what}: weld_tol {t!r} of mesh {b}: a non-negative finite number")
    if max_links is not None and (isinstance(max_links, bool) or not isinstance(max_links, (int, np.integer)) or max_links < 0):
        raise ValueError(f"{what}: max_links {max_links!r}: a number of links")
    return dict(tol=np.array([float(t) for t in given], dtype=np.float64), rel=bool(weld_tol_rel), max_links=max_links)


def _tolerance_weld(ops, batch: MeshBatch, what: str, tol: dict, rows, rep0, nonfinite, vp) -> dict:
    """Steps 2 to 4 of the tolerance rule behind the exact weld ``rep0``: the nodes in their grid cells, sorted
    by (mesh, cell); the links counted, ONE host read (their total against ``max_links``), emitted; the component rounds of
    ``diagnose`` on all rows under the links -> dict(rep: the final representatives, columns: what the report table gains)."""
    dev, B, N = batch.device, batch.n, int(batch.vptr_host[-1])
    eps = tol["tol"]
    if tol["rel"]:                                                                                 # times the diagonal of the finite box
        finite = torch.where((nonfinite != 0).unsqueeze(1), torch.full_like(batch.verts, float("nan")), batch.verts)   # a NaN never enters a box
        box = ops.mesh_bbox(finite.contiguous(), batch.vptr).cpu().numpy()                         # a read: the tolerance is a host value
        ext = box[:, 3:] - box[:, :3]
        ext[~(ext >= 0)] = 0.0                                                                     # a mesh without a finite vertex
        with np.errstate(all="ignore"):                                                            # an overflow is refused just below
            eps = eps * np.sqrt((ext[:, 0] * ext[:, 0] + ext[:, 1] * ext[:, 1]) + ext[:, 2] * ext[:, 2])
        for b in np.nonzero(~np.isfinite(eps))[0]:
            raise ValueError(f"{what}: weld_tol of mesh {b}: the tolerance times the bounding-box diagonal is not finite")
    limit = (1 << 31) - 257 - N                                                                    # the int32 rows of one cc_round launch next to N
    max_links = limit if tol["max_links"] is None else min(int(tol["max_links"]), limit)
    eps_dev, eps2 = torch.from_numpy(eps).to(dev), torch.from_numpy(eps * eps).to(dev)
    ckeys, _ = ops.proxweld_cell_keys(batch.verts, nonfinite, rep0, batch.vptr, eps_dev)
    order = torch.sort(ckeys, stable=True).indices
    if B > 1:                                                                                      # (mesh, key, row): the positions of a mesh are its rows'
        order = order[torch.sort(torch.searchsorted(vp[1:].contiguous(), order, right=True), stable=True).indices]
    order = order.contiguous()
    skeys, spos = ckeys[order].contiguous(), batch.verts[order].contiguous()
    count = ops.proxweld_count_links(skeys, order, spos, batch.vptr, eps2)
    lrank = torch.cumsum(count, 0, dtype=torch.int64)
    per_mesh = _seg_sum(count, vp)
    total = per_mesh.cpu().numpy()                                                                 # THE added read: the links to allocate
    for b in range(B):
        if total[:b + 1].sum() > max_links:
            raise ValueError(f"{what}: weld_tol {float(eps[b])!r} of mesh {b} is too large for this mesh: more than max_links = {max_links} links")
    links = ops.proxweld_emit_links(skeys, order, spos, batch.vptr, eps2, count, lrank, int(total.sum()))
    label, _ = _component_rounds(ops, rows, links, batch.vptr, int(batch.nv.max()) + 2, what)
    rep = label[rep0.long()].contiguous()                                                          # the lowest node of the class: its lowest row
    spread = ops.proxweld_spread(batch.verts, rep, nonfinite, batch.vptr)
    return dict(rep=rep, tol=eps, columns=[_seg_sum((rep0 == rows) & (rep != rows), vp), per_mesh, spread])


def _tolerance_kw(weld_tol, weld_tol_rel, max_links) -> dict:
    """the tolerance keywords that are set: a call without them is the call it always was"""
    kw = dict(weld_tol=weld_tol, weld_tol_rel=weld_tol_rel, max_links=max_links)
    return {k: v for k, v in kw.items() if v is not None and v is not False}


def _topology(ops, batch: MeshBatch, weld: bool, what: str, tol: Optional[dict] = None, blame: Optional[str] = None) -> dict:
    """Steps 1 to 9 of the rule for a packed batch: everything stays on the device but the per-mesh ``changed``
    words of the component rounds (one read per round) and the report table (ONE read, the status word with it). ``tol``: the classes
    of the tolerance weld (section 32) take the place of the exact ones; ``blame``: the public function its errors name."""
    dev, B = batch.device, batch.n
    N, F = int(batch.vptr_host[-1]), int(batch.fptr_host[-1])
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    keys, nonfinite = ops.meshcheck_coord_keys(batch.verts)
    if weld:
        order = torch.arange(N, dtype=torch.int64, device=dev)
        for c in (2, 1, 0):                                                                        # stable: equal rows stay in ascending order
            order = order[torch.sort(keys[c][order], stable=True).indices]
        order = order.contiguous()
        flags = ops.meshcheck_weld_mark(keys, nonfinite, order, batch.vptr)
        rep = ops.meshcheck_run_rep(order, flags, torch.cumsum(flags, 0, dtype=torch.int64))
    else:
        rep = rows
    vp, fp = torch.from_numpy(batch.vptr_host).to(dev), torch.from_numpy(batch.fptr_host).to(dev)
    welded = None
    if tol is not None:
        welded = _tolerance_weld(ops, batch, blame or what, tol, rows, rep, nonfinite, vp)
        rep = welded["rep"]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    tri, major, minor, degenerate = ops.meshcheck_face_keys(batch.faces, batch.fptr, batch.vptr, rep, status)
    by_minor = torch.sort(minor, stable=True).indices
    forder = by_minor[torch.sort(major[by_minor], stable=True).indices].contiguous()              # the lowest input face first among equals
    fflags = ops.meshcheck_face_mark(major, minor, forder)
    surv = ops.meshcheck_run_rep(forder, fflags, torch.cumsum(fflags, 0, dtype=torch.int64), degenerate)
    referenced, zero_area, ekeys = ops.meshcheck_face_edges(batch.verts, tri, surv)
    ekeys = torch.sort(ekeys).values.contiguous()
    label, last = _component_rounds(ops, rows, ekeys, batch.vptr, int(batch.nv.max()) + 2, what)
    eclass, root_boundary = ops.meshcheck_edge_classify(ekeys, label)
    ep = torch.searchsorted(ekeys, vp << 32)                                                       # the first edge key of every mesh
    kept = surv == torch.arange(F, dtype=torch.int32, device=dev)
    is_root = (referenced != 0) & (label == rows)
    col = dict(input_verts=vp[1:] - vp[:-1], input_faces=fp[1:] - fp[:-1], nonfinite_verts=_seg_sum(nonfinite, vp),
               duplicate_verts=_seg_sum(rep != rows, vp), degenerate_faces=_seg_sum(surv < 0, fp), duplicate_faces=_seg_sum((surv >= 0) & ~kept, fp),
               faces=_seg_sum(kept, fp), zero_area_faces=_seg_sum(zero_area, fp), verts=_seg_sum(referenced, vp),
               edges=_seg_sum(eclass > 0, ep), boundary_edges=_seg_sum(eclass == ops.EDGE_BOUNDARY, ep),
               nonmanifold_edges=_seg_sum(eclass == ops.EDGE_NONMANIFOLD, ep), orientation_conflicts=_seg_sum(eclass == ops.EDGE_CONFLICT, ep),
               components=_seg_sum(is_root, vp))
    col["unreferenced_verts"] = col["input_verts"] - col["duplicate_verts"] - col["verts"]
    col["euler"] = col["verts"] - col["edges"] + col["faces"]
    table = torch.stack([col[k] for k in REPORT_FIELDS], 1)
    sent = table if welded is None else torch.cat([table, torch.stack(welded["columns"], 1)], 1)   # the spread travels as its bit pattern
    flat = torch.cat([sent.reshape(-1), status.long()]).cpu().numpy()                              # THE read: the table and the status word
    if flat[-1] & ops.MESHCHECK_BAD_FACE:
        raise bad_face(what)
    table_host = flat[:-1].reshape(B, sent.shape[1])
    reports = []
    for b in range(B):
        r = {k: int(x) for k, x in zip(REPORT_FIELDS, table_host[b])}
        r["watertight"] = bool(r["faces"] > 0 and r["boundary_edges"] == 0 and r["nonmanifold_edges"] == 0 and r["orientation_conflicts"] == 0)
        r["rounds"] = int(last[b]) + 1
        if welded is not None:
            near, n_links, bits = (int(x) for x in table_host[b, len(REPORT_FIELDS):])
            r.update(near_verts=near, weld_links=n_links, weld_tol=float(welded["tol"][b]),
                     weld_spread=math.sqrt(np.array([bits], dtype=np.int64).view(np.float64)[0]))   # the correctly rounded root
        reports.append(r)
    return dict(rows=rows, rep=rep, tri=tri, surv=surv, referenced=referenced, label=label, ekeys=ekeys, eclass=eclass, ep=ep,
                root_boundary=root_boundary, is_root=is_root, vp=vp, fp=fp, table=table, reports=reports, N=N, F=F)


def _component_tables(ops, batch: MeshBatch, st: dict) -> dict:
    """per root (ascending row = ascending mesh, then label): its row, its counts and its area; ``cptr``: the components in front of every mesh"""
    dev = batch.device
    roots = torch.nonzero(st["is_root"]).flatten()                                                 # a size read
    root_verts, root_faces, face_root = ops.meshcheck_comp_counts(st["tri"], st["surv"], st["referenced"], st["label"])
    sroot, order = torch.sort(face_root, stable=True)                                              # the faces of a component in ascending input order
    kptr = torch.searchsorted(sroot, torch.cat([roots, torch.full((1,), ROOT_NONE, dtype=torch.int64, device=dev)])).contiguous()
    area = ops.meshcheck_comp_area(batch.verts, st["tri"], order.contiguous(), kptr)
    cptr = np.concatenate([[0], np.cumsum([r["components"] for r in st["reports"]])]).astype(np.int64)
    return dict(roots=roots, verts=root_verts[roots].long(), faces=root_faces[roots].long(), boundary_edges=st["root_boundary"][roots].long(),
                area=area, cptr=cptr, root_faces=root_faces)


def diagnose(verts: Sequence, faces: Sequence, *, weld: bool = True, return_components: bool = False, weld_tol=None, weld_tol_rel: bool = False,
             max_links: Optional[int] = None) -> List[dict]:
    """The topology report of every mesh by this product's own rule (no parity with open3d, trimesh or MeshLab is
    claimed). Per mesh, integers or float64 in a fixed order:

    1. a vertex with a non-finite coordinate is counted (``nonfinite_verts``), never welds and is otherwise kept;
    2. ``weld``: vertices whose three coordinates are equal as numbers (-0.0 equals +0.0; exact, no tolerance) are one class, its
       representative the lowest input index; ``duplicate_verts`` = V - classes. ``weld=False``: every vertex is its own class;
    3. a face, mapped through the representatives, with two corners in one class is degenerate and dropped (``degenerate_faces``);
    4. among the rest, faces with the same vertex SET are duplicates: the lowest input face survives (``duplicate_faces``);
    5. the survivors are the kept faces (``faces``); ``zero_area_faces`` of them have a normal (B - A) x (C - A) of exactly (0, 0, 0);
    6. a class that a kept face names is referenced (``verts``), the others are ``unreferenced_verts``;
    7. ``edges``: the distinct undirected pairs of the kept faces. With n the kept faces on an edge and f those that traverse it
       low -> high: n = 1 a boundary edge, n >= 3 a non-manifold edge, n = 2 and f != 1 an orientation conflict;
    8. ``components``: the connected components of the referenced classes under those edges;
    9. ``euler`` = verts - edges + faces; ``watertight`` = faces > 0 and no boundary edge, non-manifold edge or orientation conflict.

    -> one dict per mesh: the ``REPORT_FIELDS`` as Python ints, ``watertight`` as a bool and ``rounds``, the rounds of the component rule
    that mesh took (the verifying one included). It describes the mesh that ``clean(keep="all")`` would leave, with the counts of what
    that removes. ``return_components``: also ``component_table`` = dict(root, verts, faces, boundary_edges int64 [C], area float64 [C])
    on the device, components in ascending order of their lowest vertex ``root`` (a face belongs to the component of its first corner;
    the area is summed in the order section 29 states), ``labels`` int64 [V]: per input vertex the lowest vertex of the component of its
    class (its own representative where the class is unreferenced), and ``boundary_edge_list`` int64 [n, 2]: the boundary edges as
    (low, high) representatives, ascending. A face index outside its mesh raises before any launch.

    ``weld_tol``: the TOLERANCE weld, by this product's own rule (no parity with open3d's ``merge_close_vertices``,
    trimesh's ``merge_vertices``, MeshLab or any DCC tool is claimed, and nobody has measured what it does to the networks' accuracy). A
    non-negative finite number, or one per mesh, in the units of the vertices; ``weld_tol_rel=True``: times the diagonal of the mesh's
    bounding box over its finite vertices, the product rounded once on the host. It needs ``weld=True``. Behind step 2: the NODES are
    the exact representatives with three finite coordinates; two nodes of a mesh are linked when (d0 d0 + d1 d1) + d2 d2 <= eps eps (no
    fused multiply-add, not strict, eps eps rounded once on the host; a square below 2^-1022, the smallest normal double -- a tolerance of
    0 or below 1.5e-154 --, links nothing); the classes are the connected
    components of the links together with the exact classes -- SINGLE LINKAGE: a chain of vertices each within the tolerance of the
    next welds into one class however long it is --, the representative is the lowest input index and the class takes ITS coordinates
    (no averaging). So two representatives of different classes are farther apart than the tolerance, and a cleaned mesh cleans to
    itself under the same absolute tolerance. Steps 3 to 9 run on these classes. ``weld_tol=0`` gives the bits of the exact weld. The
    report then gains ``near_verts`` (exact classes - final classes; ``duplicate_verts`` stays V - classes), ``weld_links``, ``weld_tol``
    (the absolute tolerance used, a float) and ``weld_spread``, the largest distance from a vertex to its representative:
    ``weld_spread > weld_tol`` says that chains formed. ``max_links`` bounds the links of a call (default: what one launch of the
    component round takes next to the vertices, 2^31 - 257 - V); above it the call raises ValueError, before anything is emitted: the
    tolerance is too large for this mesh. One host read is added (the number of links)."""
    batch = MeshBatch("diagnose", verts=verts, faces=faces, check_faces="host")
    tol = _weld_tolerance("diagnose", batch.n, bool(weld), weld_tol, weld_tol_rel, max_links)
    if batch.n == 0:
        return []
    ops = get_ops()
    st = _topology(ops, batch, bool(weld), "diagnose", **({} if tol is None else dict(tol=tol)))
    reports = st["reports"]
    if return_components:
        ct = _component_tables(ops, batch, st)
        is_b = st["eclass"] == ops.EDGE_BOUNDARY
        bkeys = st["ekeys"][is_b]
        bp = torch.cat([torch.zeros(1, dtype=torch.int64, device=batch.device), torch.cumsum(is_b, 0, dtype=torch.int64)])[st["ep"]].cpu().numpy()
        for b, r in enumerate(reports):
            c0, c1, v0 = int(ct["cptr"][b]), int(ct["cptr"][b + 1]), int(batch.vptr_host[b])
            r["labels"] = st["label"][st["rep"][v0:int(batch.vptr_host[b + 1])].long()].long() - v0
            r["component_table"] = dict(root=ct["roots"][c0:c1] - v0, verts=ct["verts"][c0:c1], faces=ct["faces"][c0:c1],
                                        boundary_edges=ct["boundary_edges"][c0:c1], area=ct["area"][c0:c1])
            k = bkeys[int(bp[b]):int(bp[b + 1])]
            r["boundary_edge_list"] = torch.stack([(k >> 32) - v0, ((k & 0xffffffff) >> 1) - v0], 1)
    return reports


def clean(verts: Sequence, faces: Sequence, *, weld: bool = True, keep="all", drop_unreferenced: bool = True, return_report: bool = False,
          weld_tol=None, weld_tol_rel: bool = False, max_links: Optional[int] = None, _what: str = "clean"):
    """The lossless cleaning pass of ``diagnose``'s rule (steps 2 to 8): duplicate vertices welded, degenerate and duplicate faces
    dropped, and the components chosen by ``keep``: "all"; "largest": the component with the most faces, ties to the lowest label; an
    int n: the components with at least n faces. -> per mesh (verts float64 [V', 3], faces int64 [F', 3], vertex_map int64 [V],
    face_map int64 [F]) on the device. The kept faces leave in ascending input order, corners unrotated; the output vertices are the
    representatives of the kept referenced classes in ascending input order (``drop_unreferenced=False``: of ALL classes).
    ``vertex_map[v]``: the output vertex of input vertex v, -1 where it is dropped; ``face_map[f]``: the output face of input face f (a
    dropped duplicate: that of its survivor), -1 where the face was degenerate or its component was dropped. Cleaning is idempotent:
    the output cleans to itself with identity maps. ``return_report``: also the ``diagnose`` report of every INPUT mesh.
    ``weld_tol`` / ``weld_tol_rel`` / ``max_links``: the tolerance weld of ``diagnose`` (single linkage; the output vertex of a class has
    the coordinates of its lowest input vertex); idempotent under the same ABSOLUTE tolerance."""
    if isinstance(keep, str):
        if keep not in ("all", "largest"):
            raise ValueError(f'clean: keep {keep!r}: supported are "all", "largest" or a face count')
    elif isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or keep < 0:
        raise ValueError(f'clean: keep {keep!r}: supported are "all", "largest" or a face count')
    batch = MeshBatch("clean", verts=verts, faces=faces, check_faces="host")
    tol = _weld_tolerance(_what, batch.n, bool(weld), weld_tol, weld_tol_rel, max_links)
    if batch.n == 0:
        return ([], []) if return_report else []
    ops, dev = get_ops(), batch.device
    st = _topology(ops, batch, bool(weld), "clean", **({} if tol is None else dict(tol=tol, blame=_what)))
    N, F = st["N"], st["F"]
    if isinstance(keep, str) and keep == "all":
        keep_root = torch.ones(N, dtype=torch.int32, device=dev)
    elif isinstance(keep, str):
        ct = _component_tables(ops, batch, st)
        roots, nfaces = ct["roots"].cpu().numpy(), ct["faces"].cpu().numpy()
        best = [int(roots[c0 + int(np.argmax(nfaces[c0:c1]))]) for c0, c1 in zip(ct["cptr"][:-1], ct["cptr"][1:]) if c1 > c0]   # first maximum: lowest label
        keep_root = torch.zeros(N, dtype=torch.int32, device=dev)
        keep_root[torch.tensor(best, dtype=torch.int64, device=dev)] = 1
    else:
        root_faces = ops.meshcheck_comp_counts(st["tri"], st["surv"], st["referenced"], st["label"])[1]
        keep_root = (root_faces >= int(keep)).to(torch.int32)
    vkeep, fkeep = ops.meshcheck_keep_flags(st["rep"], st["referenced"], st["label"], keep_root, bool(drop_unreferenced), st["tri"], st["surv"])
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    vrank, frank = torch.cumsum(vkeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
    ovptr, ofptr = torch.cat([zero, vrank])[st["vp"]].contiguous(), torch.cat([zero, frank])[st["fp"]].contiguous()
    sizes = torch.cat([ovptr, ofptr]).cpu().numpy()                                                # the size read
    ov, of = sizes[:batch.n + 1], sizes[batch.n + 1:]
    out_v, out_f, vmap, fmap = ops.meshcheck_compact(batch.verts, st["rep"], vkeep, vrank, batch.vptr, ovptr, st["tri"], st["surv"], fkeep, frank,
                                                     batch.fptr, ofptr, int(ov[-1]), int(of[-1]))
    vh, fh = batch.vptr_host, batch.fptr_host
    out = [(out_v[ov[b]:ov[b + 1]], out_f[of[b]:of[b + 1]], vmap[vh[b]:vh[b + 1]], fmap[fh[b]:fh[b + 1]]) for b in range(batch.n)]
    return (out, st["reports"]) if return_report else out


_clean_meshes = clean            # prepare_mesh has an argument of that name


# ------------------------------------------------------------------------------------------------------------------------- fans
SPLIT_FIELDS = ("nonmanifold_edges", "nonmanifold_verts", "fans", "max_fans", "added_verts", "verts", "faces")
SPLIT_MAX_FACES = ((1 << 31) - 257) // 6     # a component round runs over the 3 F corner nodes and the 3 F record slots of a batch


def _split_fans(ops, batch: MeshBatch, what: str):
    """Steps 2 to 4 of ``split_nonmanifold`` for a packed batch of CLEANED meshes: the corner links from the sorted edge records, the
    fans by the component rule of ``diagnose`` on the 3 F corner nodes (one read per round), the lowest fan of every vertex, ONE host read
    (the report columns, the totals that size the outputs and the status word), then the apply launch -> (per mesh (verts, faces,
    source), per mesh the report: ``SPLIT_FIELDS`` and ``split_rounds``)."""
    dev, B = batch.device, batch.n
    N, F = int(batch.vptr_host[-1]), int(batch.fptr_host[-1])
    if F > SPLIT_MAX_FACES:
        raise ValueError(f"{what}: {F} faces in one call: the split supports at most {SPLIT_MAX_FACES}")
    vp, fp = torch.from_numpy(batch.vptr_host).to(dev), torch.from_numpy(batch.fptr_host).to(dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # 2. the corner links
    tri, keys, vals = ops.meshfix_edge_records(batch.faces, batch.fptr, batch.vptr, N, status)
    skeys, rorder = torch.sort(keys, stable=True)                                                  # face-major records: the faces of a run ascend
    skeys, rorder, svals = skeys.contiguous(), rorder.contiguous(), vals[rorder].contiguous()
    links, nm = ops.meshsplit_links(skeys, svals, rorder, F)
    # 3. the fans: the components of the corner nodes under the component rule of ``diagnose``
    nodes = torch.arange(3 * F, dtype=torch.int32, device=dev)
    lab, last = _component_rounds(ops, nodes, links, int32_table(3 * batch.fptr_host, dev, what), 3 * int(batch.nf.max()) + 2, what)
    first, nfans = ops.meshsplit_fans(lab, tri, N)
    # 4. the numbering: a fan that is not the lowest of its vertex is a new vertex, in ascending label
    is_fan = lab == nodes
    new = is_fan & (first[tri.reshape(-1).clamp(min=0).long()] != nodes)
    rank = torch.cumsum(new, 0, dtype=torch.int64)
    np3 = 3 * fp
    aptr = torch.cat([zero, rank])[np3].contiguous()                                               # the new vertices in front of every mesh
    mesh_of_row = torch.searchsorted(vp[1:].contiguous(), torch.arange(N, dtype=torch.int64, device=dev), right=True)
    col = dict(nonmanifold_edges=_seg_sum(nm, torch.searchsorted(skeys, vp << 32)), nonmanifold_verts=_seg_sum(nfans > 1, vp),
               fans=_seg_sum(is_fan, np3), added_verts=aptr[1:] - aptr[:-1], faces=fp[1:] - fp[:-1],
               max_fans=torch.zeros(B, dtype=torch.int64, device=dev).scatter_reduce(0, mesh_of_row, nfans.long(), "amax", include_self=True))
    col["verts"] = vp[1:] - vp[:-1] + col["added_verts"]
    table = torch.stack([col[k] for k in SPLIT_FIELDS], 1)
    flat = torch.cat([table.reshape(-1), status.long()]).cpu().numpy()                             # THE read: the table and the status word
    if flat[-1] & ops.MESHCHECK_BAD_FACE:
        raise bad_face(what)
    table_host = flat[:-1].reshape(B, len(SPLIT_FIELDS))
    ap = np.concatenate([[0], np.cumsum(table_host[:, SPLIT_FIELDS.index("added_verts")])]).astype(np.int64)
    out_faces, source, out_verts = ops.meshsplit_apply(lab, tri, first, rank, batch.fptr, batch.vptr, aptr, batch.verts, N + int(ap[-1]))
    vh, fh = batch.vptr_host, batch.fptr_host
    parts, reports = [], []
    for b in range(B):
        r0, r1 = int(vh[b] + ap[b]), int(vh[b + 1] + ap[b + 1])
        parts.append((out_verts[r0:r1], out_faces[fh[b]:fh[b + 1]], source[r0:r1]))
        r = {k: int(x) for k, x in zip(SPLIT_FIELDS, table_host[b])}
        r["split_rounds"] = int(last[b]) + 1
        reports.append(r)
    return parts, reports


def split_nonmanifold(verts: Sequence, faces: Sequence, *, weld: bool = True, keep="all", return_report: bool = False, weld_tol=None,
                      weld_tol_rel: bool = False, max_links: Optional[int] = None):
    """Non-manifold edges and pinched ("bow-tie") vertices split: every FAN of faces around a vertex gets its own copy of that vertex.
    The rule is this product's own (no parity with open3d, trimesh, MeshLab, CGAL or any DCC tool is claimed, and
    nobody has measured what the split does to the networks' accuracy). Per mesh, integers only:

    1. ``clean(weld=weld, keep=keep, ...)``; everything below works on its output and its two maps are returned as they are;
    2. the corner c of cleaned face f is the node 3 f + c. Two faces f < g ALONE on an edge (lo, hi) link the corner of f at lo with the
       corner of g at lo, and the corner of f at hi with that of g at hi, whichever way they traverse the edge (an orientation conflict
       still links). An edge with one face links nothing; an edge with three or more links nothing and is a ``nonmanifold_edges``;
    3. a FAN is a connected component of the links (``diagnose``'s component rule on the 3 F nodes); all its corners name one vertex, its
       label is its lowest node, so the fans are ordered by lowest face, then corner;
    4. the lowest fan of a vertex keeps that vertex, index unchanged; every other fan gets a new vertex with the same coordinate bits,
       appended after the V' cleaned vertices in ascending fan label. Faces keep their order and their corners; nothing moves. A vertex
       with k fans counts once in ``nonmanifold_verts`` and k - 1 times in ``added_verts``.

    -> per mesh (verts float64 [V'', 3], faces int64 [F', 3], vertex_map int64 [V], face_map int64 [F], source int64 [V'']) on the device;
    ``source`` names the cleaned vertex that every output vertex copies and is the identity on the first V' rows: ``values[source]``
    carries per-vertex attributes up, ``[:V']`` carries them down. ``return_report``: also, per mesh, a dict of Python ints:
    ``SPLIT_FIELDS``, ``split_rounds`` (the rounds of the component rule, the verifying one included) and under ``"input"`` the
    ``diagnose`` report of the input. At most ``SPLIT_MAX_FACES`` faces per call (the component round runs over 3 F nodes and 3 F links).

    After one application every edge has at most two faces, and the faces of every vertex form one path or one cycle, so ``repair``'s
    ``tangled_boundary_edges`` is 0 on every orientable component: inside one fan a face has at most two links at a vertex; a face on an
    edge of three or more faces has lost one of them there, so it is an end of its chain; a chain has two ends, so at most two faces of
    such an edge share both end copies. A second application with ``weld=False`` is the identity.

    THE COPIES COINCIDE. Any later ``diagnose`` / ``clean`` / ``repair`` with the default ``weld=True`` or with a ``weld_tol`` joins them
    again, and so does ``simplify``, whose clustering merges the vertices of one cell: after a split call these with ``weld=False``.

    Not done: the radial pairing of sheets at a non-manifold edge (all its faces come apart unless their fans rejoin them, as two
    tetrahedra on one edge do); anything for non-orientable components (a Moebius strip is returned as it is)."""
    tolerance = _tolerance_kw(weld_tol, weld_tol_rel, max_links)
    if tolerance:                                                                                  # its errors name the function that was called
        _weld_tolerance("split_nonmanifold", len(verts), bool(weld), weld_tol, weld_tol_rel, max_links)
        tolerance["_what"] = "split_nonmanifold"
    cleaned, inputs = clean(verts, faces, weld=weld, keep=keep, return_report=True, **tolerance)
    if not cleaned:
        return ([], []) if return_report else []
    batch = MeshBatch("split_nonmanifold", verts=[c[0] for c in cleaned], faces=[c[1] for c in cleaned])
    parts, reports = _split_fans(get_ops(), batch, "split_nonmanifold")
    out = [(p[0], p[1], c[2], c[3], p[2]) for p, c in zip(parts, cleaned)]
    for r, i in zip(reports, inputs):
        r["input"] = i
    return (out, reports) if return_report else out


_split_meshes = split_nonmanifold    # prepare_mesh has an argument of a like name


# ------------------------------------------------------------------------------------------------------------------------- repair
REPAIR_FIELDS = ("orientation_components", "nonorientable_components", "closed_components", "flipped_faces", "inverted_components",
                 "boundary_loops", "tangled_boundary_edges", "filled_loops", "added_verts", "added_faces")
REPAIR_MAX_FACES = ((1 << 31) - 257) // 8    # a component round runs over the 2 F cover nodes and the 6 F record slots of a batch
LOOP_NONE = (1 << 31) - 1                    # the sort key of a row on no simple loop


def repair(verts: Sequence, faces: Sequence, *, weld: bool = True, keep="all", orient: bool = True, fill_holes=None, return_report: bool = False,
           weld_tol=None, weld_tol_rel: bool = False, max_links: Optional[int] = None, split: bool = False):
    """``clean``, then a consistent orientation per component and a centroid fan over every simple boundary loop, by this product's own
    rule (no parity with open3d, trimesh or MeshLab is claimed, a fan may be non-planar or intersect the mesh, and
    nobody has measured what the repair does to the networks' accuracy). Where the repair is not well defined the case is counted and
    the mesh is left alone. Per mesh, integers or float64 in a fixed order:

    1. ``clean(weld=weld, keep=keep)``; everything below works on its output and its two maps are returned as they are;
    2. ``orient``: two faces alone on an edge are linked, with parity 1 where both traverse it the same way (``diagnose``'s
       orientation conflict); an edge with one face or with three and more links nothing and makes its faces OPEN. The components of
       the links, and every face's parity relative to the lowest face of its component, are the components of the DOUBLE COVER (node
       2 f + sign) under ``diagnose``'s component rule; a component whose two covers meet is not orientable: counted, left alone;
    3. an orientable component without an open face is closed: with S the sum of t = (Ax (By Cz - Bz Cy) + Ay (Bz Cx - Bx Cz)) +
       Az (Bx Cy - By Cx) over its faces, negated at parity 1, S > 0 flips the parity-1 faces and S < 0 the parity-0 faces (outward
       normals). An open component, or S = 0 or NaN: the parity class with fewer faces flips, parity 1 on a tie. A flip exchanges
       corners 1 and 2; face order and corner 0 never change;
    4. every edge with one face is a directed half-edge of its face as it stands after the flips (``orient=False``: as it came). A
       vertex with exactly one half-edge out and one in is regular; a SIMPLE LOOP is a cycle of regular vertices, its label its lowest
       vertex. Half-edges that leave any other boundary vertex, or a chain that runs into one, are ``tangled_boundary_edges``;
    5. ``fill_holes``: None, "all", or an int L >= 3 (simple loops of at most L edges). Per filled loop, in ascending label, one vertex at
       the mean of the loop's vertices is appended after the cleaned vertices, and per half-edge from -> to the face (to, from, new
       vertex) after the cleaned faces, in ascending ``from``.

    -> per mesh (verts float64 [V', 3], faces int64 [F', 3], vertex_map int64 [V], face_map int64 [F], flipped bool [F']), tensors on the
    device; ``flipped`` is False on the appended faces. ``return_report``: also, per mesh, a dict of Python ints: ``REPAIR_FIELDS``,
    ``orient_rounds`` (the rounds of the component rule on the cover, the verifying one included; 0 with ``orient=False``) and under
    ``"input"`` the ``diagnose`` report of the input mesh. A repaired mesh repairs to itself (nothing flips, nothing is added, identity
    maps) unless a fill closed a component that the majority had left facing inward: closed, it is judged by its volume.
    ``weld_tol`` / ``weld_tol_rel`` / ``max_links`` go to the ``clean`` of step 1 (the tolerance weld of ``diagnose``).

    ``split=True``: steps 2 to 4 of ``split_nonmanifold`` run between step 1 and step 2, so steps 2 to 5 see the split mesh: two closed
    parts on one edge are closed components judged by their volume, and a hole that touches another at one vertex is a simple loop and
    is fanned. The fill vertices come after the split vertices. The tuple gains a sixth element ``source`` int64 [V'']: the cleaned
    vertex that every output vertex copies, -1 on a fill centroid; the report gains under ``"split"`` the ``SPLIT_FIELDS`` and
    ``split_rounds`` (a dict of its own: ``added_verts`` is a field of both). The face limit is the smaller of the two. The copies
    coincide: repair the result again only with ``weld=False``. ``split=False``: exactly the launches, the tuple and the keys without it."""
    if fill_holes is not None and not (isinstance(fill_holes, str) and fill_holes == "all"):
        if isinstance(fill_holes, (str, bool)) or not isinstance(fill_holes, (int, np.integer)) or fill_holes < 3:
            raise ValueError(f'repair: fill_holes {fill_holes!r}: supported are None, "all" or a loop length of at least 3')
    tolerance = _tolerance_kw(weld_tol, weld_tol_rel, max_links)
    if tolerance:                                                                                  # its errors name the function that was called
        _weld_tolerance("repair", len(verts), bool(weld), weld_tol, weld_tol_rel, max_links)
        tolerance["_what"] = "repair"
    cleaned, inputs = clean(verts, faces, weld=weld, keep=keep, return_report=True, **tolerance)
    if not cleaned:
        return ([], []) if return_report else []
    batch = MeshBatch("repair", verts=[c[0] for c in cleaned], faces=[c[1] for c in cleaned])
    ops, dev, B = get_ops(), batch.device, batch.n
    N, F = int(batch.vptr_host[-1]), int(batch.fptr_host[-1])
    if F > REPAIR_MAX_FACES:
        raise ValueError(f"repair: {F} faces in one call: supported are at most {REPAIR_MAX_FACES}")
    parts = None
    if split:                                                                                      # REPAIR_MAX_FACES is the smaller limit
        parts, split_reports = _split_fans(ops, batch, "repair")
        batch = MeshBatch("repair", verts=[p[0] for p in parts], faces=[p[1] for p in parts])
        N = int(batch.vptr_host[-1])
    i32 = lambda n, fill=None: (torch.empty(n, dtype=torch.int32, device=dev) if fill is None else torch.full((n,), fill, dtype=torch.int32, device=dev))
    vp, fp = torch.from_numpy(batch.vptr_host).to(dev), torch.from_numpy(batch.fptr_host).to(dev)
    none = torch.zeros(B, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # 2. the edge runs
    tri, keys, vals = ops.meshfix_edge_records(batch.faces, batch.fptr, batch.vptr, N, status)
    skeys, rorder = torch.sort(keys, stable=True)                                                  # face-major records: the faces of a run ascend
    skeys, svals = skeys.contiguous(), vals[rorder].contiguous()
    cover, face_open, bflag = ops.meshfix_links(skeys, svals, F)
    col = {k: none for k in REPAIR_FIELDS}
    rounds = np.zeros(B, dtype=np.int64)
    if orient:
        # the double cover under the component rule of ``diagnose``, then 3. which way
        nodes = torch.arange(2 * F, dtype=torch.int32, device=dev)
        lab, last = _component_rounds(ops, nodes, cover, int32_table(2 * batch.fptr_host, dev, "repair"), 2 * int(batch.nf.max()) + 2, "repair")
        rounds = last + 1
        root, parity, face_root, root_open = ops.meshfix_orient_stats(lab, face_open)
        roots = torch.nonzero(root == torch.arange(F, dtype=torch.int32, device=dev)).flatten()     # a size read
        forder = torch.sort(face_root, stable=True).indices.contiguous()                           # the faces of a component in ascending order
        kptr = torch.searchsorted(face_root[forder], torch.cat([roots, torch.full((1,), F, dtype=torch.int64, device=dev)])).contiguous()
        vol, cnt, cnt1 = ops.meshfix_signed_volume(batch.verts, tri, parity, forder, kptr, roots.contiguous())
        out_faces, flipped, info = ops.meshfix_orient_apply(tri, batch.fptr, batch.vptr, lab, root, parity, root_open, vol, cnt, cnt1)
        col.update(orientation_components=_seg_sum(info != 0, fp), nonorientable_components=_seg_sum((info & ops.MESHFIX_NONORIENTABLE) != 0, fp),
                   closed_components=_seg_sum((info & ops.MESHFIX_CLOSED) != 0, fp), flipped_faces=_seg_sum(flipped, fp),
                   inverted_components=_seg_sum((info & ops.MESHFIX_INVERTED) != 0, fp))
    else:
        out_faces, flipped = batch.faces.long(), i32(F, 0)
    # 4. the boundary loops: a fixed number of doubling rounds, no host read
    hfrom, hto, nxt0, lab0, vclass = ops.meshfix_boundary_init(skeys, svals, bflag, flipped, N)
    widest = int(batch.nv.max())
    state, spare = (lab0, nxt0), [(i32(N), i32(N)), (i32(N), i32(N))]
    for r in range((widest - 1).bit_length() + 1 if widest else 0):                                # ceil(log2(max nv)) + 1
        ops.meshfix_loop_round(*state, *spare[r % 2])
        state = spare[r % 2]
    llab = state[0]
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    on_loop = (vclass == ops.MESHFIX_REGULAR) & (llab >= 0)
    loop_root = on_loop & (llab == rows)
    tangled = (hfrom >= 0) & (llab[hfrom.clamp(min=0).long()] < 0)
    col.update(boundary_loops=_seg_sum(loop_root, vp), tangled_boundary_edges=_seg_sum(tangled, torch.searchsorted(skeys, vp << 32)))
    # 5. the fill
    centroid = new_faces = None
    if fill_holes is not None and N:
        labels = torch.nonzero(loop_root).flatten()                                                # a size read
        skey, vorder = torch.sort(torch.where(on_loop, llab.long(), LOOP_NONE), stable=True)       # the rows of a loop in ascending order
        lptr = torch.searchsorted(skey, torch.cat([labels, torch.full((1,), LOOP_NONE, dtype=torch.int64, device=dev)])).contiguous()
        if isinstance(fill_holes, str):
            sel = torch.arange(labels.numel(), dtype=torch.int64, device=dev)
        else:
            sel = torch.nonzero(lptr[1:] - lptr[:-1] <= int(fill_holes)).flatten()                 # a size read
        chosen = labels[sel]
        slot = i32(N, -1)
        slot[chosen] = torch.arange(chosen.numel(), dtype=torch.int32, device=dev)
        centroid = ops.meshfix_loop_centroid(batch.verts, vorder.contiguous(), lptr, sel.contiguous())
        emit = ops.meshfix_fill_mark(vclass, llab, slot)
        erank = torch.cumsum(emit, 0, dtype=torch.int64)
        sptr = torch.searchsorted(chosen, vp).contiguous()                                         # the filled loops in front of every mesh
        new_faces = ops.meshfix_fill_emit(nxt0, emit, erank, llab, slot, batch.vptr, sptr, int(erank[-1]))   # a size read
        col.update(filled_loops=sptr[1:] - sptr[:-1], added_verts=sptr[1:] - sptr[:-1], added_faces=_seg_sum(emit, vp))
    table = torch.stack([col[k] for k in REPAIR_FIELDS], 1)
    flat = torch.cat([table.reshape(-1), status.long()]).cpu().numpy()                             # THE read: the table and the status word
    if flat[-1] & ops.MESHCHECK_BAD_FACE:
        raise bad_face("repair")
    table_host = flat[:-1].reshape(B, len(REPAIR_FIELDS))
    vh, fh = batch.vptr_host, batch.fptr_host
    sp = np.concatenate([[0], np.cumsum(table_host[:, REPAIR_FIELDS.index("added_verts")])])
    ap = np.concatenate([[0], np.cumsum(table_host[:, REPAIR_FIELDS.index("added_faces")])])
    out, reports = [], []
    for b in range(B):
        v, f, fl = batch.verts[vh[b]:vh[b + 1]], out_faces[fh[b]:fh[b + 1]], flipped[fh[b]:fh[b + 1]].bool()
        if sp[b + 1] > sp[b]:
            v = torch.cat([v, centroid[sp[b]:sp[b + 1]]], 0)
            f = torch.cat([f, new_faces[ap[b]:ap[b + 1]]], 0)
            fl = torch.cat([fl, torch.zeros(int(ap[b + 1] - ap[b]), dtype=torch.bool, device=dev)])
        if parts is None:
            out.append((v, f, cleaned[b][2], cleaned[b][3], fl))
        else:
            src = torch.cat([parts[b][2], torch.full((int(sp[b + 1] - sp[b]),), -1, dtype=torch.int64, device=dev)])
            out.append((v, f, cleaned[b][2], cleaned[b][3], fl, src))
        r = {k: int(x) for k, x in zip(REPAIR_FIELDS, table_host[b])}
        r["orient_rounds"] = int(rounds[b])
        if parts is not None:
            r["split"] = split_reports[b]
        r["input"] = inputs[b]
        reports.append(r)
    return (out, reports) if return_report else out


_repair_meshes = repair          # prepare_mesh has an argument of that name


# ------------------------------------------------------------------------------------------------------------------------- refine
REFINE_FIELDS = ("passes", "edges_split", "faces_kept", "faces_split_1", "faces_split_2", "faces_split_3", "degenerate_kept", "stalled", "converged",
                 "verts", "faces")
REFINE_MAX_FACES = ((1 << 31) - 257) // 3    # the three edge records of every face are rows of one sort
INT64_MAX = (1 << 63) - 1


def refine(verts, faces, *, max_edge=None, min_verts=None, max_passes: int = 32, return_report: bool = False):
    """Coarse meshes brought UP to a density by edge splits, by this product's own rule (no parity with open3d's
    ``subdivide_midpoint`` / ``subdivide_loop``, with MeshLab or with any DCC tool is claimed, no position is smoothed, and nobody has
    measured what refinement does to the networks' accuracy). ``verts`` / ``faces``: lists with one entry per mesh, or the arrays of
    one mesh. At least one of ``max_edge`` (a length) and ``min_verts`` (a vertex count) is given. Per mesh, float64 in a fixed order:

    1. a pass looks at the undirected edges (lo, hi) of the faces that name three different vertices; the squared length of an edge is
       (d0 d0 + d1 d1) + d2 d2, d = v[hi] - v[lo], without a fused multiply-add. Every face on an edge sees the same decision, so the
       result has no cracks, a fan of any number of faces on one edge included;
    2. ``max_edge`` = L: an edge is marked when its squared length is finite and > L L (strict). Passes repeat until one marks nothing;
    3. ``min_verts`` = N, after 2. where both are given and while the mesh has fewer than N vertices: marked are the edges with a finite
       squared length > 0.25 (the largest finite squared length of the mesh), of these only the N - V longest where there are more (by
       length descending, then key ascending): the mesh ends with exactly N vertices. A mesh without a positive finite edge is ``stalled``;
    4. a marked edge gets the vertex 0.5 (v[lo] + v[hi]), numbered V + (its rank among the marked edges of the mesh in key order);
    5. a face is replaced, winding kept, by: no marked edge: itself; three: the corner triangles at corners 0, 1, 2, then the centre; one:
       the two triangles on the median, listed from the marked edge's first corner; two: the corner triangle at their apex, then the quad
       cut by its shorter diagonal (squared lengths on the new positions; a tie goes to the diagonal through the lower old vertex);
    6. a face that names a vertex twice is copied as it is (``degenerate_kept``) and takes part in nothing; a face that names a vertex
       outside its mesh raises ValueError;
    7. ``max_passes`` caps the passes of a mesh. It is a safety cap: a mesh stopped by it is reported ``converged=False``, also where
       one more look would have found nothing to mark.

    -> per mesh (verts float64 [V', 3], faces int64 [F', 3], parents int64 [V', 2], face_map int64 [F']) on the device. The input
    vertices are the first V rows, so a result on the refined mesh restricts to the input by ``[:V]``. ``parents[v]`` = (v, v) there;
    for a new vertex the two ends of the edge it halves, both lower rows (``interpolate`` carries per-vertex values up along them).
    ``face_map``: the input face of every output face; children are contiguous and in input order, so it is non-decreasing.
    ``return_report``: also, per mesh, a dict of the ``REFINE_FIELDS``: Python ints, ``edges_split`` a list with one entry per pass,
    ``faces_kept`` / ``faces_split_k`` the faces of its passes by their number of marked edges, ``stalled`` / ``converged`` bools,
    ``degenerate_kept`` as the first look at the mesh saw it (0 for a mesh that was never looked at). All meshes of a call pass together
    with ONE host read per pass (the sizes to allocate); a mesh alone gives the bits it gives in a batch, two runs give the same bits."""
    single = not isinstance(verts, (list, tuple))
    if single:
        verts, faces = [verts], [faces]
    if max_edge is None and min_verts is None:
        raise ValueError("refine: give max_edge, min_verts or both")
    if max_edge is not None:
        if isinstance(max_edge, bool) or not isinstance(max_edge, (int, float, np.integer, np.floating)) or not (np.isfinite(max_edge) and max_edge > 0):
            raise ValueError(f"refine: max_edge {max_edge!r}: a positive finite length")
    if min_verts is not None and (isinstance(min_verts, bool) or not isinstance(min_verts, (int, np.integer)) or min_verts < 0):
        raise ValueError(f"refine: min_verts {min_verts!r}: a vertex count")
    if isinstance(max_passes, bool) or not isinstance(max_passes, (int, np.integer)) or max_passes < 0:
        raise ValueError(f"refine: max_passes {max_passes!r}: a number of passes")
    batch = MeshBatch("refine", verts=verts, faces=faces)
    B = batch.n
    if B == 0:
        return ([], []) if return_report else []
    ops, dev = get_ops(), batch.device
    limit2 = float(max_edge) * float(max_edge) if max_edge is not None else 0.0
    nv, nf = batch.nv.copy(), batch.nf.copy()
    local = lambda ptr, n: torch.arange(int(ptr[-1]), dtype=torch.int64, device=dev) - torch.repeat_interleave(
        torch.from_numpy(ptr[:-1]).to(dev), torch.from_numpy(n).to(dev), output_size=int(ptr[-1]))
    v, f = batch.verts, batch.faces
    parents = local(batch.vptr_host, nv).unsqueeze(1).repeat(1, 2).contiguous()
    face_map = local(batch.fptr_host, nf)
    phase = np.full(B, ops.REFINE_LENGTH if max_edge is not None else ops.REFINE_LONGEST, dtype=np.int32)
    reports = [dict(passes=0, edges_split=[], faces_kept=0, faces_split_1=0, faces_split_2=0, faces_split_3=0, degenerate_kept=0, stalled=False,
                    converged=False) for _ in range(B)]
    looked = np.zeros(B, dtype=bool)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    while True:
        for b in range(B):                                                                         # what needs no look at the mesh
            if phase[b] == ops.REFINE_LONGEST and nv[b] >= min_verts:
                phase[b], reports[b]["converged"] = ops.REFINE_IDLE, True
            if phase[b] != ops.REFINE_IDLE and reports[b]["passes"] >= max_passes:
                phase[b] = ops.REFINE_IDLE
        if not phase.any():
            break
        vh, fh = ptr_of(nv), ptr_of(nf)
        N, F = int(vh[-1]), int(fh[-1])
        if F > REFINE_MAX_FACES:
            raise ValueError(f"refine: {F} faces in one pass: supported are at most {REFINE_MAX_FACES}")
        vptr, fptr = int32_table(vh, dev, "refine"), int32_table(fh, dev, "refine")
        vp, fp = torch.from_numpy(vh).to(dev), torch.from_numpy(fh).to(dev)
        keys, len2, maxbits, degenerate = ops.refine_edge_records(v, f, fptr, vptr, status)
        skeys, order = torch.sort(keys, stable=True)
        skeys, order = skeys.contiguous(), order.contiguous()
        flags = ops.tpl_edge_flags(skeys)
        mark, image = ops.refine_mark(skeys, order, flags, len2, vptr, torch.from_numpy(phase).to(dev), limit2, maxbits)
        rptr = torch.searchsorted(skeys, vp << 32).contiguous()                                    # the first record of every mesh
        counting = phase == ops.REFINE_LONGEST
        if counting.any():                                                                         # the budget: (mesh, length descending, key)
            by_len = torch.sort(image, descending=True, stable=True).indices
            mesh = torch.searchsorted(rptr[1:].contiguous(), by_len, right=True)
            perm = by_len[torch.sort(mesh, stable=True).indices].contiguous()
            budget = np.where(counting, (min_verts if min_verts is not None else 0) - nv, INT64_MAX).astype(np.int64)
            ops.refine_budget(perm, rptr, torch.from_numpy(budget).to(dev), mark)
        erank = torch.cumsum(mark, 0, dtype=torch.int64)
        mptr = torch.cat([zero, erank])[rptr].contiguous()                                         # the marked edges in front of every mesh
        edge_mid = ops.refine_number(skeys, order, mark, erank, vptr, mptr)
        nchild, pattern = ops.refine_pattern(edge_mid, degenerate)
        crank = torch.cumsum(nchild, 0, dtype=torch.int64)
        table = torch.stack([mptr[1:] - mptr[:-1], _seg_sum(nchild, fp)] + [_seg_sum(pattern == k, fp) for k in range(4)] + [_seg_sum(degenerate, fp)], 1)
        flat = torch.cat([table.reshape(-1), status.long()]).cpu().numpy()                         # THE read of the pass: sizes and status
        if flat[-1] & ops.MESHCHECK_BAD_FACE:
            raise bad_face("refine")
        table_host = flat[:-1].reshape(B, 7)
        marked = table_host[:, 0]
        for b in np.nonzero(phase)[0]:
            r = reports[b]
            if not looked[b]:
                looked[b], r["degenerate_kept"] = True, int(table_host[b, 6])
            if marked[b] == 0:
                if phase[b] == ops.REFINE_LENGTH and min_verts is not None and nv[b] < min_verts:
                    phase[b] = ops.REFINE_LONGEST
                else:
                    r["stalled" if phase[b] == ops.REFINE_LONGEST else "converged"] = True
                    phase[b] = ops.REFINE_IDLE
                continue
            r["passes"] += 1
            r["edges_split"].append(int(marked[b]))
            for k, name in enumerate(("faces_kept", "faces_split_1", "faces_split_2", "faces_split_3")):
                r[name] += int(table_host[b, 2 + k])
        if not marked.any():
            continue
        v, parents, f, face_map = ops.refine_emit(v, parents, f, face_map, edge_mid, crank, fptr, vptr, mptr, skeys, mark, erank, N + int(marked.sum()),
                                                  int(table_host[:, 1].sum()))
        nv, nf = nv + marked, table_host[:, 1].copy()
    vh, fh = ptr_of(nv), ptr_of(nf)
    out = [(v[vh[b]:vh[b + 1]], f[fh[b]:fh[b + 1]].long(), parents[vh[b]:vh[b + 1]], face_map[fh[b]:fh[b + 1]]) for b in range(B)]
    for b, r in enumerate(reports):
        r.update(verts=int(nv[b]), faces=int(nf[b]))
    if single:
        return (out[0], reports[0]) if return_report else out[0]
    return (out, reports) if return_report else out


def interpolate(values, parents):
    """Per-vertex values carried UP a refinement: ``values`` [V, ...] float32 or float64 of the input vertices and the ``parents`` int64
    [V', 2] of ``refine`` -> [V', ...] in the dtype of ``values``: the first V rows as they are, a new row 0.5 * (x[p0] + x[p1]) per
    element in that dtype. Skin weights, ``vtx_traj`` [V, T, 3] clips and soft labels go up this way; ``[:V]`` carries a result down.
    Lists (one entry per mesh) or one mesh. The parents of a vertex are lower rows made in earlier passes, so the rows of one pass are
    one launch; the pass boundaries are found from ``parents`` with one host read."""
    if isinstance(values, (list, tuple)):
        if not isinstance(parents, (list, tuple)) or len(parents) != len(values):
            raise ValueError("interpolate: one parents array per mesh")
        return [interpolate(x, p) for x, p in zip(values, parents)]
    x, p = as_tensor(values), as_tensor(parents)
    if x.dtype not in (torch.float32, torch.float64) or x.dim() < 1:
        raise ValueError("interpolate: values are float32 or float64 [V, ...]")
    if p.dim() != 2 or p.shape[1] != 2 or p.is_floating_point() or p.shape[0] < x.shape[0]:
        raise ValueError("interpolate: parents are integer [V', 2] with V' >= V")
    dev = device_of(x, p)
    V, W = x.shape[0], p.shape[0]
    out = torch.empty((W,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
    out[:V] = x.to(dev)
    if W == V or out.numel() == 0:
        return out
    p = p.to(device=dev, dtype=torch.int64).contiguous()
    born = p[V:]
    top = torch.cummax(born.max(1).values, 0).values
    own = torch.arange(V, W, dtype=torch.int64, device=dev)
    bad = ((born.min(1).values < 0) | (born.max(1).values >= own)).any()
    host = torch.cat([top, bad.long().reshape(1)]).cpu().numpy()                                   # the read: where every pass begins
    if host[-1]:
        raise ValueError("interpolate: a parent is not a lower vertex")
    ops, flat, row = get_ops(), out.reshape(W, -1), V
    while row < W:
        end = V + int(np.searchsorted(host[:-1], row, side="left"))                               # the first row with a parent at or past ``row``
        ops.refine_interpolate(flat, p, row, end)
        row = end
    return out


_refine_meshes = refine          # prepare_mesh has arguments of that name


# ------------------------------------------------------------------------------------------------------------------------- all of it
def prepare_mesh(verts, faces, *, radius: float = 0.06, max_nn: int = 15, seed: int = 0, n_samples: int = 4000, oversample: int = 5,
                 dims: int = 88, self_loops: bool = True, simplify_to: Optional[int] = None, clean: bool = False, repair: bool = False,
                 refine_max_edge: Optional[float] = None, refine_min_verts: Optional[int] = None, weld_tol=None, weld_tol_rel: bool = False, split: bool = False):
    """From raw meshes to the inputs of every stage: ``normalize``, ``tpl_edges``, ``sample_surface``,
    geodesic.surface_geodesic_batched, the geodesic ball graph of graph_build (``radius``, ``max_nn``, ``seed``: get_geo_edges of the
    reference) and ``voxelize``, each on the normalised vertices and each one batch. ``verts`` / ``faces``: lists with one entry per
    mesh (-> a list of dicts), or the arrays of one mesh (-> one dict). Per mesh: dict(verts float64 [V, 3], pivot, scale,
    tpl_edge_index, geo_edge_index int64 [2, E] -- with the datasets' self loops unless ``self_loops`` is False --, vox formats.Voxels,
    samples, normals float64 [n_samples, 3]). ``simplify_to``: a face target -- every mesh goes through ``simplify`` after ``normalize``
    (the frame stays that of the full mesh), every later stage runs on the simplified mesh, ``verts`` are its vertices and the dict also
    carries ``faces`` int64 [F', 3] and ``vertex_map`` int64 [V]. None: no simplification, the dict above. ``clean``: every mesh goes through
    ``clean`` (its defaults) BEFORE ``normalize``, every later stage runs on the cleaned mesh, and the dict also carries ``faces``, ``report``
    (the ``diagnose`` report of the input mesh) and ``vertex_map``, from input vertex to final vertex (-1: dropped), composed with that of
    ``simplify_to`` where both are asked for. False: exactly the launches made without the argument. ``repair``: ``repair(fill_holes="all")``
    takes the place of the ``clean`` step (which it contains): the later stages run on the oriented, filled mesh -- the voxel grid of a
    mesh whose only holes were simple loops is solid, the sample normals of a closed component point outward --, ``report`` is the
    repair report (the ``diagnose`` report of the input under ``"input"``) and the dict also carries ``flipped`` bool [F'], per face
    of the repaired mesh (in front of ``simplify_to``). False: exactly the launches made without the argument. ``refine_max_edge`` /
    ``refine_min_verts``: every mesh goes through ``refine(max_edge=, min_verts=)`` after ``normalize`` (lengths are in the networks' frame:
    ``refine_max_edge=0.06`` is the radius of the ball graph; the frame stays that of the input mesh) and after ``simplify_to`` where both
    are asked for; every later stage runs on the refined mesh, whose first vertices are those in front of the refinement, and the dict
    also carries ``faces``, ``parents`` int64 [V', 2], ``face_map`` int64 [F'] (the face in front of the refinement) and ``vertex_map``
    (that of ``clean`` / ``repair`` / ``simplify_to``, the identity without them: refinement moves no vertex). Both None: exactly the
    launches made without the arguments. ``weld_tol`` / ``weld_tol_rel``: the tolerance weld of ``diagnose``, handed to the ``clean`` /
    ``repair`` step (ValueError where neither is asked for). That step runs BEFORE ``normalize``, so an absolute tolerance is in the
    asset's own units, not in the networks' frame; None: exactly the calls made without the arguments. ``split``: non-manifold edges and
    pinched vertices are split (``split_nonmanifold``) inside that step: with ``repair`` it is handed on as ``repair(split=True)``, with
    ``clean`` the function ``split_nonmanifold`` takes the place of the clean step and ``report`` is its report (ValueError where neither
    is asked for); the dict also carries ``source`` int64 [V''], the cleaned vertex that every vertex of the step's output copies (-1 on a
    fill centroid), and ``vertex_map`` composes as without it. The copies of a split vertex coincide: ``simplify_to`` behind it merges
    copies that fall in one cell. False: exactly the calls made without the argument."""
    from . import geodesic, graph_build
    single = not isinstance(verts, (list, tuple))
    if single:
        verts, faces = [verts], [faces]
    cleaned = None
    tolerance = _tolerance_kw(weld_tol, weld_tol_rel, None)
    if tolerance and not (repair or clean):
        raise ValueError("prepare_mesh: weld_tol belongs to the clean / repair step: ask for clean=True or repair=True")
    if split and not (repair or clean):
        raise ValueError("prepare_mesh: split belongs to the clean / repair step: ask for clean=True or repair=True")
    if repair:
        cleaned, reports = _repair_meshes(verts, faces, fill_holes="all", return_report=True, **tolerance, **(dict(split=True) if split else {}))
        verts, faces = [c[0] for c in cleaned], [c[1] for c in cleaned]
    elif clean:
        cleaned, reports = (_split_meshes if split else _clean_meshes)(verts, faces, return_report=True, **tolerance)
        verts, faces = [c[0] for c in cleaned], [c[1] for c in cleaned]
    normed = normalize(verts)
    nverts = [v for v, _, _ in normed]
    simple = None
    if simplify_to is not None:
        simple = simplify(nverts, faces, target_faces=simplify_to)
        nverts, faces = [s[0] for s in simple], [s[1] for s in simple]
    refined = None
    if refine_max_edge is not None or refine_min_verts is not None:
        before = [v.shape[0] for v in nverts]
        refined = _refine_meshes(list(nverts), list(faces), max_edge=refine_max_edge, min_verts=refine_min_verts)
        nverts, faces = [r[0] for r in refined], [r[1] for r in refined]
    tpl = tpl_edges(faces, [v.shape[0] for v in nverts], self_loops=self_loops)
    pts, normals = sample_surface(nverts, faces, n_samples=n_samples, oversample=oversample, seed=seed)
    dist = geodesic.surface_geodesic_batched(nverts, pts, normals)
    geo = [graph_build.get_geo_edges_from_distance(d, radius, max_nn, seed, self_loops) for d in dist]
    vox = voxelize(nverts, faces, dims=dims)
    out = [dict(verts=nverts[b], pivot=normed[b][1], scale=normed[b][2], tpl_edge_index=tpl[b], geo_edge_index=geo[b], vox=vox[b],
                samples=pts[b], normals=normals[b]) for b in range(len(nverts))]
    if simple is not None:
        for d, s in zip(out, simple):
            d.update(faces=s[1], vertex_map=s[2])
    if cleaned is not None:
        for d, c, r, f in zip(out, cleaned, reports, faces):
            vm = c[2]
            if simple is not None:                                                                 # input vertex -> cleaned -> simplified; -1 stays
                vm = torch.where(vm >= 0, d["vertex_map"][vm.clamp(min=0)], vm)
            d.update(faces=f, report=r, vertex_map=vm)
            if repair:
                d.update(flipped=c[4])
            if split:
                d.update(source=c[5] if repair else c[4])
    if refined is not None:
        for d, r, n in zip(out, refined, before):
            d.update(faces=r[1], parents=r[2], face_map=r[3])
            d.setdefault("vertex_map", torch.arange(n, dtype=torch.int64, device=r[0].device))
    return out[0] if single else out
