"""Fixtures of the mesh front end (tests/golden/meshprep_*.npz), made by the reference's own functions. Nothing of the reference is
written into the repository: only inputs, results and the reference's seconds.

  * data_proc.common_ops.normalize and get_tpl_edges, imported with open3d / cv2 / tqdm stubbed (open3d.utility.Vector3dVector is the
    identity) and a duck-typed mesh that has ``vertices``.
  * utils.binvox_rw.write and read_as_3d_array(fix_coords=True) on a Voxels object of the reference's own class.

Cases:
  meshprep_normalize   a rotated, shifted 24 x 24 torus and a random cloud; also one run with a given pivot and scale
  meshprep_tpl_edges   a cube, the 24 x 24 torus, and a mesh with an isolated vertex, a face (a, a, b), a duplicate face and a fan vertex;
                       ref_seconds of get_tpl_edges on the 64 x 64 torus (4096 vertices, 8192 faces), whose edges are not stored
  meshprep_binvox      the oracle's 88^3 solid torus, and a crafted 16^3 grid with runs of exactly 255, 510 and 256 voxels (the
                       reference writes a pair of count 0 after a run that is a multiple of 255) that ends on a run of 255

Run from the repository root:  python tools/make_meshprep_golden.py
"""
import io
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim              # noqa: E402
import meshprep_oracle as mo         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _reference():
    sys.path.insert(0, shim.REFERENCE_ROOT)
    for name in ("open3d", "cv2", "tqdm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["open3d"].utility = types.SimpleNamespace(Vector3dVector=lambda a: a)
    if not hasattr(np, "int"):
        np.int = int
    if not hasattr(np, "bool"):
        np.bool = bool
    co = __import__("data_proc.common_ops", fromlist=["normalize"])
    rw = __import__("utils.binvox_rw", fromlist=["write"])
    return co, rw


class DuckMesh:
    def __init__(self, verts):
        self.vertices = verts


def save(name, meta, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrs)
    size = os.path.getsize(path)
    assert size <= 1 << 20, (path, size)
    print(f"  {name}: {size} bytes")


def normalize_case(co):
    rng = np.random.default_rng(0x6E6F726D)
    tv, _ = mo.torus(24)
    a = tv @ mo.rotation(rng).T * 3.7 + [12.5, -3.25, 0.875]
    b = rng.normal(size=(1000, 3)) * [0.3, 2.0, 0.7] + [-4.0, 9.0, 1e-3]
    arrs, meta = {}, dict(case="meshprep_normalize", meshes=2)
    for k, v in enumerate((a, b)):
        mesh, pivot, scale = co.normalize(DuckMesh(v.copy()))
        arrs.update({f"in{k}": v, f"out{k}": np.asarray(mesh.vertices), f"pivot{k}": np.asarray(pivot, dtype=np.float64), f"scale{k}": np.float64(scale)})
    given_pivot, given_scale = np.array([0.5, -1.0, 2.0]), 0.3125
    mesh, pivot, scale = co.normalize(DuckMesh(a.copy()), pivot=given_pivot, scale=given_scale)
    assert scale == given_scale and np.array_equal(pivot, given_pivot)
    arrs.update(given_pivot=given_pivot, given_scale=np.float64(given_scale), out_given=np.asarray(mesh.vertices))
    save("meshprep_normalize", meta, **arrs)


def odd_mesh():
    """12 vertices: vertex 7 is in no face; a face (3, 3, 4); the face (0, 1, 2) twice, once rotated; vertex 11 a fan of valence 6"""
    faces = [[0, 1, 2], [1, 2, 0], [0, 1, 2], [3, 3, 4], [4, 5, 6], [2, 3, 5]]
    faces += [[11, 8 + k % 3, k % 7] for k in range(6)]
    return np.array(faces), 12


def edges_case(co):
    cube_v, cube_f = mo.box([0, 0, 0], [1, 1, 1])
    tv, tf = mo.torus(24)
    of, on = odd_mesh()
    arrs, meta = {}, dict(case="meshprep_tpl_edges")
    for name, v, f in (("cube", cube_v, cube_f), ("torus", tv, tf), ("odd", np.zeros((on, 3)), of)):
        t0 = time.perf_counter()
        e = co.get_tpl_edges(v, f)
        meta[f"ref_seconds_{name}"] = time.perf_counter() - t0
        assert e.shape[1] == 2 and len({(int(a), int(b)) for a, b in e}) == len(e)
        arrs.update({f"{name}_faces": f.astype(np.int32), f"{name}_n": np.int64(len(v)), f"{name}_edges": e.astype(np.int32)})
    bv, bf = mo.torus(64)
    t0 = time.perf_counter()
    e = co.get_tpl_edges(bv, bf)
    meta.update(ref_seconds_torus64=time.perf_counter() - t0, torus64_vertices=len(bv), torus64_faces=len(bf), torus64_edges=len(e),
                note="ref_seconds_*: get_tpl_edges on the generating CPU")
    print(f"  get_tpl_edges: 24 x 24 torus {meta['ref_seconds_torus']:.3f} s, 64 x 64 torus {meta['ref_seconds_torus64']:.3f} s")
    save("meshprep_tpl_edges", meta, **arrs)


def binvox_case(rw):
    tv, tf = mo.torus(24)
    nv, _, _ = mo.normalize(tv)
    r = mo.voxelize(nv, tf, 88)
    flat = np.zeros(16 ** 3, dtype=bool)                                               # in the file's x-z-y order
    at = 3
    for run, value in ((255, True), (510, False), (256, True), (1, False), (700, True), (254, False), (2, True)):
        flat[at:at + run] = value
        at += run
    flat[-255:] = True
    flat[-256] = False
    crafted = np.ascontiguousarray(np.transpose(flat.reshape(16, 16, 16), (0, 2, 1)))
    arrs, meta = {}, dict(case="meshprep_binvox")
    for name, data, dims, translate, scale in (("torus", r["data"], [88, 88, 88], [float(t) for t in r["translate"]], float(r["scale"])),
                                               ("crafted", crafted, [16, 16, 16], [-0.5, 0.0, 0.25], 1.0421052631578946)):
        buf = io.BytesIO()
        rw.write(rw.Voxels(data, dims, translate, scale, "xyz"), buf)
        raw = buf.getvalue()
        back = rw.read_as_3d_array(io.BytesIO(raw), fix_coords=True)
        assert np.array_equal(back.data, data) and back.dims == dims and back.translate == translate and back.scale == scale
        pairs = np.frombuffer(raw[raw.index(b"data\n") + 5:], dtype=np.uint8).reshape(-1, 2)
        meta[f"{name}_zero_count_pairs"] = int((pairs[:, 1] == 0).sum())
        arrs.update({f"{name}_bits": np.packbits(data.reshape(-1)), f"{name}_dims": np.array(dims, dtype=np.int64),
                     f"{name}_translate": np.array(translate, dtype=np.float64), f"{name}_scale": np.float64(scale),
                     f"{name}_file": np.frombuffer(raw, dtype=np.uint8), f"{name}_read_bits": np.packbits(np.asarray(back.data).reshape(-1))})
    assert meta["crafted_zero_count_pairs"] >= 2
    save("meshprep_binvox", meta, **arrs)


def main():
    co, rw = _reference()
    normalize_case(co)
    edges_case(co)
    binvox_case(rw)


if __name__ == "__main__":
    main()
