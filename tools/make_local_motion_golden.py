"""Fixtures of the local rigid motion (tests/golden/local_motion.npz), made by the reference's own ``get_gt_rotation_icp``
(data_proc/common_ops.py:47-78), imported where it lies at generation time (open3d, cv2 and tqdm stubbed as empty modules). The mesh is
a duck-typed object (``.vertices``, ``.triangles``). Nothing of the reference is written into the repository: only the inputs and the
recorded ``R_all``, ``T_all`` and ``nnids`` (flattened to a prefix sum and the concatenated indices).

  grid_a, grid_b   jittered, bumped vertex grids at spacings 0.012 and 0.018 under a bend
  strip            two rows at spacing 0.005: the ring limit binds before the radius does
  shuffled         a grid with its vertices renumbered at random
  rungs            a fan whose hub has 4 candidates under the first rung and 6 under the second, and a rim vertex at 0.0625

Every case also runs a second time with the recorded ``nnids`` handed back in, which must give the same numbers.

Run from the repository root:  python tools/make_local_motion_golden.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (save)
import local_motion_oracle as lo                                               # noqa: E402


def reference():
    for name in ("open3d", "cv2", "tqdm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    if not hasattr(np, "int"):
        np.int = int
    if not hasattr(np, "bool"):
        np.bool = bool
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    return __import__("data_proc.common_ops", fromlist=["get_gt_rotation_icp"]).get_gt_rotation_icp


class Mesh:
    def __init__(self, vertices, triangles):
        self.vertices, self.triangles = vertices, triangles


def main():
    icp = reference()
    cases = lo.golden_cases()
    arrs = dict(names=np.array(",".join(cases)))
    for name, (v0, faces, vt) in cases.items():
        R_all, T_all, nnids = icp(Mesh(v0.copy(), faces.copy()), v0.copy(), vt.copy(), None)
        R2, T2, _ = icp(Mesh(v0.copy(), faces.copy()), v0.copy(), vt.copy(), nnids)
        assert np.array_equal(R_all, R2) and np.array_equal(T_all, T2), name
        want = lo.patch_lists(v0, faces)
        assert all(np.array_equal(a, b) for a, b in zip(want["lists"], nnids)), name   # the oracle is held against the reference here already
        ptr, ids = lo.flat([np.asarray(r, dtype=np.int64) for r in nnids])
        arrs.update({f"{name}_verts0": v0, f"{name}_faces": faces.astype(np.int64), f"{name}_verts_t": vt,
                     f"{name}_R_all": np.asarray(R_all, dtype=np.float64), f"{name}_T_all": np.asarray(T_all, dtype=np.float64),
                     f"{name}_ptr": ptr, f"{name}_ids": ids})
        sizes = np.diff(ptr)
        print(f"  {name}: V {len(v0)}, F {len(faces)}, patch sizes {sizes.min()}..{sizes.max()}, rungs {np.bincount(want['rung'], minlength=3).tolist()}")
    msg.save("local_motion", dict(cases=list(cases)), **arrs)
    print(f"  K0 measured: {lo.measure_k0(verbose=False):.1f}")


if __name__ == "__main__":
    main()
