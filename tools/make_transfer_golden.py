"""Fixtures of the remesh transfer (tests/golden/transfer_remesh.npz), made by the reference's own ``transfer_rig_to_remesh``
(data_proc/common_ops.py:229-259), imported where it lies at generation time (open3d, cv2 and tqdm stubbed as empty modules). The meshes
and the rig are duck-typed objects (``.vertices``, ``.triangles``, ``.skins``). Nothing of the reference is written into the repository:
only the inputs, the skins it returned and the source rows recovered from a second run.

Every case runs twice: with its skins, and with the marker rows skins[o] = (o + 1, 1), whose normalised image (o + 1, 1) / (o + 2 + 1e-8)
names the original vertex o a remeshed vertex received: o = round(row[0] / row[1]) - 1.

  grid_k       shuffled vertex grids with a share of coincident vertices (seeds chosen so that the conditions below hold)
  quirk        a shuffled grid on which the reference's neighbour set gives another source than neighbours="faces" (the oracle's)
  chain_down   a descending-index chain of 24 vertices: "faces" needs 23 sweeps; the reference's own set needs fewer (faces 0, 1, 2)
  chain_up     the same chain ascending: one sweep
  root_tie     two filled neighbours whose squared distances differ while the correctly rounded roots are equal: the lowest index wins
  underflow    a coincidence through an underflowing square and a signed zero; two coincident originals: the lowest gives the row

Run from the repository root:  python tools/make_transfer_golden.py
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
import transfer_oracle as to                                                   # noqa: E402


def reference():
    for name in ("open3d", "cv2", "tqdm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    if not hasattr(np, "int"):
        np.int = int
    if not hasattr(np, "bool"):
        np.bool = bool
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    return __import__("data_proc.common_ops", fromlist=["transfer_rig_to_remesh"]).transfer_rig_to_remesh


class Mesh:
    def __init__(self, vertices, triangles=None):
        self.vertices, self.triangles = vertices, triangles


class Skins:
    def __init__(self, skins):
        self.skins = skins


def run(transfer, vo, vr, faces, skins):
    out = transfer(Mesh(vo), Mesh(vr, faces), Skins(skins)).skins
    marker = np.stack([np.arange(len(vo)) + 1.0, np.ones(len(vo))], 1)
    rows = transfer(Mesh(vo), Mesh(vr, faces), Skins(marker)).skins
    source = np.rint(rows[:, 0] / rows[:, 1]).astype(np.int64) - 1
    assert np.all((source >= 0) & (source < len(vo)))
    return np.asarray(out, dtype=np.float64), source


def main():
    transfer = reference()
    cases = {}
    for k, (nx, ny, every) in enumerate([(5, 4, 3), (7, 6, 5), (9, 5, 12)]):
        cases[f"grid_{k}"] = to.remesh_case(nx, ny, every, seed=20261020 + k)
    for seed in range(100, 400):                                               # the quirk changes the answer
        c = to.remesh_case(6, 6, 9, seed)
        a, b = to.remesh_loop(*c, neighbours="reference"), to.remesh_loop(*c, neighbours="faces")
        if b["n_unreachable"] == 0 and not np.array_equal(a["source"], b["source"]) and b["n_sweeps"] > a["n_sweeps"]:
            cases["quirk"] = c
            break
    else:
        raise SystemExit("quirk: no admissible seed")
    cases["chain_down"], cases["chain_up"] = to.chain_case(24, True), to.chain_case(24, False)
    cases["root_tie"], cases["underflow"] = to.root_tie_case(), to.underflow_case()
    meta, arrs = dict(cases=list(cases)), {}
    for name, (vo, vr, faces, skins) in cases.items():
        out, source = run(transfer, vo, vr, faces, skins)
        want = to.remesh_loop(vo, vr, faces, skins)
        assert np.array_equal(want["source"], source), name                    # the oracle is held against the reference here already
        arrs.update({f"{name}_vo": vo, f"{name}_vr": vr, f"{name}_faces": faces.astype(np.int64), f"{name}_skins_ori": skins,
                     f"{name}_skins": out, f"{name}_source": source})
        print(f"  {name}: V {len(vo)}, V' {len(vr)}, F {len(faces)}, sweeps {want['n_sweeps']}")
    assert to.remesh_loop(*cases["chain_down"], neighbours="faces")["n_sweeps"] == 23
    msg.save("transfer_remesh", meta, **arrs)


if __name__ == "__main__":
    main()
