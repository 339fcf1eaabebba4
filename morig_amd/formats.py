"""On-disk formats either side of the hot path. Host-side Python, as in the reference.

IN  -- what ``datasets/dataset_rig.py:78-140`` (``RigDataset.process``) reads per model ``{id}`` and how it turns the files
       into the tensors the networks consume:
         {id}_vtx_traj.npy  V x T x 3 trajectory; pos = frame 0; gt_flow = frames 20,40,..,100 minus frame 0   (:105-108)
         {id}_attn.txt      V attention ground truth                                                           (:83)
         {id}_tpl_e.txt / {id}_geo_e.txt   rows "src dst", np.loadtxt(...).T, + one self loop per vertex        (:84-85,119-122)
         {id}_rig.txt       joints / root / skin / hier lines, utils/rig_parser.py:21-45 (``Rig``)
         {id}_skin.txt      bones / bind / influence lines, dataset_rig.py:30-76 (``load_skin``)
         pred_flow/{id}_{1..5}_pred_flow.npy   DeformNet's output per keyframe, concatenated to V x 15           (:111-115)
         {id}.binvox        the solid voxel grid of the external ``binvox`` program: ``read_binvox`` / ``write_binvox`` (the run-length
                            format of utils/binvox_rw.py); ``Voxels`` is what the voxel-reading stages take, from a file or from
                            ``meshprep.voxelize``
         {id}.obj           ``read_obj``: the ``v`` and ``f`` lines of a Wavefront mesh
OUT -- ``{id}.ply`` (ASCII, 7 header lines, '%f %f %f'; utils/io_utils.py:29-41, read back by ``readPly`` :18-26) and
       ``{id}_attn.npy``: writers in morig_amd/harness.py, reader here.
"""
from __future__ import annotations

import os
from typing import List

import numpy as np
import torch

from .synth import MeshData

NUM_NEAREST_BONE = 20          # dataset_rig.py:80
NUM_MAX_JOINT = 48             # dataset_rig.py:81


def read_ply(filename: str) -> np.ndarray:
    """utils/io_utils.py:18-26: skips the 7 header lines, float64 [n, 3]."""
    with open(filename, "r") as f:
        lines = f.readlines()
    return np.array([[float(w) for w in li.split()[:3]] for li in lines[7:]], dtype=np.float64).reshape(-1, 3)


class Rig:
    """utils/rig_parser.py:4-80: names, pos (after the reference's forward-kinematics pass with identity frames),
    hierarchy (parent id, -1 for the root), skins (V x J), root_id. Pose state (tracking): local_frames [J, 3, 3] (identity after
    load), global_transforms [J, 3, 3], ``fk()`` and ``global_transforms_homogeneous``."""

    def __init__(self, filename: str):
        self.names: List[str] = []
        pos, skins = [], []
        self.hierarchy = None
        self.root_name, self.root_id = None, None
        with open(filename, "r") as f:
            for line in f.readlines():
                w = line.split()
                if w[0] == "joints":
                    self.names.append(w[1])
                    pos.append(np.array([float(w[2]), float(w[3]), float(w[4])]))
                elif w[0] == "root":
                    self.root_name = w[1]
                    self.root_id = self.names.index(w[1])
                    self.hierarchy = np.zeros(len(self.names), dtype=int)
                    self.hierarchy[self.root_id] = -1
                elif w[0] == "skin":
                    row = np.zeros(len(self.names))
                    for i in range(2, len(w), 2):
                        row[self.names.index(w[i])] = float(w[i + 1])
                    skins.append(row)
                elif w[0] == "hier":
                    self.hierarchy[self.names.index(w[2])] = self.names.index(w[1])
        pos = np.stack(pos, axis=0)
        self.skins = np.stack(skins, axis=0) if skins else []
        self._frames_and_offsets(pos)

    def _frames_and_offsets(self, pos: np.ndarray) -> None:
        # calc_frames_and_offsets + FK (:47-78) with identity local frames: positions are rebuilt parent-first as
        # offset + parent position -- kept because (p - parent) + parent is not always p in floating point. Offsets are float64,
        # the rebuilt positions keep the dtype of ``pos`` (np.zeros_like): float32 joints stay float32, as in predict_skeleton
        offset = np.zeros((len(self.names), 3))
        for i in range(len(pos)):
            offset[i] = pos[i] - pos[self.hierarchy[i]] if i != self.root_id else pos[i]
        res = np.zeros_like(pos)
        res[self.root_id] = pos[self.root_id]
        frontier = [self.root_id]
        eye = np.eye(3)
        while frontier:
            nxt = []
            for j in range(len(self.names)):
                if self.hierarchy[j] in frontier:
                    res[j] = np.matmul(eye, offset[j][:, None]).squeeze(axis=1) + res[self.hierarchy[j]]
                    nxt.append(j)
            frontier = nxt
        self.offset = offset
        self.pos = res
        # the pose state calc_frames_and_offsets leaves (:53, :66-75): identity frames, so every global transform is the identity
        self.local_frames = np.repeat(np.eye(3)[np.newaxis, ...], len(self.names), axis=0)
        self.global_transforms = self.local_frames.copy()

    def fk(self) -> None:
        """Rig.FK (utils/rig_parser.py:63-79) in the number formats it has after a tracking update: global_transforms and pos take the
        dtype of local_frames and pos (np.zeros_like: float32 once the solver's results are assigned), offset stays float64 -- its root
        row is overwritten with the root position -- so every position is a float64 product and sum rounded on store."""
        root, hier = self.root_id, self.hierarchy
        self.offset[root] = self.pos[root]
        glob = np.zeros_like(self.local_frames)
        glob[root] = self.local_frames[root]
        res = np.zeros_like(self.pos)
        res[root] = self.pos[root]
        frontier = [root]
        while frontier:
            nxt = []
            for j in range(len(self.names)):
                if hier[j] in frontier:
                    glob[j] = np.matmul(glob[hier[j]], self.local_frames[j])
                    res[j] = np.matmul(glob[hier[j]], self.offset[j][:, None]).squeeze(axis=1) + res[hier[j]]
                    nxt.append(j)
            frontier = nxt
        self.global_transforms = glob
        self.pos = res

    @property
    def global_transforms_homogeneous(self) -> np.ndarray:
        """[J, 4, 4] float64: [global_transforms | pos; 0 0 0 1] (utils/rig_parser.py:82-87)"""
        out = np.repeat(np.eye(4)[np.newaxis, ...], len(self.names), axis=0)
        out[:, 0:3, 0:3] = self.global_transforms
        out[:, 0:3, 3] = self.pos
        return out

    @classmethod
    def from_arrays(cls, pos, hierarchy, root_id: int, names=None, skins=None) -> "Rig":
        """A rig from arrays, as evaluate/joint2rig.py:222-228 fills one in: ``pos`` [J, 3] (its dtype is kept), ``hierarchy`` the
        parent index per joint with -1 at ``root_id``, names ``joint_{i}`` unless given, then calc_frames_and_offsets."""
        rig = cls.__new__(cls)
        pos = np.array(pos)
        hier = np.array(hierarchy, dtype=int).reshape(-1)
        n = len(pos)
        root_id = int(root_id)
        if pos.ndim != 2 or pos.shape[1] != 3 or len(hier) != n or not 0 <= root_id < n:
            raise ValueError("Rig.from_arrays: pos [J, 3], hierarchy [J] and a root id below J")
        if hier[root_id] != -1 or np.any(np.delete(hier, root_id) < 0) or np.any(hier >= n):
            raise ValueError("Rig.from_arrays: hierarchy holds parent indices, -1 at the root only")
        rig.names = [f"joint_{i}" for i in range(n)] if names is None else [str(x) for x in names]
        if len(rig.names) != n or len(set(rig.names)) != n:
            raise ValueError("Rig.from_arrays: one distinct name per joint")
        rig.hierarchy = hier
        rig.root_id, rig.root_name = root_id, rig.names[root_id]
        rig.skins = [] if skins is None or len(skins) == 0 else np.asarray(skins)
        reached = np.arange(n) == root_id
        for _ in range(n):
            reached = reached | np.where(hier >= 0, reached[np.maximum(hier, 0)], False)
        if not reached.all():
            raise ValueError("Rig.from_arrays: hierarchy is not a tree rooted at root_id")
        rig._frames_and_offsets(pos)
        return rig

    def save(self, filename: str) -> None:
        """utils/rig_parser.py:90-113 byte for byte: joints lines (%.8f), root, one skin line per vertex (joints with weight > 0,
        %.4f), hier lines breadth first from the root, children in ascending joint index."""
        parts = []
        for i in range(len(self.pos)):
            parts.append("joints {0} {1:.8f} {2:.8f} {3:.8f}\n".format(self.names[i], self.pos[i, 0], self.pos[i, 1], self.pos[i, 2]))
        parts.append("root {}\n".format(self.root_name))
        for vid, skw in enumerate(self.skins):
            line = "skin {0} ".format(vid)
            for j in np.argwhere(skw > 0).squeeze(axis=1):
                line += "{0} {1:.4f} ".format(self.names[j], float(skw[j]))
            parts.append(line + "\n")
        hier = np.asarray(self.hierarchy)
        level = [self.root_id]
        while level:
            nxt = []
            for pid in level:
                for cid in np.argwhere(hier == pid).squeeze(axis=1):
                    parts.append("hier {0} {1}\n".format(self.names[pid], self.names[cid]))
                    nxt.append(cid)
            level = nxt
        with open(filename, "w") as f:
            f.write("".join(parts))


def load_skin(filename: str, num_nearest_bone: int = NUM_NEAREST_BONE):
    """dataset_rig.py:30-76 -> (skin_input V x 8k, nearest_bone_ids V x k, label, loss_mask V x k, bone_names)."""
    bones, bone_names, inputs, labels, nn_ids, masks = [], [], [], [], [], []
    with open(filename, "r") as f:
        for li in f.readlines():
            w = li.strip().split()
            if w[0] == "bones":
                bone_names.append([w[1], w[2]])
                bones.append([float(x) for x in w[3:]])
            elif w[0] == "bind":
                v = [float(x) for x in w[1:]]
                row, ids, mask = [], [], []
                for i in range(num_nearest_bone):
                    valid = int(v[3 * i + 1]) != -1
                    b = 3 * i + 1 if valid else 1                     # invalid slot: repeat the nearest bone, masked out (:50-56)
                    ids.append(int(v[b]))
                    row += bones[int(v[b])]
                    row.append(v[b + 1])
                    row.append(int(v[b + 2]))
                    mask.append(1 if valid else 0)
                inputs.append(np.array(row)[np.newaxis, :])
                nn_ids.append(np.array(ids)[np.newaxis, :])
                masks.append(np.array(mask)[np.newaxis, :])
            elif w[0] == "influence":
                labels.append(np.array([float(x) for x in w[1:]])[np.newaxis, :])
    return (np.concatenate(inputs, axis=0), np.concatenate(nn_ids, axis=0), np.concatenate(labels, axis=0),
            np.concatenate(masks, axis=0), bone_names)


def _with_self_loops(e: torch.Tensor, n: int) -> torch.Tensor:
    """torch_geometric.utils.add_self_loops(e, num_nodes=n) as the dataset applies it (:121-122): existing loops stay."""
    loops = torch.arange(n, dtype=torch.long).unsqueeze(0).repeat(2, 1)
    return torch.cat([e, loops], dim=1)


def load_rig_sample(vtx_filename: str) -> MeshData:
    """One ``Data`` of RigDataset.process (dataset_rig.py:82-138) from ``.../{id}_vtx_traj.npy`` and its siblings."""
    root = os.path.dirname(vtx_filename)
    sib = lambda suffix: vtx_filename.replace("_vtx_traj.npy", suffix)
    v_traj = np.load(vtx_filename)
    m = np.loadtxt(sib("_attn.txt"))
    tpl_e = np.loadtxt(sib("_tpl_e.txt")).T
    geo_e = np.loadtxt(sib("_geo_e.txt")).T
    rig = Rig(sib("_rig.txt"))
    joints = rig.pos
    name = int(os.path.basename(vtx_filename).split("_")[0])
    first = v_traj[:, 0, :]
    nearest_jid = np.argmin(np.sum((joints[:, None, :] - first[None, ...]) ** 2, axis=-1), axis=0)
    offsets = joints[nearest_jid] - first
    gt_skin = np.zeros((rig.skins.shape[0], NUM_MAX_JOINT))
    gt_skin[:, 0:rig.skins.shape[1]] = rig.skins
    skin_input, skin_nn, skin_label, loss_mask, bone_names = load_skin(sib("_skin.txt"))
    skin_nnjids = np.stack([np.array([rig.names.index(bone_names[b][0]) for b in skin_nn[v]]) for v in range(len(v_traj))], 0)
    gt_flow = np.concatenate([v_traj[:, t, :] - first for t in np.arange(20, 110, 20)], axis=1)
    pred_flow = np.concatenate([np.load(os.path.join(root, f"pred_flow/{name}_{t}_pred_flow.npy")) for t in np.arange(1, 6)], axis=1)

    d = MeshData()
    d.pos = torch.from_numpy(first).float()
    n = d.pos.size(0)
    d.mask = torch.from_numpy(m).float()
    d.tpl_edge_index = _with_self_loops(torch.from_numpy(tpl_e).long(), n)
    d.geo_edge_index = _with_self_loops(torch.from_numpy(geo_e).long(), n)
    d.offsets = torch.from_numpy(offsets).float()
    d.gt_flow = torch.from_numpy(gt_flow).float()
    d.pred_flow = torch.from_numpy(pred_flow).float()
    d.joints = torch.from_numpy(joints).float()
    d.skin_input = torch.from_numpy(skin_input).float()
    d.skin_label = torch.from_numpy(skin_label).float()
    d.skin_nn = torch.from_numpy(skin_nn).long()
    d.skin_nnjids = torch.from_numpy(skin_nnjids).long()
    d.loss_mask = torch.from_numpy(loss_mask).long()
    d.gt_skin = torch.from_numpy(gt_skin).float()
    d.name = name
    d.batch = torch.zeros(n, dtype=torch.long)
    return d


# ------------------------------------------------------------------------------------------------------------------------- voxels, meshes
class Voxels:
    """The four members the voxel-reading stages take (joints.inside_check, skeleton.make_data / connectivity_cost, skinning): ``data``
    bool [dims]^3 numpy array indexed [x][y][z], ``dims`` [d, d, d], ``translate`` [x, y, z], ``scale``. Voxel (i, j, k) is the cube
    translate + scale * [i, i + 1] x [j, j + 1] x [k, k + 1] / dims, its centre at (i + 0.5) / dims (utils/binvox_rw.py:34-41)."""

    def __init__(self, data, dims, translate, scale):
        self.data = data
        self.dims = [int(d) for d in dims]
        self.translate = [float(t) for t in translate]
        self.scale = float(scale)


def read_binvox(filename: str) -> Voxels:
    """utils/binvox_rw.py:62-109, ``read_as_3d_array(fp, fix_coords=True)``: the header lines (#binvox, dim, translate, scale, data), then
    (value, count) byte pairs over the x-z-y storage order, returned indexed [x][y][z]."""
    with open(filename, "rb") as f:
        if not f.readline().strip().startswith(b"#binvox"):
            raise IOError("Not a binvox file")
        dims = [int(w) for w in f.readline().strip().split(b" ")[1:]]
        translate = [float(w) for w in f.readline().strip().split(b" ")[1:]]
        scale = [float(w) for w in f.readline().strip().split(b" ")[1:]][0]
        f.readline()
        raw = np.frombuffer(f.read(), dtype=np.uint8)
    data = np.repeat(raw[::2], raw[1::2]).astype(bool).reshape(dims)
    return Voxels(np.ascontiguousarray(np.transpose(data, (0, 2, 1))), dims, translate, scale)


def write_binvox(vox, filename: str) -> None:
    """utils/binvox_rw.py:197-242 byte for byte for a dense [x][y][z] grid: the five header lines with ``str`` of every number, then the
    runs of the x-z-y flattened grid as (value, count) pairs. A run is cut every 255 voxels; as in the reference, a run whose length is a
    multiple of 255 is followed by a pair of count 0 unless it is the last one."""
    data = np.asarray(vox.data).astype(bool)
    if data.ndim != 3 or data.size == 0:
        raise ValueError("write_binvox: data is a non-empty 3-D grid")
    flat = np.transpose(data, (0, 2, 1)).reshape(-1)
    starts = np.concatenate([[0], np.nonzero(flat[1:] != flat[:-1])[0] + 1])
    lengths = np.diff(np.concatenate([starts, [flat.size]]))
    full, rest = lengths // 255, lengths % 255
    tail = rest > 0
    tail[:-1] = True
    pairs = full + tail
    counts = np.full(int(pairs.sum()), 255, dtype=np.uint8)
    counts[(np.cumsum(pairs) - 1)[tail]] = rest[tail]
    body = np.stack([np.repeat(flat[starts].astype(np.uint8), pairs), counts], 1)
    number = lambda x: str(x.item() if isinstance(x, np.generic) else x)
    head = "#binvox 1\ndim {}\ntranslate {}\nscale {}\ndata\n".format(" ".join(number(d) for d in vox.dims), " ".join(number(t) for t in vox.translate),
                                                                   number(vox.scale))
    with open(filename, "wb") as f:
        f.write(head.encode())
        f.write(body.tobytes())


def read_obj(filename: str):
    """The ``v`` and ``f`` lines of a Wavefront OBJ file -> (verts float64 [V, 3], faces int64 [F, 3], 0-based). An index is ``a``,
    ``a/b``, ``a//c`` or ``a/b/c`` (the vertex index is the first field); a negative index counts back from the vertices read so far;
    a polygon is fanned from its first vertex. Every other line is ignored."""
    verts, faces = [], []
    with open(filename, "r") as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                verts.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                ids = []
                for field in w[1:]:
                    i = int(field.split("/")[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if not 0 <= i < len(verts):
                        raise ValueError(f"read_obj: {filename}: face index {field!r} names no vertex read so far")
                    ids.append(i)
                for k in range(1, len(ids) - 1):
                    faces.append([ids[0], ids[k], ids[k + 1]])
    return np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3)
