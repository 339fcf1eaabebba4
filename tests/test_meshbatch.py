"""CPU: morig_amd/meshbatch.py, the one packing of a list of meshes, under the ``runtime._test_ops`` seam. The
expected values are literals; they were generated once from the two classes this module replaced (``labels._Meshes`` for
check_faces="device", ``meshprep._Batch`` for "host") on the inputs of ``mixed()`` and ``out_of_range()`` and are not computed here.
``vertex_adjacency`` is checked against a numpy statement of the sort and the row pointers, on the keys of tests/transfer_emulate.py."""
import numpy as np
import pytest
import torch

import transfer_emulate
from morig_amd import meshbatch, ragged, runtime
from morig_amd.meshbatch import MeshBatch

BIG, SMALL = 2 ** 31, -2 ** 31 - 1


@pytest.fixture(autouse=True)
def seam():
    runtime._test_ops = transfer_emulate.TransferOps()
    try:
        yield runtime._test_ops
    finally:
        runtime._test_ops = None


def mixed():
    """four meshes: no vertices and no faces; numpy float32 vertices with torch int32 faces; a list of vertices with a list of faces;
    a float64 tensor with numpy int64 faces"""
    verts = [np.zeros((0, 3)), np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.float32), [[0.5, 0.0, 0.0], [0.0, 0.25, 0.0]],
             torch.tensor([[-1.0, -2.0, -3.0]], dtype=torch.float64)]
    faces = [np.zeros((0, 3), dtype=np.int64), torch.tensor([[0, 1, 2], [2, 1, 0]], dtype=torch.int32), [[0, 1, 1]],
             np.array([[0, 0, 0]], dtype=np.int64)]
    return verts, faces


def out_of_range():
    return [np.zeros((2, 3)), np.zeros((2, 3))], [np.array([[0, BIG, 1]], dtype=np.int64), np.array([[SMALL, 0, 0], [1, 0, 1]], dtype=np.int64)]


MIXED = dict(n=4, verts=[[1, 2, 3], [4, 5, 6], [7, 8, 9], [0.5, 0, 0], [0, 0.25, 0], [-1, -2, -3]], faces=[[0, 1, 2], [2, 1, 0], [0, 1, 1], [0, 0, 0]],
             nv=[0, 3, 2, 1], nf=[0, 2, 1, 1], vptr=[0, 0, 3, 5, 6], fptr=[0, 0, 2, 3, 4])
CLAMPED = dict(n=2, verts=[[0, 0, 0]] * 4, faces=[[0, 2 ** 31 - 1, 1], [-2 ** 31, 0, 0], [1, 0, 1]], nv=[2, 2], nf=[1, 2], vptr=[0, 2, 4],
               fptr=[0, 1, 3])


def check(mb, want, what="f"):
    assert mb.what == what and mb.n == want["n"] and mb.device == torch.device("cpu")
    for name in ("nv", "nf", "vptr_host", "fptr_host"):
        got = getattr(mb, name)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == want[name.replace("_host", "")], name
    for name in ("vptr", "fptr"):
        got = getattr(mb, name)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and got.is_contiguous() and got.tolist() == want[name], name
    if want["verts"] is None:
        assert mb.verts is None
    else:
        assert mb.verts.dtype == torch.float64 and mb.verts.is_contiguous() and tuple(mb.verts.shape) == (len(want["verts"]), 3)
        assert mb.verts.tolist() == want["verts"]
    assert mb.faces.dtype == torch.int32 and mb.faces.is_contiguous() and tuple(mb.faces.shape) == (len(want["faces"]), 3)
    assert mb.faces.tolist() == want["faces"]


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_mixed_batch_packs_to_the_same_literals_in_both_modes(mode):
    check(MeshBatch("f", *mixed(), check_faces=mode), MIXED)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_an_empty_list(mode):
    mb = MeshBatch("f", [], [], check_faces=mode)
    check(mb, dict(n=0, verts=[], faces=[], nv=[], nf=[], vptr=[0], fptr=[0]))
    assert mb.split_v(torch.zeros(0)) == [] and mb.blocks(256)[1] == 0
    only = MeshBatch("f", [])
    assert only.faces is None and only.n == 0 and tuple(only.verts.shape) == (0, 3)


def test_pack_faces_alone():
    faces, nf, fptr_host, fptr = meshbatch.pack_faces("f", mixed()[1], "cpu")
    assert faces.dtype == torch.int32 and faces.is_contiguous() and faces.tolist() == MIXED["faces"]
    assert nf.dtype == np.int64 and nf.tolist() == MIXED["nf"] and fptr_host.dtype == np.int64 and fptr_host.tolist() == MIXED["fptr"]
    assert fptr.dtype == torch.int32 and fptr.tolist() == MIXED["fptr"]
    faces, nf, fptr_host, fptr = meshbatch.pack_faces("f", [], "cpu")
    assert faces.dtype == torch.int32 and tuple(faces.shape) == (0, 3) and nf.tolist() == [] and fptr_host.tolist() == fptr.tolist() == [0]


def test_values_past_int32_are_clamped_on_the_device_path_and_refused_on_the_host_path():
    check(MeshBatch("f", *out_of_range()), CLAMPED)                                  # 2^31 and -2^31 - 1 stay outside [0, nv)
    with pytest.raises(ValueError, match="^f: a face names a vertex outside its mesh$"):
        MeshBatch("f", *out_of_range(), check_faces="host")
    for bad in ([[0, 1, 2]], [[-1, 0, 1]]):                                          # one past the mesh, one below it
        with pytest.raises(ValueError, match="^f: a face names a vertex outside its mesh$"):
            MeshBatch("f", [np.zeros((2, 3))], [bad], check_faces="host")
        assert MeshBatch("f", [np.zeros((2, 3))], [bad]).faces.tolist() == bad       # the stage's kernel flags it
    assert str(meshbatch.bad_face("g")) == "g: a face names a vertex outside its mesh"
    assert MeshBatch("f", [np.zeros((0, 3))], [np.zeros((0, 3), dtype=np.int64)], check_faces="host").faces.shape == (0, 3)   # nothing to read


@pytest.mark.parametrize("mode", ["device", "host"])
def test_refusals(mode):
    v = [np.zeros((2, 3))]
    for faces in ([np.zeros((1, 3))], [torch.zeros(1, 3, dtype=torch.float32)], [np.zeros((1, 4), dtype=np.int64)], [np.zeros(3, dtype=np.int64)],
                  [[[0, 1]]]):
        with pytest.raises(ValueError, match=r"^f: faces are integer \[F, 3\] per mesh$"):
            MeshBatch("f", v, faces, check_faces=mode)
    for verts in ([np.zeros((2, 2))], [np.zeros(3)], [np.zeros((1, 3, 1))]):
        with pytest.raises(ValueError, match=r"^f: verts are \[V, 3\] per mesh$"):
            MeshBatch("f", verts, [np.zeros((0, 3), dtype=np.int64)], check_faces=mode)
    for faces in ([], [np.zeros((0, 3), dtype=np.int64)] * 2):
        with pytest.raises(ValueError, match="^f: one faces array per mesh$"):
            MeshBatch("f", v, faces, check_faces=mode)


def test_the_vertex_count_path():
    faces = mixed()[1]
    mb = MeshBatch("f", faces=faces, n_verts=[0, 3, np.int64(2), 1], check_faces="host")
    check(mb, dict(MIXED, verts=None))
    for counts in ([0, 3, 2], [0, 3, -2, 1], [0, 3, 2, 1, 1]):
        with pytest.raises(ValueError, match="^f: one vertex count per mesh$"):
            MeshBatch("f", faces=faces, n_verts=counts, check_faces="host")
    with pytest.raises(ValueError, match="^f: a face names a vertex outside its mesh$"):
        MeshBatch("f", faces=faces, n_verts=[0, 2, 2, 1], check_faces="host")


def test_take_and_split_v():
    mb = MeshBatch("f", *mixed(), check_faces="host")
    sub = mb.take([2, 1, 2], "g")
    check(sub, dict(n=3, verts=[[0.5, 0, 0], [0, 0.25, 0], [1, 2, 3], [4, 5, 6], [7, 8, 9], [0.5, 0, 0], [0, 0.25, 0]],
                    faces=[[0, 1, 1], [0, 1, 2], [2, 1, 0], [0, 1, 1]], nv=[2, 3, 2], nf=[1, 2, 1], vptr=[0, 2, 5, 7], fptr=[0, 1, 3, 4]), "g")
    parts = mb.split_v(torch.arange(6) * 10)
    assert [p.tolist() for p in parts] == [[], [0, 10, 20], [30, 40], [50]]
    assert [p.tolist() for p in sub.split_v(torch.arange(7))] == [[0, 1], [2, 3, 4], [5, 6]]


@pytest.mark.parametrize("block", [1, 3, 256])
def test_blocks_at_the_edges_of_a_block(block):
    counts = [0, 1, block - 1, block, block + 1]
    want = {1: [0, 0, 1, 1, 2, 4], 3: [0, 0, 1, 2, 3, 5], 256: [0, 0, 1, 2, 3, 5]}[block]
    mb = MeshBatch("f", faces=[np.zeros((0, 3), dtype=np.int64)] * 5, n_verts=counts)
    for blk, n_blk in (mb.blocks(block), ragged.blocks(counts, block, "cpu", "f"), ragged.blocks(np.array(counts, dtype=np.int32), block, "cpu", "f")):
        assert blk.dtype == torch.int32 and blk.device.type == "cpu" and blk.tolist() == want and n_blk == want[-1]
    with pytest.raises(ValueError, match="^f: more than"):
        ragged.blocks([2 ** 31], 1, "cpu", "f")


# ------------------------------------------------------------------------------------------------------------------- vertex adjacency
def _adjacency(nv, faces, per_face):
    """numpy: per mesh and face the directed pairs (v, n), v != n, of a face inside its mesh (a bad face gives none) as
    (global v) << 32 | n, absent ones as int64 max, sorted; rowptr[v] = the number of keys below v << 32"""
    none, keys, v0 = np.iinfo(np.int64).max, [], 0
    for n, fb in zip(nv, faces):
        for row in np.asarray(fb, dtype=np.int64).reshape(-1, 3):
            ok = row.min() >= 0 and row.max() < n
            pairs = [(row[k], row[(k + j) % 3]) for k in range(3) for j in (1, 2)]
            keys += [((v0 + v) << 32) | m if ok and v != m else none for v, m in pairs]
        v0 += n
    keys = np.sort(np.array(keys, dtype=np.int64))
    return keys, np.searchsorted(keys, np.arange(v0 + 1, dtype=np.int64) << 32)


def test_vertex_adjacency_equals_the_numpy_statement(seam):
    nv = [5, 0, 3]
    faces = [[[0, 1, 2], [0, 1, 2], [2, 2, 3], [1, 0, 3]],       # a duplicate face, a degenerate face; vertex 4 is isolated
             np.zeros((0, 3), dtype=np.int64), [[0, 1, 3], [2, 1, 0]]]                                  # a bad index
    mesh = MeshBatch("f", [np.zeros((n, 3)) for n in nv], faces)
    status = torch.zeros(mesh.n + 1, dtype=torch.int32)
    keys, rowptr = meshbatch.vertex_adjacency(seam, mesh, 6, status)
    want_keys, want_rows = _adjacency(nv, faces, 6)
    assert keys.dtype == torch.int64 and keys.is_contiguous() and np.array_equal(keys.numpy(), want_keys)
    assert rowptr.dtype == torch.int32 and rowptr.is_contiguous() and tuple(rowptr.shape) == (sum(nv) + 1,)
    assert np.array_equal(rowptr.numpy(), want_rows)
    assert status[0] == seam.TRANSFER_BAD_FACE and seam.calls == ["transfer_keys"]
    rows = [sorted(set((keys[rowptr[v]:rowptr[v + 1]] & 0xffffffff).tolist())) for v in range(sum(nv))]
    assert rows == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [], [1, 2], [0, 2], [0, 1]]
    assert rowptr[4] == rowptr[5] and int(rowptr[-1]) == 36 - 2 - 6             # the degenerate face's two (2, 2), the bad face's six
