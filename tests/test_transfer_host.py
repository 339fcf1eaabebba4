"""CPU: the host logic of morig_amd/transfer.py on an emulated op layer (tests/transfer_emulate.py through ``runtime._test_ops``): ragged
batches with different joint counts, empty meshes, every refusal, the rigs that come back -- saved, read back and fed to
``playback.skin_trajectory`` (tests/playback_emulate.py) -- and csrc/pointtri_core.h as the stand-alone program
tools/pointtri_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import transfer_emulate as te
import transfer_oracle as to
from morig_amd import runtime, transfer
from morig_amd.formats import Rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = te.TransferOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def same(a, b):
    a, b = (x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def star_rig(J, skins, seed=0):
    pos = np.random.default_rng(seed).uniform(-0.3, 0.3, (J, 3))
    return Rig.from_arrays(pos, [-1] + [0] * (J - 1), 0, skins=skins)


def remesh_batch():
    cases = [to.remesh_case(5, 4, 3, 11, J=4), to.chain_case(9, True, J=2), to.remesh_case(6, 6, 9, 12, J=7), to.underflow_case(), to.root_tie_case()]
    none = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 5)))          # a mesh without anything
    return cases[:2] + [none] + cases[2:]


# ------------------------------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("neighbours", ["reference", "faces"])
def test_remesh_transfer_of_a_ragged_batch_equals_the_loop(ops, neighbours):
    cases = remesh_batch()
    rigs = [to.PlainRig(c[3]) for c in cases]
    out = transfer.transfer_to_remesh([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], rigs, neighbours=neighbours,
                                      return_info=True)
    assert ops.calls == ["transfer_keys", "transfer_coincide", "transfer_flood", "transfer_rows"] and len(out) == len(cases)
    for c, rig_in, (rig, source, info) in zip(cases, rigs, out):
        want = to.remesh_loop(*c, neighbours=neighbours)
        assert source.dtype == torch.int64 and same(source, want["source"]) and same(info["sweep"], want["sweep"].astype(np.int32))
        assert same(rig.skins, want["skins"]) and same(rig.skins_device, want["skins"])
        assert rig is not rig_in and rig.pos is not rig_in.pos and same(rig.pos, rig_in.pos) and same(rig_in.skins, c[3])      # a copy
    alone = transfer.transfer_to_remesh([cases[3][0]], [cases[3][1]], [cases[3][2]], [rigs[3]], neighbours=neighbours)
    assert same(alone[0][0].skins, out[3][0].skins) and same(alone[0][1], out[3][1])
    assert transfer.transfer_to_remesh([], [], [], []) == []


def test_remesh_transfer_refusals(ops):
    vo, vr, faces, skins = to.remesh_case(4, 4, 3, 5)
    rig = to.PlainRig(skins)
    run = lambda vo=vo, vr=vr, faces=faces, rig=rig, **k: transfer.transfer_to_remesh([vo], [vr], [faces], [rig], **k)
    with pytest.raises(ValueError, match="neighbours"):
        run(neighbours="edges")
    with pytest.raises(ValueError, match="unreachable"):
        run(unreachable="skip")
    with pytest.raises(ValueError, match="one original mesh"):
        transfer.transfer_to_remesh([vo, vo], [vr], [faces], [rig])
    with pytest.raises(ValueError, match="one row per source vertex"):
        run(rig=to.PlainRig(skins[:-1]))
    assert ops.calls == []                                                              # refused before any op
    with pytest.raises(ValueError, match="outside its mesh"):
        run(faces=faces + 1)
    with pytest.raises(ValueError, match="outside its mesh"):
        run(faces=np.concatenate([faces, [[0, -1, 2]]]))
    for bad in (np.nan, np.inf, -1.5e7):
        moved = vr.copy()
        moved[3, 1] = bad
        with pytest.raises(ValueError, match="1e\\+07"):
            run(vr=moved)
        far = vo.copy()
        far[0, 2] = bad
        with pytest.raises(ValueError, match="1e\\+07"):
            run(vo=far)
    edge = vr.copy()
    edge[vr[:, 0] == vr[:, 0].max(), 0] = 1e7                                           # the limit itself is allowed
    run(vr=edge)
    big = np.zeros((transfer.MAX_FLOOD_VERTS + 1, 3))
    with pytest.raises(ValueError, match="at most 8192 per mesh"):
        run(vr=big)


def test_unreachable_vertices_raise_or_take_the_nearest(ops):
    vo, vr, faces, skins = to.remesh_case(4, 4, 3, 5)
    lone = np.concatenate([vr, [[5.0, 5.0, 5.0]]])                                      # in no face
    rig = to.PlainRig(skins)
    with pytest.raises(transfer.TransferError, match="mesh 1: 1 of 17"):
        transfer.transfer_to_remesh([vo, vo], [vr, lone], [faces, faces], [rig, rig])
    (_, _), (got, source) = transfer.transfer_to_remesh([vo, vo], [vr, lone], [faces, faces], [rig, rig], unreachable="nearest")
    want = to.remesh_loop(vo, lone, faces, skins, unreachable="nearest")
    assert same(source, want["source"]) and same(got.skins, want["skins"]) and source[-1] == want["nearest"][-1]
    island = vr + 10.0                                                                  # a component without a coincident vertex
    both_v, both_f = np.concatenate([vr, island]), np.concatenate([faces, faces + len(vr)])
    with pytest.raises(transfer.TransferError, match="16 of 32"):
        transfer.transfer_to_remesh([vo], [both_v], [both_f], [rig], neighbours="faces")
    with pytest.raises(transfer.TransferError, match="no original vertex"):
        transfer.transfer_to_remesh([vo[:0]], [vr], [faces], [to.PlainRig(skins[:0])], unreachable="nearest")


# ------------------------------------------------------------------------------------------------------------------------- part B
def surface_batch():
    sv, sf = to.torus(10, 6)
    dv, _ = to.torus(16, 9)
    gv, gf = to.grid_mesh(4, 5, seed=2)
    rng = np.random.default_rng(3)
    return [(sv, sf, to.random_skins(len(sv), 6, 1), dv), (gv, gf, to.random_skins(len(gv), 3, 2), rng.uniform(-0.2, 0.8, (300, 3))),
            (gv, np.zeros((0, 3), dtype=np.int64), to.random_skins(len(gv), 2, 3), rng.uniform(0, 1, (4, 3))),           # no faces
            (sv, sf, to.random_skins(len(sv), 9, 4), np.zeros((0, 3))),                                                  # no destination
            (to.COLLAPSED_VERTS, to.COLLAPSED_FACES, np.eye(4), np.array([to.COLLAPSED_POINT, to.TIE_POINT]))]


def test_surface_transfer_of_a_ragged_batch_equals_the_oracle(ops):
    cases = surface_batch()
    out = transfer.transfer_skins(*[[c[k] for c in cases] for k in range(4)])
    assert ops.calls == ["transfer_closest", "transfer_rows"] and len(out) == len(cases)
    for c, (skins, face, bary, dist) in zip(cases, out):
        want = to.transfer_skins(*c)
        assert face.dtype == torch.int32 and same(face, want["face"]) and same(bary, want["bary"]) and same(dist, want["distance"])
        assert same(skins, want["skins"]) and tuple(skins.shape) == (len(c[3]), c[2].shape[1])
    assert out[2][1].tolist() == [-1] * 4 and not out[2][0].any() and out[4][1].tolist()[0] == 1
    alone = transfer.transfer_skins(*[[cases[1][k]] for k in range(4)])
    assert all(same(a, b) for a, b in zip(alone[0], out[1]))
    assert transfer.transfer_skins([], [], [], []) == []
    with pytest.raises(ValueError, match="outside its mesh"):
        transfer.transfer_skins([cases[1][0]], [cases[1][1] + 7], [cases[1][2]], [cases[1][3]])
    with pytest.raises(ValueError, match="one row per source vertex"):
        transfer.transfer_skins([cases[1][0]], [cases[1][1]], [cases[1][2][1:]], [cases[1][3]])
    with pytest.raises(ValueError, match="one source mesh"):
        transfer.transfer_skins([cases[1][0]], [cases[1][1]], [cases[1][2]], [])


def test_transferred_rigs_save_read_back_and_play(ops, tmp_path):
    import playback_emulate as pe
    from morig_amd import playback
    sv, sf = to.torus(10, 6)
    dv, _ = to.torus(16, 9)
    J = 5
    rig = star_rig(J, to.random_skins(len(sv), J, 7))
    with pytest.raises(ValueError, match="without faces"):
        transfer.transfer_rigs([rig], [(sv, sf[:0])], [dv])
    (moved,) = transfer.transfer_rigs([rig], [(sv, sf)], [dv])
    want = to.transfer_skins(sv, sf, rig.skins, dv)
    assert isinstance(moved, Rig) and moved is not rig and same(moved.skins, want["skins"]) and same(moved.skins_device, want["skins"])
    assert same(moved.pos, rig.pos) and same(moved.hierarchy, rig.hierarchy) and moved.names == rig.names and len(rig.skins) == len(sv)
    assert (moved.skins >= 0).all() and np.abs(moved.skins.sum(1) - 1.0).max() < 1e-7
    name = str(tmp_path / "moved_rig.txt")
    moved.save(name)
    back = Rig(name)
    assert back.skins.shape == moved.skins.shape and np.abs(back.skins - moved.skins).max() <= 5e-5 + 1e-12       # %.4f
    vo, vr, faces, skins = to.remesh_case(5, 4, 3, 11, J=J)
    ((remeshed, _),) = transfer.transfer_to_remesh([vo], [vr], [faces], [star_rig(J, skins)])
    remeshed.save(name)
    assert Rig(name).skins.shape == (len(vr), J)
    quats = np.zeros((J, 4, 4))
    quats[..., 3] = 1.0
    quats[1, :, 0] = np.linspace(0.0, 0.3, 4)
    runtime._test_ops = pe.PlaybackOps()
    (traj,) = playback.skin_trajectory([moved], [dv], [quats])
    assert tuple(traj.shape) == (len(dv), 4, 3) and np.abs(traj[:, 0].numpy() - dv).max() < 1e-6 and np.isfinite(traj.numpy()).all()
    assert np.abs(traj[:, 3].numpy() - dv).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_pointtri_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "pointtri_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "pointtri_host_check.cpp"), "-o", exe], check=True)
    sv, sf = to.torus(9, 7)
    dv, _ = to.torus(14, 11, r=0.23)
    rng = np.random.default_rng(5)
    grid_pts = np.array([t[0] for t in to.REGION_POINTS + to.DEGENERATE_POINTS] + [to.TIE_POINT, to.COLLAPSED_POINT])
    grid_tri = np.concatenate([to.REGION_TRIANGLE[None], to.DEGENERATE_TRIANGLE[None], to.TIE_VERTS[to.TIE_FACES], to.COLLAPSED_VERTS[to.COLLAPSED_FACES]])
    sets = [(dv, sv[sf]), (grid_pts, grid_tri), (rng.integers(-4, 5, (200, 3)) / 4.0, rng.integers(-4, 5, (40, 3, 3)) / 4.0),
            (dv[:3], np.zeros((0, 3, 3))), (np.zeros((0, 3)), sv[sf][:2]), (grid_pts, to.COLLAPSED_VERTS[to.COLLAPSED_FACES[:1]])]
    seen = set()
    for pts, tri in sets:
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("=ii", len(pts), len(tri)))
            fh.write(np.ascontiguousarray(pts, dtype=np.float64).tobytes())
            fh.write(np.ascontiguousarray(tri, dtype=np.float64).tobytes())
        done = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
        raw = open(dst, "rb").read()
        ints = np.frombuffer(raw[:8 * len(pts)], dtype=np.int32).reshape(-1, 2)
        real = np.frombuffer(raw[8 * len(pts):], dtype=np.float64).reshape(-1, 4)
        face, bary, dist, region = to.closest_face(pts, tri.reshape(-1, 3), np.arange(3 * len(tri)).reshape(-1, 3))
        assert same(ints[:, 0], face) and same(ints[:, 1], region.astype(np.int32)) and same(real[:, :3], bary)
        assert same(np.sqrt(real[:, 3]), dist)
        seen |= set(region.tolist())
    assert seen == {-1, 0, 1, 2, 3, 4, 5, 6}
