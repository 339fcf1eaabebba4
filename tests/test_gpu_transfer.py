"""GPU: morig_amd/transfer.py (csrc/transfer.hip) against tests/transfer_oracle.py, bit for bit and with nothing excused -- the arithmetic
is the same on both sides: the recorded reference cases, the smallest shapes at which the kernels branch (the LDS tiles of 256 original
vertices and of 256 faces, the workgroup of 256 vertices, the flood's limit of 8 192), shallow and deep floods, unreachable vertices,
batches against the same meshes alone, determinism, and the transferred rig going through ``playback.skin_trajectory``."""
import json
import os

import numpy as np
import pytest
import torch

import transfer_oracle as to
from morig_amd import meshprep, native, playback, transfer
from morig_amd.formats import Rig

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_remesh.npz")


def host(t):
    return t.cpu().numpy()


def same_bits(got, want):
    """equal shapes, types and bits; every NaN counts as the same NaN"""
    got, want = host(got) if isinstance(got, torch.Tensor) else np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()
    return got.tobytes() == want.tobytes()


def run_remesh(cases, **kw):
    return transfer.transfer_to_remesh([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [to.PlainRig(c[3]) for c in cases],
                                       return_info=True, **kw)


def check_remesh(case, got, neighbours, unreachable="raise"):
    want = to.remesh_loop(*case, neighbours=neighbours, unreachable=unreachable)
    rig, source, info = got
    assert source.is_cuda and same_bits(source, want["source"]) and same_bits(info["sweep"], want["sweep"].astype(np.int32))
    assert same_bits(info["coincident"], want["coincident"].astype(np.int32)) and same_bits(info["nearest"], want["nearest"].astype(np.int32))
    assert same_bits(rig.skins, want["skins"]) and same_bits(rig.skins_device, want["skins"])
    return want


def chain_with_originals(n, n_ori, descending=True, J=4):
    """a chain of n vertices whose originals are n_ori of its vertices, evenly spread from the LAST index down: with one original the
    flood fills one vertex per sweep"""
    vr, faces = to.chain_mesh(n, descending)
    pick = np.unique(np.linspace(n - 1, 0, n_ori).astype(np.int64)) if n_ori else np.zeros(0, dtype=np.int64)
    vo = vr[pick][np.random.default_rng(n).permutation(len(pick))] if n_ori else np.zeros((0, 3))
    return vo, vr, faces, to.random_skins(len(vo), J, n + n_ori)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    names = json.loads(bytes(z["meta"]).decode())["cases"]
    return {n: tuple(z[f"{n}_{k}"] for k in ("vo", "vr", "faces", "skins_ori")) + (z[f"{n}_source"],) for n in names}


# ------------------------------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("neighbours", ["reference", "faces"])
def test_golden_cases_equal_the_oracle_and_the_reference(golden, neighbours):
    cases = [c[:4] for c in golden.values()]
    out = run_remesh(cases, neighbours=neighbours)
    for c, got in zip(golden.values(), out):
        check_remesh(c[:4], got, neighbours)
        if neighbours == "reference":
            assert np.array_equal(host(got[1]), c[4])                                   # what the reference itself recorded


@pytest.mark.parametrize("neighbours", ["reference", "faces"])
def test_original_counts_around_the_tile_and_remeshed_counts_around_the_workgroup(neighbours):
    cases = [chain_with_originals(300, n) for n in (1, 255, 256, 257)] + [chain_with_originals(n, 20, descending=n != 256) for n in (255, 256, 257)]
    cases += [chain_with_originals(257, 1), to.remesh_case(20, 26, 9, 4)]               # 520 vertices: three workgroups
    cases += [chain_with_originals(n, 40) for n in (1023, 1024, 1025)]                  # around the flood's 1 024 threads
    sweeps = [check_remesh(c, got, neighbours)["n_sweeps"] for c, got in zip(cases, run_remesh(cases, neighbours=neighbours))]
    assert neighbours == "reference" or (sweeps[0] == 299 and sweeps[5] == 1 and sweeps[7] == 256)   # one sweep, and many


def test_a_mesh_without_originals_is_refused_under_both_options():
    c = chain_with_originals(40, 0)
    for unreachable in ("raise", "nearest"):
        with pytest.raises(transfer.TransferError, match="40 of 40"):
            run_remesh([c], unreachable=unreachable)


@pytest.mark.parametrize("neighbours", ["reference", "faces"])
def test_the_largest_supported_mesh_and_one_vertex_beyond(neighbours):
    vo, vr, faces, skins = to.remesh_case(64, 128, 40, 6, J=3)
    assert len(vr) == transfer.MAX_FLOOD_VERTS == 8192
    (got,) = run_remesh([(vo, vr, faces, skins)], neighbours=neighbours)
    want = check_remesh((vo, vr, faces, skins), got, neighbours)
    assert want["n_sweeps"] >= 1 and want["n_unreachable"] == 0
    beyond = np.concatenate([vr, vr[:1] + 1.0])
    with pytest.raises(ValueError, match="at most 8192 per mesh"):
        run_remesh([(vo, beyond, faces, skins)], neighbours=neighbours)


def test_the_library_refuses_the_flood_beyond_its_limit():
    ops, dev = native.get_ops(), "cuda"
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)
    with pytest.raises(native.MorigNativeError):
        ops.transfer_flood(torch.zeros(3, 3, dtype=torch.float64, device=dev), torch.tensor([0, 3], dtype=torch.int32, device=dev), 8193, z(4),
                           z(0, torch.int64), z(3), z(3), False, z(2))


def test_unreachable_vertices_and_bad_input():
    vo, vr, faces, skins = to.remesh_case(6, 6, 5, 8)
    lone = np.concatenate([vr, [[5.0, 5.0, 5.0]]])
    island_v, island_f = np.concatenate([vr, vr + 10.0]), np.concatenate([faces, faces + len(vr)])
    a, b = (vo, lone, faces, skins), (vo, island_v, island_f, skins)
    with pytest.raises(transfer.TransferError, match="mesh 1: 1 of 37"):
        run_remesh([(vo, vr, faces, skins), a])
    with pytest.raises(transfer.TransferError, match="mesh 0: 36 of 72"):
        run_remesh([b, a], neighbours="faces")
    for c, got in zip((a, b), run_remesh([a, b], neighbours="faces", unreachable="nearest")):
        want = check_remesh(c, got, "faces", "nearest")
        assert (want["sweep"] == -1).any() and (want["source"] >= 0).all()
    with pytest.raises(ValueError, match="outside its mesh"):
        run_remesh([(vo, vr, faces + 1, skins)])
    bad = vr.copy()
    bad[5, 2] = np.nan
    with pytest.raises(ValueError, match="1e\\+07"):
        run_remesh([(vo, bad, faces, skins)])


def test_a_mixed_batch_equals_its_meshes_alone(golden):
    cases = [golden["quirk"][:4], chain_with_originals(257, 3), golden["underflow"][:4], to.remesh_case(20, 26, 9, 4), golden["root_tie"][:4],
             (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 2))), chain_with_originals(90, 256, descending=False)]
    for neighbours in ("reference", "faces"):
        batch, again = run_remesh(cases, neighbours=neighbours), run_remesh(cases, neighbours=neighbours)
        for c, got, rerun in zip(cases, batch, again):
            (alone,) = run_remesh([c], neighbours=neighbours)
            for x, y, z in zip((got[0].skins_device, got[1], got[2]["sweep"]), (alone[0].skins_device, alone[1], alone[2]["sweep"]),
                               (rerun[0].skins_device, rerun[1], rerun[2]["sweep"])):
                assert same_bits(x, host(y)) and same_bits(x, host(z))


SEGMENT_EDGES = [0, 1, 256, 0, 257, 255, 0]                    # empty meshes in front, between and behind; a full workgroup, one row more, one less


def test_remeshed_counts_at_the_segment_edges_equal_the_meshes_alone_and_the_oracle():
    empty = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 2)))
    cases = [chain_with_originals(n, min(n, 3), descending=False) if n else empty for n in SEGMENT_EDGES]
    for c, got in zip(cases, run_remesh(cases, neighbours="faces")):
        check_remesh(c, got, "faces")
        (alone,) = run_remesh([c], neighbours="faces")
        for x, y in zip((got[0].skins_device, got[1], got[2]["sweep"], got[2]["coincident"], got[2]["nearest"]),
                        (alone[0].skins_device, alone[1], alone[2]["sweep"], alone[2]["coincident"], alone[2]["nearest"])):
            assert same_bits(x, host(y)), len(c[1])


# ------------------------------------------------------------------------------------------------------------------------- part B
def check_surface(case, got):
    want = to.transfer_skins(*case)
    skins, face, bary, dist = got
    assert skins.is_cuda and same_bits(face, want["face"]) and same_bits(bary, want["bary"]) and same_bits(dist, want["distance"])
    assert same_bits(skins, want["skins"])
    return want


def surface_case(n_faces, n_dst, seed, J=5):
    sv, sf = to.torus(16, 9)                                                            # 144 vertices, 288 faces
    rng = np.random.default_rng(seed)
    dv = to.torus(23, 17)[0][rng.permutation(23 * 17)[:n_dst]] + rng.normal(size=(n_dst, 3)) * 0.02
    return sv, sf[rng.permutation(len(sf))[:n_faces]], to.random_skins(len(sv), J, seed), dv


def test_face_counts_around_the_tile_and_destination_counts_around_the_block():
    cases = [surface_case(nf, 70, nf) for nf in (0, 1, 255, 256, 257)] + [surface_case(288, nd, nd, J=3) for nd in (255, 256, 257, 0)]
    out = transfer.transfer_skins(*[[c[k] for c in cases] for k in range(4)])
    wants = [check_surface(c, got) for c, got in zip(cases, out)]
    assert (wants[0]["face"] == -1).all() and not wants[0]["skins"].any() and (wants[5]["face"] >= 256).any() and len(set(wants[6]["region"])) >= 3


def test_destination_counts_at_the_segment_edges_equal_the_meshes_alone_and_the_oracle():
    cases = [surface_case(288, nd, 1000 + nd, J=3) for nd in SEGMENT_EDGES]
    for c, got in zip(cases, transfer.transfer_skins(*[[c[k] for c in cases] for k in range(4)])):
        check_surface(c, got)
        (alone,) = transfer.transfer_skins(*[[c[k]] for k in range(4)])
        assert all(same_bits(x, host(y)) for x, y in zip(got, alone)) and tuple(got[0].shape) == (len(c[3]), 3)


def test_regions_degenerate_triangles_and_ties_on_the_grid():
    eye = np.eye(3)
    grid = [(tri, np.arange(3).reshape(1, 3), eye, np.array([t[0] for t in table]))
            for tri, table in ((to.REGION_TRIANGLE, to.REGION_POINTS), (to.DEGENERATE_TRIANGLE, to.DEGENERATE_POINTS))]
    grid.append((to.TIE_VERTS, to.TIE_FACES, np.eye(4), np.array([to.TIE_POINT])))
    grid.append((to.TIE_VERTS, to.TIE_FACES[::-1].copy(), np.eye(4), np.array([to.TIE_POINT])))
    grid.append((to.COLLAPSED_VERTS, to.COLLAPSED_FACES, np.eye(4), np.array([to.COLLAPSED_POINT])))
    out = transfer.transfer_skins(*[[c[k] for c in grid] for k in range(4)])
    for c, got in zip(grid, out):
        check_surface(c, got)
    for (skins, face, bary, dist), table in zip(out[:2], (to.REGION_POINTS, to.DEGENERATE_POINTS)):
        assert host(bary).tolist() == [t[2] for t in table] and host(dist).tolist() == [float(np.sqrt(t[3])) for t in table]
    assert host(out[2][1]).tolist() == [0] and host(out[3][1]).tolist() == [0] and host(out[2][2]).tolist() == [[0.5, 0.0, 0.5]]
    assert host(out[4][1]).tolist() == [1] and host(out[4][2]).tolist() == [[0.75, 0.25, 0.0]]
    with pytest.raises(ValueError, match="outside its mesh"):
        transfer.transfer_skins([to.TIE_VERTS], [to.TIE_FACES + 3], [np.eye(4)], [[to.TIE_POINT]])


@pytest.fixture(scope="module")
def simplified_tori():
    originals = [to.torus(24, 16), to.torus(20, 12, R=0.4, r=0.15), to.torus(30, 10, r=0.1)]
    simple = meshprep.simplify([o[0] for o in originals], [o[1] for o in originals], target_faces=200)
    return originals, [(host(s[0]), host(s[1])) for s in simple]


def test_simplified_tori_back_to_their_originals_twice(simplified_tori):
    originals, simple = simplified_tori
    cases = [(sv, sf, to.random_skins(len(sv), 4 + b, b), ov) for b, ((ov, _), (sv, sf)) in enumerate(zip(originals, simple))]
    assert all(0 < len(c[1]) <= 200 and len(c[3]) >= 240 for c in cases)
    args = [[c[k] for c in cases] for k in range(4)]
    first, second = transfer.transfer_skins(*args), transfer.transfer_skins(*args)
    for c, got, again in zip(cases, first, second):
        want = check_surface(c, got)
        assert all(same_bits(x, host(y)) for x, y in zip(got, again))
        assert (want["skins"] >= 0).all() and np.abs(want["skins"].sum(1) - 1.0).max() < 1e-7 and len(set(want["region"])) >= 3
    (alone,) = transfer.transfer_skins(*[[c] for c in cases[1]])
    assert all(same_bits(x, host(y)) for x, y in zip(first[1], alone))


# ------------------------------------------------------------------------------------------------------------------------- end to end
def test_a_rig_of_the_simplified_mesh_plays_back_on_the_original(simplified_tori):
    originals, simple = simplified_tori
    J, T = 6, 5
    rng = np.random.default_rng(1)
    rigs = [Rig.from_arrays(rng.uniform(-0.3, 0.3, (J, 3)), [-1, 0, 0, 1, 1, 2], 0, skins=to.random_skins(len(sv), J, 10 + b))
            for b, (sv, _) in enumerate(simple)]
    moved = transfer.transfer_rigs(rigs, simple, [o[0] for o in originals])
    quats = np.zeros((J, T, 4))
    quats[..., 3] = 1.0
    quats[1, :, 2] = np.linspace(0.0, 0.4, T)
    traj = playback.skin_trajectory(moved, [o[0] for o in originals], [quats] * len(moved))
    for rig, src_rig, (ov, _), (sv, sf), tr in zip(moved, rigs, originals, simple, traj):
        want = to.transfer_skins(sv, sf, src_rig.skins, ov)
        assert same_bits(rig.skins, want["skins"]) and rig.skins.shape == (len(ov), J)
        assert (rig.skins >= 0).all() and np.abs(rig.skins.sum(1) - 1.0).max() < 1e-7                  # the 1e-8 term
        assert tuple(tr.shape) == (len(ov), T, 3) and bool(torch.isfinite(tr).all())
        assert np.abs(host(tr[:, 0]) - ov).max() < 1e-6 and np.abs(host(tr[:, T - 1]) - ov).max() > 1e-3
