"""CPU: tests/scan_oracle.py held to known answers -- a sphere's depth image against the analytic ray-sphere depth, the visibility of a convex
mesh against the facing of its faces, a plate hidden behind a plate -- the share of near-margin pixels and vertices on the scenes of the
GPU tests, and csrc/raytri_core.h as the stand-alone program tools/raytri_host_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program (never loaded into Python), against the oracle bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scan_oracle as so
from morig_amd import scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = {"orthographic": lambda W, H: scan.Camera.orthographic((0.4, 0.3, 4.0), (0, 0, 0), (0, 1, 0), 1.2, 1.2 * H / W, W, H),
        "pinhole": lambda W, H: scan.Camera.pinhole((0.4, 0.3, 4.0), (0, 0, 0), (0, 1, 0), 35.0, W, H)}


def test_module_exists_and_camera_rules():
    c = scan.Camera.orthographic(**so.on_grid_camera(63, 5))
    assert c.px == 0.5 and c.py == 0.5 and np.array_equal(c.f, [0, 0, -1]) and np.array_equal(c.r, [1, 0, 0]) and np.array_equal(c.u, [0, 1, 0])
    o, d = so.pixel_rays(c.row(), c.kind, 63, 5)
    assert np.array_equal(o[..., 0], np.broadcast_to(np.arange(63) + 0.5, (5, 63))) and np.array_equal(o[:, 0, 1], 5 - np.arange(5) - 0.5)
    p = scan.Camera.pinhole((0, 0, 2), (0, 0, 0), (0, 1, 0), 90.0, 128, 64)
    assert p.near == 1e-3 and abs(p.py * 64 - 1.0) < 1e-15 and abs(p.px * 128 - 2.0) < 1e-15
    for w in (0, 1025):
        with pytest.raises(ValueError):
            scan.Camera.orthographic((0, 0, 1), (0, 0, 0), (0, 1, 0), 1, 1, w, 8)
        with pytest.raises(ValueError):
            scan.Camera.pinhole((0, 0, 1), (0, 0, 0), (0, 1, 0), 60, 8, w)


def _sphere_depth(o, d, radius):
    """the smaller root of |o + t d|^2 = radius^2 per ray, nan where the ray misses"""
    a, b, c = so.dot3(d, d), so.dot3(o, d), so.dot3(o, o) - radius * radius
    with np.errstate(invalid="ignore"):
        return (-b - np.sqrt(b * b - a * c)) / a


@pytest.mark.parametrize("kind", sorted(CAMS))
def test_sphere_depth_is_the_analytic_depth_within_the_sagitta(kind):
    """The 32 x 16 sphere is a convex polyhedron inscribed in the unit sphere. A face with circumradius rho lies in a plane at distance
    sqrt(1 - rho^2) from the centre, so the polyhedron contains the ball of radius h = sqrt(1 - max rho^2) and lies inside the unit ball:
    1 - h is its largest sagitta. Along any ray that meets the inner ball the polyhedron's depth therefore lies between the depth of the
    unit sphere and that of the inner sphere; a ray that misses the unit sphere hits nothing."""
    verts, faces = so.sphere(32, 16)
    assert len(faces) == 2 * 32 + 2 * 32 * 14 and np.allclose(np.linalg.norm(verts, axis=1), 1.0, atol=1e-15)
    A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    la, lb, lc = np.linalg.norm(B - C, axis=1), np.linalg.norm(C - A, axis=1), np.linalg.norm(A - B, axis=1)
    rho = la * lb * lc / (2 * np.linalg.norm(np.cross(B - A, C - A), axis=1))           # abc / (4 area)
    h = np.sqrt(1 - rho.max() ** 2)
    W, H = 80, 64
    cam = CAMS[kind](W, H)
    img = so.render(verts, faces, cam.row(), cam.kind, W, H)
    o, d = so.pixel_rays(cam.row(), cam.kind, W, H)
    outer, inner = _sphere_depth(o, d, 1.0), _sphere_depth(o, d, h)
    hit = img["face"] >= 0
    print(f"{kind}: sagitta {1 - h:.4f}, {int(hit.sum())} hit pixels, {int((~np.isnan(inner)).sum())} rays into the inner ball")
    assert 0.005 < 1 - h < 0.02 and hit.sum() > 500                                    # about 1 - cos(pi / 32) twice over: a quad's diagonal
    assert not hit[np.isnan(outer)].any() and hit[~np.isnan(inner)].all()
    sure = ~np.isnan(inner)
    assert np.all(img["depth"][sure] >= outer[sure] - 1e-12) and np.all(img["depth"][sure] <= inner[sure] + 1e-12)
    assert np.all(img["depth"][hit] >= outer[hit] - 1e-12) and np.all(np.isinf(img["depth"][~hit]))
    p = img["point"][hit]
    assert np.all(np.linalg.norm(p, axis=1) <= 1 + 1e-12) and np.all(np.linalg.norm(p, axis=1) >= h - 1e-12)


def test_a_convex_mesh_shows_exactly_its_front_facing_vertices():
    """From infinitely far away a vertex of a convex polyhedron is seen when one of its faces looks at the camera (normal . f < 0).
    Vertices with a face within 1e-9 of edge-on are left out."""
    verts, faces = so.sphere(32, 16)
    verts = verts @ so.rotation(3).T
    cam = scan.Camera.orthographic((1.0, 2.0, 5.0), (0, 0, 0), (0, 1, 0), 1.5, 1.5, 64, 64)
    vis, firm = so.visibility(verts, faces, cam.row(), cam.kind, 64, 64, 1e-4)
    n = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.sign(np.sum(n * verts[faces].mean(axis=1), axis=1, keepdims=True))             # outward
    facing = n @ cam.f
    front, edge_on = np.zeros(len(verts), dtype=bool), np.zeros(len(verts), dtype=bool)
    for k in range(3):
        np.logical_or.at(front, faces[:, k], facing < 0)
        np.logical_or.at(edge_on, faces[:, k], np.abs(facing) < 1e-9)
    assert edge_on.sum() < 5 and 100 < front.sum() < len(verts) - 100
    assert np.array_equal(vis[~edge_on] != 0, front[~edge_on])
    assert firm.mean() > 0.99


def test_a_plate_behind_a_plate_is_invisible():
    near_plate = np.array([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)
    far_plate = near_plate * [0.5, 0.5, 1] + [0.1, -0.2, -2]
    verts, faces = np.concatenate([near_plate, far_plate]), np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    for cam in (scan.Camera.orthographic((0, 0, 5), (0, 0, 0), (0, 1, 0), 2, 2, 32, 32), scan.Camera.pinhole((0, 0, 5), (0, 0, 0), (0, 1, 0), 60, 32, 32)):
        vis, firm = so.visibility(verts, faces, cam.row(), cam.kind, 32, 32, 1e-4)
        assert vis.tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and firm.all()
        img = so.render(verts, faces, cam.row(), cam.kind, 32, 32)
        assert set(np.unique(img["face"])) <= {-1, 0, 1}                                 # the far plate is nowhere in the image
    away = scan.Camera.orthographic((0, 0, 5), (0, 0, 10), (0, 1, 0), 2, 2, 32, 32)       # both plates behind the image plane
    assert not so.visibility(verts, faces, away.row(), away.kind, 32, 32, 1e-4)[0].any()


def test_nearest_takes_the_lowest_index_and_respects_the_mask():
    t = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], dtype=np.float64)
    q = np.array([[1, 1, 0], [1.5, 1, 0], [9, 9, 9]], dtype=np.float64)
    idx, d2 = so.nearest(q, t)
    assert idx.tolist() == [0, 1, 3] and d2[:2].tolist() == [2.0, 1.25]
    idx, d2 = so.nearest(q, t, np.array([0, 0, 1, 1], dtype=np.uint8))
    assert idx.tolist() == [2, 3, 3]
    idx, d2 = so.nearest(q, t, np.zeros(4, dtype=np.uint8))
    assert idx.tolist() == [-1, -1, -1] and np.all(np.isinf(d2))


@pytest.mark.parametrize("scene", ["torus", "triangles"])
@pytest.mark.parametrize("cam_name", ["orthographic", "pinhole"])
def test_generated_gpu_scenes_leave_out_at_most_a_thousandth(scene, cam_name):
    """the cap of the GPU tests (tests/test_gpu_scan.py), shown here without a device: pixels and vertices within MARGIN of flipping"""
    kw = so.generated_cameras(so.GEN_W, so.GEN_H)[cam_name]
    cam = getattr(scan.Camera, cam_name)(**kw)
    img, vis, firm = so.generated_reference(scene, tuple(cam.row()), cam.kind)
    hits, loose = int((img["face"] >= 0).sum()), int((img["margin"] < so.MARGIN).sum())
    print(f"{scene} / {cam_name}: {hits} hit pixels, {loose} within {so.MARGIN} of flipping; {int(vis.sum())} of {len(vis)} vertices visible, "
          f"{int((~firm).sum())} not firm")
    assert hits > 800 and loose <= 0.001 * hits
    assert (~firm).sum() <= 0.001 * len(vis) and 0 < vis.sum() < len(vis)


# ------------------------------------------------------------------------------------------------------------------------- raytri_core.h
def _decisions():
    """(rows [n, 16], exact bool [n]): rays and triangles, a good third of them on a quarter-integer grid where every product is exact --
    with rays through edges and corners, parallel to the plane, and triangles behind the origin among them"""
    rng = np.random.default_rng(11)
    rows, exact = [], []

    def add(o, d, A, B, C, near, ex):
        rows.append(np.concatenate([o, d, A, B, C, [near]]).astype(np.float64))
        exact.append(ex)
    for _ in range(1500):                                                                  # on grid, rays along -z from half-integer pixels
        tri = rng.integers(-8, 9, size=(3, 3)) / 4.0
        tri[:, 2] = rng.integers(-3, 4, size=3)
        o = np.array([rng.integers(-4, 5) + 0.5, rng.integers(-4, 5) + 0.5, 4.0])
        add(o, [0, 0, -1], *tri, 0.0, True)
    for _ in range(400):                                                                   # through a corner, along an edge point
        tri = rng.integers(-6, 7, size=(3, 3)).astype(np.float64)
        k, w = rng.integers(0, 3), rng.integers(0, 5) / 4.0
        on = tri[k] if rng.random() < 0.5 else (1 - w) * tri[k] + w * tri[(k + 1) % 3]
        z0 = float(rng.integers(8, 12)) * (1 if rng.random() < 0.8 else -1)                # some triangles lie behind the origin
        add([on[0], on[1], z0], [0, 0, -1], *tri, 0.0, True)
    for _ in range(200):                                                                   # in the triangle's plane: det == 0
        tri = rng.integers(-6, 7, size=(3, 3)).astype(np.float64)
        tri[:, 2] = 1.0
        add([rng.integers(-8, 9), rng.integers(-8, 9), 1.0], [1, rng.integers(-2, 3), 0], *tri, 0.0, True)
    for _ in range(3000):                                                                  # generic
        tri = rng.normal(size=(3, 3))
        o = rng.normal(size=3) * 3
        d = tri.mean(axis=0) + rng.normal(scale=0.6, size=3) - o
        add(o, d, *tri, float(rng.choice([0.0, 1e-3, 0.5])), False)
    bad = np.zeros(16)
    for v in (np.nan, np.inf, -np.inf, 1e308):                                             # must not trip the sanitizers
        r = bad.copy()
        r[:] = [0.5, 0.5, 4, 0, 0, -1, 0, 0, v, 2, 0, 0, 0, 2, 0, 0]
        rows.append(r)
        exact.append(False)
    return np.stack(rows), np.array(exact)


def test_raytri_core_under_the_sanitizers_equals_the_oracle_bit_for_bit(tmp_path):
    exe = str(tmp_path / "raytri_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "raytri_host_check.cpp"), "-o", exe], check=True)
    rows, exact = _decisions()
    cams, px = [], []
    for W, H, cam in [(63, 5, scan.Camera.orthographic(**so.on_grid_camera(63, 5))), (65, 3, scan.Camera.orthographic(**so.on_grid_camera(65, 3))),
                      (40, 30, CAMS["pinhole"](40, 30)), (40, 30, CAMS["orthographic"](40, 30))]:
        for i in range(H):
            for j in range(W):
                cams.append(cam.row())
                px.append([cam.kind, W, H, i, j])
    cams, px = np.stack(cams), np.array(px, dtype=np.int32)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(rows)))
        f.write(np.ascontiguousarray(rows).tobytes())
        f.write(struct.pack("i", len(cams)))
        f.write(np.ascontiguousarray(cams).tobytes())
        f.write(np.ascontiguousarray(px).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    raw = np.frombuffer(open(dst, "rb").read(), dtype=np.float64)
    assert raw.size == 6 * (len(rows) + len(cams))
    got, rays = raw[:6 * len(rows)].reshape(-1, 6), raw[6 * len(rows):].reshape(-1, 6)
    det, un, vn, tn = so.numerators(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12], rows[:, 12:15])
    with np.errstate(all="ignore"):
        t = tn / det
        hit = so.inside(det, un, vn, tn) & (t > rows[:, 15])
    want = np.stack([hit.astype(np.float64), det, un, vn, tn, np.where(hit, t, 0.0)], 1)
    fin = np.isfinite(want).all(axis=1)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(got[fin]), bits(want[fin])) and np.array_equal(got[:, 0], want[:, 0]) and not got[~fin, 0].any()
    n_exact = int(exact.sum())
    on_edge = exact & hit & ((un == 0) | (vn == 0) | (un + vn == det))
    print(f"raytri_core.h vs the oracle: {len(rows)} decisions, {int(hit.sum())} hits, {n_exact} exact ({int((exact & hit).sum())} hits, "
          f"{int(on_edge.sum())} on an edge or corner, {int((exact & (det == 0)).sum())} parallel, {int((exact & ~hit & so.inside(det, un, vn, tn)).sum())} behind)")
    assert len(rows) >= 5000 and n_exact >= len(rows) / 3 and on_edge.sum() > 100 and (exact & (det == 0)).sum() > 100
    assert (exact & ~hit & so.inside(det, un, vn, tn)).sum() > 20 and (exact & hit).sum() > 300 and (~exact & hit).sum() > 300
    at = 0
    for W, H, kind in [(63, 5, 0), (65, 3, 0), (40, 30, 1), (40, 30, 0)]:
        o, d = so.pixel_rays(cams[at], kind, W, H)
        assert np.array_equal(bits(rays[at:at + W * H, :3]), bits(o.reshape(-1, 3))) and np.array_equal(bits(rays[at:at + W * H, 3:]), bits(d.reshape(-1, 3)))
        at += W * H
