"""CPU: the work lists of the persistent kernels (csrc/tile_list.h: edge_pp.hip, edge_ws.hip, edge_rl.hip, gemm_dmap.hip) as the stand-alone
program tools/tile_list_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program (never loaded into
Python): for every tile count 0..300, grid 8..64 and run length 1, 2, 4, 8 every tile is visited exactly once, tile_of past the end of a
list repeats its last tile, and the tiles of a run are consecutive and stay with one owner."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_lists_under_the_sanitizers_visit_every_tile_once(tmp_path):
    exe = str(tmp_path / "tile_list_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "tile_list_host_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    # 301 tile counts x 8 grids x (the two tile lists together + 4 run lengths x the two run lists)
    assert done.stdout.strip() == f"ok {301 * 8 * (1 + 4 * 2)}"
