"""CPU: the kernel choice of morig_gemm / morig_edgeconv / morig_edge_hidden / morig_segmax_gemm / morig_edgeconv_x3
(csrc/dispatch_core.h: Switches, gemm_plan, edge_plan and the table of the tile engine's instantiations) as the stand-alone program
tools/dispatch_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program (never loaded into
Python). For every enumerated call, at default switches and with each switch alone at each non-default value: every accepted plan
names an instantiation that exists, every instantiation that exists is reached, the refusals the header documents hold,
NativeOps.gemm_takes_tail implies a tail-taking plan, and morig_edgeconv_can_split_out agrees with the launch plan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_plans_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "dispatch_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "dispatch_host_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    settings = 1 + 18                                        # default, then each switch alone at each non-default value
    # M x N x K x weight image x x_split x y_split x (no pool, pool, pool + Y) x row bias x Y alignment x tail
    gemm = 8 * 9 * 6 * 4 * 2 * 2 * 3 * 3 * 2 * 2
    # H x CSR form x split image x hidden affine x out_split x out alignment x replicas x exact_arith (morig_edgeconv + morig_edge_hidden)
    edge = 6 * 3 * 2 * 2 * 2 * 2 * 2 * 2
    segmax = 8 * 2                                           # N x split image
    x3 = 2 * 2 * 2                                           # H x split image x out alignment
    pairs = 4 * 3 * 11                                       # H x CSR form x combination of the paired-pass flags
    assert done.stdout.strip() == f"ok {settings * (gemm + edge + pairs + segmax + x3)}"
