"""CPU: (1) morig_amd/ragged.py, the host vocabulary of the ragged batches: the prefix sum, the int32 upload and its bound, the ptr
validation, the device rule under the test seam; (2) csrc/ragged_core.h as the stand-alone program tools/ragged_host_check.cpp, built with
the address and undefined-behaviour sanitizers and run as a program (never loaded into Python), against numpy's searchsorted on every
ascending ptr of up to 6 segments: segment_of, and block_row over the workgroup tables ragged.blocks makes."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from morig_amd import geodesic, ragged, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _RecordingOps:
    """an op layer that records what nearest_point is called with"""

    def __init__(self):
        self.calls = []

    def nearest_point(self, v, v_ptr, p, p_ptr, squared):
        self.calls.append((v, v_ptr, p, p_ptr, squared))
        return torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)


@pytest.fixture()
def seam():
    ops = _RecordingOps()
    runtime._test_ops = ops
    try:
        yield ops
    finally:
        runtime._test_ops = None


# ------------------------------------------------------------------------------------------------------------------- the host vocabulary
def test_ptr_of_on_empty_single_and_zero_counts():
    for counts, want in (([], [0]), ([5], [0, 5]), ([0], [0, 0]), ([2, 0, 0, 3], [0, 2, 2, 2, 5]), (np.array([1, 2], dtype=np.int32), [0, 1, 3])):
        got = ragged.ptr_of(counts)
        assert got.dtype == np.int64 and got.tolist() == want
    big = ragged.ptr_of(np.array([2 ** 31 - 1, 2], dtype=np.int32))          # summed in int64, whatever the counts' type
    assert big.tolist() == [0, 2 ** 31 - 1, 2 ** 31 + 1]


def test_int32_table_takes_the_last_int32_and_refuses_the_next():
    t = ragged.int32_table(np.array([0, 2 ** 31 - 1]), "cpu", "some_function")
    assert t.dtype == torch.int32 and t.device.type == "cpu" and t.tolist() == [0, 2 ** 31 - 1]
    with pytest.raises(ValueError, match="some_function"):
        ragged.int32_table(np.array([0, 2 ** 31]), "cpu", "some_function")
    assert ragged.int32_table([], "cpu", "some_function").shape == (0,)
    assert ragged.int32_table([0, 3, 7], "cpu", "some_function").tolist() == [0, 3, 7]


def test_a_geodesic_table_past_int32_raises_instead_of_wrapping():
    """what geodesic.py's uploads did before: astype(np.int32) on 2^31 gives -2^31, silently"""
    assert np.array([0, 2 ** 31]).astype(np.int32)[1] == -2 ** 31
    with pytest.raises(ValueError, match="surface_geodesic_samples"):
        ragged.int32_table(ragged.ptr_of([2 ** 30, 2 ** 30]), "cpu", "surface_geodesic_samples")


def test_check_ptr_takes_a_good_ptr_and_names_what_it_refuses():
    for good in ([0, 2, 2, 5], np.array([0, 5], dtype=np.int32), torch.tensor([0, 0, 5])):
        p = ragged.check_ptr(good, 5, "f: ptr")
        assert p.dtype == np.int64 and p.tolist() == np.asarray(good).tolist()
    assert ragged.check_ptr([0, 0], 0, "f: ptr").tolist() == [0, 0]
    bad = {"does not start at 0": [1, 2, 5], "does not end at n": [0, 2, 4], "descends": [0, 3, 2, 5], "float": [0.0, 2.0, 5.0],
           "length 1": [0], "length 0": [], "two-dimensional": [[0, 5]]}
    for name, ptr in bad.items():
        with pytest.raises(ValueError, match="f: ptr"):
            ragged.check_ptr(ptr, 5, "f: ptr")
            pytest.fail(f"check_ptr accepted a ptr that {name}")


def test_device_of_under_the_seam(seam):
    a, b = torch.zeros(3), np.zeros(3)
    assert ragged.device_of(a, b) == torch.device("cpu")
    assert ragged.device_of() == torch.device("cpu")
    assert ragged.device_of(a, device="meta") == torch.device("meta")                # an explicit device wins
    assert ragged.device_of(a, device=torch.device("cuda", 1)) == torch.device("cuda", 1)
    assert ragged.device_of(torch.zeros(3, device="meta"), a) == torch.device("cpu")  # only CUDA tensors name a device


def test_geodesic_resolves_cpu_inputs_to_cpu_under_the_seam(seam):
    """geodesic.py used to reach for the current CUDA device whatever was installed; the tables it uploads are int32 prefix sums"""
    verts, pts = np.zeros((5, 3)), np.ones((4, 3))
    out = geodesic.nearest_sample(verts, pts, v_ptr=[0, 2, 5], p_ptr=torch.tensor([0, 1, 4]), squared=True)
    (v, v_ptr, p, p_ptr, squared), = seam.calls
    assert out.shape == (5,) and squared is True
    assert all(t.device.type == "cpu" for t in (v, v_ptr, p, p_ptr))
    assert v_ptr.dtype == p_ptr.dtype == torch.int32 and v_ptr.tolist() == [0, 2, 5] and p_ptr.tolist() == [0, 1, 4]
    with pytest.raises(ValueError, match="nearest_sample: ptr"):
        geodesic.nearest_sample(verts, pts, v_ptr=[0, 3, 2, 5], p_ptr=[0, 1, 2, 4])


def test_as_tensor_cat_to():
    t = torch.arange(3)
    assert ragged.as_tensor(t) is t and ragged.as_tensor([1, 2]).tolist() == [1, 2]
    c = ragged.cat_to([np.zeros((2, 3), dtype=np.float32), torch.ones(1, 3, dtype=torch.float64)], "cpu", torch.float64)
    assert c.dtype == torch.float64 and c.shape == (3, 3) and c.is_contiguous() and c[2].tolist() == [1.0, 1.0, 1.0]
    assert ragged.cat_to([torch.zeros(2, dtype=torch.int32), torch.ones(1, dtype=torch.int32)], "cpu").dtype == torch.int32


# ------------------------------------------------------------------------------------------------------------------- the device lookup
def _expected(ptr, queries):
    """numpy's statement of segment_of: the last b in [0, n) with ptr[b] <= i, 0 when there is none or n <= 1"""
    n = len(ptr) - 1
    if n <= 1:
        return [0] * len(queries)
    return np.clip(np.searchsorted(np.asarray(ptr, dtype=np.int64), queries, side="right") - 1, 0, n - 1).tolist()


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ragged") / "ragged_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "ragged_host_check.cpp"), "-o", exe], check=True)
    return exe


def test_segment_of_under_the_sanitizers_equals_searchsorted(host_check, tmp_path):
    exe = host_check
    small = list(range(-1, 6))                                                      # -1 .. one past the largest end
    cases = [(list(ptr), small) for n in range(0, 7) for ptr in itertools.combinations_with_replacement(range(5), n + 1)]
    assert len(cases) == 791 and ([0, 0, 2, 2, 4, 4, 4], small) in cases and ([3], small) in cases and ([0, 4], small) in cases
    n_small = len(cases)
    wide = [2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + 2, -2 ** 32 + 1]  # narrowed to 32 bits these would read -1, 0, 1, 2
    cases.append(([0, 1, 3], wide))                                                # 64-bit rows over an int32 table
    cases.append(([0, 2 ** 31, 2 ** 32 + 1, 2 ** 33], wide + [0, 1]))              # a 64-bit table (pair and sample offsets)
    src = str(tmp_path / "in.txt")
    with open(src, "w") as f:
        f.write(f"{len(cases)}\n")
        for ptr, queries in cases:
            f.write(f"{len(ptr) - 1} {len(queries)}\n{' '.join(map(str, ptr))}\n{' '.join(map(str, queries))}\n")
    done = subprocess.run([exe, src], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    lines = done.stdout.split("\n")
    assert len(lines) == 4 * len(cases) + 1 and lines[-1] == ""
    for k, (ptr, queries) in enumerate(cases):
        want = " ".join(map(str, _expected(ptr, queries)))
        got = lines[4 * k:4 * k + 4]                                                # (int32, int), (int32, int64), (int64, int), (int64, int64)
        if k < n_small:
            assert got == [want] * 4, (ptr, got, want)
        elif k == n_small:
            assert got == ["-", want, "-", want], (ptr, got, want)
        else:
            assert got == ["-", "-", "-", want], (ptr, got, want)
    assert _expected([0, 1, 3], wide) == [1, 1, 1, 1, 1, 0] and _expected([0, 2, 2, 5], [1, 2, 4, 5]) == [0, 2, 2, 2]


def test_block_row_under_the_sanitizers_enumerates_every_row_once(host_check, tmp_path):
    """every ascending row ptr of up to 6 segments over range(5), at 1, 2 and 3 rows per workgroup, with the blk_ptr ragged.blocks makes:
    the live (seg, row) of all (workgroup, thread) pairs are every row of every segment exactly once, in numpy's searchsorted order"""
    cases = [(list(ptr), width) for width in (1, 2, 3) for n in range(0, 7) for ptr in itertools.combinations_with_replacement(range(5), n + 1)]
    assert len(cases) == 3 * 791
    src = str(tmp_path / "in.txt")
    tables = []
    with open(src, "w") as f:
        f.write(f"{len(cases)}\n")
        for ptr, width in cases:
            blk, n_blk = ragged.blocks(np.diff(ptr), width, "cpu", "test")
            tables.append(blk.numpy().astype(np.int64))
            assert n_blk == tables[-1][-1]
            f.write(f"{len(ptr) - 1} {width}\n{' '.join(map(str, ptr))}\n{' '.join(map(str, tables[-1].tolist()))}\n")
    done = subprocess.run([host_check, "--block-row", src], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    lines = done.stdout.split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1] == ""
    for (ptr, width), blk, line in zip(cases, tables, lines):
        got = [tuple(map(int, w.split(":"))) for w in line.split()]
        rows = np.diff(ptr)
        assert sorted(got) == [(b, r) for b in range(len(rows)) for r in range(rows[b])] and len(set(got)) == len(got), (ptr, width, got)
        g, t = np.divmod(np.arange(int(blk[-1]) * width), width)                    # numpy's statement, in (workgroup, thread) order
        seg = np.clip(np.searchsorted(blk, g, side="right") - 1, 0, max(len(rows) - 1, 0))
        row = (g - blk[seg]) * width + t
        live = (row >= 0) & (row < rows[seg]) if len(rows) else np.zeros(0, dtype=bool)
        assert got == list(zip(seg[live].tolist(), row[live].tolist())), (ptr, width, got)
