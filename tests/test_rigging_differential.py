"""csrc/rig_assemble.hip on the device at the sizes its kernels branch on: the generated rigs of tests/rigging_cases.py (conditions
asserted on the CPU by tests/test_rigging_cases.py) through ``rigging.assemble_rigs`` as one ragged batch, and hand-made CSR tables
through ``get_ops().rig_assemble``. Everything is copies and fixed-order float64 sums of identical inputs: the bar is bit equality, with
the shared compare functions. Every device result is computed once and shared."""
import numpy as np
import pytest
import torch

import rigging_cases as rc
import rigging_emulate
from morig_amd import rigging
from morig_amd.runtime import get_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def batch(keep):
    return cached(("batch", keep), lambda: rc.run_batch(rc.cases(), DEV, keep))


# ------------------------------------------------------------------------------------------------------------------- entry chunks
@pytest.mark.parametrize("keep", [False, True], ids=["final", "dup"])
@pytest.mark.parametrize("k", range(len(rc.SPECS)), ids=[f"{kind}{J}_V{V}_{dt}" for kind, J, V, dt in rc.SPECS])
def test_skins_and_entries_equal_the_oracle_bit_for_bit(k, keep):
    """rows of 2 to 210 joints: 1 to 4 chunks of 64 columns in rig_entries_kernel, 1 to 257 vertices at 4 per workgroup"""
    rc.check_rig(batch(keep)[0][k], rc.cases()[k], keep)


# ------------------------------------------------------------------------------------------------------------------- ragged block
@pytest.mark.parametrize("keep", [False, True], ids=["final", "dup"])
def test_the_block_is_zero_past_each_mesh_and_the_order_does_not_matter(keep):
    cs = rc.cases()
    per, block = batch(keep)
    rc.check_block(block, cs, per)
    back, block_back = rc.run_batch(cs[::-1], DEV, keep)
    rc.check_block(block_back, cs[::-1], back)
    for c, a, b in zip(cs, back[::-1], per):
        rc.check_bits(a["skins"], b["skins"], f"{c['name']}: the other order")
        assert all(rc.same_bits(x, y) for x, y in zip(a["entries"], b["entries"])), c["name"]


def test_each_mesh_alone_and_a_second_run_give_the_batch_bits():
    cs = rc.cases()
    per, _ = batch(False)
    again, _ = rc.run_batch(cs, DEV, False)
    for c, a, b in zip(cs, again, per):
        rc.check_bits(a["skins"], b["skins"], f"{c['name']}: second run")
        assert all(rc.same_bits(x, y) for x, y in zip(a["entries"], b["entries"])), c["name"]
    for k, c in enumerate(cs):
        (alone,), _ = rc.run_batch([c], DEV, False)
        rc.check_bits(alone["skins"], per[k]["skins"], f"{c['name']}: alone")
        assert all(rc.same_bits(x, y) for x, y in zip(alone["entries"], per[k]["entries"])), c["name"]


# ----------------------------------------------------------------------------------------------------------------- tables (ops layer)
@pytest.mark.parametrize("raw", [False, True], ids=["threshold", "raw"])
def test_hand_made_tables_equal_the_emulation(raw):
    """a joint without segments, segments without bones, 1 / 2 / 7 bones with the last above / at / below 1e-5; MORIG_RIG_RAW with
    NaN, -0.0 and 1e-7 as the last bone (NaNs as NaNs, the sign of zero kept); without RAW the NaN is skipped"""
    c = rc.table_case()
    want = rc.run_tables(rigging_emulate.RigOps(), c["W"], c["tables"], c["ld_out"], raw, "cpu")
    rc.check_bits(want, rc.walk_tables(c["W"], c["tables"], c["ld_out"], raw), "the emulation against the header's rule")
    got = rc.run_tables(get_ops(), c["W"], c["tables"], c["ld_out"], raw, DEV)
    print(got[:4])
    rc.check_bits(got, want, f"hand-made tables (raw={raw})")
    wider = rc.run_tables(get_ops(), c["W"], c["tables"], c["ld_out"] + 3, raw, DEV)                # ld_out past every mesh's joints
    rc.check_bits(wider[:, :c["ld_out"]], want, "a wider block")
    assert not wider[:, c["ld_out"]:].any()


def test_clamped_tables_are_skipped_as_the_header_says():
    """Only tables the kernel bounds before any access they guide (csrc/rig_assemble.hip, rig_assemble_kernel): a row no mesh names is
    tested against vtx_ptr before anything else is read; `j0 >= 0 && j1 <= n_joints && j < j1 - j0` precedes every seg_ptr read; s0 / s1
    are clamped to [0, n_segs] and b0 / b1 to [0, n_bones] before their loops; `c < 0 || c >= n_cols` precedes the read of W."""
    c = rc.table_case()
    clean = rc.run_tables(get_ops(), c["W"], c["tables"], c["ld_out"], False, DEV)
    rc.check_bits(clean, rc.walk_tables(c["W"], c["tables"], c["ld_out"], False), "clean tables")
    for name, t, same_rows in rc.clamped_variants():
        got = rc.run_tables(get_ops(), c["W"], t, c["ld_out"], False, DEV)
        rc.check_bits(got, rc.walk_tables(c["W"], t, c["ld_out"], False), name)
        rc.check_bits(got[same_rows], clean[same_rows], f"{name}: the rows of the other meshes")


# ----------------------------------------------------------------------------------------------------------------------- strided W
def test_strided_weights_are_read_in_place_and_give_the_same_bits():
    cs = rc.cases()
    wide = max(c["n_bones"] for c in cs) + 5
    block = torch.full((sum(c["V"] for c in cs), wide), 0.5, dtype=torch.float64, device=DEV)
    views, r = [], 0
    for c in cs:
        block[r:r + c["V"], :c["n_bones"]] = torch.from_numpy(c["weights"]).to(DEV)
        views.append(block[r:r + c["V"], :c["n_bones"]])
        r += c["V"]
    taken = rigging._weight_block(views, torch.device(DEV))
    assert taken.data_ptr() == block.data_ptr() and taken.stride(0) == wide                        # the in-place path: no copy
    separate = [torch.from_numpy(c["weights"]).to(DEV) for c in cs]
    assert rigging._weight_block(separate, torch.device(DEV)).data_ptr() not in {w.data_ptr() for w in separate}
    per, _ = rc.run_batch(cs, DEV, False, weights=views)
    for c, got, b in zip(cs, per, batch(False)[0]):
        rc.check_rig(got, c, False)
        rc.check_bits(got["skins"], b["skins"], c["name"])
