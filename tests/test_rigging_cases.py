"""CPU: the generated cases of tests/rigging_cases.py, judged from the oracle alone (tests/rigging_oracle.py) before the device sees them
(tests/test_rigging_differential.py): every case reaches the branch it is named for, the fixture condition on the nearest new bone
holds, and the packing the device file uses gives the oracle's results when sent through morig_amd/rigging.py on the emulated
operators (tests/rigging_emulate.py). The hand-made tables are walked by a restatement of the header's rule and by the emulation. Last,
the shared compare functions are shown to reject planted errors: one entry moved one slot, one weight replaced by the previous bone's."""
import numpy as np
import pytest
import torch

import rigging_cases as rc
import rigging_emulate
import rigging_oracle as ro
from morig_amd import rigging, runtime

DEV = "cpu"


@pytest.fixture()
def ops(monkeypatch):
    o = rigging_emulate.RigOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


def test_the_cases_are_the_listed_ones_and_reach_their_chunks():
    cs = rc.cases()
    assert [(c["kind"], c["J"]) for c in cs] == [("chain", j) for j in (2, 63, 64, 65, 128, 129)] + [("tree", j) for j in (40, 70, 130)]
    assert {c["V"] for c in cs} == {1, 3, 4, 5, 257} and {c["dtype"] for c in cs} == {"float32", "float64"}
    for c in cs:
        w = c["want"]
        assert rc.nearest_bone_condition(c), c["name"]
        assert str(w["final"][2].dtype) == str(w["dup"][2].dtype) == c["dtype"] and len(w["final"][0]) == c["J"]
        if c["kind"] == "chain":
            assert w["dup"][0] == w["final"][0] == c["names"]                                    # exact control of J, no duplicate
        else:
            assert len(w["dup"][0]) > 1.4 * c["J"] and any("_dup" in n for n in w["dup"][0])
        for keep in (False, True):
            skins = rc.wanted(c, keep)[3]
            j = skins.shape[1]
            for col in (64, 128, 192):
                if j > col:
                    assert (skins[:, col:col + rc.CHUNK] != 0).any(), (c["name"], keep, col)     # every later chunk holds an entry
            if not keep:                                                                         # (a joint that only carries duplicates is an empty column)
                assert (skins[:, j - 1] != 0).any(), c["name"]                                   # the last column of the last chunk
                assert all((skins[:, col] != 0).any() for col in (64, 128) if j > col), c["name"]   # the first column of a later chunk
            if c["V"] >= 3:
                assert not skins[-1].any() and (skins[0] != 0).sum() >= 0.6 * min(j, c["n_bones"])
    dup130 = len(cs[8]["want"]["dup"][0])
    assert dup130 > 3 * rc.CHUNK and len(cs[7]["want"]["dup"][0]) > rc.CHUNK                      # four chunks, and two
    flat = np.concatenate([c["weights"].reshape(-1) for c in cs])
    for special in rc.SPECIAL:
        assert ((flat == special) & (np.signbit(flat) == np.signbit(special))).any(), special
    assert 0.3 < (flat == 0).mean() < 0.7


def test_the_threshold_is_strict_in_the_oracle():
    """1e-5 itself and the float64 below it are dropped, the one above is kept: the values the weights carry"""
    out = ro.assemble(np.array([[rc.MIN_W, rc.BELOW, rc.ABOVE, -0.0, 3e-6]]), [0, 1, 2, 3, 4], 5)
    assert out.tolist() == [[0.0, 0.0, rc.ABOVE, 0.0, 0.0]]
    cs = [c for c in rc.cases() if c["V"] == 257]                                                # where the specials surely sit below ordinary rows
    for c in cs:
        w = c["weights"]
        assert (w[1:-1] == rc.MIN_W).any() and (w[1:-1] == rc.ABOVE).any()
        wrong = ro.assemble(np.where(w == rc.MIN_W, rc.ABOVE, w), c["want"]["new_of_bone"], len(c["want"]["dup"][0]))   # `>=` for `>`
        assert not rc.same_bits(wrong, c["want"]["dup_skins"]), c["name"]


@pytest.mark.parametrize("keep", [False, True])
def test_the_batch_through_the_emulated_ops(ops, keep):
    cs = rc.cases()
    per, block = rc.run_batch(cs, DEV, keep)
    for c, got in zip(cs, per):
        rc.check_rig(got, c, keep)
    rc.check_block(block, cs, per)
    back, block_back = rc.run_batch(cs[::-1], DEV, keep)                                          # the other order
    rc.check_block(block_back, cs[::-1], back)
    for a, b in zip(back[::-1], per):
        rc.check_bits(a["skins"], b["skins"], "the other order")
    (alone,), _ = rc.run_batch(cs[3:4], DEV, keep)
    rc.check_bits(alone["skins"], per[3]["skins"], "alone")


def test_hand_made_tables(ops):
    c = rc.table_case()
    t, W = c["tables"], c["W"]
    assert np.diff(t["seg_ptr"])[:8].tolist() == [0, 1, 2, 1, 1, 1, 3, 1] and 0 in np.diff(t["bone_ptr"]) and {1, 2, 7} <= set(np.diff(t["bone_ptr"]))
    for raw in (False, True):
        walked = rc.walk_tables(W, t, c["ld_out"], raw)
        rc.check_bits(rc.run_tables(ops, W, t, c["ld_out"], raw, DEV), walked, f"the emulation against the header's rule (raw={raw})")
    plain, raw = rc.walk_tables(W, t, 8, False), rc.walk_tables(W, t, 8, True)
    assert not plain[:4, :2].any() and plain[0, 2] == W[0, 0]                                      # no segment, no bones, an empty first segment
    assert plain[:3, 3].tolist() == [rc.ABOVE, 0.0, 0.0]                                          # 1 bone: above / at / below
    assert plain[:3, 4].tolist() == [rc.ABOVE, W[1, 2], W[2, 2]]                                  # 2 bones: the last, else the one before
    assert plain[:3, 5].tolist() == [rc.ABOVE, W[1, 9], W[2, 9]]                                  # 7 bones
    assert plain[:3, 7].tolist() == [rc.ABOVE, 0.0, 0.0]                                          # without RAW the NaN is skipped
    assert np.isnan(raw[0, 7]) and raw[1, 7] == 0.0 and np.signbit(raw[1, 7]) and raw[2, 7] == 1e-7
    assert np.isnan(raw[0, 6]) and raw[3, 6] == (W[3, 0] + 0.0) + W[3, 11]


def test_clamped_tables_on_the_header_rule():
    c = rc.table_case()
    clean = rc.walk_tables(c["W"], c["tables"], c["ld_out"], False)
    names = []
    for name, t, same_rows in rc.clamped_variants():
        got = rc.walk_tables(c["W"], t, c["ld_out"], False)
        rc.check_bits(got[same_rows], clean[same_rows], name)
        names.append(name)
        if name in ("bone_minus_one", "bone_at_n_cols"):
            assert not rc.same_bits(got[4:], clean[4:]), name                                      # the skipped bone was one that counted
        if name == "joint_ptr_past":
            assert not got[4:].any() and clean[4:].any()
        if name == "rows_unnamed":
            assert not got[[0, 6]].any() and clean[0].any() and clean[6].any()
    assert names == ["bone_minus_one", "bone_at_n_cols", "seg_ptr_end_past", "bone_ptr_end_past", "joint_ptr_past", "rows_unnamed"]


def test_strided_weights_are_read_in_place(ops):
    cs = rc.cases()
    wide = max(c["n_bones"] for c in cs) + 5
    block = torch.full((sum(c["V"] for c in cs), wide), 0.5, dtype=torch.float64)
    views, r = [], 0
    for c in cs:
        block[r:r + c["V"], :c["n_bones"]] = torch.from_numpy(c["weights"])
        views.append(block[r:r + c["V"], :c["n_bones"]])
        r += c["V"]
    taken = rigging._weight_block(views, torch.device(DEV))
    assert taken.data_ptr() == block.data_ptr() and taken.stride(0) == wide
    per, _ = rc.run_batch(cs, DEV, False, weights=views)
    assert ops.last_W.data_ptr() == block.data_ptr()
    for c, got in zip(cs, per):
        rc.check_rig(got, c, False)


def test_planted_errors_are_rejected():
    c = rc.cases()[7]
    skins = c["want"]["skins"]
    good = ro.entries(skins)
    good = (good[0], good[1], good[2], good[3])
    rc.check_entries(good, skins, "self")
    ej = good[2].copy()
    k = int(np.flatnonzero(np.diff(ej) > 1)[0])
    ej[k] += 1                                                                                     # one entry moved one slot
    with pytest.raises(AssertionError, match="another slot"):
        rc.check_entries((good[0], good[1], ej, good[3]), skins, "planted")
    vptr = good[0].copy()
    vptr[1] += 1
    with pytest.raises(AssertionError, match="entry offsets"):
        rc.check_entries((vptr,) + good[1:], skins, "planted")
    w = c["weights"].copy()
    v, b = [(v, b) for v in range(1, 6) for b in range(1, c["n_bones"]) if w[v, b] > 1e-3 and w[v, b - 1] > 1e-3 and w[v, b] != w[v, b - 1]][0]
    w[v, b] = w[v, b - 1]                                                                          # one weight replaced by the previous bone's
    wrong = ro.assemble_rig(c["rig"], w)["skins"]
    with pytest.raises(AssertionError, match="not bit-equal"):
        rc.check_bits(wrong, skins, "planted")
    assert (wrong != skins).sum() == 1
    with pytest.raises(AssertionError, match="not bit-equal"):
        rc.check_bits(np.array([-0.0]), np.array([0.0]), "signed zero")
    with pytest.raises(AssertionError, match="not bit-equal"):
        rc.check_bits(np.array([np.nan, 1.0]), np.array([0.0, 1.0]), "a NaN for a number")
