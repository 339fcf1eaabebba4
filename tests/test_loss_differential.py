"""GPU: csrc/losses.hip and csrc/losses_skin.hip through the public functions of morig_amd.losses, forward and backward, against the
float64 oracles (tests/loss_oracle.py, tests/skin_loss_oracle.py) on the generated cases of tests/loss_cases.py: the sizes the kernels
branch on -- key counts and row counts around the 32-key tile and the 128-row workgroup of infoNCE, 64-row apply tiles and the 256-column
loop of the multi-positive backward, up to 64 positives / 256 negatives / width 128, all four joint slots and several LDS fills of the
chamfer backward, one and two rounds of the folded pair order of the log-ratio forward, K = 1 .. 8 and K = 1 .. 128 of the two
cross-entropies -- ragged batches with non-zero offsets, strided views read in place, and an upstream gradient other than 1 on about
half of the cases. tests/test_loss_cases.py proves the case conditions and this file's comparison code without a device.

Bounds: FACTOR times the family maximum of the float32 oracle's deviation from the float64 oracle, floored at one float32 ulp; computed
at test time, printed next to every device figure before the assert (run with -s). Where the project claims bits -- rows without
gradient, vert_mask, a second run, a mesh's share of a power-of-two batch -- bits are asserted."""
import pytest
import torch

import loss_cases as lc
import loss_oracle as lo
from morig_amd import losses, native

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _grad_on():
    """conftest.py runs every test under torch.no_grad(); these need the graph"""
    with torch.enable_grad():
        yield
    losses.check_inputs()                                  # no launch of the test found its inputs wrong


@pytest.mark.parametrize("family,name", lc.ALL)
def test_against_the_float64_oracle(family, name):
    lc.check(family, name, DEV)


def test_bounds_in_use():
    print("\n" + lc.table())


def test_multipos_without_a_negative():
    """n_neg = 0: log(exp(p)) - p, loss and gradient exactly 0 in the kernel's arithmetic -- but an empty neg_ids tensor has no storage, and
    the library refuses the null pointer by name before any launch"""
    c = lc.mp_no_negative_case()
    with pytest.raises(native.MorigNativeError, match="morig_multipos_forward"):
        lc.mp_run(c, DEV)
    losses.check_inputs()


def test_chamfer_swap_through_the_reference_signature():
    """chamfer_distance_with_average(1023 points, 1025 points): the second set is over the LDS limit and the first is not"""
    c = lc.case("chamfer", "ragged_b")
    got = lc.ch_swapped_run(c, DEV)
    s, sq = c["batch"] == 2, c["q_batch"] == 2
    z = lambda n: torch.zeros(n, dtype=torch.long)
    want = [t.numpy() for t in lo.chamfer(c["p"][s].double(), z(int(s.sum())), c["q"][sq].double(), z(int(sq.sum())), 1)]
    lc.ch_compare("swapped (1023 | 1025)", c, got, lc.bounds("chamfer"), want=want)
    assert lc.same_bits(got, lc.ch_swapped_run(c, DEV))


def test_skin_ce_all_masked_is_nan():
    c = lc.case("skin_ce", "k8_n513")
    x = c["x"].to(DEV).requires_grad_(True)
    loss = losses.skin_ce_loss(x, c["label"].to(DEV), torch.zeros_like(c["mask"]).to(DEV), nearest_bone=c["K"])
    assert torch.isnan(loss)


# ------------------------------------------------------------------------------------------------------------------- one above each limit
def _refused(match, call):
    with pytest.raises((losses.LossInputError, native.MorigNativeError), match=match):
        call()
    losses.check_inputs()                                  # the refusal left nothing behind


def test_one_above_each_limit_is_refused():
    z = lambda n: torch.zeros(n, dtype=torch.long, device=DEV)
    rnd = lambda *shape: torch.rand(*shape, device=DEV)
    ids = lambda *shape: torch.zeros(*shape, dtype=torch.long, device=DEV)
    sid = torch.arange(4, device=DEV)[None]
    mp = lambda D, P, N: losses.multi_pos_infoNCE(rnd(6, D), None, z(6), samples=(sid, ids(1, 4, P), ids(1, 4, N)), num_graphs=1)
    _refused("65 positives.*at most 64 / 256", lambda: mp(8, 65, 4))
    _refused("257 negatives.*at most 64 / 256", lambda: mp(8, 4, 257))
    _refused("multiple of 4 up to 128, got 132", lambda: mp(132, 4, 4))
    assert torch.isfinite(mp(128, 64, 256))                                                 # the limits themselves run
    lr = lambda S, D, W: losses.log_ratio_loss(rnd(70, D), rnd(70, W), z(70), samples=torch.arange(S, device=DEV)[None], num_graphs=1)
    _refused("n_sample from 3 to 64, got 65", lambda: lr(65, 8, 8))
    _refused("from 4 to 128, got 132", lambda: lr(8, 132, 8))
    _refused("up to 128, got 132", lambda: lr(8, 8, 132))
    assert torch.isfinite(lr(64, 128, 128))
    _refused("nearest_bone from 1 to 8, got 9", lambda: losses.skin_ce_loss(rnd(5, 9), rnd(5, 9), torch.ones(5, 9, device=DEV)))
    _refused("at most 128 classes, got 129", lambda: losses.cross_entropy_with_probs(rnd(5, 129), rnd(5, 129)))


def test_one_joint_above_the_limit_in_a_batch_is_reported():
    """mesh 1 of a batch of three has 1025 joints: found on the device, the loss is NaN, the next look at the status word raises"""
    counts = (3, 1025, 2)
    q = torch.rand(sum(counts), 3, device=DEV).requires_grad_(True)
    p = torch.rand(30, 3, device=DEV).requires_grad_(True)
    loss = losses.chamfer_batched(p, lc.batch_vector((10, 10, 10)).to(DEV), q, lc.batch_vector(counts).to(DEV), num_graphs=3)
    assert torch.isnan(loss)
    with pytest.raises(losses.LossInputError, match="more than 1024 joints"):
        losses.check_inputs()
    losses.check_inputs()
