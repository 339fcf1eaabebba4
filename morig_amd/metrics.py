"""Rig evaluation metrics on the device (csrc/metrics.hip): the numbers evaluate/eval_rigging.py:107-131 and utils/eval_utils.py:72-119
report for predicted joints and rigs -- CD-J2J, joint IoU / precision / recall from an optimal one-to-one matching judged against per-joint
feature sizes, CD-J2B and CD-B2B -- for all meshes of a batch at once.

Everything is float64 (the reference computes these in numpy float64) and ragged: point sets of all meshes are concatenated and described
by ``ptr`` arrays [B + 1], as in joints.py and skeleton.py. A ptr is HOST metadata (a list, a numpy array or a CPU tensor: the sizes of a
batch are known where the batch was made) and is checked on the host; the ptr ``sample_skel`` returns lives on the device, and the
functions that only forward a ptr to a kernel (``nearest_distance``, the chamfers) take such a device tensor too. There is no CPU path
and no floating-point atomic: two runs give the same bits, and a mesh scores the same alone as inside a batch.

HOST READS. ``sample_skel`` reads ONE small vector back, the total of the bone samples (the size of its output depends on the bone
lengths) together with the number of bones the kernel refused (a NaN joint, more than 2^24 samples: ValueError, never a skeleton
sampled without that bone); ``chamfer_j2b``, ``chamfer_b2b`` and ``evaluate_rigs(pred_rigs=...)`` sample both rig lists in one call and so read once as
well. Nothing else reads the device: ``match_joints`` sizes its workspace and finds the meshes it must refuse from the host ptrs.
``format_report`` is where results come to the host, as text. Walking the hierarchy of every ``formats.Rig`` to list its bones is host
work on host objects; everything computed from coordinates runs in kernels.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .ragged import check_ptr, device_of, ptr_of
from .runtime import get_ops

MAX_SMALL, MAX_LARGE = 128, 256           # what one mesh of match_joints may have on its smaller / larger side (MORIG_ASSIGN_MAX_*)


class AssignmentSizeError(ValueError):
    """match_joints was given meshes beyond the size the kernel supports. ``meshes``: their indices in the batch; ``sizes``: their
    (n_gt, n_pred); ``result``: what match_joints returns otherwise -- the other meshes are solved, the refused ones hold -1 / NaN pairs
    and MORIG_ASSIGN_ST_SIZE in ``result["status"]``. There is no slow path."""

    def __init__(self, meshes, sizes, result):
        self.meshes, self.sizes, self.result = list(meshes), list(sizes), result
        super().__init__(f"match_joints: meshes {self.meshes} with (n_gt, n_pred) = {self.sizes} exceed the supported {MAX_SMALL} x {MAX_LARGE} "
                         f"(smaller side x larger side)")


def _pts(x, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float64).reshape(-1, 3))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("metrics: point sets are [n, 3]")
    return t.to(device=device, dtype=torch.float64).contiguous()


def _host_ptr(ptr, n: int, what: str) -> np.ndarray:
    if isinstance(ptr, torch.Tensor):
        if ptr.is_cuda:
            raise TypeError(f"metrics: {what} is host metadata (a list, a numpy array or a CPU tensor); reading it back from the device is "
                            f"what this module avoids")
        ptr = ptr.numpy()
    p = check_ptr(ptr, n, f"metrics: {what}")
    if n >= 2 ** 31:
        raise ValueError(f"metrics: {what}: more than 2^31 rows")
    return p


def _dev_ptr(ptr, n: int, what: str, device) -> torch.Tensor:
    """a ptr for a kernel: host ptrs are checked and uploaded, a device int32 tensor is forwarded (the kernels skip what a bad one names)"""
    if isinstance(ptr, torch.Tensor) and ptr.is_cuda:
        if ptr.dtype != torch.int32 or ptr.dim() != 1 or ptr.numel() < 2:
            raise ValueError(f"metrics: a device {what} is int32 [B + 1]")
        return ptr.contiguous()
    return torch.from_numpy(_host_ptr(ptr, n, what).astype(np.int32)).to(device)


# ---- bone samples ----------------------------------------------------------------------------------------------------------------
def rig_bones(rig) -> np.ndarray:
    """int64 [n, 2] (parent, child), breadth first from the root, children in ascending joint index: the order Rig.save writes hier lines
    in, so a file round trip through the reference's rig_parser.Info visits the same bones in the same order"""
    hier = np.asarray(rig.hierarchy).reshape(-1)
    kids = [[] for _ in range(len(hier))]
    for c, p in enumerate(hier):
        if c != rig.root_id and 0 <= p < len(hier):
            kids[p].append(c)
    out, level = [], [int(rig.root_id)]
    while level:
        nxt = []
        for p in level:
            out += [(p, c) for c in kids[p]]
            nxt += kids[p]
        level = nxt
        if len(out) > len(hier):
            raise ValueError("metrics: the hierarchy is not a tree")
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def _pack_rigs(rigs: Sequence, device):
    """-> (joints float64 [J, 3] on the device, joint ptr (host), bones int32 [n, 2] global joint rows on the device, bone ptr (host))"""
    if len(rigs) == 0:
        raise ValueError("metrics: at least one rig")
    pos = [np.asarray(r.pos, dtype=np.float64).reshape(-1, 3) for r in rigs]
    jptr = ptr_of([len(p) for p in pos])
    bones = [rig_bones(r) for r in rigs]
    for b, bl in enumerate(bones):
        if len(bl) == 0:
            raise ValueError(f"sample_skel: rig {b} has no bones (a single joint): there is nothing to sample")
    bptr = ptr_of([len(bl) for bl in bones])
    flat = np.concatenate([bl + jptr[b] for b, bl in enumerate(bones)], axis=0).astype(np.int32)
    return (torch.from_numpy(np.concatenate(pos, axis=0)).to(device), jptr, torch.from_numpy(flat).to(device).contiguous(), bptr)


def _sample(joints: torch.Tensor, bones: torch.Tensor, bptr: np.ndarray):
    ops = get_ops()
    counts = ops.bone_sample_counts(joints, bones)
    off = torch.zeros(bones.shape[0] + 1, dtype=torch.int64, device=joints.device)
    off[1:] = torch.cumsum(counts, 0)
    # THE host read of this module: the output's size depends on the bone lengths. The refused bones (count 0: a NaN joint, or more than
    # MORIG_BONE_MAX_SAMPLES samples -- a zero-length bone counts 1) come with it: how many, and the first one
    refused = counts == 0
    where = torch.where(refused, torch.arange(counts.numel(), device=counts.device), counts.numel())
    total, n_refused, first = torch.stack([off[-1], refused.sum(), where.min() if counts.numel() else off[-1]]).tolist()
    if n_refused:
        rig = int(np.searchsorted(bptr, first, side="right")) - 1
        raise ValueError(f"sample_skel: bone {first - int(bptr[rig])} of rig {rig} cannot be sampled (a NaN joint, or more than 2^24 samples); "
                         f"{n_refused} such bone(s) in this call. The reference never drops a bone: nothing is sampled without it")
    if total >= 2 ** 31:
        raise ValueError("sample_skel: more than 2^31 bone samples in one call")
    samples = ops.bone_samples(joints, bones, off, total)
    ptr = off[torch.from_numpy(bptr).to(joints.device)].to(torch.int32)
    return samples, ptr


def sample_skel(rigs: Sequence, device=None):
    """eval_utils.sample_skel / sample_bone (utils/eval_utils.py:72-97) for a list of ``formats.Rig`` -> (samples float64 [N, 3], ptr int32
    [B + 1], both on the device). Every (parent, child) pair gives round(len / 0.005) + 1 points p + (ray / (n + 1e-30)) * k, bones in
    ``rig_bones`` order. Reproduced to the bit: np.round's half-to-even, len = sqrt((dx^2 + dy^2) + dz^2), a multiply then an add (no
    FMA). A rig without bones raises ValueError (the reference's np.concatenate of an empty list raises there too), and so does a bone
    the kernel refuses (count 0: a NaN joint, or more than 2^24 samples), named by rig and bone. One host read."""
    device = device_of(device=device)
    joints, _, bones, bptr = _pack_rigs(rigs, device)
    return _sample(joints, bones, bptr)


# ---- nearest distance, chamfers ------------------------------------------------------------------------------------------------------
def nearest_distance(a, a_ptr, b, b_ptr, squared: bool = False, return_flags: bool = False, device=None):
    """For every point of ``a`` the distance to the nearest point of ``b`` in the same mesh -> float64 [len(a)] on the device; squared
    distances are (dx^2 + dy^2) + dz^2. A mesh with points in ``a`` and none in ``b`` gets NaN there and 1 in the per-mesh flags
    (``return_flags=True`` -> (distances, int32 [B]))."""
    device = device_of(a, b, device=device)
    a, b = _pts(a, device), _pts(b, device)
    pa, pb = _dev_ptr(a_ptr, a.shape[0], "a_ptr", device), _dev_ptr(b_ptr, b.shape[0], "b_ptr", device)
    if pa.numel() != pb.numel():
        raise ValueError("nearest_distance: a_ptr and b_ptr describe the same meshes")
    d, flags = get_ops().nearest_distance(a, pa, b, pb, bool(squared))
    return (d, flags) if return_flags else d


def _oneway(a, pa, b, pb):
    ops = get_ops()
    d, _ = ops.nearest_distance(a, pa, b, pb, False)
    return ops.segment_mean(d, pa)


def _chamfer(a, pa, b, pb):
    return (_oneway(a, pa, b, pb) + _oneway(b, pb, a, pa)) / 2


def chamfer_j2j(pred, pred_ptr, gt, gt_ptr, device=None):
    """eval_utils.chamfer_dist per mesh -> float64 [B]: the half-sum of the two one-way means of nearest distances. A mesh with an empty
    side gives NaN."""
    device = device_of(pred, gt, device=device)
    pred, gt = _pts(pred, device), _pts(gt, device)
    pp, pg = _dev_ptr(pred_ptr, pred.shape[0], "pred_ptr", device), _dev_ptr(gt_ptr, gt.shape[0], "gt_ptr", device)
    if pp.numel() != pg.numel():
        raise ValueError("chamfer_j2j: pred_ptr and gt_ptr describe the same meshes")
    return _chamfer(pred, pp, gt, pg)


def _bone_sets(rigs_a, rigs_b, device):
    """Joints and bone samples of two rig lists -> (joints, ja, jb, samples, sa, sb). Both lists are sampled in ONE call (one host read);
    list b's joints and samples are addressed inside the common arrays by ptrs (jb, sb) that start where list a's end -- nothing is sliced
    at a position only the device knows."""
    if len(rigs_a) != len(rigs_b):
        raise ValueError("metrics: one rig of each list per mesh")
    B = len(rigs_a)
    joints, jptr, bones, bptr = _pack_rigs(list(rigs_a) + list(rigs_b), device)
    samples, sptr = _sample(joints, bones, bptr)
    jp = torch.from_numpy(jptr.astype(np.int32)).to(device)
    return joints, jp[:B + 1].contiguous(), jp[B:].contiguous(), samples, sptr[:B + 1].contiguous(), sptr[B:].contiguous()


def _j2b(joints, ja, jb, samples, sa, sb):
    return (_oneway(joints, ja, samples, sb) + _oneway(joints, jb, samples, sa)) / 2


def chamfer_j2b(rigs_a: Sequence, rigs_b: Sequence, device=None):
    """eval_utils.joint2bone_chamfer_dist per mesh -> float64 [B]: the joints of each rig against the bone samples of the other, both
    ways, halved. One host read (the sample total of both lists)."""
    return _j2b(*_bone_sets(rigs_a, rigs_b, device_of(device=device)))


def chamfer_b2b(rigs_a: Sequence, rigs_b: Sequence, device=None):
    """eval_utils.bone2bone_chamfer_dist per mesh -> float64 [B]: chamfer_dist of the two bone-sample sets. One host read."""
    _, _, _, samples, sa, sb = _bone_sets(rigs_a, rigs_b, device_of(device=device))
    return _chamfer(samples, sa, samples, sb)


# ---- matching and scores -------------------------------------------------------------------------------------------------------------
def match_joints(pred, pred_ptr, gt, gt_ptr, device=None) -> dict:
    """The optimal assignment on dist[g, p] = |pred_p - gt_g| per mesh (rows = ground truth, columns = predictions, as
    eval_rigging.py:113-114 has it): shortest augmenting paths with dual potentials, the algorithm behind scipy's
    linear_sum_assignment, one wave per mesh. -> dict(row_ind, col_ind int32 [M] local to the mesh, row_ind ascending inside a mesh;
    dist float64 [M]; match_ptr int32 [B + 1]; status int32 [B]; all on the device) plus ``match_ptr_host``, ``n_pred``, ``n_gt`` (numpy).
    Mesh b holds min(n_gt, n_pred) pairs. Where the optimum is not unique the matching may differ from scipy's by an equally optimal one.

    A mesh whose smaller side exceeds 128 or whose larger side exceeds 256 is refused by the kernel through ``status``; this raises
    AssignmentSizeError, which names the meshes and carries the result of the others. No host read: the ptrs are host metadata."""
    device = device_of(pred, gt, device=device)
    pred, gt = _pts(pred, device), _pts(gt, device)
    pp, pg = _host_ptr(pred_ptr, pred.shape[0], "pred_ptr"), _host_ptr(gt_ptr, gt.shape[0], "gt_ptr")
    if len(pp) != len(pg):
        raise ValueError("match_joints: pred_ptr and gt_ptr describe the same meshes")
    n_pred, n_gt = np.diff(pp), np.diff(pg)
    small, large = np.minimum(n_pred, n_gt), np.maximum(n_pred, n_gt)
    refused = (small > MAX_SMALL) | (large > MAX_LARGE)
    mptr = ptr_of(small)
    cptr = ptr_of(np.where(refused, 0, n_pred * n_gt))
    up = lambda a, dt: torch.from_numpy(a.astype(dt)).to(device)
    ops = get_ops()
    assert (ops.ASSIGN_MAX_SMALL, ops.ASSIGN_MAX_LARGE) == (MAX_SMALL, MAX_LARGE)
    match_ptr = up(mptr, np.int32)
    row, col, dist, status = ops.assign_joints(pred, up(pp, np.int32), gt, up(pg, np.int32), match_ptr, int(mptr[-1]), up(cptr, np.int64),
                                               int(cptr[-1]))
    result = dict(row_ind=row, col_ind=col, dist=dist, match_ptr=match_ptr, status=status, match_ptr_host=mptr, n_pred=n_pred, n_gt=n_gt)
    if refused.any():
        which = np.nonzero(refused)[0]
        raise AssignmentSizeError(which.tolist(), [(int(n_gt[b]), int(n_pred[b])) for b in which], result)
    return result


def joint_scores(match: dict, n_pred, n_gt, featuresize, fs_ptr, device=None) -> dict:
    """eval_rigging.py:115-120 per mesh: hits = sum(d < fs[row]) over the matched pairs (strict), IoU = 2 hits / (n_pred + n_gt),
    precision = hits / n_pred, recall = hits / n_gt -> dict(hits int32 [B], iou, precision, recall float64 [B]) on the device.
    ``featuresize`` holds one value per ground-truth joint in the ground-truth joint order, meshes concatenated (``fs_ptr`` [B + 1])."""
    device = device_of(match["dist"], device=device)
    fs = featuresize if isinstance(featuresize, torch.Tensor) else torch.from_numpy(np.asarray(featuresize, dtype=np.float64))
    fs = fs.to(device=device, dtype=torch.float64).reshape(-1).contiguous()
    n_pred, n_gt = np.asarray(n_pred, dtype=np.int64).reshape(-1), np.asarray(n_gt, dtype=np.int64).reshape(-1)
    fp = _host_ptr(fs_ptr, fs.numel(), "fs_ptr")
    B = match["match_ptr"].numel() - 1
    if not (len(n_pred) == len(n_gt) == len(fp) - 1 == B):
        raise ValueError("joint_scores: one n_pred, n_gt and feature-size segment per mesh of the matching")
    if np.any(np.diff(fp) != n_gt):
        raise ValueError("joint_scores: one feature size per ground-truth joint")
    up = lambda a: torch.from_numpy(a.astype(np.int32)).to(device)
    hits, out = get_ops().joint_scores(match["row_ind"], match["dist"], match["match_ptr"], up(ptr_of(n_pred)), up(ptr_of(n_gt)), fs, up(fp))
    return dict(hits=hits, iou=out[0], precision=out[1], recall=out[2])


KEYS = ("chamfer_j2j", "iou", "precision", "recall")
BONE_KEYS = ("chamfer_j2b", "chamfer_b2b")


def evaluate_rigs(pred_joints, pred_ptr, gt_rigs: Sequence, featuresize, pred_rigs: Optional[Sequence] = None, device=None) -> dict:
    """The loop body of eval_rig (evaluate/eval_rigging.py:100-126) for a batch. ``pred_joints`` [N, 3] with ``pred_ptr`` [B + 1] (host);
    ``gt_rigs``: B ``formats.Rig`` (their ``pos`` are the ground-truth joints); ``featuresize``: one array (or tensor) per mesh, or all of them
    concatenated, one value per ground-truth joint in ``pos`` order; ``pred_rigs``: B rigs (entries of meshes without predicted joints
    are not looked at) to add CD-J2B and CD-B2B.

    -> dict: chamfer_j2j, iou, precision, recall [, chamfer_j2b, chamfer_b2b] float64 [B] and hits int32 [B] (NaN / 0 on the skipped
    meshes), valid bool [B], mean {key: float64 scalar}, all on the device; num_invalid (int), match (match_joints' result). A mesh with
    zero predicted joints is skipped and counted in num_invalid (:107-109); the means add the valid meshes in batch order and divide by
    B - num_invalid (:123-126). Host reads: none, or one with ``pred_rigs``.

    Non-finite joints (the reference crashes on them: scipy raises): a predicted joint with a NaN or infinite coordinate is never matched;
    when the finite ones suffice nothing else changes, otherwise ``result["match"]["status"]`` of that mesh is MORIG_ASSIGN_ST_INFEASIBLE
    (4), its pairs are -1 / NaN and its hits 0 (a NaN ground-truth joint always ends so). The status stays on the device: no host read
    is added for it. CD-J2J of such a mesh is NaN (np.min's rule)."""
    device = device_of(pred_joints, device=device)
    pred = _pts(pred_joints, device)
    B = len(gt_rigs)
    pp = _host_ptr(pred_ptr, pred.shape[0], "pred_ptr")
    if len(pp) != B + 1 or B == 0:
        raise ValueError("evaluate_rigs: one ground-truth rig per mesh of pred_ptr")
    gt_pos = [np.asarray(r.pos, dtype=np.float64).reshape(-1, 3) for r in gt_rigs]
    n_gt, n_pred = np.array([len(p) for p in gt_pos], dtype=np.int64), np.diff(pp)
    gp = ptr_of(n_gt)
    if isinstance(featuresize, (list, tuple)):
        if len(featuresize) != B or any(len(f) != n for f, n in zip(featuresize, n_gt)):
            raise ValueError("evaluate_rigs: one feature size per ground-truth joint")
        if all(isinstance(f, torch.Tensor) for f in featuresize):                        # labels.bone_ray_labels' results stay on their device
            featuresize = torch.cat([f.to(device=device, dtype=torch.float64).reshape(-1) for f in featuresize])
        else:
            featuresize = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1) for f in featuresize])
    gt = torch.from_numpy(np.concatenate(gt_pos, axis=0)).to(device)
    valid_host = n_pred > 0
    num_invalid = int((~valid_host).sum())
    ops = get_ops()
    match = match_joints(pred, pp, gt, gp, device)
    sc = joint_scores(match, n_pred, n_gt, featuresize, gp, device)
    valid = torch.from_numpy(valid_host).to(device)
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=device)
    per = dict(chamfer_j2j=chamfer_j2j(pred, pp, gt, gp, device), iou=sc["iou"], precision=sc["precision"], recall=sc["recall"])
    keys = KEYS
    if pred_rigs is not None:
        if len(pred_rigs) != B:
            raise ValueError("evaluate_rigs: one predicted rig per mesh")
        keys = KEYS + BONE_KEYS
        idx = np.nonzero(valid_host)[0]
        j2b, b2b = nan.clone(), nan.clone()
        if len(idx):
            sets = _bone_sets([pred_rigs[b] for b in idx], [gt_rigs[b] for b in idx], device)
            where = torch.from_numpy(idx).to(device)
            j2b[where], b2b[where] = _j2b(*sets), _chamfer(sets[3], sets[4], sets[3], sets[5])
        per.update(chamfer_j2b=j2b, chamfer_b2b=b2b)
    per = {k: torch.where(valid, per[k], nan) for k in keys}
    means = ops.valid_mean(torch.stack([per[k] for k in keys]).contiguous(), valid.to(torch.int32))
    out = dict(per)
    out.update(hits=torch.where(valid, sc["hits"], torch.zeros_like(sc["hits"])), valid=valid, num_invalid=num_invalid, match=match,
               mean={k: means[i] for i, k in enumerate(keys)})
    return out


def format_report(result: dict) -> str:
    """The four lines eval_rig prints (evaluate/eval_rigging.py:127-131): value * 100 to three decimals. This is where the means come to
    the host."""
    m = {k: float(result["mean"][k]) for k in KEYS}
    return "\n".join(["\tJ2J_chamfer_distance {:.03f}%".format(m["chamfer_j2j"] * 100), "\tjoint_IoU {:.03f}%".format(m["iou"] * 100),
                      "\tjoint_precision {:.03f}%".format(m["precision"] * 100), "\tjoint_recall {:.03f}%".format(m["recall"] * 100)])
