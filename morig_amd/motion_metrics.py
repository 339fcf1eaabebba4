"""Motion-stage evaluation on the device (csrc/motion_metrics.hip, csrc/curve_core.h): the numbers the reference's three motion scripts
report, for all pairs / meshes of a batch at once and without the ``.npy`` round trip of the training scripts' test loops --

    corr_accuracy          evaluate/eval_corr.py:6-24     correspondence accuracy (%) at ten tolerances
    pr_curve               evaluate/eval_attn.py:15-55    precision / recall of the attention prediction at ten thresholds
    keyframe_flow_errors   evaluate/eval_deform.py:6-20   mean vertex distance of the predicted key-frame flow
    nearest_points         training/train_corr_pose.py:117-118   the arg-max the test loop saves as ``_nnind.npy``

Batches are ragged in the ``losses`` convention: the rows of all pairs / meshes are concatenated, batch vectors are sorted, indices are
local to their pair exactly as ``losses.infoNCE`` takes ``corr_v2p`` (GraphData.__inc__ does not increment the correspondence keys, so
what ``test()`` holds plugs in unchanged), ``num_graphs`` is optional (``None`` costs one read of the last batch value). Segment offsets
come from ``morig_loss_segment_ptr``; an unsorted or out-of-range batch vector arrives through its status bits.

THE RULES that make the counts equal the reference's bit for bit (include/morig_hip.h): the correspondence distance
is float32 in numpy's order, ``(d0^2 + d1^2) + d2^2`` then the correctly rounded float32 root, a hit is ``dist < float32(tol)``; the
attention values are normalised per mesh in float32, ``(x - mn) / (mx - mn)`` with ``np.min``'s NaN rule, a predicted positive is
``x' > float32(t)``. Counts are integers: no floating-point atomic, two runs give the same bits, a pair alone the counts it gives in a
batch. Ratios and means are float64, taken here on the host from the integer tables after ONE read that fetches the tables and the
status word together; every function returns numpy arrays.

STATED DEVIATIONS from the reference:
  * thresholds and tolerances are rounded to float32 BEFORE the comparison. The reference pins numpy 1.21.5, where a Python float and an
    ``np.float64`` scalar from ``np.arange`` both compare with a float32 array in float32. numpy 2 compares the scalar in float64, which
    moves every vertex whose normalised value equals ``float32(t)`` (``np.float32(0.1) > np.float64(0.1)`` is True there). This module
    follows the reference's environment.
  * ``corr_accuracy``'s ``curve`` adds the pairs that have correspondences, in pair order, and divides by their number ``n_valid``; the
    reference divides by the number of files and would propagate the NaN of a pair without correspondences.
  * ``pr_curve``'s ``gp`` counts the non-zero labels; the reference sums the label values. Equal for the 0 / 1 files ``_attn.txt`` holds.
  * ``keyframe_flow_errors`` is float64 in a fixed order (``morig_pose_traj_errors``); the reference's is numpy float32 with pairwise means.
  * ``nearest_points`` is ``morig_cosine_nn``'s arg-max (split-fp16 products, fp32 sums): near-ties may resolve differently from a float32
    BLAS.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .abi import CONSTANTS as _K
from .ragged import as_tensor, device_of
from .runtime import get_ops

__all__ = ["TOLERANCES", "THRESHOLDS", "MotionMetricsInputError", "nearest_points", "corr_accuracy", "pr_curve", "keyframe_flow_errors",
           "evaluate_motion", "format_motion_report"]

TOLERANCES = (0.02, 0.04, 0.06, 0.08, 0.10, 0.12, 0.14, 0.16, 0.18, 0.20)        # eval_corr.py's ratio_list
THRESHOLDS = np.arange(0.0, 1.0, 0.1)                                          # eval_attn.py:31
MAX_BINS = _K["MORIG_CURVE_MAX_BINS"]
NN_WIDTH = 64                                                                  # morig_cosine_nn is built for this feature width
_BITS = (("MORIG_MOTION_ST_INDEX", _K["MORIG_MOTION_ST_INDEX"], "an index lies outside its pair"),
         ("MORIG_LOSS_ST_UNSORTED", _K["MORIG_LOSS_ST_UNSORTED"], "a batch vector is not sorted"),
         ("MORIG_LOSS_ST_SEGMENT", _K["MORIG_LOSS_ST_SEGMENT"], "a batch value lies outside [0, num_graphs)"))


class MotionMetricsInputError(ValueError):
    """The device found the DATA wrong: an index outside its pair, an unsorted or out-of-range batch vector. Raised after the one host
    read. ``bits``: the status word; ``result``: what the call returns otherwise -- a row with a bad index counts nothing and the other
    rows count as they would without it; with a bad batch vector every count is 0."""

    def __init__(self, what: str, bits: int, result=None):
        self.bits, self.result = int(bits), result
        found = [f"{name} ({text})" for name, bit, text in _BITS if bits & bit]
        super().__init__(f"{what}: {'; '.join(found) or 'status %d' % bits}")


# ------------------------------------------------------------------------------------------------------------------------- helpers
def _bins(values, what: str) -> np.ndarray:
    """Python floats / float64 -> float32, once: the comparison rule of the reference's numpy"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if not 1 <= v.size <= MAX_BINS:
        raise ValueError(f"{what}: between 1 and {MAX_BINS} values (MORIG_CURVE_MAX_BINS), got {v.size}")
    return v.astype(np.float32)


def _batch(b, n: int, name: str, device) -> torch.Tensor:
    b = as_tensor(b)
    if b.dim() != 1 or b.numel() != n:
        raise ValueError(f"{name}: expected a vector of {n} entries, got {tuple(b.shape)}")
    return b.to(device=device, dtype=torch.int64).contiguous()


def _num_graphs(batch: torch.Tensor, num_graphs: Optional[int]) -> int:
    if num_graphs is not None:
        if int(num_graphs) < 1:
            raise ValueError("num_graphs must be at least 1")
        return int(num_graphs)
    if batch.numel() == 0:
        raise ValueError("an empty batch vector needs num_graphs")
    return int(batch.max()) + 1


def _read(*tensors) -> list:
    """ONE host read: integer tensors concatenated on the device, split again here"""
    flat = torch.cat([t.reshape(-1).to(torch.int64) for t in tensors]).cpu().numpy()
    out, at = [], 0
    for t in tensors:
        out.append(flat[at:at + t.numel()].reshape(tuple(t.shape)))
        at += t.numel()
    return out


def _unit_rows(f, name: str, device) -> torch.Tensor:
    f = as_tensor(f)
    if f.dim() != 2 or f.dtype != torch.float32:
        raise ValueError(f"{name}: a float32 [rows, {NN_WIDTH}] matrix, got {f.dtype} {tuple(f.shape)}")
    if f.shape[1] != NN_WIDTH:
        raise ValueError(f"{name}: feature width {f.shape[1]}; morig_cosine_nn is built for width {NN_WIDTH} only")
    return f.to(device).contiguous()


def _nearest_global(vtx_feature, pts_feature, ptr_v, ptr_p) -> torch.Tensor:
    """int32 [V]: rows of the point array, -1 for a pair without points"""
    from .native import Mat
    V, P = vtx_feature.shape[0], pts_feature.shape[0]
    if V == 0 or P == 0:
        return torch.full((V,), -1, dtype=torch.int32, device=vtx_feature.device)
    # the largest vertex count of a pair sizes the grid only: the total is an upper bound that needs no host read
    nn, _ = get_ops().cosine_nn(Mat.of(vtx_feature), ptr_v, Mat.of(pts_feature), ptr_p, ptr_v.numel() - 1, V)
    return nn


# ------------------------------------------------------------------------------------------------------------------------- correspondences
def nearest_points(vtx_feature, pts_feature, vtx_batch, pts_batch, *, num_graphs=None) -> torch.Tensor:
    """Per vertex the local index of the point of its pair with the largest ``vtx_f . pts_f`` -> int64 [V] on the device: the
    ``np.argmax(vtx_f @ pts_f.T / tau, axis=1)`` of training/train_corr_pose.py:117-118 (``tau > 0`` does not change an arg-max, so it is
    no parameter). A wrapper over ``morig_cosine_nn``: unit rows of width 64; any other width raises. Near-ties may resolve differently
    from a float32 BLAS: the products are split-fp16 with fp32 sums (about 1e-7 on unit rows), the lowest index wins an exact tie. A pair
    without points gives -1. One host read (the status word)."""
    device = device_of(vtx_feature, pts_feature)
    vf, pf = _unit_rows(vtx_feature, "vtx_feature", device), _unit_rows(pts_feature, "pts_feature", device)
    vb, pb = _batch(vtx_batch, vf.shape[0], "vtx_batch", device), _batch(pts_batch, pf.shape[0], "pts_batch", device)
    B = _num_graphs(pb if pb.numel() else vb, num_graphs)
    ops = get_ops()
    status = ops.loss_status(device)
    ptr_v, ptr_p = ops.segment_ptr(vb, B, status), ops.segment_ptr(pb, B, status)
    nn = _nearest_global(vf, pf, ptr_v, ptr_p).long()
    local = torch.where(nn >= 0, nn - ptr_p.long()[vb.clamp(0, B - 1)], nn)
    bits = int(status)
    if bits:
        raise MotionMetricsInputError("nearest_points", bits)
    return local


def corr_accuracy(pts, corr_v2p, pts_batch, corr_v2p_batch, *, nnind=None, vtx_feature=None, pts_feature=None, vtx_batch=None,
                  tolerances=TOLERANCES, num_graphs=None) -> dict:
    """evaluate/eval_corr.py:17-22 per pair. ``pts`` float32 [P, 3]; ``corr_v2p`` [n, 2] rows (vertex, ground-truth point), local to the
    pair. Give exactly one of ``nnind`` ([V] local point indices, what the reference saves as ``_nnind.npy``) or the two feature
    matrices (unit rows, width 64: the arg-max is taken by ``morig_cosine_nn`` and handed to the kernel as rows of ``pts``, no index
    arithmetic in between). ``vtx_batch`` [V] is needed either way: it alone states the vertex counts per pair.

    -> dict of numpy arrays: hits int64 [B, n_tol] (rows with ``|pts[nn[v]] - pts[p_gt]| < float32(tol)``), count int64 [B], acc float64
    [B, n_tol] = hits / count * 100 (0 / 0 = NaN as in numpy), curve float64 [n_tol] = the sum of acc over the pairs that have
    correspondences, in pair order, over their number n_valid (the reference divides by the number of files and would propagate the
    NaN), n_valid int, tolerances float64 [n_tol]. An index outside its pair raises MotionMetricsInputError (its ``result`` holds the
    counts without that row). One host read."""
    features = vtx_feature is not None or pts_feature is not None
    if nnind is not None and features:
        raise ValueError("corr_accuracy: give nnind or the features, not both")
    if nnind is None and (vtx_feature is None or pts_feature is None):
        raise ValueError("corr_accuracy: give nnind, or both vtx_feature and pts_feature")
    if vtx_batch is None:
        raise ValueError("corr_accuracy: vtx_batch states the vertex counts per pair and is needed with nnind and with features alike")
    tol = _bins(tolerances, "corr_accuracy: tolerances")
    device = device_of(pts, corr_v2p, nnind, vtx_feature)
    pts, corr = as_tensor(pts), as_tensor(corr_v2p)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32:
        raise ValueError(f"corr_accuracy: pts is float32 [P, 3] (the distance rule is float32), got {pts.dtype} {tuple(pts.shape)}")
    if corr.dim() != 2 or corr.shape[1] != 2 or corr.is_floating_point():
        raise ValueError(f"corr_accuracy: corr_v2p is an integer [n, 2] (vertex, point), got {tuple(corr.shape)}")
    pts, corr = pts.to(device).contiguous(), corr.to(device=device, dtype=torch.int64).contiguous()
    n_vtx = as_tensor(vtx_batch).numel()
    vb, pb = _batch(vtx_batch, n_vtx, "vtx_batch", device), _batch(pts_batch, pts.shape[0], "pts_batch", device)
    cb = _batch(corr_v2p_batch, corr.shape[0], "corr_v2p_batch", device)
    B = _num_graphs(pb if pb.numel() else vb, num_graphs)
    ops = get_ops()
    status = ops.loss_status(device)
    ptr_v, ptr_p, ptr_c = (ops.segment_ptr(b, B, status) for b in (vb, pb, cb))
    if nnind is not None:
        nn = as_tensor(nnind)
        if nn.dim() != 1 or nn.numel() != n_vtx or nn.is_floating_point():
            raise ValueError(f"corr_accuracy: nnind is an integer vector with one entry per vertex ({n_vtx}), got {tuple(nn.shape)}")
        nn = nn.to(device).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()           # an index past int32 stays out of range
    else:
        vf, pf = _unit_rows(vtx_feature, "vtx_feature", device), _unit_rows(pts_feature, "pts_feature", device)
        if vf.shape[0] != n_vtx or pf.shape[0] != pts.shape[0]:
            raise ValueError("corr_accuracy: one feature row per vertex of vtx_batch and per point of pts")
        nn = _nearest_global(vf, pf, ptr_v, ptr_p)
    hits_dev = ops.corr_hits(pts, ptr_p, nn, ptr_v, nnind is None, corr, ptr_c, torch.from_numpy(tol).to(device), status)
    hits, ptr_host, bits = _read(hits_dev, ptr_c, status)
    count = np.diff(ptr_host) if not bits[0] & ~_K["MORIG_MOTION_ST_INDEX"] else np.zeros(B, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = hits.astype(np.float64) / count.astype(np.float64)[:, None] * 100.0
    curve, n_valid = np.zeros(len(tol)), 0
    for b in range(B):                                                                   # pair order, as the reference adds its files
        if count[b] > 0:
            curve += acc[b]
            n_valid += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        curve = curve / np.float64(n_valid)
    result = dict(hits=hits, count=count, acc=acc, curve=curve, n_valid=n_valid, tolerances=np.asarray(tolerances, dtype=np.float64).reshape(-1))
    if bits[0]:
        raise MotionMetricsInputError("corr_accuracy", int(bits[0]), result)
    return result


# ------------------------------------------------------------------------------------------------------------------------- attention
def pr_curve(pred, gt, batch, *, thresholds=THRESHOLDS, normalize=True, num_graphs=None) -> dict:
    """evaluate/eval_attn.py:21, 31-36, 50-51 per mesh. ``pred`` float32 [V] or [V, 1] (``harness.attention_probability``, what the
    reference saves as ``_attn.npy``); ``gt`` [V], read as boolean (non-zero is True, as ``astype(np.bool)``). With ``normalize`` the
    values of a mesh become ``(x - min) / (max - min)`` in float32 first; a constant mesh (0 / 0) or a mesh holding a NaN then predicts
    nothing: tp = pp = 0 and precision 0, as the reference. A predicted positive is ``x' > float32(t)``, strict -- float32 as under the
    reference's numpy 1.21, see the module docstring.

    ``normalize=False`` with the sigmoid of ``pred_vismask`` scores the visibility masks by the same rule; a NaN element alone counts
    nothing there. The reference saves those masks and never scores them: that use is this product's own.

    -> dict of numpy arrays: tp, pp int64 [B, n_thr], gp int64 [B] (the number of non-zero labels; the reference sums the label values,
    equal for 0 / 1 labels), precision = tp / (pp + 1e-6), recall = tp / (gp + 1e-6) float64 [B, n_thr], mean_precision, mean_recall
    float64 [n_thr] = the sum in mesh order over B, thresholds float64 [n_thr]. A mesh without vertices raises ValueError naming it (the
    reference's ``np.min`` raises there too). One host read."""
    thr = _bins(thresholds, "pr_curve: thresholds")
    device = device_of(pred, gt)
    pred, gt = as_tensor(pred), as_tensor(gt)
    if pred.dim() == 2 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 1 or pred.dtype != torch.float32:
        raise ValueError(f"pr_curve: pred is float32 [V] or [V, 1], got {pred.dtype} {tuple(pred.shape)}")
    if gt.dim() != 1 or gt.numel() != pred.numel():
        raise ValueError(f"pr_curve: gt has one label per vertex ({pred.numel()}), got {tuple(gt.shape)}")
    pred = pred.to(device).contiguous()
    gt = (gt.to(device) != 0).to(torch.uint8).contiguous()
    bvec = _batch(batch, pred.numel(), "batch", device)
    B = _num_graphs(bvec, num_graphs)
    ops = get_ops()
    status = ops.loss_status(device)
    ptr = ops.segment_ptr(bvec, B, status)
    tp, pp, gp, ptr_host, bits = _read(*ops.pr_counts(pred, gt, ptr, torch.from_numpy(thr).to(device), bool(normalize), status), ptr, status)
    precision = tp / (pp + 1e-6)
    recall = tp / (gp[:, None] + 1e-6)
    mean_precision, mean_recall = np.zeros(len(thr)), np.zeros(len(thr))
    for b in range(B):                                                                   # mesh order, as the reference adds its files
        mean_precision += precision[b]
        mean_recall += recall[b]
    result = dict(tp=tp, pp=pp, gp=gp, precision=precision, recall=recall, mean_precision=mean_precision / B, mean_recall=mean_recall / B,
                  thresholds=np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if bits[0]:
        raise MotionMetricsInputError("pr_curve", int(bits[0]), result)
    empty = np.nonzero(np.diff(ptr_host) == 0)[0]
    if len(empty):
        raise ValueError(f"pr_curve: mesh {int(empty[0])} has no vertices (meshes without vertices: {empty.tolist()})")
    return result


# ------------------------------------------------------------------------------------------------------------------------- key-frame flow
def keyframe_flow_errors(pred_flow, gt_flow, batch, *, num_graphs=None) -> tuple:
    """evaluate/eval_deform.py:18-19 per mesh. Both flows are [V, 3 K] in the ``dataset_rig`` layout, columns 3 t .. 3 t + 2 of key frame
    t (``models.deformnet``'s ``pred_flow``). -> (float64 [B, K]: per mesh and key frame the mean vertex distance; float64 [B]: the mean
    over the key frames, the number the reference appends per model), numpy. No kernel of its own: ``morig_pose_traj_errors`` on the
    [V, K, 3] view with every vertex visible, float64 in a fixed order (the reference's is float32 with numpy's pairwise means). A mesh
    without vertices gives NaN. One host read."""
    device = device_of(pred_flow, gt_flow)
    pred, gt = as_tensor(pred_flow), as_tensor(gt_flow)
    if pred.dim() != 2 or pred.shape[1] % 3 or pred.shape[1] == 0 or pred.shape != gt.shape:
        raise ValueError(f"keyframe_flow_errors: pred_flow and gt_flow are [V, 3 K], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    V, K = pred.shape[0], pred.shape[1] // 3
    bvec = _batch(batch, V, "batch", device)
    B = _num_graphs(bvec, num_graphs)
    if V == 0:
        raise ValueError("keyframe_flow_errors: no vertices")
    ops = get_ops()
    status = ops.loss_status(device)
    ptr = ops.segment_ptr(bvec, B, status)
    as64 = lambda t: t.to(device=device, dtype=torch.float64).reshape(V, K, 3).contiguous()
    full, _ = ops.pose_traj_errors(as64(pred), as64(gt), torch.ones(V, K, dtype=torch.uint8, device=device), ptr)
    host = torch.cat([full.reshape(-1), status.to(torch.float64)]).cpu().numpy()        # the one read
    bits, per_frame = int(host[-1]), host[:-1].reshape(B, K)
    if bits:
        raise MotionMetricsInputError("keyframe_flow_errors", bits)
    total = per_frame[:, 0].copy()
    for t in range(1, K):                                                                # key-frame order
        total += per_frame[:, t]
    return per_frame, total / np.float64(K)


# ------------------------------------------------------------------------------------------------------------------------- the driver
def evaluate_motion(*, corr: Optional[dict] = None, attn: Optional[dict] = None, vismask: Optional[dict] = None,
                    flow: Optional[dict] = None) -> dict:
    """Whichever of the scores has its inputs, each given as the keyword arguments of its function: ``corr`` -> ``corr_accuracy``,
    ``attn`` -> ``pr_curve``, ``vismask`` -> ``pr_curve(normalize=False)`` (``pred``: the sigmoid of ``pred_vismask``), ``flow`` ->
    ``keyframe_flow_errors`` (as ``dict(per_frame=, per_mesh=, mean=)``, mean = the sum in mesh order over B). -> dict with the keys that
    were given. One host read per score."""
    out = {}
    if corr is not None:
        out["corr"] = corr_accuracy(**corr)
    if attn is not None:
        out["attn"] = pr_curve(**attn)
    if vismask is not None:
        out["vismask"] = pr_curve(**dict(vismask, normalize=False))
    if flow is not None:
        per_frame, per_mesh = keyframe_flow_errors(**flow)
        total = np.float64(0.0)
        for v in per_mesh:
            total = total + v
        out["flow"] = dict(per_frame=per_frame, per_mesh=per_mesh, mean=total / np.float64(len(per_mesh)))
    if not out:
        raise ValueError("evaluate_motion: give at least one of corr, attn, vismask, flow")
    return out


def format_motion_report(result: dict) -> str:
    """One line per curve of an ``evaluate_motion`` result: the bins, then the values to three decimals."""
    row = lambda vals, fmt: " ".join(fmt.format(v) for v in vals)
    lines = []
    if "corr" in result:
        r = result["corr"]
        lines.append(f"\tcorr_accuracy(%) over {r['n_valid']} of {len(r['count'])} pairs at tolerances {row(r['tolerances'], '{:.2f}')}: "
                     f"{row(r['curve'], '{:.03f}')}")
    for key in ("attn", "vismask"):
        if key in result:
            r = result[key]
            lines.append(f"\t{key}_precision over {len(r['gp'])} meshes at thresholds {row(r['thresholds'], '{:.1f}')}: "
                         f"{row(r['mean_precision'], '{:.03f}')}")
            lines.append(f"\t{key}_recall over {len(r['gp'])} meshes at thresholds {row(r['thresholds'], '{:.1f}')}: "
                         f"{row(r['mean_recall'], '{:.03f}')}")
    if "flow" in result:
        r = result["flow"]
        lines.append(f"\tkeyframe_flow_error over {len(r['per_mesh'])} meshes and {r['per_frame'].shape[1]} key frames: {r['mean']:.06f}")
    return "\n".join(lines)
