"""Training losses on the device: the functions of models/customized_losses.py that the four training scripts import and call, and the
masked cross-entropy of the skin training step, as ``torch.autograd.Function``s over csrc/losses.hip and csrc/losses_skin.hip.

    infoNCE(vtx_feature, pts_feature, corr_v2p, corr_p2v, vtx_batch, pts_batch, corr_v2p_batch, corr_p2v_batch, tau)      (:107-134)
    multi_pos_infoNCE(pred_feature, gt_skin, batch)                                                                    (:137-158)
    chamfer_distance_with_average(p1, p2)                                                                              (:231-251)
    chamfer_batched(y_pred, batch, joints, joints_batch)       what training/train_rig.py:176-181 computes with its loop over meshes
    log_ratio_loss(pred_feature, gt_skin, batch)                                                                        (:11-44)
    log_ratio_frames(motion_all, motion_aggr, gt_skin, batch)  the T + 1 calls of training/train_skin.py:155-158 as one launch
    skin_ce_loss(skin_pred, skin_label, loss_mask)             training/train_skin.py:168-174
    cross_entropy_with_probs(input, target, weight, reduction)                                                          (:216-228)

All meshes / pairs of a batch run in one launch; there is no per-mesh Python loop, no floating-point atomic (two runs give the same bits)
and no CPU fallback: a shape the kernels do not take raises and names the limit.

Host reads. With ``num_graphs`` given nothing is read back on the way to the loss (``num_graphs=None`` costs one read of the last batch
value). What the kernels find wrong with the DATA -- an unsorted batch vector, an index outside its pair -- cannot be known without a read:
they clamp the index (no access leaves its array), set a bit in a status word and the loss comes out NaN. The status word travels to pinned
host memory behind the launch and is looked at, without waiting, at the next call into this module and in ``backward``; ``check_inputs()``
waits for every outstanding one. On tensors whose status is at hand at once the error is raised by the call itself.

``multi_pos_infoNCE`` draws its samples as the reference does unless ``samples=`` passes them; ``draw_multi_pos_samples`` is the batched
sampler (its validation -- a mesh with fewer than n_sample vertices, a row without a negative -- costs one host read).
``log_ratio_loss`` / ``log_ratio_frames`` do the same with ``draw_log_ratio_samples``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import runtime
from .abi import CONSTANTS as _K

__all__ = ["infoNCE", "multi_pos_infoNCE", "draw_multi_pos_samples", "chamfer_distance_with_average", "chamfer_batched", "check_inputs",
           "LossInputError", "log_ratio_loss", "log_ratio_frames", "draw_log_ratio_samples", "skin_ce_loss", "cross_entropy_with_probs"]

ST_INDEX, ST_UNSORTED, ST_SEGMENT, ST_SIZE = (_K["MORIG_LOSS_ST_" + n] for n in ("INDEX", "UNSORTED", "SEGMENT", "SIZE"))
NCE_WIDTH = 64
MULTIPOS_MAX_WIDTH = 128
CHAMFER_MAX_JOINTS = _K["MORIG_CHAMFER_MAX_JOINTS"]
LOGRATIO_MAX_WIDTH, LOGRATIO_MIN_SAMPLE, LOGRATIO_MAX_SAMPLE = _K["MORIG_LOGRATIO_MAX_WIDTH"], 3, _K["MORIG_LOGRATIO_MAX_SAMPLE"]
SKIN_CE_MAX_K, CE_PROBS_MAX_K = _K["MORIG_SKIN_CE_MAX_K"], _K["MORIG_CE_PROBS_MAX_K"]


class LossInputError(ValueError):
    pass


def _unsupported(msg: str):
    return LossInputError("MORIG_E_UNSUPPORTED: " + msg)


# ------------------------------------------------------------------------------------------------------- deferred input status
_pending = []


def _status_message(bits: int, what: str) -> str:
    parts = []
    if bits & ST_INDEX:
        parts.append("an index lies outside its pair / mesh")
    if bits & ST_UNSORTED:
        parts.append("a batch vector is not sorted")
    if bits & ST_SEGMENT:
        parts.append("a batch value lies outside [0, num_graphs)")
    if bits & ST_SIZE:
        parts.append(f"a mesh has more than {CHAMFER_MAX_JOINTS} joints")
    return f"{what}: {'; '.join(parts) or 'status %d' % bits} (the loss of that call is NaN)"


def _post(status: torch.Tensor, what: str) -> None:
    if not status.is_cuda:
        bits = int(status)
        if bits:
            raise LossInputError(_status_message(bits, what))
        return
    host = torch.empty(1, dtype=torch.int32, pin_memory=True)
    host.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _pending.append((host, ev, what))


def _poll(wait: bool = False) -> None:
    keep, bad = [], None
    for host, ev, what in _pending:
        if wait:
            ev.synchronize()
        if ev.query():
            if int(host[0]) and bad is None:
                bad = _status_message(int(host[0]), what)
        else:
            keep.append((host, ev, what))
    _pending[:] = keep
    if bad:
        raise LossInputError(bad)


def check_inputs() -> None:
    """waits for every loss launched so far and raises if one of them found its inputs wrong"""
    _poll(wait=True)


# ------------------------------------------------------------------------------------------------------- helpers
def _num_graphs(batch: torch.Tensor, num_graphs: Optional[int]) -> int:
    if num_graphs is not None:
        if int(num_graphs) < 1:
            raise LossInputError("num_graphs must be at least 1")
        return int(num_graphs)
    if batch.numel() == 0:
        raise LossInputError("an empty batch vector needs num_graphs")
    return int(batch.max()) + 1                          # the one host read


def _batch_vec(b: torch.Tensor, n: int, name: str) -> torch.Tensor:
    if b.dim() != 1 or b.numel() != n:
        raise LossInputError(f"{name}: expected a vector of {n} entries, got {tuple(b.shape)}")
    return b.long().contiguous()


def _features(f: torch.Tensor, name: str) -> torch.Tensor:
    if f.dim() != 2:
        raise LossInputError(f"{name}: expected a [rows, width] matrix, got {tuple(f.shape)}")
    if f.dtype != torch.float32:
        raise LossInputError(f"{name}: float32 only, got {f.dtype}")
    return f


def _row_major(f: torch.Tensor) -> torch.Tensor:
    """a strided view is read in place when its rows are 16-byte aligned float runs; anything else is made contiguous"""
    if f.stride(1) != 1 or f.stride(0) % 4 or f.data_ptr() % 16 or f.stride(0) < f.shape[1]:
        return f.contiguous()
    return f


def _upstream(g: torch.Tensor) -> torch.Tensor:
    return g.detach().reshape(1).to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------- infoNCE
class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vtx, pts, corr_v2p, corr_p2v, cb_v2p, cb_p2v, ptrs, tau, status):
        ops = runtime.get_ops()
        vtx_r, pts_r = _row_major(vtx.detach()), _row_major(pts.detach())
        loss, lse = ops.infonce_forward(vtx_r, pts_r, corr_v2p, corr_p2v, ptrs, tau, status)
        ctx.save_for_backward(vtx_r, pts_r, corr_v2p, corr_p2v, cb_v2p, cb_p2v, lse, status, *ptrs)
        ctx.tau = tau
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        _poll()
        ops = runtime.get_ops()
        vtx, pts, corr_v2p, corr_p2v, cb_v2p, cb_p2v, lse, status = ctx.saved_tensors[:8]
        ptrs = ctx.saved_tensors[8:]
        B = ptrs[0].numel() - 1

        def groups(corr, cb, ptr_anchor, n_anchor):
            # the rows of one direction grouped by their GLOBAL anchor, in row order (stable): the order the anchor-side sums run in
            base = ptr_anchor.long()[cb.clamp(0, B - 1)] if corr.shape[0] else corr.new_zeros(0)
            key = (base + corr[:, 0]).clamp(0, max(n_anchor - 1, 0))
            skey, order = torch.sort(key, stable=True)
            rowptr = torch.searchsorted(skey, torch.arange(n_anchor + 1, device=corr.device))
            return rowptr.int().contiguous(), order.int().contiguous()
        rp_v, ord_v = groups(corr_v2p, cb_v2p, ptrs[0], vtx.shape[0])
        rp_p, ord_p = groups(corr_p2v, cb_p2v, ptrs[1], pts.shape[0])
        g_vtx, g_pts = ops.infonce_backward(vtx, pts, corr_v2p, corr_p2v, ptrs, ctx.tau, lse, _upstream(grad_out), (rp_v, ord_v, rp_p, ord_p),
                                            status)
        return g_vtx, g_pts, None, None, None, None, None, None, None


def infoNCE(vtx_feature, pts_feature, corr_v2p, corr_p2v, vtx_batch, pts_batch, corr_v2p_batch, corr_p2v_batch, tau, *, num_graphs=None):
    """customized_losses.py:107-134. Per pair and direction the mean over correspondence rows of the cross-entropy of
    ``anchor . keys^T / tau`` against the label column; indices are local to the pair, duplicates allowed. A pair without v2p rows
    contributes nothing (its p2v term is skipped too); a pair without p2v rows contributes its v2p term; the sum is divided by the number
    of pairs. Feature width 64."""
    _poll()
    vtx, pts = _features(vtx_feature, "vtx_feature"), _features(pts_feature, "pts_feature")
    if vtx.shape[1] != NCE_WIDTH or pts.shape[1] != NCE_WIDTH:
        raise _unsupported(f"infoNCE is built for feature width {NCE_WIDTH}, got {vtx.shape[1]} and {pts.shape[1]}")
    if not float(tau) > 0:
        raise LossInputError("tau must be positive")
    for c, name in ((corr_v2p, "corr_v2p"), (corr_p2v, "corr_p2v")):
        if c.dim() != 2 or c.shape[1] != 2:
            raise LossInputError(f"{name}: expected [rows, 2] (anchor, label), got {tuple(c.shape)}")
    ops = runtime.get_ops()
    vb, pb = _batch_vec(vtx_batch, vtx.shape[0], "vtx_batch"), _batch_vec(pts_batch, pts.shape[0], "pts_batch")
    cvb, cpb = _batch_vec(corr_v2p_batch, corr_v2p.shape[0], "corr_v2p_batch"), _batch_vec(corr_p2v_batch, corr_p2v.shape[0], "corr_p2v_batch")
    B = _num_graphs(vb, num_graphs)
    status = ops.loss_status(vtx.device)
    ptrs = tuple(ops.segment_ptr(b, B, status) for b in (vb, pb, cvb, cpb))
    loss = _InfoNCE.apply(vtx, pts, corr_v2p.long().contiguous(), corr_p2v.long().contiguous(), cvb, cpb, ptrs, float(tau), status)
    _post(status, "infoNCE")
    return loss


# ------------------------------------------------------------------------------------------------------- multi-positive infoNCE
def draw_multi_pos_samples(gt_skin, batch, n_sample=512, n_pos=10, n_neg=200, generator=None, num_graphs=None) -> Tuple[torch.Tensor, ...]:
    """The draws of customized_losses.py:141-149 for every mesh at once, on the device of ``gt_skin``:
    sample_ids [B, n_sample] vertex indices local to the mesh, without replacement; pos_ids [B, n_sample, n_pos] indices into the samples,
    with replacement among gt_sim > 0.9 (gt_sim = (2 - sum |skin_a - skin_b|) / 2); neg_ids [B, n_sample, n_neg] among the rest.
    Raises where the reference raises: a mesh with fewer than n_sample vertices, a row without any negative (one host read)."""
    if gt_skin.dim() != 2 or batch.dim() != 1 or batch.numel() != gt_skin.shape[0]:
        raise LossInputError("draw_multi_pos_samples: gt_skin [N, bones] and batch [N]")
    dev = gt_skin.device
    batch = batch.long()
    B = _num_graphs(batch, num_graphs)
    N = batch.numel()
    counts = torch.bincount(batch.clamp(0, B - 1), minlength=B)
    ptr = torch.cumsum(counts, 0) - counts
    # without replacement: a random key per vertex, sorted inside its mesh, the first n_sample taken
    keys = batch.double() + torch.rand(N, dtype=torch.float64, device=dev, generator=generator).clamp_(max=1 - 2.0 ** -40)
    order = torch.argsort(keys)
    take = (ptr[:, None] + torch.arange(n_sample, device=dev)[None, :]).clamp_(max=max(N - 1, 0))
    glob = order[take]                                                   # [B, n_sample] global vertex rows
    sample_ids = glob - ptr[:, None]
    skin = gt_skin[glob].float()
    sim = (2.0 - torch.cdist(skin, skin, p=1.0)) / 2.0
    posmask = sim > 0.9
    ok = torch.stack([counts.min() >= n_sample, (~posmask).sum(-1).min() > 0]).tolist()          # the one host read
    if not ok[0]:
        raise LossInputError(f"draw_multi_pos_samples: a mesh has fewer than {n_sample} vertices")
    if not ok[1]:
        raise LossInputError("draw_multi_pos_samples: a sample row has no negative (every sample of its mesh has gt_sim > 0.9)")
    w = posmask.reshape(B * n_sample, n_sample).float()
    pos_ids = torch.multinomial(w, n_pos, replacement=True, generator=generator).reshape(B, n_sample, n_pos)
    neg_ids = torch.multinomial(1.0 - w, n_neg, replacement=True, generator=generator).reshape(B, n_sample, n_neg)
    return sample_ids, pos_ids, neg_ids


class _MultiPos(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rows, pos_ids, neg_ids, B, S, status):
        from .native import Mat
        ops = runtime.get_ops()
        src = feat.detach()
        if src.stride(1) != 1:
            src = src.contiguous()
        F = torch.empty(B * S, src.shape[1], dtype=torch.float32, device=src.device)
        ops.gather_rows(Mat.of(src), rows, Mat.of(F))
        loss, neg_max, neg_sum = ops.multipos_forward(F, pos_ids, neg_ids, B, S, status)
        ctx.save_for_backward(F, rows, pos_ids, neg_ids, neg_max, neg_sum, status)
        ctx.dims = (B, S, feat.shape[0])
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        _poll()
        ops = runtime.get_ops()
        F, rows, pos_ids, neg_ids, neg_max, neg_sum, status = ctx.saved_tensors
        B, S, n_total = ctx.dims
        grad = ops.multipos_backward(F, pos_ids, neg_ids, B, S, neg_max, neg_sum, _upstream(grad_out), rows, n_total, status)
        return grad, None, None, None, None, None, None


def multi_pos_infoNCE(pred_feature, gt_skin, batch, *, samples=None, num_graphs=None):
    """customized_losses.py:137-158 with the draws of ``samples = (sample_ids, pos_ids, neg_ids)`` (``None``: drawn here). Per mesh
    ``(1 / n_pos) sum_j mean_rows [log(exp(p_rj) + sum_negs exp(n_r.)) - p_rj]`` on the products of the sampled feature rows, no
    temperature, duplicates counted as often as drawn; over the batch ``sum / B``. ``pred_feature`` may be a strided view such as
    ``motion_all[:, t, :]``; its width a multiple of 4 up to 128. ``gt_skin`` gets no gradient; unsampled rows get exact zeros."""
    _poll()
    feat = _features(pred_feature, "pred_feature")
    D = feat.shape[1]
    if D % 4 or not 4 <= D <= MULTIPOS_MAX_WIDTH:
        raise _unsupported(f"multi_pos_infoNCE takes feature widths that are a multiple of 4 up to {MULTIPOS_MAX_WIDTH}, got {D}")
    bvec = _batch_vec(batch, feat.shape[0], "batch")
    B = _num_graphs(bvec, num_graphs)
    if samples is None:
        samples = draw_multi_pos_samples(gt_skin, bvec, num_graphs=B)
    sample_ids, pos_ids, neg_ids = samples
    if sample_ids.dim() != 2 or sample_ids.shape[0] != B or pos_ids.shape[:2] != sample_ids.shape or neg_ids.shape[:2] != sample_ids.shape:
        raise LossInputError(f"samples: sample_ids [B, S], pos_ids [B, S, P], neg_ids [B, S, N] with B = {B}")
    S = sample_ids.shape[1]
    ops = runtime.get_ops()
    dev = feat.device
    status = ops.loss_status(dev)
    ptr = ops.segment_ptr(bvec, B, status).long()
    sid = sample_ids.to(dev).long()
    counts = (ptr[1:] - ptr[:-1])[:, None]
    bad = ((sid < 0) | (sid >= counts)).any()
    srt = torch.sort(sid, dim=1).values
    bad = bad | (srt[:, 1:] == srt[:, :-1]).any()                       # a repeated sample would be stored twice
    status |= (bad.to(torch.int32) * ST_INDEX)
    rows = (ptr[:-1, None] + sid).clamp_(0, max(feat.shape[0] - 1, 0)).int().reshape(-1).contiguous()
    loss = _MultiPos.apply(feat, rows, pos_ids.to(dev).int().contiguous(), neg_ids.to(dev).int().contiguous(), B, S, status)
    _post(status, "multi_pos_infoNCE")
    return loss


# ------------------------------------------------------------------------------------------------------- chamfer
class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q, ptr_p, ptr_q, status):
        ops = runtime.get_ops()
        pc, qc = p.detach().contiguous(), q.detach().contiguous()
        loss, arg1, d1, key2 = ops.chamfer_forward(pc, qc, ptr_p, ptr_q, status)
        ctx.save_for_backward(pc, qc, ptr_p, ptr_q, arg1, d1, key2, status)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        _poll()
        ops = runtime.get_ops()
        pc, qc, ptr_p, ptr_q, arg1, d1, key2, status = ctx.saved_tensors
        gp, gq = ops.chamfer_backward(pc, qc, ptr_p, ptr_q, arg1, d1, key2, _upstream(grad_out), status)
        return gp, gq, None, None, None


def _points(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2 or t.shape[1] != 3:
        raise _unsupported(f"{name}: point dimension 3 only, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise LossInputError(f"{name}: float32 only, got {t.dtype}")
    if t.shape[0] == 0:
        raise LossInputError(f"{name}: no points")
    return t


def chamfer_batched(y_pred, batch, joints, joints_batch, *, num_graphs=None):
    """mean over meshes of 0.5 (mean_i min_j |y_i - j_j| + mean_j min_i |y_i - j_j|): training/train_rig.py:176-181 without its loop.
    At most 1024 joints per mesh. Ties go to the smallest index; a zero distance has a zero gradient."""
    _poll()
    p, q = _points(y_pred, "y_pred"), _points(joints, "joints")
    ops = runtime.get_ops()
    pb, qb = _batch_vec(batch, p.shape[0], "batch"), _batch_vec(joints_batch, q.shape[0], "joints_batch")
    B = _num_graphs(qb, num_graphs)
    status = ops.loss_status(p.device)
    ptr_p, ptr_q = ops.segment_ptr(pb, B, status), ops.segment_ptr(qb, B, status)
    loss = _Chamfer.apply(p, q, ptr_p, ptr_q, status)
    _post(status, "chamfer_batched")
    return loss


def chamfer_distance_with_average(p1, p2):
    """customized_losses.py:231-251: p1 [1, N, 3], p2 [1, M, 3] -> 0.5 (mean_i min_j + mean_j min_i) of the distances"""
    _poll()
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != 1 or p2.shape[0] != 1:
        raise LossInputError(f"chamfer_distance_with_average: [1, N, 3] and [1, M, 3], got {tuple(p1.shape)} and {tuple(p2.shape)}")
    a, b = _points(p1[0], "p1"), _points(p2[0], "p2")
    if b.shape[0] > CHAMFER_MAX_JOINTS:                                  # the loss is symmetric: the smaller set goes to LDS
        a, b = b, a
    if b.shape[0] > CHAMFER_MAX_JOINTS:
        raise _unsupported(f"chamfer: one of the two sets must have at most {CHAMFER_MAX_JOINTS} points, got {a.shape[0]} and {b.shape[0]}")
    ops = runtime.get_ops()
    status = ops.loss_status(a.device)
    ptr_p = torch.tensor([0, a.shape[0]], dtype=torch.int32).to(a.device)
    ptr_q = torch.tensor([0, b.shape[0]], dtype=torch.int32).to(a.device)
    loss = _Chamfer.apply(a, b, ptr_p, ptr_q, status)
    _post(status, "chamfer_distance_with_average")
    return loss


# ------------------------------------------------------------------------------------------------------- log-ratio
def draw_log_ratio_samples(batch, n_sample=50, n_sets=1, generator=None, num_graphs=None) -> torch.Tensor:
    """The draws of customized_losses.py:19 for every mesh and ``n_sets`` calls at once, on the device of ``batch``: [n_sets, B, n_sample]
    vertex indices local to the mesh, without replacement (a random key per vertex, sorted inside its mesh, the first n_sample taken).
    Raises where the reference's np.random.choice raises: a mesh with fewer than n_sample vertices (one host read)."""
    if batch.dim() != 1:
        raise LossInputError("draw_log_ratio_samples: batch [N]")
    dev = batch.device
    batch = batch.long()
    B = _num_graphs(batch, num_graphs)
    N = batch.numel()
    counts = torch.bincount(batch.clamp(0, B - 1), minlength=B)
    ptr = torch.cumsum(counts, 0) - counts
    keys = batch.double()[None, :] + torch.rand(n_sets, N, dtype=torch.float64, device=dev, generator=generator).clamp_(max=1 - 2.0 ** -40)
    order = torch.argsort(keys, dim=1)
    take = (ptr[:, None] + torch.arange(n_sample, device=dev)[None, :]).clamp_(max=max(N - 1, 0))
    if not bool(counts.min() >= n_sample):                                  # the one host read
        raise LossInputError(f"draw_log_ratio_samples: a mesh has fewer than {n_sample} vertices")
    return order[:, take] - ptr[None, :, None]


def _view3(f: torch.Tensor) -> torch.Tensor:
    """[N, T, C] read in place when every (vertex, keyframe) row is a 16-byte aligned float run; anything else is made contiguous"""
    if f.stride(2) != 1 or f.stride(0) % 4 or f.stride(1) % 4 or f.data_ptr() % 16:
        return f.contiguous()
    return f


class _LogRatio(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_all, feat_aggr, gt, ptr, samples, status):
        ops = runtime.get_ops()
        fa = None if feat_all is None else _view3(feat_all.detach())
        fg = None if feat_aggr is None else _row_major(feat_aggr.detach())
        loss, tab = ops.logratio_forward(fa, fg, gt, ptr, samples, status)
        ctx.save_for_backward(*(t for t in (fa, fg) if t is not None), gt, ptr, samples, tab, status)
        ctx.has = (fa is not None, fg is not None)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        _poll()
        ops = runtime.get_ops()
        saved = list(ctx.saved_tensors)
        fa = saved.pop(0) if ctx.has[0] else None
        fg = saved.pop(0) if ctx.has[1] else None
        gt, ptr, samples, tab, status = saved
        g_all, g_aggr = ops.logratio_backward(fa, fg, gt, ptr, samples, tab, _upstream(grad_out), status)
        return g_all, g_aggr, None, None, None, None


def _log_ratio(feat_all, feat_aggr, gt_skin, batch, samples, num_graphs, what):
    _poll()
    D = (feat_aggr if feat_aggr is not None else feat_all).shape[-1]
    n = (feat_aggr if feat_aggr is not None else feat_all).shape[0]
    gt = _features(gt_skin, "gt_skin")
    W = gt.shape[1]
    if D % 4 or not 4 <= D <= LOGRATIO_MAX_WIDTH:
        raise _unsupported(f"{what} takes feature widths that are a multiple of 4 from 4 to {LOGRATIO_MAX_WIDTH}, got {D}")
    if W % 4 or not 4 <= W <= LOGRATIO_MAX_WIDTH:
        raise _unsupported(f"{what} takes gt_skin widths that are a multiple of 4 up to {LOGRATIO_MAX_WIDTH}, got {W}")
    if gt.shape[0] != n:
        raise LossInputError(f"gt_skin: expected {n} rows, got {gt.shape[0]}")
    bvec = _batch_vec(batch, n, "batch")
    B = _num_graphs(bvec, num_graphs)
    n_sets = (0 if feat_all is None else feat_all.shape[1]) + (feat_aggr is not None)
    if samples is None:
        samples = draw_log_ratio_samples(bvec, n_sets=n_sets, num_graphs=B)
    if samples.dim() == 2:
        samples = samples[None]
    if samples.dim() != 3 or samples.shape[0] != n_sets or samples.shape[1] != B:
        raise LossInputError(f"samples: expected [{n_sets}, {B}, n_sample] ids local to the mesh, got {tuple(samples.shape)}")
    S = samples.shape[2]
    if S == 2:
        raise _unsupported(f"{what}: n_sample = 2 is one pair, the mean over no pair of pairs (0 / 0 in the reference)")
    if not LOGRATIO_MIN_SAMPLE <= S <= LOGRATIO_MAX_SAMPLE:
        raise _unsupported(f"{what} takes n_sample from {LOGRATIO_MIN_SAMPLE} to {LOGRATIO_MAX_SAMPLE}, got {S}")
    ops = runtime.get_ops()
    dev = gt.device
    status = ops.loss_status(dev)
    ptr = ops.segment_ptr(bvec, B, status)
    loss = _LogRatio.apply(feat_all, feat_aggr, _row_major(gt.detach()), ptr, samples.to(dev).int().contiguous(), status)
    _post(status, what)
    return loss


def log_ratio_loss(pred_feature, gt_skin, batch, *, samples=None, num_graphs=None):
    """customized_losses.py:11-44 with the draws of ``samples`` ([B, n_sample] ids local to the mesh; ``None``: 50 per mesh, drawn here).
    With L[i][j] = log(|f_i - f_j|^2 + 1e-6) - log(|g_i - g_j|^2 + 1e-6) on the sampled rows and the pairs p = (a, b), a < b, in
    ``itertools.combinations`` order, per mesh the mean over p < q of (L[a_q][b_p] - L[a_p][b_q])^2; over the batch ``sum / B``.
    ``pred_feature`` may be a strided view such as ``motion_all[:, t, :]``; its width a multiple of 4 from 4 to 128, the width of
    ``gt_skin`` a multiple of 4 up to 128, n_sample from 3 to 64. ``gt_skin`` gets no gradient; unsampled rows get exact zeros."""
    feat = _features(pred_feature, "pred_feature")
    return _log_ratio(None, feat, gt_skin, batch, samples, num_graphs, "log_ratio_loss")


def log_ratio_frames(motion_all, motion_aggr, gt_skin, batch, *, samples=None, num_graphs=None):
    """training/train_skin.py:155-158 before its factor: ``sum_t log_ratio_loss(motion_all[:, t, :]) + log_ratio_loss(motion_aggr)`` in
    one forward and one backward launch. ``samples`` [T + 1, B, n_sample] (the reference draws afresh for every call); the sum over
    the sets runs in float64 in set order. The gradient of ``motion_all`` is written in place, set by set."""
    if motion_all.dim() != 3:
        raise LossInputError(f"motion_all: expected [vertices, keyframes, width], got {tuple(motion_all.shape)}")
    if motion_all.dtype != torch.float32:
        raise LossInputError(f"motion_all: float32 only, got {motion_all.dtype}")
    aggr = _features(motion_aggr, "motion_aggr")
    if aggr.shape[0] != motion_all.shape[0] or aggr.shape[1] != motion_all.shape[2]:
        raise LossInputError(f"motion_aggr: expected {(motion_all.shape[0], motion_all.shape[2])}, got {tuple(aggr.shape)}")
    if motion_all.shape[1] < 1:
        raise LossInputError("motion_all: no keyframe")
    return _log_ratio(motion_all, aggr, gt_skin, batch, samples, num_graphs, "log_ratio_frames")


# ------------------------------------------------------------------------------------------------------- masked soft-label cross-entropy
class _SkinCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, label, mask, K):
        ops = runtime.get_ops()
        xd = x.detach()
        if xd.stride(1) != 1:
            xd = xd.contiguous()
        loss, vert_mask, sums = ops.skin_ce_forward(xd, label, mask, K)
        ctx.save_for_backward(xd, label, mask, sums)
        ctx.K = K
        ctx.mark_non_differentiable(vert_mask)
        return loss.reshape(()), vert_mask

    @staticmethod
    def backward(ctx, grad_out, _grad_mask):
        ops = runtime.get_ops()
        xd, label, mask, sums = ctx.saved_tensors
        return ops.skin_ce_backward(xd, label, mask, ctx.K, sums, _upstream(grad_out)), None, None, None


def skin_ce_loss(skin_pred, skin_label, loss_mask, *, nearest_bone=None, return_vert_mask=False):
    """training/train_skin.py:168-174: with K = ``nearest_bone`` (``None``: the width of ``skin_pred``; at most 8), g = skin_label[:, :K] *
    loss_mask[:, :K], q = g / (sum |g| + 1e-8), vert_mask = |sum q - 1| < 1e-8 and w = loss_mask * vert_mask:
    ``sum(-q log_softmax(skin_pred) w) / sum(w)``; a batch where nothing survives the masks is 0 / 0 = NaN. The two label sums run in
    index order in float32 -- vert_mask is an equality test on a rounded sum, and this order is the rule.
    ``return_vert_mask``: -> (loss, vert_mask float [N])."""
    _poll()
    x = _features(skin_pred, "skin_pred")
    K = x.shape[1] if nearest_bone is None else int(nearest_bone)
    if not 1 <= K <= SKIN_CE_MAX_K:
        raise _unsupported(f"skin_ce_loss takes nearest_bone from 1 to {SKIN_CE_MAX_K}, got {K}")
    if x.shape[1] != K:
        raise LossInputError(f"skin_pred: expected [vertices, {K}] (nearest_bone columns), got {tuple(x.shape)}")
    label = _features(skin_label, "skin_label")
    if loss_mask.dim() != 2:
        raise LossInputError(f"loss_mask: expected a [vertices, bones] matrix, got {tuple(loss_mask.shape)}")
    for t, name in ((label, "skin_label"), (loss_mask, "loss_mask")):
        if t.shape[0] != x.shape[0] or t.shape[1] < K:
            raise LossInputError(f"{name}: expected [{x.shape[0]}, >= {K}], got {tuple(t.shape)}")
    label, mask = label.detach(), loss_mask.detach().float()
    label = label if label.stride(1) == 1 else label.contiguous()
    mask = mask if mask.stride(1) == 1 else mask.contiguous()
    loss, vert_mask = _SkinCE.apply(x, label, mask, K)
    return (loss, vert_mask) if return_vert_mask else loss


class _CEProbs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, weight, reduction):
        ops = runtime.get_ops()
        xd = x.detach().contiguous()
        out = ops.ce_probs_forward(xd, target, weight, reduction)
        ctx.save_for_backward(xd, target, *(() if weight is None else (weight,)))
        ctx.reduction = reduction
        return out if reduction == "none" else out.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        ops = runtime.get_ops()
        xd, target = ctx.saved_tensors[:2]
        weight = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        up = grad_out.detach().to(torch.float32).contiguous() if ctx.reduction == "none" else _upstream(grad_out)
        return ops.ce_probs_backward(xd, target, weight, ctx.reduction, up), None, None, None


def cross_entropy_with_probs(input, target, weight=None, reduction="mean"):
    """customized_losses.py:216-228: ``-target * log_softmax(input, 1)`` (times ``weight``, broadcast to [N, K]); "none" returns the
    [N, K] matrix, "mean" the mean over rows of the row sums, "sum" the sum. At most 128 classes. ``input`` alone gets a gradient."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("Keyword 'reduction' must be one of ['none', 'mean', 'sum']")
    _poll()
    x = _features(input, "input")
    if not 1 <= x.shape[1] <= CE_PROBS_MAX_K:
        raise _unsupported(f"cross_entropy_with_probs takes at most {CE_PROBS_MAX_K} classes, got {x.shape[1]}")
    if x.shape[0] == 0:
        raise LossInputError("input: no rows")
    if tuple(target.shape) != tuple(x.shape):
        raise LossInputError(f"target: expected {tuple(x.shape)}, got {tuple(target.shape)}")
    t = target.detach().to(torch.float32).contiguous()
    w = None
    if weight is not None:
        try:
            w = torch.broadcast_to(weight.detach().to(torch.float32), x.shape).contiguous()
        except RuntimeError:
            raise LossInputError(f"weight: {tuple(weight.shape)} does not broadcast to {tuple(x.shape)}") from None
    return _CEProbs.apply(x, t, w, reduction)
