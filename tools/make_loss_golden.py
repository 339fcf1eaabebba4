"""Fixtures of the training losses (tests/golden/loss_*.npz), made by the reference's own functions: infoNCE, multi_pos_infoNCE and
chamfer_distance_with_average of models/customized_losses.py, imported from where the reference lies (oracle.shim stands in for its
third-party imports, a stub for torch_cluster.fps). Nothing of the reference is written into the repository: only inputs and results.

  loss_nce_inputs   the batch of five pairs of tests/test_gpu_losses.py: features (width 64, unit rows), correspondences, batch vectors
  loss_nce_<case>   per case (tau 0.07, tau 0.01, rows of norm 3 at tau 0.07) the reference's float32 loss and autograd gradients
  loss_multipos     meshes of 512 and 700 vertices, width 32, 6 bones: features, skin, the reference's DRAWS (np.random.choice and
                    torch.multinomial are wrapped while it runs), its float32 loss and gradient
  loss_chamfer      (N, M) = (600, 17), (1, 1), (64, 1), (65, 33), (1025, 3) and a case whose joint 2 IS vertex 7: per mesh the
                    reference's float32 loss and gradients

Per case the deviation of the reference's float32 result from tests/loss_oracle.py (float64, closed-form gradients) is stored: relative
for the loss, relative to max |grad| for each gradient. The device is held to ten times these (tests/test_gpu_losses.py).

Conditions enforced here (the run fails rather than write a fixture that misses one) and re-checked by tests/test_loss_oracle.py: no
chamfer minimum within 1e-5 of its runner-up; no gt_sim within 1e-4 of 0.9; every mesh has at least 512 vertices; every sample row has at
least one negative. Ids are stored as uint16.

Run from the repository root:  python tools/make_loss_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (save)
import loss_oracle as lo                                                       # noqa: E402

CHAMFER_MARGIN, SIM_MARGIN, N_SAMPLE = 1e-5, 1e-4, 512
NCE_PAIRS = [(70, 200, 40, 33), (130, 129, 0, 17), (65, 64, 65, 0), (1, 1, 1, 1), (129, 513, 300, 257)]
NCE_CASES = {"tau007": dict(tau=0.07, scale=1.0), "tau001": dict(tau=0.01, scale=1.0), "norm3": dict(tau=0.07, scale=3.0)}
CHAMFER_SHAPES = [(600, 17), (1, 1), (64, 1), (65, 33), (1025, 3)]
MAX_BYTES = max(os.path.getsize(os.path.join(msg.OUT, f)) for f in os.listdir(msg.OUT) if not f.startswith("loss_"))


def reference():
    shim.install()
    stub = types.ModuleType("torch_cluster")
    stub.fps = None
    sys.modules["torch_cluster"] = stub
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    return __import__("models.customized_losses", fromlist=["infoNCE"])


def save(name, meta, **arrs):
    msg.save(name, meta, **arrs)
    size = os.path.getsize(os.path.join(msg.OUT, name + ".npz"))
    assert size <= MAX_BYTES, (name, size, MAX_BYTES)


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def rel_max(a, b):
    b = np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / scale) if scale > 0 else float(np.abs(np.asarray(a)).max())


def unit_rows(rng, n, c):
    x = rng.standard_normal((n, c))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- infoNCE
def nce_inputs(rng):
    vtx = np.concatenate([unit_rows(rng, nv, 64) for nv, _, _, _ in NCE_PAIRS])
    pts = np.concatenate([unit_rows(rng, npt, 64) for _, npt, _, _ in NCE_PAIRS])
    cv, cp = [], []
    for nv, npt, rv, rp in NCE_PAIRS:
        # labels drawn from a small set so that they repeat; 300 anchors among 129 vertices repeat by counting
        cv.append(np.stack([rng.integers(0, nv, rv), rng.integers(0, min(npt, 40), rv)], axis=1))
        cp.append(np.stack([rng.integers(0, npt, rp), rng.integers(0, min(nv, 40), rp)], axis=1))
    rep = lambda k: np.repeat(np.arange(len(NCE_PAIRS)), [p[k] for p in NCE_PAIRS])
    return dict(vtx=vtx, pts=pts, corr_v2p=np.concatenate(cv).astype(np.uint16), corr_p2v=np.concatenate(cp).astype(np.uint16),
                vtx_batch=rep(0).astype(np.uint16), pts_batch=rep(1).astype(np.uint16), corr_v2p_batch=rep(2).astype(np.uint16),
                corr_p2v_batch=rep(3).astype(np.uint16))


def nce_case(ref, inp, tau, scale):
    t = {k: torch.from_numpy(v.astype(np.int64)) for k, v in inp.items() if v.dtype == np.uint16}
    vtx = (torch.from_numpy(inp["vtx"]) * np.float32(scale)).requires_grad_(True)
    pts = (torch.from_numpy(inp["pts"]) * np.float32(scale)).requires_grad_(True)
    loss = ref.infoNCE(vtx, pts, t["corr_v2p"], t["corr_p2v"], t["vtx_batch"], t["pts_batch"], t["corr_v2p_batch"], t["corr_p2v_batch"], tau)
    loss.backward()
    want = lo.infonce(vtx.detach().double(), pts.detach().double(), t["corr_v2p"], t["corr_p2v"], t["vtx_batch"], t["pts_batch"],
                      t["corr_v2p_batch"], t["corr_p2v_batch"], tau, len(NCE_PAIRS))
    dev = dict(dev_loss=rel(loss, want[0]), dev_grad_vtx=rel_max(vtx.grad.numpy(), want[1].numpy()),
               dev_grad_pts=rel_max(pts.grad.numpy(), want[2].numpy()))
    return dict(loss=np.float32(loss.item()), grad_vtx=vtx.grad.numpy(), grad_pts=pts.grad.numpy()), dev


# ------------------------------------------------------------------------------------------------------------------- multi-positive
def multipos_inputs(rng):
    sizes, bones = [512, 700], 6
    n = sum(sizes)
    feat = (unit_rows(rng, n, 32) * np.float32(1.5)).astype(np.float32)
    primary = rng.integers(0, 4, n)
    skin = np.zeros((n, bones), dtype=np.float32)
    skin[np.arange(n), primary] = 1.0
    blend = rng.random(n) < 0.3                                            # 0.7 / 0.3 blends: gt_sim 0.7 against the plain rows
    skin[blend] *= np.float32(0.7)
    skin[np.nonzero(blend)[0], (primary[blend] + 1) % 4] = np.float32(0.3)
    skin[5] = 0.0
    skin[5, 4] = skin[5, 5] = 0.5                                          # the vertex no other shares its row with (mesh 0 samples every vertex)
    return feat, skin, np.repeat(np.arange(2), sizes)


def multipos_case(ref, feat, skin, batch):
    draws = dict(choice=[], multinomial=[])
    real_choice, real_multinomial = np.random.choice, torch.multinomial

    def choice(*a, **kw):
        r = real_choice(*a, **kw)
        draws["choice"].append(np.asarray(r).copy())
        return r

    def multinomial(*a, **kw):
        r = real_multinomial(*a, **kw)
        draws["multinomial"].append(r.numpy().copy())
        return r
    f = torch.from_numpy(feat).requires_grad_(True)
    np.random.seed(7)
    torch.manual_seed(7)
    np.random.choice, torch.multinomial = choice, multinomial
    try:
        loss = ref.multi_pos_infoNCE(f, torch.from_numpy(skin), torch.from_numpy(batch))
    finally:
        np.random.choice, torch.multinomial = real_choice, real_multinomial
    loss.backward()
    sample_ids = np.stack(draws["choice"])
    pos_ids, neg_ids = np.stack(draws["multinomial"][0::2]), np.stack(draws["multinomial"][1::2])
    for b in range(2):                                                     # the fixture conditions
        assert (batch == b).sum() >= N_SAMPLE
        sim = lo.gt_similarity(torch.from_numpy(skin[batch == b][sample_ids[b]]).double())
        assert float((sim - 0.9).abs().min()) >= SIM_MARGIN, "a gt_sim too close to 0.9"
        assert bool(((sim <= 0.9).sum(1) > 0).all()), "a sample row without a negative"
    own = int(np.nonzero(sample_ids[0] == 5)[0][0])
    assert (pos_ids[0, own] == own).all(), "the lone vertex must have itself as its only positive"
    tl = lambda a: torch.from_numpy(a.astype(np.int64))
    want = lo.multipos(f.detach().double(), tl(batch), tl(sample_ids), tl(pos_ids), tl(neg_ids), 2)
    dev = dict(dev_loss=rel(loss, want[0]), dev_grad=rel_max(f.grad.numpy(), want[1].numpy()))
    return dict(sample_ids=sample_ids.astype(np.uint16), pos_ids=pos_ids.astype(np.uint16), neg_ids=neg_ids.astype(np.uint16),
                loss=np.float32(loss.item()), grad=f.grad.numpy()), dev


# ------------------------------------------------------------------------------------------------------------------- chamfer
def chamfer_case(ref, p, q):
    assert lo.chamfer_margin(torch.from_numpy(p).double(), torch.from_numpy(q).double()) >= CHAMFER_MARGIN, "a chamfer minimum too close to its runner-up"
    tp, tq = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(q).requires_grad_(True)
    loss = ref.chamfer_distance_with_average(tp.unsqueeze(0), tq.unsqueeze(0))
    loss.backward()
    assert np.isfinite(tp.grad.numpy()).all() and np.isfinite(tq.grad.numpy()).all() and np.isfinite(loss.item())
    z = torch.zeros
    want = lo.chamfer(tp.detach().double(), z(len(p), dtype=torch.long), tq.detach().double(), z(len(q), dtype=torch.long), 1)
    dev = dict(dev_loss=rel(loss, want[0]), dev_grad_p=rel_max(tp.grad.numpy(), want[1].numpy()), dev_grad_q=rel_max(tq.grad.numpy(), want[2].numpy()))
    return dict(loss=np.float32(loss.item()), grad_p=tp.grad.numpy(), grad_q=tq.grad.numpy()), dev


def main():
    ref = reference()
    rng = np.random.default_rng(20240917)
    print("infoNCE")
    inp = nce_inputs(rng)
    save("loss_nce_inputs", dict(pairs=NCE_PAIRS, cases=NCE_CASES), **inp)
    for name, par in NCE_CASES.items():
        res, dev = nce_case(ref, inp, par["tau"], par["scale"])
        print(f"  {name}: loss {res['loss']:.6f}  deviations {dev}")
        save(f"loss_nce_{name}", dict(par, deviations=dev), **res)
    print("multi-positive infoNCE")
    feat, skin, batch = multipos_inputs(rng)
    res, dev = multipos_case(ref, feat, skin, batch)
    print(f"  loss {res['loss']:.6f}  deviations {dev}")
    save("loss_multipos", dict(deviations=dev, lone_vertex=5, n_sample=N_SAMPLE), feat=feat, skin=skin, batch=batch.astype(np.uint16), **res)
    print("chamfer")
    arrs, devs, names = {}, {}, []
    for n, m in CHAMFER_SHAPES:
        name = f"n{n}_m{m}"
        p, q = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (m, 3)).astype(np.float32)
        res, devs[name] = chamfer_case(ref, p, q)
        names.append(name)
        arrs.update({f"{name}_p": p, f"{name}_q": q, **{f"{name}_{k}": v for k, v in res.items()}})
        print(f"  {name}: loss {res['loss']:.6f}  deviations {devs[name]}")
    p, q = rng.uniform(-0.5, 0.5, (40, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (5, 3)).astype(np.float32)
    q[2] = p[7]
    res, devs["coincide"] = chamfer_case(ref, p, q)
    arrs.update({"coincide_p": p, "coincide_q": q, **{f"coincide_{k}": v for k, v in res.items()}})
    print(f"  coincide: loss {res['loss']:.6f}  deviations {devs['coincide']}")
    save("loss_chamfer", dict(batch=names, deviations=devs, coincide=dict(vertex=7, joint=2)), **arrs)


if __name__ == "__main__":
    main()
