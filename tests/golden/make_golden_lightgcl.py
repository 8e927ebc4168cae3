"""Generate the golden vectors of LightGCL by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_lightgcl.py

Same rules as make_golden.py, whose helpers are reused: a fresh process, only data is written.  One more cosmetic shim is
needed, kept here: ``torch.Tensor.cuda = identity`` -- the reference calls ``.cuda(device)`` even on a CPU device
(LightGCL.py:196,200).

Recorded: E_u_0 and E_i_0 before and after, the four SVD factors (an SVD is only defined up to signs and its algorithm: the
tests inject these), the normalised adjacency's CSR values, per training step the batch (a recording wrapper around
``PairwiseIterator``) and the loss, per evaluation the report and the dense ``predict(test_users)`` matrix, the best report.

The run is then replayed in float64 (torch autograd, ``Adam(weight_decay = 2 * lambda2)``) in the FOLDED formulation the
kernels use -- G_u = E_u_0 + u_mul_s (vt S_i), S the sum of the layers below the last -- ranking every evaluation with the
sums of the last training forward, as the reference does (LightGCL.py:110).  ``f64_dev_params`` / ``f64_dev_scores`` are the
largest differences between that replay and the reference: the reference's own fp32 noise, from which the tests derive their
tolerances.  No fixture is written when the replay differs by more than ten times the first trial's figures (F64_TRIAL), when
an evaluation has more than 3 users with a top-22 gap <= 5e-6, or when a positive score lies within 1e-4 of a clamp bound.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

CONFIG = dict(lr=1e-2, lambda1=0.2, d=64, gnn_layer=2, batch_size=256, svd_q=5, dropout=0.0, temp=0.2, lambda2=1e-4, epochs=3)
# the first trial's replay differences: losses (relative), E_u_0, E_i_0, the scores of the three evaluations
F64_TRIAL = dict(loss=3.0e-7, E_u_0=2.0e-7, E_i_0=4.2e-7, scores=(2.4e-7, 2.1e-7, 2.7e-7))


def replay_f64(A, factors, init, steps, cfg, eval_every, test_users):
    """the run in float64, folded -> (E_u_0, E_i_0, losses, scores per evaluation, smallest distance of a positive score to
    a clamp bound)"""
    import torch
    t = lambda a, g=False: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=g)    # noqa: E731
    A = t(A)
    u_mul_s, v_mul_s, ut, vt = (t(f) for f in factors)
    Eu0, Ei0 = t(init[0], True), t(init[1], True)
    opt = torch.optim.Adam([Eu0, Ei0], lr=cfg["lr"], weight_decay=2 * cfg["lambda2"])
    L, temp, lam1 = cfg["gnn_layer"], cfg["temp"], cfg["lambda1"]
    losses, scores, clamp_dist = [], [], np.inf
    for s, (uids, pos, neg) in enumerate(steps):
        uids, pos, neg = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (uids, pos, neg))
        iids = torch.cat([pos, neg])
        xu, xi, Su, Si = Eu0, Ei0, 0, 0
        Eu, Ei = Eu0, Ei0
        for _ in range(L):
            Su, Si = Su + xu, Si + xi
            xu, xi = A @ xi, A.T @ xu
            Eu, Ei = Eu + xu, Ei + xi
        Gu, Gi = Eu0[uids] + u_mul_s[uids] @ (vt @ Si), Ei0[iids] + v_mul_s[iids] @ (ut @ Su)
        neg_score = torch.log(torch.exp(Gu @ Eu.T / temp).sum(1) + 1e-8).mean() \
            + torch.log(torch.exp(Gi @ Ei.T / temp).sum(1) + 1e-8).mean()
        ps_u, ps_i = (Gu * Eu[uids]).sum(1) / temp, (Gi * Ei[iids]).sum(1) / temp
        pos_score = torch.clamp(ps_u, -5.0, 5.0).mean() + torch.clamp(ps_i, -5.0, 5.0).mean()
        x = (Eu[uids] * Ei[pos]).sum(-1) - (Eu[uids] * Ei[neg]).sum(-1)
        loss = -torch.nn.functional.logsigmoid(x).mean() + lam1 * (neg_score - pos_score)
        with torch.no_grad():
            ps = torch.cat([ps_u, ps_i]).abs()
            clamp_dist = min(clamp_dist, float((ps - 5.0).abs().min()))
            reg = cfg["lambda2"] * ((Eu0 ** 2).sum() + (Ei0 ** 2).sum())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item() + reg.item())
        if (s + 1) % eval_every == 0:
            scores.append((Eu.detach()[np.asarray(test_users)] @ Ei.detach().T).numpy())
    return Eu0.detach().numpy(), Ei0.detach().numpy(), np.array(losses), scores, clamp_dist


def make_lightgcl():
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        G.make_dataset()
    G._install()
    import torch
    torch.set_num_threads(1)
    torch.Tensor.cuda = lambda self, *a, **k: self            # the reference calls .cuda(device) on a CPU device
    import skrec.recommender.LightGCL as M
    G._seed_all()
    batches, loss_rec, pred_rec = [], [], []
    orig_iter = M.PairwiseIterator

    class RecordingIterator(object):
        def __init__(self, *a, **k):
            self.it = orig_iter(*a, **k)

        def __len__(self):
            return len(self.it)

        def __iter__(self):
            for u, i, j in self.it:
                batches.append(tuple(np.asarray(c, np.int32).copy() for c in (u, i, j)))
                yield u, i, j
    M.PairwiseIterator = RecordingIterator
    model = M.LightGCL(G._run_config(recommender="LightGCL"), dict(CONFIG))
    net = model.model
    out = {"E_u_00": net.E_u_0.detach().numpy().copy(), "E_i_00": net.E_i_0.detach().numpy().copy()}
    factors = tuple(f.detach().numpy().copy() for f in (net.u_mul_s, net.v_mul_s, net.ut, net.vt))
    adj = net.adj_norm.coalesce()
    idx, val = adj.indices().numpy(), adj.values().numpy()
    nu, ni = model.num_users, model.num_items
    A = np.zeros((nu, ni), np.float64)
    A[idx[0], idx[1]] = val
    orig_fwd = net.forward

    def forward(uids, iids, pos, neg, test=False):
        r = orig_fwd(uids, iids, pos, neg, test=test)
        if not test:
            loss_rec.append(float(r.detach()))
        return r
    net.forward = forward
    test_users = list(model.evaluator.user_pos_test.keys())
    orig_eval = model.evaluate

    def evaluate(tu=None):
        r = orig_eval(tu)
        pred_rec.append(model.predict(test_users).astype(np.float32))
        return r
    model.evaluate = evaluate
    reports = G._record_reports(model)
    best = model.fit()
    out["E_u_01"], out["E_i_01"] = net.E_u_0.detach().numpy().copy(), net.E_i_0.detach().numpy().copy()
    assert len(batches) == len(loss_rec) == 9 and len(pred_rec) == 3
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    # float64 replay, folded
    eu, ei, l64, s64, clamp_dist = replay_f64(A, factors, (out["E_u_00"], out["E_i_00"]), batches, CONFIG, 3, test_users)
    dev_p = [float(np.abs(eu - out["E_u_01"]).max()), float(np.abs(ei - out["E_i_01"]).max())]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, pred_rec)]
    dev_l = float(np.abs(l64 / np.float64(loss_rec) - 1).max())
    print("f64_dev params", dev_p, "scores", dev_s, "loss (relative)", dev_l, "clamp distance", clamp_dist)
    if dev_l > 10 * F64_TRIAL["loss"]:
        raise SystemExit(f"float64 replay differs from the reference by {dev_l:.3g} in the losses: fixture NOT written")
    for k, v in zip(("E_u_0", "E_i_0"), dev_p):
        if v > 10 * F64_TRIAL[k]:
            raise SystemExit(f"float64 replay differs from the reference by {v:.3g} in {k}: fixture NOT written")
    for v, lim in zip(dev_s, F64_TRIAL["scores"]):
        if v > 10 * lim:
            raise SystemExit(f"float64 replay differs from the reference by {v:.3g} in the scores: fixture NOT written")
    if clamp_dist < 1e-4:
        raise SystemExit(f"a positive score lies {clamp_dist:.3g} from a clamp bound: fixture NOT written")
    # users whose 22 best scores hold a pair closer than 5e-6 (rankings of the tests leave them out)
    ev = model.evaluator
    close = []
    for sc in pred_rec:
        c = 0
        for r, u in enumerate(test_users):
            row = sc[r].astype(np.float64).copy()
            row[np.asarray(ev.user_pos_train.get(u, []), dtype=np.int64)] = -np.inf
            top = np.sort(row)[::-1][:22]
            c += int(np.min(top[:-1] - top[1:]) <= 5e-6)
        close.append(c)
    print("users with a top-22 gap <= 5e-6 per evaluation:", close)
    if max(close) > 3:
        raise SystemExit(f"{max(close)} near-tie users in one evaluation: fixture NOT written")
    order = np.lexsort((idx[1], idx[0]))
    out.update(u_mul_s=factors[0], v_mul_s=factors[1], ut=factors[2], vt=factors[3],
               adj_rows=idx[0][order].astype(np.int32), adj_cols=idx[1][order].astype(np.int32), adj_val=val[order].astype(np.float32),
               step_users=np.concatenate([b[0] for b in batches]), step_pos=np.concatenate([b[1] for b in batches]),
               step_neg=np.concatenate([b[2] for b in batches]), step_sizes=np.int32([len(b[0]) for b in batches]),
               loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s), f64_dev_loss=np.float64(dev_l),
               close_users=np.int32(close), clamp_distance=np.float64(clamp_dist))
    print("lightgcl: steps", len(batches), "loss", loss_rec[0], loss_rec[-1], "NDCG@10", dict(best.items())["NDCG@10"],
          "max |score|", float(np.abs(pred_rec[-1]).max()))
    np.savez_compressed(os.path.join(HERE, "golden_lightgcl.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_lightgcl()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
