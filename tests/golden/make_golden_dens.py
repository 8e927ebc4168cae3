"""Generate the golden vectors of DENS by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_dens.py

Same rules as make_golden.py, whose helpers are reused: a fresh process, only data is written.  One cosmetic shim is kept
here: ``torch.sparse.FloatTensor`` where the installed torch no longer has the legacy constructor (DENS.py:194 builds the
adjacency with it) -- it is ``torch.sparse_coo_tensor`` with float32 values.

Recorded: the six parameters before and after, per training step the batch and its candidates (a recording wrapper around
``PairwiseIterator``), the loss, the reference's chosen candidate per (row, hop) -- the index whose row the reference's
``dise_negative_sampling`` returned -- and that group's RELATIVE MARGIN, computed in float64 from the reference's own hop
tables and gates: the best score minus the best score of a DIFFERENT item, over the group's largest sum of |terms| (duplicate
candidates tie exactly and select the same row); per evaluation the report and the dense ``predict(test_users)`` matrix; the
best report.

The run is then replayed in float64 (tests/dens_twin.py: torch autograd, ``Adam``) with the recorded choices.
``f64_dev_params`` / ``f64_dev_scores`` / ``f64_dev_loss`` are the largest differences between that replay and the reference:
the reference's own fp32 noise, from which the tests derive their tolerances.  No fixture is written when more than 0.5 % of the
(row, hop) groups have a margin under 2^-12, or when an evaluation has more than 3 users whose 22 best scores hold a pair
closer than the near-tie gap, 12 x the largest ``f64_dev_scores`` (twice the deviation the tests allow a score).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

CONFIG = dict(lr=1e-2, l2=1e-4, gamma=0.3, dim=64, batch_size=256, context_hops=2, K=1, n_negs=6, warmup=4, epochs=3)
MARGIN = 2.0 ** -12
MARGIN_CAP = 0.005


def make_dens():
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        G.make_dataset()
    G._install()
    sys.path.insert(0, os.path.dirname(HERE))
    import dens_twin as T
    import torch
    torch.set_num_threads(1)
    try:
        torch.sparse.FloatTensor(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0), (1, 1))
    except Exception:
        torch.sparse.FloatTensor = lambda i, v, shape: torch.sparse_coo_tensor(i, v.float(), tuple(shape))
    import skrec.recommender.DENS as M
    G._seed_all()
    batches, loss_rec, pred_rec, choice_rec, margin_rec, item_rec, second_rec = [], [], [], [], [], [], []
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
    model = M.DENS(G._run_config(recommender="DENS"), dict(CONFIG))
    net = model.model
    names = T.NAMES
    params = dict(net.named_parameters())
    assert set(names) == set(params)
    out = {"init." + k: params[k].detach().numpy().copy() for k in names}
    nu, ni = model.num_users, model.num_items
    adj = net.sparse_norm_adj.coalesce()
    idx, val = adj.indices().numpy(), adj.values().numpy()
    A = np.zeros((nu + ni, nu + ni), np.float64)
    A[idx[0], idx[1]] = val
    orig_sel = net.dise_negative_sampling

    def dise(cur_epoch, user_gcn_emb, item_gcn_emb, user, neg_candidates, pos_item):
        ret = orig_sel(cur_epoch, user_gcn_emb, item_gcn_emb, user, neg_candidates, pos_item)
        with torch.no_grad():
            n_e = item_gcn_emb[neg_candidates]                          # [B, K, H+1, d]
            match = (n_e == ret.unsqueeze(1)).all(-1)                   # [B, K, H+1]
            assert bool(match.any(1).all())
            choice = match.float().argmax(1).numpy()                    # the first candidate holding the returned row
            P64 = {k: v.detach().double() for k, v in net.named_parameters()}
            w = 1 - min(1, cur_epoch / net.warmup)
            _, _, _, scores, scale, _ = T.gates_and_scores(P64, user_gcn_emb[user].double(), item_gcn_emb[pos_item].double(),
                                                           n_e.double(), w)
            cand = neg_candidates.numpy()
            m, best_item, second = T.margins(scores.numpy(), scale.numpy(), cand)
            item = np.take_along_axis(cand, choice, 1)                  # [B, H+1]
            # the reference's fp32 choice against the float64 ranking: the best item, or the runner-up inside the margin
            agree = item == best_item
            assert ((agree) | ((m < MARGIN) & (item == second))).all(), "the reference's choice is neither of the float64 top two"
            choice_rec.append(choice.astype(np.int32))
            item_rec.append(item.astype(np.int32))
            margin_rec.append(m)
            second_rec.append(np.where(agree, second, best_item).astype(np.int32))   # the other admissible item of a near tie
        return ret
    net.dise_negative_sampling = dise
    orig_fwd = net.forward

    def forward(cur_epoch, batch=None):
        r = orig_fwd(cur_epoch, batch)
        loss_rec.append([float(x.detach()) for x in (r[1], r[2], r[0])])
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
    final = {k: v.detach().numpy().copy() for k, v in net.named_parameters()}
    out.update({"final." + k: final[k] for k in names})
    assert len(batches) == len(loss_rec) == len(choice_rec) == 9 and len(pred_rec) == 3
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    margin = np.concatenate(margin_rec)
    under = int((margin < MARGIN).sum())
    print("groups", margin.size, "under 2^-12:", under, f"({100.0 * under / margin.size:.2f} %)", "smallest margin", margin.min())
    if under > MARGIN_CAP * margin.size:
        raise SystemExit(f"{under} of {margin.size} groups have a margin under 2^-12: fixture NOT written")
    # float64 replay with the recorded choices
    init = {k: out["init." + k] for k in names}
    p64, l64, s64 = T.replay_f64(A, init, batches, CONFIG, choice_rec, 3, test_users)
    dev_p = [float(np.abs(p64[k] - final[k]).max()) for k in names]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, pred_rec)]
    dev_l = float(np.abs(l64 / np.float64([l[2] for l in loss_rec]) - 1).max())
    print("f64_dev params", dict(zip(names, dev_p)), "scores", dev_s, "loss (relative)", dev_l)
    if dev_l > 1e-5:             # the tests compare losses at rtol 1e-5: a replay further off than that explains nothing
        raise SystemExit(f"float64 replay differs from the reference by {dev_l:.3g} in the losses: fixture NOT written")
    # users whose 22 best scores hold a pair closer than the near-tie gap (rankings of the tests leave them out).  The tests
    # allow a score to differ from the reference's by 6 x f64_dev_scores, so two scores further apart than twice that keep
    # their order: gap = 12 x the largest f64_dev_scores (LightGCL's 5e-6 is the same rule at that model's score scale)
    gap = 12.0 * max(dev_s)
    ev = model.evaluator
    close = []
    for sc in pred_rec:
        c = 0
        for r, u in enumerate(test_users):
            row = sc[r].astype(np.float64).copy()
            row[np.asarray(ev.user_pos_train.get(u, []), dtype=np.int64)] = -np.inf
            top = np.sort(row)[::-1][:22]
            c += int(np.min(top[:-1] - top[1:]) <= gap)
        close.append(c)
    print(f"users with a top-22 gap <= {gap:.3g} per evaluation:", close)
    if max(close) > 3:
        raise SystemExit(f"{max(close)} near-tie users in one evaluation: fixture NOT written")
    order = np.lexsort((idx[1], idx[0]))
    out.update(adj_rows=idx[0][order].astype(np.int32), adj_cols=idx[1][order].astype(np.int32), adj_val=val[order].astype(np.float32),
               step_users=np.concatenate([b[0] for b in batches]), step_pos=np.concatenate([b[1] for b in batches]),
               step_cand=np.concatenate([b[2] for b in batches]), step_sizes=np.int32([len(b[0]) for b in batches]),
               step_choice=np.concatenate(choice_rec), step_item=np.concatenate(item_rec), step_second=np.concatenate(second_rec),
               step_margin=margin, loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               param_names=np.array(names), f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s),
               f64_dev_loss=np.float64(dev_l), close_users=np.int32(close), near_tie_gap=np.float64(gap), groups_under_margin=np.int32(under))
    print("dens: steps", len(batches), "loss", loss_rec[0], loss_rec[-1], "NDCG@10", dict(best.items())["NDCG@10"],
          "max |score|", float(np.abs(pred_rec[-1]).max()))
    np.savez_compressed(os.path.join(HERE, "golden_dens.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_dens()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
