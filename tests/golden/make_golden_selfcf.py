"""Generate the golden vectors of SelfCF by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_selfcf.py

Same rules as make_golden.py, whose helpers are reused: a fresh process, only data is written.  The tiny set's two text files
are written from tests/golden/tiny_dataset.npz when they are missing (the committed .npz is not touched).

Recorded: the four parameters before and after, the normalised adjacency (asserted to be row-major with ascending columns,
then stored in R order and in R^T order), per training step the batch (a recording wrapper around ``InteractionIterator``),
the dropout rate and the edge mask (``sparse_dropout`` is wrapped: the mask is recomputed from the recorded ``torch.rand`` by
the reference's own expression, checked against the number of entries it keeps, and split by (row, col) into k1 -- the user
rows, R order -- and k2 -- the item rows, R^T order), the two target masks (``F.dropout`` is wrapped inside the module: the user
side is drawn first) and the loss; per evaluation the report and the dense ``predict(test_users)`` matrix; the best report.
Flags are packed with ``np.packbits``.

The run is then replayed in float64 (tests/selfcf_twin.py: torch autograd on the dense masked blocks, ``Adam``).
``f64_dev_params`` / ``f64_dev_scores`` / ``f64_dev_loss`` are the largest differences between that replay and the reference:
the reference's own fp32 noise, from which the tests derive their tolerances.  No fixture is written when the replay differs
by more than 1e-5 anywhere (a replay that has left the reference's trajectory), or when an evaluation has more than 3 users
with a top-22 gap <= 5e-6.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402

CONFIG = dict(lr=1e-2, reg=1e-3, embed_dim=64, n_layers=2, dropout=0.5, batch_size=256, epochs=3)


def _write_tiny_files():
    d = np.load(os.path.join(HERE, "tiny_dataset.npz"))
    os.makedirs(G.DATA_DIR, exist_ok=True)
    for name in ("train", "test"):
        with open(os.path.join(G.DATA_DIR, "tiny." + name), "w") as f:
            for u, i, ts in d[name]:
                f.write(f"{int(u)}\t{int(i)}\t1.0\t{int(ts)}\n")


def make_selfcf():
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        _write_tiny_files()
    import selfcf_twin as T
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.SelfCF as M
    G._seed_all()
    batches, rates, rands, nkept, tkeeps, loss_rec, pred_rec = [], [], [], [], [], [], []
    orig_iter = M.InteractionIterator

    class RecordingIterator(object):
        def __init__(self, *a, **k):
            self.it = orig_iter(*a, **k)

        def __len__(self):
            return len(self.it)

        def __iter__(self):
            for u, i in self.it:
                batches.append(tuple(np.asarray(c, np.int32).copy() for c in (u, i)))
                yield u, i
    M.InteractionIterator = RecordingIterator
    model = M.SelfCF(G._run_config(recommender="SelfCF"), dict(CONFIG))
    net = model.model
    enc = net.online_encoder
    nu, ni = model.num_users, model.num_items

    def params():
        return {"user_emb": enc.embedding_dict["user_emb"], "item_emb": enc.embedding_dict["item_emb"],
                "predictor.weight": net.predictor.weight, "predictor.bias": net.predictor.bias}
    out = {k.replace(".", "_") + "_0": v.detach().numpy().copy() for k, v in params().items()}
    # the square adjacency as the reference holds it: not coalesced, row-major with ascending columns
    adj = enc.sparse_norm_adj
    idx, val = adj._indices().numpy(), adj._values().numpy()
    key = idx[0].astype(np.int64) * (nu + ni) + idx[1]
    assert (np.diff(key) > 0).all(), "sparse_norm_adj is not row-major with ascending columns"
    top = idx[0] < nu
    n_top = int(top.sum())
    assert top[:n_top].all() and 2 * n_top == len(val) and (idx[1][:n_top] >= nu).all() and (idx[1][n_top:] < nu).all()

    orig_sd = enc.sparse_dropout

    def sparse_dropout(x, rate, noise_shape):
        orig_rand = torch.rand

        def rec_rand(*a, **k):
            r = orig_rand(*a, **k)
            rands.append(r.clone())
            return r
        torch.rand = rec_rand
        try:
            o = orig_sd(x, rate, noise_shape)
        finally:
            torch.rand = orig_rand
        rates.append(float(rate))
        nkept.append(int(o._nnz()))
        return o
    enc.sparse_dropout = sparse_dropout
    orig_dropout = M.F.dropout

    def rec_dropout(x, *a, **k):
        o = orig_dropout(x, *a, **k)
        tkeeps.append((o != 0).numpy().astype(np.uint8))
        return o
    M.F.dropout = rec_dropout
    orig_loss = net.calculate_loss

    def calculate_loss(users, pos_items):
        r = orig_loss(users, pos_items)
        loss_rec.append(float(r.detach()))
        return r
    net.calculate_loss = calculate_loss
    test_users = list(model.evaluator.user_pos_test.keys())
    orig_eval = model.evaluate

    def evaluate(tu=None):
        r = orig_eval(tu)
        pred_rec.append(model.predict(test_users).astype(np.float32))
        return r
    model.evaluate = evaluate
    reports = G._record_reports(model)
    best = model.fit()
    M.F.dropout = orig_dropout
    for k, v in params().items():
        out[k.replace(".", "_") + "_1"] = v.detach().numpy().copy()
    n_steps = len(batches)
    assert n_steps == len(loss_rec) == len(rates) == len(rands) == 9 and len(tkeeps) == 18 and len(pred_rec) == 3
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    # the edge masks by the reference's own expression (SelfCF.py:134-136), split into the two halves
    k1s, k2s = [], []
    for rate, r, nk in zip(rates, rands, nkept):
        random_tensor = 1 - rate
        random_tensor += r
        mask = torch.floor(random_tensor).type(torch.bool).numpy()
        assert int(mask.sum()) == nk
        k1s.append(mask[:n_top].astype(np.uint8))
        k2s.append(mask[n_top:].astype(np.uint8))
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(idx[0][:n_top], minlength=nu))
    items = (idx[1][:n_top] - nu).astype(np.int32)
    order, _ = T.transpose_order(rowptr, items)
    # the item rows of the square matrix ARE the transpose's order: by item, then by user
    assert np.array_equal(idx[0][n_top:] - nu, items[order]) and np.array_equal(idx[1][n_top:], T.csr_rows(rowptr)[order])
    assert np.array_equal(val[n_top:], val[:n_top][order])
    steps = [dict(users=b[0], items=b[1], rate=rates[s], k1=k1s[s], k2=k2s[s], ku=tkeeps[2 * s], ki=tkeeps[2 * s + 1])
             for s, b in enumerate(batches)]
    init = {k: out[k.replace(".", "_") + "_0"] for k in T.PARAMS}
    P64, l64, s64 = T.replay_f64((rowptr, items, ni), val[:n_top], init, steps, CONFIG, 3, test_users)
    dev_p = [float(np.abs(P64[k] - out[k.replace(".", "_") + "_1"]).max()) for k in T.PARAMS]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, pred_rec)]
    dev_l = float(np.abs(l64 / np.float64(loss_rec) - 1).max())
    print("f64_dev params", dev_p, "scores", dev_s, "loss (relative)", dev_l)
    if max(dev_p + dev_s + [dev_l]) > 1e-5:
        raise SystemExit("the float64 replay has left the reference's trajectory: fixture NOT written")
    ev = model.evaluator
    close = []
    for sc in pred_rec:
        c = 0
        for r, u in enumerate(test_users):
            row = sc[r].astype(np.float64).copy()
            row[np.asarray(ev.user_pos_train.get(u, []), dtype=np.int64)] = -np.inf
            t = np.sort(row)[::-1][:22]
            c += int(np.min(t[:-1] - t[1:]) <= 5e-6)
        close.append(c)
    print("users with a top-22 gap <= 5e-6 per evaluation:", close)
    if max(close) > 3:
        raise SystemExit(f"{max(close)} near-tie users in one evaluation: fixture NOT written")
    out.update(adj_rows=T.csr_rows(rowptr).astype(np.int32), adj_cols=items, adj_val=val[:n_top].astype(np.float32),
               adj_t_rows=items[order].astype(np.int32), adj_t_cols=T.csr_rows(rowptr)[order].astype(np.int32),
               adj_t_val=val[n_top:].astype(np.float32),
               step_users=np.concatenate([b[0] for b in batches]), step_items=np.concatenate([b[1] for b in batches]),
               step_sizes=np.int32([len(b[0]) for b in batches]), step_rate=np.float64(rates),
               step_k1=np.stack([np.packbits(k) for k in k1s]), step_k2=np.stack([np.packbits(k) for k in k2s]),
               step_ku=np.packbits(np.concatenate([tkeeps[2 * s].reshape(-1) for s in range(n_steps)])),
               step_ki=np.packbits(np.concatenate([tkeeps[2 * s + 1].reshape(-1) for s in range(n_steps)])),
               loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s), f64_dev_loss=np.float64(dev_l),
               close_users=np.int32(close))
    print("selfcf: steps", n_steps, "rates", np.round(rates, 3), "loss", loss_rec[0], loss_rec[-1], "NDCG@10",
          [dict(zip(model.evaluator.metrics_list, r))["NDCG@10"] for r in reports])
    np.savez_compressed(os.path.join(HERE, "golden_selfcf.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_selfcf()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
