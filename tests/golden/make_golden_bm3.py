"""Generate the golden vectors of BM3 by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_bm3.py

Same rules as make_golden_selfcf.py, whose helpers are reused: a fresh process, only data is written.  The tiny set gets
seeded synthetic features of our own (not reference data), written beside its text files as ``tiny.img.npz`` [96, 100] and
``tiny.txt.npz`` [96, 37] -- odd widths on purpose.

Recorded: every parameter before and after (the initial feature tables are the features themselves), the normalised
adjacency (asserted to be row-major with ascending columns, stored in R order and in R^T order), per training step the
batch (a recording wrapper around ``InteractionIterator``), the four full-table target masks (``F.dropout`` is wrapped: user,
item, text, image, in that order) and the loss; per evaluation the report and the dense ``predict(test_users)`` matrix; the
best report.  Flags are packed with ``np.packbits``.

The run is then replayed in float64 (tests/bm3_twin.py).  ``f64_dev_params`` / ``f64_dev_scores`` / ``f64_dev_loss`` are the
largest differences between that replay and the reference: the reference's own fp32 noise, from which the tests derive their
tolerances.  No fixture is written when the replay differs by more than 1e-5 anywhere, or when an evaluation has more than 3
users with a top-22 gap <= 5e-6.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
from make_golden_selfcf import _write_tiny_files  # noqa: E402

CONFIG = dict(lr=1e-2, reg=0.1, embed_dim=64, n_layers=2, dropout=0.3, cl_weight=2.0, batch_size=256, epochs=3)
FEATURE_SEED, IMG_SHAPE, TXT_SHAPE = 20260302, (96, 100), (96, 37)


def _write_features():
    rng = np.random.default_rng(FEATURE_SEED)
    img = rng.standard_normal(IMG_SHAPE).astype(np.float32)
    txt = rng.standard_normal(TXT_SHAPE).astype(np.float32)
    np.savez(os.path.join(G.DATA_DIR, "tiny.img.npz"), features=img)
    np.savez(os.path.join(G.DATA_DIR, "tiny.txt.npz"), features=txt)
    return img, txt


def _shims():
    """what the reference's BM3 needs on this image beyond ref_harness.install(): the legacy sparse constructor
    ``torch.sparse.FloatTensor(indices, values, size)`` (BM3.py:140), where this torch no longer takes it"""
    import torch
    try:
        torch.sparse.FloatTensor(torch.zeros((2, 1), dtype=torch.long), torch.ones(1), torch.Size((2, 2)))
    except Exception:  # noqa: BLE001
        torch.sparse.FloatTensor = lambda i, v, size: torch.sparse_coo_tensor(i, v, size, dtype=torch.float32)


def make_bm3():
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        _write_tiny_files()
    img, txt = _write_features()
    import bm3_twin as T
    G._install()
    import torch
    torch.set_num_threads(1)
    _shims()
    import skrec.recommender.BM3 as M
    G._seed_all()
    batches, masks, loss_rec, pred_rec = [], [], [], []
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
    model = M.BM3(G._run_config(recommender="BM3"), dict(CONFIG))
    net = model.model
    nu, ni, d = model.num_users, model.num_items, CONFIG["embed_dim"]
    names = T.param_names(True, True)
    assert [n for n, _ in net.named_parameters()] == list(names)
    params = dict(net.named_parameters())
    out = {T._key(k, 0): params[k].detach().numpy().copy() for k in names}
    assert np.array_equal(out[T._key("image_embedding.weight", 0)], img) and np.array_equal(out[T._key("text_embedding.weight", 0)], txt)
    # the square adjacency as the reference holds it: row-major with ascending columns
    adj = net.norm_adj
    idx, val = adj._indices().numpy(), adj._values().numpy()
    key = idx[0].astype(np.int64) * (nu + ni) + idx[1]
    assert (np.diff(key) > 0).all(), "norm_adj is not row-major with ascending columns"
    top = idx[0] < nu
    n_top = int(top.sum())
    assert top[:n_top].all() and 2 * n_top == len(val) and (idx[1][:n_top] >= nu).all() and (idx[1][n_top:] < nu).all()
    orig_dropout = M.F.dropout

    def rec_dropout(x, *a, **k):
        o = orig_dropout(x, *a, **k)
        masks.append((o != 0).numpy().astype(np.uint8))
        return o
    M.F.dropout = rec_dropout
    orig_loss = net.calculate_loss

    def calculate_loss(users, items):
        r = orig_loss(users, items)
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
    try:
        best = model.fit()
    finally:
        M.F.dropout = orig_dropout
    for k in names:
        out[T._key(k, 1)] = params[k].detach().numpy().copy()
    n_steps = len(batches)
    assert n_steps == len(loss_rec) == 9 and len(masks) == 36 and len(pred_rec) == 3
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    for s in range(n_steps):        # drawn in the order user, item, text, image
        assert [m.shape for m in masks[4 * s:4 * s + 4]] == [(nu, d), (ni, d), (ni, d), (ni, d)]
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(idx[0][:n_top], minlength=nu))
    items = (idx[1][:n_top] - nu).astype(np.int32)
    rows = T.csr_rows(rowptr)
    order = np.lexsort((rows, items))
    assert np.array_equal(idx[0][n_top:] - nu, items[order]) and np.array_equal(idx[1][n_top:], rows[order])
    assert np.array_equal(val[n_top:], val[:n_top][order])
    steps = [dict(users=b[0], items=b[1], ku=masks[4 * s][b[0]], ki=masks[4 * s + 1][b[1]], kt=masks[4 * s + 2][b[1]],
                  kv=masks[4 * s + 3][b[1]]) for s, b in enumerate(batches)]
    init = {k: out[T._key(k, 0)] for k in names}
    P64, l64, s64 = T.replay_f64((rowptr, items, ni), val[:n_top], init, steps, CONFIG, 3, test_users)
    dev_p = [float(np.abs(P64[k] - out[T._key(k, 1)]).max()) for k in names]
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
    out.update(adj_rows=rows.astype(np.int32), adj_cols=items, adj_val=val[:n_top].astype(np.float32),
               adj_t_rows=items[order].astype(np.int32), adj_t_cols=rows[order].astype(np.int32), adj_t_val=val[n_top:].astype(np.float32),
               step_users=np.concatenate([b[0] for b in batches]), step_items=np.concatenate([b[1] for b in batches]),
               step_sizes=np.int32([len(b[0]) for b in batches]),
               loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s), f64_dev_loss=np.float64(dev_l),
               close_users=np.int32(close))
    for j, k in enumerate("uitv"):
        out[f"step_mask_{k}"] = np.stack([np.packbits(masks[4 * s + j].reshape(-1)) for s in range(n_steps)])
    print("bm3: steps", n_steps, "loss", loss_rec[0], loss_rec[-1], "NDCG@10",
          [dict(zip(model.evaluator.metrics_list, r))["NDCG@10"] for r in reports])
    np.savez_compressed(os.path.join(HERE, "golden_bm3.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_bm3()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
