"""Generate the golden vectors of MGCN by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_mgcn.py

Same rules as make_golden_bm3.py, whose helpers and seeded features (``tiny.img.npz`` [96, 100], ``tiny.txt.npz`` [96, 37]) are
reused: a fresh process, only data is written.  Two import-time shims beyond those: a ``torch_scatter`` placeholder whose
``scatter_add(src, index, dim, dim_size)`` is ``zeros(dim_size).index_add_(0, index, src)`` (MGCN.py:68-70; the package is not
installed here), and ``Tensor.cuda`` returning ``self`` (MGCN.py:162,173 call it unconditionally).  Neither touches the
numerical path.  ``reg``, ``cl_loss`` and ``lr_scheduler = [0.5, 1]`` are far from the reference's defaults on purpose, so that a
wrong or missing term cannot hide in three epochs: the generator ASSERTS that the float64 twin with the InfoNCE term, the
regulariser or the schedule switched off leaves the recorded final parameters by more than 100 times ``f64_dev_params``.

Recorded: every parameter before and after; ``norm_adj`` in R's CSR order; per modality the reference's top-k ids, similarities
and graph values; per step the batch (a recording wrapper around ``PairwiseIterator``) and the loss; per evaluation the report
and the dense ``predict(test_users)``; the best report; the config (json).  The reference's cache files of the item graphs
(``*mgcn_adj*.pt``) are deleted before and after.

The run is then replayed in float64 (tests/mgcn_twin.py): ``f64_dev_params`` / ``f64_dev_scores`` / ``f64_dev_loss`` /
``f64_dev_graph`` are the largest differences between that replay (resp. the twin's graph values) and the reference.

The fixture's conditions are FREEDOM's: no ``f64_dev_*`` above 1e-5; no evaluation with more than 3 of the test users whose
top-22 gap is <= 5e-6 (``close_ids``, padded with -1); all kept similarities' row sums positive; every row's k-th and (k+1)-th
similarity further apart than 1e-5, so that another exact kNN returns the reference's sets.  Nothing is written when one is
missed.  The seed is the first from 2021 upward whose run meets them, 2200: ``python tests/golden/make_golden_mgcn.py search``
repeats that search seed by seed; SEED_NOTE says what the earlier ones gave.
"""
import glob
import json
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
from make_golden_bm3 import _shims, _write_features  # noqa: E402
from make_golden_selfcf import _write_tiny_files  # noqa: E402

# What the 179 seeds before mgcn_twin.SEED = 2200 gave, each run by ``make_golden_mgcn.py run SEED``: 126 (2021 among them:
# f64_dev_params[item_id_embedding.weight] = 1.56e-5) ended with an f64_dev_params above 1e-5 -- one element of 40 k whose
# first gradient lies beside Adam's eps, as make_golden_freedom.py explains -- and the other 53 with 4 to 10 near-tie users in
# one evaluation: after nine steps the scores of this model are still products of xavier-sized rows, and a typical evaluation
# has 5 of 63 users with a top-22 gap <= 5e-6.  2200 gives f64_dev_params <= 5.6e-6 and [2, 3, 2] near-tie users.
SEED_NOTE = {"2021 .. 2199": "126 runs with f64_dev_params above 1e-5, 53 runs with more than 3 near-tie users in one evaluation"}
CONFIG = dict(lr=1e-2, reg=1e-2, cl_loss=0.1, n_ui_layers=2, n_layers=2, knn_k=10, lr_scheduler=[0.5, 1], batch_size=256, epochs=3)


def _drop_cache():
    for f in glob.glob(os.path.join(G.SCRATCH, "**", "*mgcn_adj*.pt"), recursive=True):
        os.remove(f)


def _mgcn_shims():
    import torch
    if "torch_scatter" not in sys.modules:
        m = types.ModuleType("torch_scatter")

        def scatter_add(src, index, dim=0, dim_size=None):
            assert dim == 0
            return torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, src)
        m.scatter_add = scatter_add
        sys.modules["torch_scatter"] = m
    torch.Tensor.cuda = lambda self, *a, **k: self


def make_mgcn(seed):
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        _write_tiny_files()
    img, txt = _write_features()
    import mgcn_twin as T
    G._install()
    import torch
    torch.set_num_threads(1)
    _shims()
    _mgcn_shims()
    import skrec.recommender.MGCN as M
    _drop_cache()
    G.SEED = seed
    G._seed_all()
    batches, loss_rec, pred_rec, knn_rec = [], [], [], []
    orig_iter = M.PairwiseIterator

    class RecordingIterator(object):
        def __init__(self, *a, **k):
            self.it = orig_iter(*a, **k)

        def __len__(self):
            return len(self.it)

        def __iter__(self):
            for u, p, q in self.it:
                batches.append(tuple(np.asarray(c, np.int32).copy() for c in (u, p, q)))
                yield u, p, q
    M.PairwiseIterator = RecordingIterator
    orig_knn = M.build_knn_normalized_graph

    def rec_knn(adj, topk, is_sparse, norm_type):
        val, ind = torch.topk(adj, topk + 1, dim=-1)
        knn_rec.append((ind.numpy().copy(), val.numpy().copy()))
        return orig_knn(adj, topk, is_sparse, norm_type)
    M.build_knn_normalized_graph = rec_knn
    cfg = dict(CONFIG)
    try:
        model = M.MGCN(G._run_config(recommender="MGCN"), dict(cfg))
    finally:
        _drop_cache()
    net = model.model
    nu, ni, k = model.num_users, model.num_items, cfg["knn_k"]
    assert [n for n, _ in net.named_parameters()] == list(T.NAMES)
    params = dict(net.named_parameters())
    out = {T._key(n, 0): params[n].detach().numpy().copy() for n in T.NAMES}
    assert np.array_equal(out[T._key("image_embedding.weight", 0)], img) and np.array_equal(out[T._key("text_embedding.weight", 0)], txt)
    # norm_adj: row-major with ascending columns; its top block in R's CSR order
    adj = net.norm_adj.coalesce()
    idx, val = adj.indices().numpy(), adj.values().numpy()
    n_top = int((idx[0] < nu).sum())
    assert 2 * n_top == len(val) and (idx[1][:n_top] >= nu).all()
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(idx[0][:n_top], minlength=nu))
    items = (idx[1][:n_top] - nu).astype(np.int32)
    rows = T.csr_rows(rowptr)
    Rc = net.R.coalesce()
    assert np.array_equal(Rc.indices().numpy()[0], rows) and np.array_equal(Rc.indices().numpy()[1], items)
    assert np.array_equal(Rc.values().numpy(), val[:n_top])
    dev_g = [float(np.abs(T.norm_adj_values(rowptr, items, ni) - val[:n_top]).max())]
    # the modality graphs: the recorded top-(k + 1), the reference's values in the lists' order
    assert len(knn_rec) == 2
    graphs = {}
    for name, (ind, sim), sp_adj, feat in (("image", knn_rec[0], net.image_original_adj, img), ("text", knn_rec[1], net.text_original_adj, txt)):
        ids, sims = ind[:, :k], sim[:, :k]
        if not (sims.sum(1) > 0).all():
            raise SystemExit(f"{name}: a row sum of the kept similarities is not positive: fixture NOT written")
        gap = float((sim[:, k - 1] - sim[:, k]).min())
        if gap <= 1e-5:
            raise SystemExit(f"{name}: k-th and (k+1)-th similarity {gap} apart: fixture NOT written")
        a_idx, a_val = sp_adj._indices().numpy(), sp_adj._values().numpy()
        assert np.array_equal(a_idx[0], np.repeat(np.arange(ni), k)) and np.array_equal(a_idx[1], ids.reshape(-1))
        gval = a_val.reshape(ni, k)
        ids64, sims64 = T.knn_f64(feat, k)
        assert np.array_equal(np.sort(ids64, 1), np.sort(ids, 1)), f"{name}: the float64 kNN sets differ from the reference's"
        want = T.dense_graph(ids64, T.weighted_graph_values(ids64, sims64))
        dev_g.append(float(np.abs(want - T.dense_graph(ids, gval)).max()))
        graphs[name] = (ids.astype(np.int32), sims.astype(np.float32), gval.astype(np.float32))
    orig_loss = net.calculate_loss

    def calculate_loss(users, pos, neg):
        r = orig_loss(users, pos, neg)
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
        _drop_cache()
    for n in T.NAMES:
        out[T._key(n, 1)] = params[n].detach().numpy().copy()
    n_steps = len(batches)
    assert n_steps == len(loss_rec) == 9 and len(pred_rec) == 3
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    assert abs(model.optimizer.param_groups[0]["lr"] - T.schedule_lr(cfg, 3)) < 1e-12
    steps = [dict(users=b[0], pos=b[1], neg=b[2]) for b in batches]
    init = {n: out[T._key(n, 0)] for n in T.NAMES}
    R = T.dense_block(rowptr, items, ni, val[:n_top])
    S = tuple(T.dense_graph(graphs[m][0], graphs[m][2]) for m in ("image", "text"))
    P64, l64, s64 = T.replay_f64(R, S, init, steps, cfg, 3, test_users)
    dev_p = [float(np.abs(P64[n] - out[T._key(n, 1)]).max()) for n in T.NAMES]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, pred_rec)]
    dev_l = float(np.abs(l64 / np.float64(loss_rec) - 1).max())
    print("seed", seed, "f64_dev params", dev_p, "scores", dev_s, "loss (relative)", dev_l, "graph", dev_g)
    if max(dev_p + dev_s + [dev_l] + dev_g) > 1e-5:
        raise SystemExit("the float64 replay has left the reference's trajectory: fixture NOT written")
    # a switched-off term must show far above the reference's own noise
    for what, kw in (("InfoNCE", dict(use_cl=False)), ("regulariser", dict(use_reg=False)), ("schedule", dict(use_schedule=False))):
        Q, _, _ = T.replay_f64(R, S, init, steps, cfg, 3, test_users, **kw)
        off = max(float(np.abs(Q[n] - out[T._key(n, 1)]).max()) for n in T.NAMES)
        print(f"without the {what}: the final parameters differ by {off:.3e} ({off / max(dev_p):.0f} x f64_dev_params)")
        assert off > 100 * max(dev_p), f"the {what} hides under the tolerances: raise its weight"
    ev = model.evaluator
    close, close_ids = [], -np.ones((len(pred_rec), 8), np.int32)
    for e, sc in enumerate(pred_rec):
        c = 0
        for r, u in enumerate(test_users):
            row = sc[r].astype(np.float64).copy()
            row[np.asarray(ev.user_pos_train.get(u, []), dtype=np.int64)] = -np.inf
            t = np.sort(row)[::-1][:22]
            if np.min(t[:-1] - t[1:]) <= 5e-6:
                if c < 8:
                    close_ids[e, c] = u
                c += 1
        close.append(c)
    print("users with a top-22 gap <= 5e-6 per evaluation:", close, "of", len(test_users))
    if max(close) > 3:
        raise SystemExit(f"{max(close)} near-tie users in one evaluation: fixture NOT written")
    out.update(shape=np.int32([nu, ni]), adj_rowptr=rowptr, adj_rows=rows.astype(np.int32), adj_cols=items, adj_val=val[:n_top].astype(np.float32),
               step_users=np.concatenate([b[0] for b in batches]), step_pos=np.concatenate([b[1] for b in batches]),
               step_neg=np.concatenate([b[2] for b in batches]), step_sizes=np.int32([len(b[0]) for b in batches]),
               loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s), f64_dev_loss=np.float64(dev_l),
               f64_dev_graph=np.float64(dev_g), close_users=np.int32(close), close_ids=close_ids, seed=np.int32(seed),
               config=np.array(json.dumps(cfg)))
    for m in ("image", "text"):
        out[m + "_knn_ids"], out[m + "_knn_sims"], out[m + "_graph_val"] = graphs[m]
    print("mgcn: steps", n_steps, "loss", loss_rec[0], loss_rec[-1], "NDCG@10",
          [dict(zip(model.evaluator.metrics_list, r))["NDCG@10"] for r in reports])
    np.savez_compressed(os.path.join(HERE, "golden_mgcn.npz"), **out)


def search(first=2021, last=2400):
    """runs the seeds from ``first`` upward, each in a fresh process, and stops at the first whose run writes the fixture; prints
    per seed which condition was missed (what SEED_NOTE summarises)"""
    import mgcn_twin
    for seed in range(first, last + 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(seed)], capture_output=True, text=True)
        why = [ln for ln in (r.stdout + r.stderr).splitlines() if "NOT written" in ln or "AssertionError" in ln]
        print(seed, "fixture written" if r.returncode == 0 else (why[-1] if why else f"exit status {r.returncode}"), flush=True)
        if r.returncode == 0:
            assert seed == mgcn_twin.SEED, f"the first seed that meets the conditions is {seed}: set mgcn_twin.SEED"
            return seed
    raise SystemExit("no seed met the fixture's conditions")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "run":
        make_mgcn(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "search":          # about ten minutes: 180 runs of the reference
        search()
    else:   # a fresh process, as the other generators: the seed the search ended at
        import mgcn_twin
        subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(mgcn_twin.SEED)], check=True)
