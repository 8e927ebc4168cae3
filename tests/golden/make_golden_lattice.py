"""Generate the golden vectors of LATTICE by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_lattice.py

Same rules as make_golden_mgcn.py, whose shims (``torch.sparse.FloatTensor``, ``Tensor.cuda`` returning ``self``) and seeded
features (``tiny.img.npz`` [96, 100], ``tiny.txt.npz`` [96, 37]) are reused: a fresh process, only data is written.  ``reg``,
``lambda_coeff = 0.5``, ``n_layers = 2`` and ``lr_scheduler = [0.5, 1]`` are far from the reference's defaults on purpose, so
that a wrong or missing term cannot hide in three epochs: the generator ASSERTS that the float64 twin with the learned graph,
the regulariser, the schedule or the Adam-skips-a-tensor-without-gradient rule switched off leaves the recorded final
parameters by more than 100 times ``f64_dev_params``.

Recorded: every parameter before and after; ``norm_adj`` (square, CSR); per modality the frozen graph's top-k ids, similarities
and values; per build -- the first step of an epoch, and the first ``predict()`` of its evaluation -- the top-(k + 1) ids and
similarities of both projected tables (a recording wrapper around ``build_knn_neighbourhood``); per step the batch and the
loss; per evaluation the report and the dense ``predict(test_users)``; Adam's step counter per tensor; the config (json).  The
reference's cache files of the frozen graphs (``*lattice_adj*.pt``) are deleted before and after.

The run is then replayed in float64 (tests/lattice_twin.py) on the recorded neighbour sets: ``f64_dev_params`` /
``f64_dev_scores`` / ``f64_dev_loss`` are the largest differences between that replay and the reference.

The fixture's conditions: no ``f64_dev_*`` above 1e-5; at every build every row's k-th and (k+1)-th similarity more than 1e-5
apart, so that another exact kNN returns the reference's sets; every kept row sum positive; no evaluation with more than 3 of
the test users whose top-22 gap is <= 5e-6 (``close_ids``, padded with -1).  Nothing is written when one is missed.  The seed is
the first from 2021 upward whose run meets them: ``python tests/golden/make_golden_lattice.py search`` repeats that search seed
by seed; SEED_NOTE says what the earlier ones gave.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
from make_golden_bm3 import _shims, _write_features  # noqa: E402
from make_golden_mgcn import _mgcn_shims  # noqa: E402
from make_golden_selfcf import _write_tiny_files  # noqa: E402

# What the seeds before lattice_twin.SEED = 2026 gave, each run by ``make_golden_lattice.py run SEED``: 2021 - 2024 have, at one
# of their six builds, a row whose k-th and (k+1)-th learned similarity lie 1.6e-6 to 4.3e-6 apart (another exact kNN could
# return another set there); 2025 has an f64_dev_params above 1e-5 -- an element whose first gradient lies beside Adam's eps,
# as make_golden_freedom.py explains.  2026 gives a smallest gap of 1.5e-5, f64_dev_params <= 4.4e-6 and [0, 3, 1] near-tie users.
SEED_NOTE = {"2021 .. 2024": "a learned k-th / (k+1)-th similarity gap of 1.6e-6 to 4.3e-6", "2025": "f64_dev_params above 1e-5"}
CONFIG = dict(lr=1e-2, reg=1e-2, lambda_coeff=0.5, n_layers=2, knn_k=10, lr_scheduler=[0.5, 1], batch_size=256, epochs=3)


def _drop_cache():
    for f in glob.glob(os.path.join(G.SCRATCH, "**", "*lattice_adj*.pt"), recursive=True):
        os.remove(f)


def make_lattice(seed):
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        _write_tiny_files()
    img, txt = _write_features()
    import lattice_twin as T
    G._install()
    import torch
    torch.set_num_threads(1)
    _shims()
    _mgcn_shims()
    import skrec.recommender.LATTICE as M
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
    orig_knn = M.build_knn_neighbourhood

    def rec_knn(adj, topk):
        val, ind = torch.topk(adj.detach(), topk + 1, dim=-1)
        knn_rec.append((ind.numpy().copy(), val.numpy().copy()))
        return orig_knn(adj, topk)
    M.build_knn_neighbourhood = rec_knn
    cfg = dict(CONFIG)
    tcfg = T.twin_config(**cfg)
    try:
        model = M.LATTICE(G._run_config(recommender="LATTICE"), dict(cfg))
    finally:
        _drop_cache()
    net = model.model
    nu, ni, k = model.num_users, model.num_items, cfg["knn_k"]
    assert [n for n, _ in net.named_parameters()] == list(T.NAMES)
    params = dict(net.named_parameters())
    out = {T._key(n, 0): params[n].detach().numpy().copy() for n in T.NAMES}
    assert np.array_equal(out[T._key("image_embedding.weight", 0)], img) and np.array_equal(out[T._key("text_embedding.weight", 0)], txt)
    # norm_adj: square, row-major with ascending columns
    adj = net.norm_adj.coalesce()
    idx, val = adj.indices().numpy(), adj.values().numpy()
    norm_rowptr = np.zeros(nu + ni + 1, np.int64)
    norm_rowptr[1:] = np.cumsum(np.bincount(idx[0], minlength=nu + ni))
    top = idx[0] < nu
    off = top & (idx[1] >= nu)
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(idx[0][off], minlength=nu))
    items = (idx[1][off] - nu).astype(np.int32)
    dev_adj = float(np.abs(T.norm_adj_dense(rowptr, items, ni)[idx[0], idx[1]] - val).max())
    assert dev_adj <= 1e-7, dev_adj
    # the frozen graphs: the recorded top-(k + 1) of the raw features, the reference's values in the lists' order
    assert len(knn_rec) == 2
    frozen = {}
    for name, (ind, sim), dense, feat in (("image", knn_rec[0], net.image_original_adj, img), ("text", knn_rec[1], net.text_original_adj, txt)):
        ids, sims = ind[:, :k], sim[:, :k]
        if not (sims.sum(1) > 0).all():
            raise SystemExit(f"{name}: a row sum of the kept similarities is not positive: fixture NOT written")
        gap = float((sim[:, k - 1] - sim[:, k]).min())
        if gap <= 1e-5:
            raise SystemExit(f"{name}: frozen k-th and (k+1)-th similarity {gap} apart: fixture NOT written")
        gval = np.take_along_axis(dense.numpy(), ids, 1)
        assert int((dense.numpy() != 0).sum()) == ni * k
        want_ids, want_val = T.frozen_lists(feat, k)
        assert np.array_equal(want_ids, np.sort(ids, 1)), f"{name}: the float64 kNN sets differ from the reference's"
        order = np.argsort(ids, axis=1, kind="stable")
        assert np.abs(want_val - np.take_along_axis(gval, order, 1)).max() <= 1e-6
        frozen[name] = (ids.astype(np.int32), sims.astype(np.float32), gval.astype(np.float32))
    del knn_rec[:]
    orig_loss = net.calculate_loss

    def calculate_loss(users, pos, neg):
        r = orig_loss(users, pos, neg)
        loss_rec.append(float(r.detach()))
        return r
    net.calculate_loss = calculate_loss
    test_users = list(model.evaluator.user_pos_test.keys())
    orig_eval = model.evaluate
    builds = []                    # per epoch: its build step's two recordings, then its evaluation's first two

    def evaluate(tu=None):
        assert len(knn_rec) == 2, len(knn_rec)          # the epoch's one build step
        builds.append(list(knn_rec))
        del knn_rec[:]
        r = orig_eval(tu)
        pred_rec.append(model.predict(test_users).astype(np.float32))
        assert len(knn_rec) >= 4 and len(knn_rec) % 2 == 0
        for c in range(2, len(knn_rec), 2):            # every predict() of one evaluation sees the same parameters
            assert np.array_equal(knn_rec[c][0], knn_rec[0][0]) and np.array_equal(knn_rec[c + 1][1], knn_rec[1][1])
        builds.append(list(knn_rec[:2]))
        del knn_rec[:]
        return r
    model.evaluate = evaluate
    reports = G._record_reports(model)
    try:
        best = model.fit()
    finally:
        _drop_cache()
    for n in T.NAMES:
        out[T._key(n, 1)] = params[n].detach().numpy().copy()
    adam_t = [int(model.optimizer.state[params[n]]["step"]) for n in T.NAMES]
    assert adam_t == [3, 9, 9, 3, 3, 3, 3, 3, 3], adam_t
    n_steps = len(batches)
    assert n_steps == len(loss_rec) == 9 and len(pred_rec) == 3 and len(builds) == 6
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    assert abs(model.optimizer.param_groups[0]["lr"] - T.schedule_lr(tcfg, 3)) < 1e-12
    min_gap, min_sum = np.inf, np.inf
    for b in builds:
        for ind, sim in b:
            min_gap = min(min_gap, float((sim[:, k - 1] - sim[:, k]).min()))
            min_sum = min(min_sum, float(sim[:, :k].sum(1).min()))
    print("seed", seed, "smallest gap between the k-th and the (k+1)-th similarity", min_gap, "smallest kept row sum", min_sum)
    if min_gap <= 1e-5:
        raise SystemExit(f"learned k-th and (k+1)-th similarity {min_gap} apart: fixture NOT written")
    if min_sum <= 0:
        raise SystemExit("a row sum of the kept learned similarities is not positive: fixture NOT written")
    knn_ids = np.stack([np.stack([b[0][0], b[1][0]]) for b in builds]).astype(np.int32)
    knn_sims = np.stack([np.stack([b[0][1], b[1][1]]) for b in builds]).astype(np.float32)
    out.update(shape=np.int32([nu, ni]), adj_rowptr=rowptr, adj_cols=items, norm_rowptr=norm_rowptr, norm_col=idx[1].astype(np.int32),
               norm_val=val.astype(np.float32), knn_ids=knn_ids, knn_sims=knn_sims)
    for m in ("image", "text"):
        out[m + "_frozen_ids"], out[m + "_frozen_sims"], out[m + "_frozen_val"] = frozen[m]
    steps = [dict(users=b[0], pos=b[1], neg=b[2]) for b in batches]
    init = {n: out[T._key(n, 0)] for n in T.NAMES}
    A, fr, knn = T.fixture_adjacency(out), T.fixture_frozen(out), T.fixture_knn(out, k)
    P64, l64, s64, ts = T.replay_f64(A, fr, init, steps, tcfg, 3, test_users, knn_builds=knn)
    assert ts == (9, 3)
    dev_p = [float(np.abs(P64[n] - out[T._key(n, 1)]).max()) for n in T.NAMES]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, pred_rec)]
    dev_l = float(np.abs(l64 / np.float64(loss_rec) - 1).max())
    print("seed", seed, "f64_dev params", dev_p, "scores", dev_s, "loss (relative)", dev_l)
    if max(dev_p + dev_s + [dev_l]) > 1e-5:
        raise SystemExit("the float64 replay has left the reference's trajectory: fixture NOT written")
    # a switched-off term must show far above the reference's own noise
    for what, kw in (("learned graph", dict(use_learned=False)), ("regulariser", dict(use_reg=False)), ("schedule", dict(use_schedule=False)),
                     ("Adam-skips-None rule", dict(skip_modal_on_ordinary_steps=False))):
        Q = T.replay_f64(A, fr, init, steps, tcfg, 3, test_users, knn_builds=knn, **kw)[0]
        off = max(float(np.abs(Q[n] - out[T._key(n, 1)]).max()) for n in T.NAMES)
        print(f"without the {what}: the final parameters differ by {off:.3e} ({off / max(dev_p):.0f} x f64_dev_params)")
        assert off > 100 * max(dev_p), f"the {what} hides under the tolerances"
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
    out.update(step_users=np.concatenate([b[0] for b in batches]), step_pos=np.concatenate([b[1] for b in batches]),
               step_neg=np.concatenate([b[2] for b in batches]), step_sizes=np.int32([len(b[0]) for b in batches]),
               loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s), f64_dev_loss=np.float64(dev_l),
               close_users=np.int32(close), close_ids=close_ids, seed=np.int32(seed), adam_steps=np.int32(adam_t),
               min_gap=np.float64(min_gap), config=np.array(json.dumps(cfg)))
    print("lattice: steps", n_steps, "loss", loss_rec[0], loss_rec[-1], "NDCG@10",
          [dict(zip(model.evaluator.metrics_list, r))["NDCG@10"] for r in reports])
    np.savez_compressed(os.path.join(HERE, "golden_lattice.npz"), **out)


def search(first=2021, last=2400):
    """runs the seeds from ``first`` upward, each in a fresh process, and stops at the first whose run writes the fixture; prints
    per seed which condition was missed (what SEED_NOTE summarises)"""
    import lattice_twin
    for seed in range(first, last + 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(seed)], capture_output=True, text=True)
        why = [ln for ln in (r.stdout + r.stderr).splitlines() if "NOT written" in ln or "AssertionError" in ln or "Error" in ln]
        print(seed, "fixture written" if r.returncode == 0 else (why[-1] if why else f"exit status {r.returncode}"), flush=True)
        if r.returncode == 0:
            assert seed == lattice_twin.SEED, f"the first seed that meets the conditions is {seed}: set lattice_twin.SEED"
            return seed
    raise SystemExit("no seed met the fixture's conditions")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "run":
        make_lattice(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "search":
        search()
    else:   # a fresh process, as the other generators: the seed the search ended at
        import lattice_twin
        subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(lattice_twin.SEED)], check=True)
