"""Generate the golden vectors of SLMRec by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_slmrec.py

Same rules as make_golden_mgcn.py, whose helpers and seeded features (``tiny.img.npz`` [96, 100], ``tiny.txt.npz`` [96, 37]) are
reused: a fresh process, only data is written.  The one import-time shim is make_golden_bm3.py's legacy sparse constructor
(SLMRec.py:102).  ``lr``, ``ssl_alpha`` and the three epochs of three steps are far from the reference's defaults on purpose, so
that a wrong or missing term cannot hide: the generator ASSERTS that the float64 twin with the main term, ``v_loss`` or
``t_loss`` switched off leaves the recorded final parameters by more than 100 times ``f64_dev_params``, and that ``g_a_iva``
after training equals ``g_a_iva`` before, bit for bit (no gradient reaches it, so Adam skips it: SLMRec.py:347-351).

Recorded: every parameter before and after; the row-normalised feature tables as the model holds them; ``norm_adj`` in R's CSR
order; per step the batch (a recording wrapper around ``InteractionIterator``) and the loss; per evaluation the report, the
dense ``predict(test_users)`` (after the sigmoid) and the raw scores before it; the best report; the config (json).

The run is then replayed in float64 (tests/slmrec_twin.py): ``f64_dev_params`` / ``f64_dev_scores`` (raw scores) /
``f64_dev_loss`` are the largest differences between that replay and the reference.

The fixture's conditions are FREEDOM's / MGCN's: no ``f64_dev_*`` above 1e-5 -- but for ``g_v_iv.bias`` and ``g_t_ivat.bias``,
whose gradient is zero in exact arithmetic and whose trajectory in the reference is rounding noise magnified by Adam
(slmrec_twin.NOISE_DRIVEN says why; their deviation is recorded like the others and is some lr); no evaluation with more than 3 of the test users
whose top-22 gap of the raw scores is <= 5e-6 (``close_ids``, padded with -1).  Nothing is written when one is missed.  The
seed is the first from 2021 upward whose run meets them: ``python tests/golden/make_golden_slmrec.py search`` repeats that
search seed by seed; SEED_NOTE says what the earlier ones gave.
"""
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
from make_golden_selfcf import _write_tiny_files  # noqa: E402

# What the seed before slmrec_twin.SEED = 2022 gave (``make_golden_slmrec.py run 2021``): embedding_item_after_GCN.weight ends
# 1.9e-3 from the float64 replay through two elements whose FIRST gradient lies beside Adam's eps (element [32][189]: -6.8e-9
# in float64, -1.8e-9 in an fp32 evaluation), where the first update magnifies an error of the gradient by up to lr / eps, as
# make_golden_freedom.py explains; from there the difference spreads to 477 elements of that tensor above 1e-5 by the ninth step.
SEED_NOTE = {"2021": "f64_dev_params[embedding_item_after_GCN.weight] = 1.9e-3: two elements whose first gradient lies beside Adam's eps"}
CONFIG = dict(lr=1e-2, ssl_alpha=0.5, layer_num=2, batch_size=256, epochs=3)


def make_slmrec(seed):
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        _write_tiny_files()
    img, txt = _write_features()
    import slmrec_twin as T
    G._install()
    import torch
    torch.set_num_threads(1)
    _shims()
    import skrec.recommender.SLMRec as M
    G.SEED = seed
    G._seed_all()
    batches, loss_rec, pred_rec, raw_rec = [], [], [], []
    orig_iter = M.InteractionIterator

    class RecordingIterator(object):
        def __init__(self, *a, **k):
            self.it = orig_iter(*a, **k)

        def __len__(self):
            return len(self.it)

        def __iter__(self):
            for u, p in self.it:
                batches.append(tuple(np.asarray(c, np.int32).copy() for c in (u, p)))
                yield u, p
    M.InteractionIterator = RecordingIterator
    cfg = dict(CONFIG)
    model = M.SLMRec(G._run_config(recommender="SLMRec"), dict(cfg))
    full = {k: getattr(model.config, k) for k in ("lr", "reg", "rec_dim", "layer_num", "ssl_alpha", "ssl_temp", "dropout_rate", "temp",
                                                  "weight_decay", "mm_fusion_mode", "adj_type", "ssl_task", "init", "batch_size",
                                                  "epochs", "early_stop")}
    net = model.model
    nu, ni = model.num_users, model.num_items
    assert [n for n, _ in net.named_parameters()] == list(T.NAMES)
    params = dict(net.named_parameters())
    out = {T._key(n, 0): params[n].detach().numpy().copy() for n in T.NAMES}
    v_feat, t_feat = net.v_feat.numpy().copy(), net.t_feat.numpy().copy()
    assert np.array_equal(v_feat, torch.nn.functional.normalize(torch.from_numpy(img), dim=1).numpy())
    assert np.array_equal(t_feat, torch.nn.functional.normalize(torch.from_numpy(txt), dim=1).numpy())
    # norm_adj: row-major with ascending columns; its top block in R's CSR order; symmetric
    adj = net.norm_adj.coalesce()
    idx, val = adj.indices().numpy(), adj.values().numpy()
    n_top = int((idx[0] < nu).sum())
    assert 2 * n_top == len(val) and (idx[1][:n_top] >= nu).all() and val.dtype == np.float32
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(idx[0][:n_top], minlength=nu))
    items = (idx[1][:n_top] - nu).astype(np.int32)
    rows = T.csr_rows(rowptr)
    dense = adj.to_dense().numpy()
    assert np.array_equal(dense, dense.T) and np.array_equal(dense[:nu, nu:][rows, items], val[:n_top])
    assert np.array_equal(T.pre_adj_values(rowptr, items, ni), val[:n_top]), "the twin's adjacency values differ from the reference's bits"
    orig_loss = net.calculate_loss

    def calculate_loss(users, pos):
        r = orig_loss(users, pos)
        loss_rec.append(float(r.detach()))
        return r
    net.calculate_loss = calculate_loss
    test_users = list(model.evaluator.user_pos_test.keys())
    orig_eval = model.evaluate

    def evaluate(tu=None):
        r = orig_eval(tu)
        pred_rec.append(model.predict(test_users).astype(np.float32))
        raw_rec.append((net.all_users[torch.as_tensor(test_users)] @ net.all_items.t()).detach().numpy().astype(np.float32))
        return r
    model.evaluate = evaluate
    reports = G._record_reports(model)
    best = model.fit()
    for n in T.NAMES:
        out[T._key(n, 1)] = params[n].detach().numpy().copy()
    for n in T.UNTRAINED:
        assert np.array_equal(out[T._key(n, 0)], out[T._key(n, 1)]), f"{n} moved"
        assert params[n].grad is None
    n_steps = len(batches)
    assert n_steps == len(loss_rec) == 9 and len(pred_rec) == 3
    assert [len(b[0]) for b in batches] == [256, 256, 251] * 3
    assert model.optimizer.param_groups[0]["lr"] == cfg["lr"]
    for e in range(3):
        assert np.array_equal(pred_rec[e], torch.sigmoid(torch.from_numpy(raw_rec[e])).numpy())
    steps = [dict(users=b[0], pos=b[1]) for b in batches]
    init = {n: out[T._key(n, 0)] for n in T.NAMES}
    R = T.dense_block(rowptr, items, ni, val[:n_top])
    V64, T64 = v_feat.astype(np.float64), t_feat.astype(np.float64)
    P64, l64, s64 = T.replay_f64(R, V64, T64, init, steps, full, 3, test_users)
    dev_p = [float(np.abs(P64[n] - out[T._key(n, 1)]).max()) for n in T.NAMES]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, raw_rec)]
    dev_l = float(np.abs(l64 / np.float64(loss_rec) - 1).max())
    print("seed", seed, "f64_dev params", dev_p, "scores", dev_s, "loss (relative)", dev_l)
    held = [d for n, d in zip(T.NAMES, dev_p) if n not in T.NOISE_DRIVEN]          # see slmrec_twin.NOISE_DRIVEN
    if max(held + dev_s + [dev_l]) > 1e-5:
        far = {n: int((np.abs(P64[n] - out[T._key(n, 1)]) > 1e-5).sum()) for n in T.NAMES if n not in T.NOISE_DRIVEN}
        print("elements further than 1e-5 from the reference:", {n: c for n, c in far.items() if c})
        raise SystemExit("the float64 replay has left the reference's trajectory: fixture NOT written")
    # a switched-off term must show far above the reference's own noise
    for what, kw in (("main term", dict(use_main=False)), ("v_loss", dict(use_v=False)), ("t_loss", dict(use_t=False))):
        Q, _, _ = T.replay_f64(R, V64, T64, init, steps, full, 3, test_users, **kw)
        off = max(float(np.abs(Q[n] - out[T._key(n, 1)]).max()) for n in T.NAMES if n not in T.NOISE_DRIVEN)
        print(f"without the {what}: the final parameters differ by {off:.3e} ({off / max(held):.0f} x f64_dev_params)")
        assert off > 100 * max(held), f"the {what} hides under the tolerances: raise its weight"
    ev = model.evaluator
    close, close_ids = [], -np.ones((len(raw_rec), 8), np.int32)
    for e, sc in enumerate(raw_rec):
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
               v_feat=v_feat, t_feat=t_feat, img=img, txt=txt,
               step_users=np.concatenate([b[0] for b in batches]), step_pos=np.concatenate([b[1] for b in batches]),
               step_sizes=np.int32([len(b[0]) for b in batches]),
               loss=np.float32(loss_rec), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users), pred=np.stack(pred_rec),
               raw=np.stack(raw_rec), f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s), f64_dev_loss=np.float64(dev_l),
               close_users=np.int32(close), close_ids=close_ids, seed=np.int32(seed), config=np.array(json.dumps(full)),
               config_given=np.array(json.dumps(cfg)))
    print("slmrec: steps", n_steps, "loss", loss_rec[0], loss_rec[-1], "NDCG@10",
          [dict(zip(model.evaluator.metrics_list, r))["NDCG@10"] for r in reports])
    np.savez_compressed(os.path.join(HERE, "golden_slmrec.npz"), **out)


def search(first=2021, last=2400):
    """runs the seeds from ``first`` upward, each in a fresh process, and stops at the first whose run writes the fixture; prints
    per seed which condition was missed (what SEED_NOTE summarises)"""
    import slmrec_twin
    for seed in range(first, last + 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(seed)], capture_output=True, text=True)
        why = [ln for ln in (r.stdout + r.stderr).splitlines() if "NOT written" in ln or "AssertionError" in ln]
        print(seed, "fixture written" if r.returncode == 0 else (why[-1] if why else f"exit status {r.returncode}"), flush=True)
        if r.returncode == 0:
            assert seed == slmrec_twin.SEED, f"the first seed that meets the conditions is {seed}: set slmrec_twin.SEED"
            return seed
    raise SystemExit("no seed met the fixture's conditions")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "run":
        make_slmrec(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "search":
        search()
    else:   # a fresh process, as the other generators: the seed the search ended at
        import slmrec_twin
        subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(slmrec_twin.SEED)], check=True)
