"""Generate the golden vectors of CDAE by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_cdae.py

Same rules as make_golden.py, whose helpers are reused: a fresh process (the negatives come from the process-global
MT19937(2020) stream, untouched before fit()), only data is written.  Per training step the fixture records the batch's
users, the reference's ``bat_items`` / ``bat_labels`` / ``bat_idx``, the raw ``randint_choice`` results before
``np.unique``, one keep flag per non-zero of the encoder's input in its coalesced order (from a wrapper around
``Tensor.uniform_`` that is active while the net is in training mode: floor(u + keep_prob), as ``dropout_sparse`` takes
it), and the loss split into its BCE sum and ``l2_loss``.  Otherwise: the five parameters before and after, per evaluation
the report and the dense ``predict(test_users)`` matrix, and the best report.

The run is then replayed in float64 from the recorded draws (tests/cdae_twin.py: torch autograd, ``torch.optim.Adam``).
``f64_dev`` is the largest difference between that replay and the reference, per parameter and per evaluation's scores:
the reference's own fp32 noise, from which the tests derive their tolerances.  A replay that is far off (F64_LIMIT) means
the recording is wrong, not the tolerance: no fixture is written then.  Nor is one written when more than MAX_CLOSE test
users have two of their 22 best reference scores within 5e-6 (the tests leave such users out of the ranking comparison).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402

CONFIG = dict(lr=1e-2, reg=1e-3, hidden_dim=64, dropout=0.5, num_neg=2, hidden_act="sigmoid", batch_size=24, epochs=3)
PARAMS = ("en_embeddings", "en_offset", "de_embeddings", "de_bias", "user_embeddings")
# fp32 against float64 over nine Adam steps of lr 1e-2: parameters move by about 0.1 and the scores are O(1), so differences
# of 1e-4 and more are a recording error, not rounding
F64_LIMIT = 1e-4
MAX_CLOSE = 3


def _params(net, sfx):
    t = dict(en_embeddings=net.en_embeddings.weight, en_offset=net.en_offset, de_embeddings=net.de_embeddings.weight,
             de_bias=net.de_bias.weight, user_embeddings=net.user_embeddings.weight)
    return {k + sfx: t[k].detach().numpy().copy() for k in PARAMS}


def make_cdae():
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        G.make_dataset()
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.CDAE as M
    import cdae_twin as T
    G._seed_all()
    rec = dict(users=[], items=[], labels=[], idx=[], neg=[], keep=[], bce=[], l2=[], pred=[])
    model = M.CDAE(G._run_config(recommender="CDAE"), dict(CONFIG))
    net = model.cdae
    out = _params(net, "0")
    keep_prob = 1 - CONFIG["dropout"]
    orig_choice = M.randint_choice

    def randint_choice(*a, **k):
        r = orig_choice(*a, **k)
        rec["neg"].append(np.atleast_1d(np.asarray(r)).astype(np.int32).copy())
        return r
    M.randint_choice = randint_choice
    orig_uniform = torch.Tensor.uniform_

    def uniform_(self, *a, **k):
        r = orig_uniform(self, *a, **k)
        if net.training:
            rec["keep"].append((self.detach() + keep_prob).floor().bool().numpy().astype(np.uint8))
        return r
    torch.Tensor.uniform_ = uniform_
    orig_fwd = net.forward

    def forward(user_ids, bat_idx, sp_item_mat, bat_items):
        rec["users"].append(user_ids.numpy().astype(np.int32).copy())
        rec["idx"].append(bat_idx.numpy().astype(np.int32).copy())
        rec["items"].append(bat_items.numpy().astype(np.int32).copy())
        return orig_fwd(user_ids, bat_idx, sp_item_mat, bat_items)
    net.forward = forward
    orig_loss, orig_l2 = model.loss_func, M.l2_loss

    def loss_func(y_pre, y_true):
        r = orig_loss(y_pre, y_true)
        rec["labels"].append(y_true.numpy().astype(np.float32).copy())
        rec["bce"].append(float(r.sum().detach()))
        return r

    def l2_loss(*w):
        r = orig_l2(*w)
        rec["l2"].append(float(r.detach()))
        return r
    model.loss_func, M.l2_loss = loss_func, l2_loss
    test_users = list(model.evaluator.user_pos_test.keys())
    orig_eval = model.evaluate

    def evaluate(tu=None):
        r = orig_eval(tu)                     # puts the net into eval mode first
        rec["pred"].append(model.predict(test_users).astype(np.float32))
        return r
    model.evaluate = evaluate
    reports = G._record_reports(model)
    best = model.fit()
    torch.Tensor.uniform_ = orig_uniform
    out.update(_params(net, "1"))
    n_steps = len(rec["users"])
    assert n_steps == len(rec["keep"]) == len(rec["bce"]) == len(rec["l2"]) == 9 and len(rec["pred"]) == 3
    assert [len(u) for u in rec["users"]] == [24, 24, 15] * 3 and len(rec["neg"]) == 63 * 3
    csr = model.dataset.train_data.to_csr_matrix().tocsr()
    csr.sort_indices()
    rowptr, items = csr.indptr.astype(np.int64), csr.indices.astype(np.int32)
    steps, at = [], 0
    for u, k, it in zip(rec["users"], rec["keep"], rec["items"]):
        negs = rec["neg"][at:at + len(u)]
        at += len(u)
        for uu, ng in zip(u, negs):
            assert len(ng) == CONFIG["num_neg"] * (rowptr[uu + 1] - rowptr[uu])
        assert len(k) == len(it)
        steps.append((u, negs, k))
    # float64 replay from the recorded draws
    init = {k: out[k + "0"] for k in PARAMS}
    p64, l64, s64 = T.replay_f64(rowptr, items, init, steps, CONFIG, 3, test_users)
    dev_p = [float(np.abs(p64[k] - out[k + "1"]).max()) for k in PARAMS]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, rec["pred"])]
    print("f64_dev params", dict(zip(PARAMS, dev_p)), "scores", dev_s)
    print("loss dev", np.abs(l64[:, 0] / np.float64(rec["bce"]) - 1).max(), np.abs(l64[:, 1] / np.float64(rec["l2"]) - 1).max())
    if max(dev_p) > F64_LIMIT or max(dev_s) > F64_LIMIT:
        raise SystemExit(f"float64 replay differs from the reference by {max(dev_p):.3g} (parameters) / {max(dev_s):.3g} "
                         f"(scores): fixture NOT written")
    # users whose 22 best scores hold a pair closer than 5e-6 (rankings of the tests leave them out)
    ev = model.evaluator
    close = []
    for sc in rec["pred"]:
        c = 0
        for r, u in enumerate(test_users):
            row = sc[r].astype(np.float64).copy()
            row[np.asarray(ev.user_pos_train.get(u, []), dtype=np.int64)] = -np.inf
            top = np.sort(row)[::-1][:22]
            c += int(np.min(top[:-1] - top[1:]) <= 5e-6)
        close.append(c)
    print("users with a top-22 gap <= 5e-6 per evaluation:", close)
    if max(close) > MAX_CLOSE:
        raise SystemExit(f"{max(close)} test users with a top-22 gap <= 5e-6 (at most {MAX_CLOSE}): pick another seed or config")
    out.update(step_users=np.concatenate(rec["users"]), step_sizes=np.int32([len(u) for u in rec["users"]]),
               bat_items=np.concatenate(rec["items"]), bat_labels=np.concatenate(rec["labels"]).astype(np.uint8),
               bat_idx=np.concatenate(rec["idx"]).astype(np.int16), pair_sizes=np.int32([len(i) for i in rec["items"]]),
               neg_raw=np.concatenate(rec["neg"]), neg_sizes=np.int32([len(n) for n in rec["neg"]]),
               keep=np.concatenate(rec["keep"]), keep_sizes=np.int32([len(k) for k in rec["keep"]]),
               bce=np.float32(rec["bce"]), l2=np.float32(rec["l2"]),
               reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users),
               pred=np.stack(rec["pred"]), f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s),
               close_users=np.int32(close))
    print("cdae: steps", n_steps, "bce", rec["bce"][0], rec["bce"][-1], "l2", rec["l2"][0], rec["l2"][-1], "NDCG@10",
          dict(best.items())["NDCG@10"], "max |score|", float(np.abs(rec["pred"][-1]).max()))
    np.savez_compressed(os.path.join(HERE, "golden_cdae.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_cdae()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
