"""Generate the golden vectors of HGN by RUNNING THE REFERENCE on the ``tiny_seq`` set of make_golden_seq.py:

    python tests/golden/make_golden_hgn.py

Same rules as make_golden.py / make_golden_seq.py, whose helpers are reused: a fresh process (the reference's sampler
stream is process-global), only data is written.  Besides the usual replay vectors the fixture holds the reference's
``user_truncated_seq`` (as two arrays, in dict order) and ``min_top_gap``: over all test users and all evaluations, the
smallest difference between neighbouring scores among the 22 best unmasked scores (top-20 metrics are decided there),
with the largest |score| next to it.  A fixture whose gap is below 1e-7 is not written: its rankings would hang on the
last bits of an fp32 score.  If a torch build produces that, change ``epochs`` or the seed handling here, not a tolerance.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_seq as S  # noqa: E402

CONFIG = dict(lr=1e-3, reg=1e-3, seq_L=5, seq_T=3, embed_size=64, batch_size=256, epochs=3)
MIN_GAP = 1e-7
PARAMS = ("user_embeddings", "item_embeddings", "feature_gate_item_weight", "feature_gate_item_bias",
          "feature_gate_user_weight", "feature_gate_user_bias", "instance_gate_item", "instance_gate_user", "W2", "b2")


def _params(h, sfx):
    t = {"user_embeddings": h.user_embeddings.weight, "item_embeddings": h.item_embeddings.weight,
         "feature_gate_item_weight": h.feature_gate_item.weight, "feature_gate_item_bias": h.feature_gate_item.bias,
         "feature_gate_user_weight": h.feature_gate_user.weight, "feature_gate_user_bias": h.feature_gate_user.bias,
         "instance_gate_item": h.instance_gate_item, "instance_gate_user": h.instance_gate_user,
         "W2": h.W2.weight, "b2": h.b2.weight}
    return {k + sfx: t[k].detach().numpy().copy() for k in PARAMS}


def make_hgn():
    if not os.path.exists(os.path.join(S.SEQ_DIR, "tiny_seq.train")):
        S.make_dataset()
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.HGN as M
    G._seed_all()
    model = M.HGN(S._cfg("HGN"), dict(CONFIG))
    out = _params(model.hgn, "0")
    bpr = []
    ob = M.bpr_loss

    def rb(a, b):
        r = ob(a, b); bpr.append(float(r.sum())); return r
    M.bpr_loss = rb
    # the gap between neighbouring top scores, measured on what every evaluation ranks
    ev = model.evaluator
    test_users = list(ev.user_pos_test.keys())
    gaps, peaks = [], []
    orig = model.evaluate

    def evaluate(test_users_=None):
        sc = model.predict(test_users).astype(np.float32)
        for r, u in enumerate(test_users):
            row = sc[r].copy()
            row[np.asarray(ev.user_pos_train[u], dtype=np.int64)] = -np.inf
            top = np.sort(row)[::-1][:22]
            gaps.append(float(np.min(top[:-1] - top[1:])))
            peaks.append(float(np.abs(top).max()))
        return orig(test_users_)
    model.evaluate = evaluate
    reports = G._record_reports(model)
    best = model.fit()
    out.update(_params(model.hgn, "1"))
    trunc = model.user_truncated_seq
    out.update(bpr_sum=np.float32(bpr), reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), pred_users=S.PRED_USERS,
               pred=model.predict(list(S.PRED_USERS)),
               trunc_users=np.array(list(trunc.keys()), np.int32),
               trunc_seqs=np.stack([np.asarray(v) for v in trunc.values()]).astype(np.int32),
               min_top_gap=np.float64([min(gaps), max(peaks)]))
    print("hgn: steps", len(bpr), "first/last bpr", bpr[0], bpr[-1], "NDCG@10", dict(best.items())["NDCG@10"],
          "min_top_gap", min(gaps), "max |score|", max(peaks))
    if min(gaps) < MIN_GAP:
        raise SystemExit(f"min_top_gap {min(gaps):.3g} < {MIN_GAP}: fixture NOT written (see the module docstring)")
    np.savez_compressed(os.path.join(HERE, "golden_hgn.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_hgn()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
