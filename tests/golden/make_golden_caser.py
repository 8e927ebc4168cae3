"""Generate the golden vectors of Caser by RUNNING THE REFERENCE on the ``tiny_seq`` set of make_golden_seq.py:

    python tests/golden/make_golden_caser.py

Same rules as make_golden_hgn.py, whose helpers and whose 1e-7 floor on ``min_top_gap`` are reused: a fresh process, only
data is written.  Besides HGN's replay vectors the fixture holds, per training step, the batch as the model received it
(users, windows, positives || negatives), the two cross-entropy sums, and the dropout's keep flags.

The keep flags are recorded as ``output != 0`` of the reference's nn.Dropout, bit-packed.  That is the mask wherever the
dropout's input is non-zero; where the input is zero (a horizontal filter whose ReLU is dead: about a seventh of the
elements here) the recorded flag is 0 whatever torch drew, and it does not matter: such an element is 0 kept or dropped and
passes no gradient.  The flags of zero inputs are therefore arbitrary, and nothing may be concluded from their mean.

The reference builds ``_Caser`` without ``item_pad_idx`` (Caser.py:179), so its padding item (id 96 here) is an ordinary
row of item_embeddings, W2 and b2: normal-initialised, read in padded windows and trained.  The fixture pins that.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import make_golden_seq as S  # noqa: E402
from make_golden_hgn import MIN_GAP  # noqa: E402
from caser_twin import CONFIG, param_names  # noqa: E402


def _params(c, sfx):
    t = {"user_embeddings": c.user_embeddings.weight, "item_embeddings": c.item_embeddings.weight,
         "conv_v_weight": c.conv_v.weight, "conv_v_bias": c.conv_v.bias, "fc1_weight": c.fc1.weight, "fc1_bias": c.fc1.bias,
         "W2": c.W2.weight, "b2": c.b2.weight}
    for i, conv in enumerate(c.conv_h):
        t[f"conv_h_weight_{i}"], t[f"conv_h_bias_{i}"] = conv.weight, conv.bias
    return {k + sfx: t[k].detach().numpy().copy() for k in param_names(len(c.conv_h))}


def make_caser():
    if not os.path.exists(os.path.join(S.SEQ_DIR, "tiny_seq.train")):
        S.make_dataset()
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.Caser as M
    G._seed_all()
    model = M.Caser(S._cfg("Caser"), dict(CONFIG))
    net = model.caser
    assert net.item_embeddings.padding_idx is None and net.W2.padding_idx is None
    out = _params(net, "0")
    bce, users, seqs, items, keeps = [], [], [], [], []
    oc = M.sigmoid_cross_entropy

    def rc(y, t):
        r = oc(y, t); bce.append(float(r.sum())); return r
    M.sigmoid_cross_entropy = rc

    def batch_hook(mod, args):
        if mod.training:
            u, s, t = args
            users.append(u.numpy().reshape(-1).astype(np.int32))
            seqs.append(s.numpy().astype(np.int32))
            items.append(t.numpy().astype(np.int32))
    net.register_forward_pre_hook(batch_hook)

    def keep_hook(mod, args, output):
        if mod.training:
            keeps.append((output != 0).numpy().astype(np.uint8))
    net.dropout.register_forward_hook(keep_hook)
    # the gap between neighbouring top scores, measured on what every evaluation ranks (eval mode: no draw is consumed)
    ev = model.evaluator
    test_users = list(ev.user_pos_test.keys())
    gaps, peaks = [], []
    orig = model.evaluate

    def evaluate(test_users_=None):
        net.eval()
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
    out.update(_params(net, "1"))
    trunc = model.user_truncated_seq
    bounds = np.cumsum([0] + [len(u) for u in users]).astype(np.int64)
    keep = np.concatenate(keeps, 0)
    out.update(bce_sums=np.float32(bce).reshape(-1, 2), step_bounds=bounds, batch_users=np.concatenate(users),
               batch_seqs=np.concatenate(seqs, 0), batch_items=np.concatenate(items, 0),
               keep_bits=np.packbits(keep.reshape(-1)), keep_shape=np.int64(keep.shape),
               reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), pred_users=S.PRED_USERS, pred=model.predict(list(S.PRED_USERS)),
               trunc_users=np.array(list(trunc.keys()), np.int32),
               trunc_seqs=np.stack([np.asarray(v) for v in trunc.values()]).astype(np.int32),
               min_top_gap=np.float64([min(gaps), max(peaks)]))
    print("caser: steps", len(bce) // 2, "first/last bce", bce[:2], bce[-2:], "NDCG@10", dict(best.items())["NDCG@10"],
          "min_top_gap", min(gaps), "max |score|", max(peaks), "mean of output != 0", float(keep.mean()))
    if min(gaps) < MIN_GAP:
        raise SystemExit(f"min_top_gap {min(gaps):.3g} < {MIN_GAP}: fixture NOT written (see make_golden_hgn.py)")
    np.savez_compressed(os.path.join(HERE, "golden_caser.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_caser()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
