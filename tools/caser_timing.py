"""Timing of Caser at bench scale on one GPU:

    python tools/caser_timing.py [--users 1000000 --items 100000 --inter 48000000 --batch 1024 --steps 200 --repeats 3
                                  --eval_users 65536 --out profiles/caser_timing.json]

Data: bench.synth_dataset (imported, not copied); a user's interactions in their stored order stand in for time, as in
tools/seq_timing.py, whose instance builder is reused: windows of seq_L consecutive items of a user's row, left-padded at the
row's start, the next seq_T items as positives, uniform negatives (no exclusion: timing only).  Settings: embed_size 64, the
reference's defaults (seq_L 5, seq_T 3, nv 4, nh 16, dropout 0.5), device draws.

Reported, as one JSON document: ms per training step with one dense skr_adam_step_wd per step and with the temporally
blocked Adam; the step's launch groups one by one (skr_caser_step_timed), the two MFMA products (the horizontal filters'
[n L, 64] x [64, rows] and fc1's [n, Fp] x [Fp, 64]) as a fraction of the 157.3 TF fp32 matrix peak -- of the launch that
holds them, which also gathers, pools and writes; skr_caser_queries over all users; evaluation users/s through the fused
top-K evaluator at 128 columns (the route RankingEvaluator takes), the same users through the dense score rows
(skr_score_matrix at 128 columns, behind a wrapper that exposes score_rows only: the route taken before the evaluator
ranked wide rows) and HGN's fused 64-column evaluation on the same data, all in one session.

Beside it, in the same session: the reference's step written with torch-ROCm ops (embedding lookups, conv2d, relu,
max_pool1d, dropout, linear, baddbmm, binary_cross_entropy_with_logits, backward, torch.optim.Adam(weight_decay) over every
parameter) -- restated here from the model's equations (recommender/Caser.py:118-157,196-207)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "scikit-recommender_amd"), os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench import synth_dataset  # noqa: E402
from seq_timing import _Epoch, _spread, _time, hgn_instances  # noqa: E402
from skrec import _hip  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
GROUPS = ("conv", "fc1", "score", "d_out", "dW1", "conv_bwd", "filter_grads", "rank", "ordered_adds", "loss")


class TorchStep(object):
    """the reference's step on torch-ROCm ops"""

    def __init__(self, nU, nI, e, L, T, nv, nh, rate, lr, wd, dev):
        import torch.nn as nn
        self.ue, self.ie = nn.Embedding(nU, e).to(dev), nn.Embedding(nI, e).to(dev)
        self.conv_v = nn.Conv2d(1, nv, (L, 1)).to(dev)
        self.conv_h = nn.ModuleList([nn.Conv2d(1, nh, (i + 1, e)) for i in range(L)]).to(dev)
        self.fc1 = nn.Linear(nv * e + nh * L, e).to(dev)
        self.W2, self.b2 = nn.Embedding(nI, 2 * e).to(dev), nn.Embedding(nI, 1).to(dev)
        self.drop, self.T, self.nv, self.e = nn.Dropout(rate), T, nv, e
        mods = [self.ue, self.ie, self.conv_v, self.conv_h, self.fc1, self.W2, self.b2]
        self.opt = torch.optim.Adam([p for m in mods for p in m.parameters()], lr=lr, weight_decay=wd)

    def step(self, u, seq, items):
        import torch.nn.functional as F
        emb = self.ie(seq).unsqueeze(1)
        out_v = self.conv_v(emb).view(-1, self.nv * self.e)
        hs = []
        for conv in self.conv_h:
            c = F.relu(conv(emb).squeeze(3))
            hs.append(F.max_pool1d(c, c.size(2)).squeeze(2))
        z = F.relu(self.fc1(self.drop(torch.cat([out_v] + hs, 1))))
        x = torch.cat([z, self.ue(u)], 1)
        y = torch.baddbmm(self.b2(items), self.W2(items), x.unsqueeze(2)).squeeze(-1)
        yp, yn = torch.split(y, [self.T, self.T], dim=1)
        bce = F.binary_cross_entropy_with_logits
        loss = (bce(yp, torch.ones_like(yp), reduction="none") + bce(yn, torch.zeros_like(yn), reduction="none")).mean()
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "caser_timing.json"))
    args = ap.parse_args()
    from skrec.recommender.Caser import Caser
    from skrec.recommender.HGN import HGN
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    nU, nI, b = args.users, args.items, args.batch
    L, T, nv, nh, e = 5, 3, 4, 16, 64
    ds = synth_dataset(nU, nI, args.inter, 2021, dev)
    cols, windows = hgn_instances(ds, nI, dev, 11, L, T, b * args.steps)
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), instances=int(cols[0].shape[0]), batch=b, embed_size=e,
               seq_L=L, seq_T=T, nv=nv, nh=nh, dropout=0.5, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    cfg = dict(lr=1e-3, l2_reg=1e-6, embed_size=e, seq_L=L, seq_T=T, nv=nv, nh=nh, dropout=0.5, batch_size=b)
    win_host = windows.cpu().numpy()
    for label, blk in (("dense", "1"), ("blocked", os.environ.get("SKR_ADAM_BLOCK", "32"))):
        os.environ["SKR_ADAM_BLOCK"] = blk
        m = Caser.detached(nU, nI, cfg, windows=win_host, seed=1)
        ep = _Epoch(cols, b, args.steps)
        res[f"step_ms_{label}"] = _spread([_time(lambda: m.train_epoch(ep)) / len(ep.bounds) for _ in range(args.repeats)])
        res[f"adam_block_{label}"] = m.adam_block
        if label == "dense":
            del m
            torch.cuda.empty_cache()
    res["n_params"] = m.optimizer.flat.numel()
    # the launch groups one by one: full batches only, the gradients left to accumulate (timing only)
    ep = _Epoch(cols, b, min(args.steps, 32))
    st = _hip.stream()
    loss = torch.zeros(2 * _hip.SKR_LOSS_SLOTS, device=dev)
    cu, cl, cp, cn = (c.data_ptr() for c in ep.cols)
    full = [a for a, z in ep.bounds if z - a == b]
    m.timed_ms = np.zeros(_hip.SKR_CASER_LAUNCHES, np.float32)

    def timed():
        acc = np.zeros(len(GROUPS))
        for a in full:
            _hip.check(m._step_launch(cu + 4 * a, cl + 4 * L * a, cp + 4 * T * a, cn + 4 * T * a, b, loss.data_ptr(), st))
            acc += m.timed_ms
        return acc / len(full)
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    m.timed_ms = None
    m.optimizer.grad.zero_()
    res["launch_us"] = {k: round(float(v) * 1e3, 2) for k, v in zip(GROUPS, per)}
    res["step_kernels_us"] = round(float(per.sum()) * 1e3, 2)
    rows, fp = _hip.caser_rows(L, nh), _hip.caser_fp(L, nv, nh)
    res["conv_product_flop"] = 2 * b * L * 64 * rows
    res["fc1_product_flop"] = 2 * b * fp * 64
    res["conv_matrix_peak_frac"] = round(res["conv_product_flop"] / (per[0] * 1e-3) / FP32_MATRIX_PEAK, 5)
    res["fc1_matrix_peak_frac"] = round(res["fc1_product_flop"] / (per[1] * 1e-3) / FP32_MATRIX_PEAK, 5)
    # the torch-ROCm restatement of the reference's step, same session
    ref = TorchStep(nU, nI + 1, e, L, T, nv, nh, 0.5, 1e-3, 1e-6, dev)
    bt = [(ep.cols[0][a:a + b].long(), ep.cols[1][a:a + b].long(), torch.cat([ep.cols[2][a:a + b], ep.cols[3][a:a + b]], 1).long())
          for a in full[:8]]
    res["torch_step_ms"] = _spread([_time(lambda: [ref.step(*x) for x in bt], 2) / len(bt) for _ in range(args.repeats)])
    res["speedup_vs_torch"] = round(res["torch_step_ms"]["median"] / min(res["step_ms_dense"]["median"], res["step_ms_blocked"]["median"]), 2)
    del ref, bt
    torch.cuda.empty_cache()
    # query rows of all users, the fused evaluation at 128 columns and the dense score rows of the same users
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"], te_ptr=te_ptr,
                   te_items=ds["test_item"])

    def queries():
        m._q_current = False
        m.predict_factors()
    res["queries_ms_all_users"] = _spread([_time(queries, 3) for _ in range(args.repeats)])
    n_eval = min(nU, args.eval_users)
    users = np.arange(n_eval, dtype=np.int32)
    m.predict_factors()
    ms = _spread([_time(lambda: ev.per_user_rows(m, users)) for _ in range(args.repeats)])
    res["eval_users"] = n_eval
    res["eval_ms"] = ms
    res["eval_users_per_s"] = round(n_eval / (ms["median"] * 1e-3))

    class ScoreRowsOnly(object):                     # the dense score-row route of the same model and users
        num_items = m.num_items

        def predict(self, users):
            raise NotImplementedError

        def score_rows(self, d_users, out):
            return m.score_rows(d_users, out)
    dense = ScoreRowsOnly()
    ev.per_user_rows(dense, users)
    ms = _spread([_time(lambda: ev.per_user_rows(dense, users)) for _ in range(args.repeats)])
    res["eval_dense_ms"] = ms
    res["eval_dense_users_per_s"] = round(n_eval / (ms["median"] * 1e-3))
    del m, dense
    torch.cuda.empty_cache()
    # HGN's fused 64-column evaluation on the same data, same session
    h = HGN.detached(nU, nI, dict(lr=1e-3, reg=1e-3, seq_L=L, seq_T=T, embed_size=e, batch_size=b), win_host)
    h.predict_factors()
    ms = _spread([_time(lambda: ev.per_user_rows(h, users)) for _ in range(args.repeats)])
    res["hgn_eval_ms"] = ms
    res["hgn_eval_users_per_s"] = round(n_eval / (ms["median"] * 1e-3))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
