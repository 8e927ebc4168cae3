"""Timing of the sequential recommenders (FPMC, TransRec) at bench scale on one GPU:

    python tools/seq_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --batch 1024 --steps 200]

Data: bench.synth_dataset (imported, not copied); a user's interactions in their stored order stand in for time, so the
triples (u, last, pos) are consecutive pairs of a user's row, shuffled once; negatives are uniform item ids (no exclusion:
timing only).  Reported, as one JSON line: ms per training step for both models with one dense skr_adam_step per step and
with the temporally blocked Adam (SKR_ADAM_BLOCK, default 32); each kernel alone (the step, the dense Adam, the score
rows) with its bytes over time against the 8 TB/s HBM peak; evaluation users/s through the evaluator's device-score path
(skr_seq_scores -> skr_mask_train -> skr_eval_scores)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "scikit-recommender_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench import synth_dataset  # noqa: E402
from skrec import _hip  # noqa: E402

HBM_PEAK = 8.0e12


class _Epoch(object):
    """K steps of (u, last, pos, neg) columns, the data_iter contract of SeqPairwiseRecommender.train_epoch"""

    def __init__(self, cols, batch_size, n_steps):
        n = min(cols[0].numel(), batch_size * n_steps)
        self.cols = [c[:n].contiguous() for c in cols]
        self.batch_size = batch_size
        self.bounds = [(a, min(a + batch_size, n)) for a in range(0, n, batch_size)]

    def epoch_columns(self):
        return self.cols, self.bounds


def _time(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                   # warm-up
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def triples(ds, n_items, dev, seed):
    rowptr, items = ds["rowptr"], ds["items"]
    users = ds["users"]
    n = items.numel()
    first = torch.zeros(n, dtype=torch.bool, device=dev)
    first[rowptr[:-1][rowptr[:-1] < rowptr[1:]]] = True
    keep = ~first                                           # positions with a previous item of the same user
    idx = torch.nonzero(keep).reshape(-1)
    u, last, pos = users[idx], items[idx - 1], items[idx]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    perm = torch.randperm(idx.numel(), generator=g, device=dev)
    neg = torch.randint(0, n_items, (idx.numel(),), generator=g, device=dev, dtype=torch.int32)
    last_item = torch.full((int(rowptr.numel()) - 1,), -1, dtype=torch.int32, device=dev)
    nonempty = rowptr[1:] > rowptr[:-1]
    last_item[nonempty] = items[rowptr[1:][nonempty] - 1]
    return [c[perm].int().contiguous() for c in (u, last, pos)] + [neg[perm].contiguous()], last_item


def model_leg(cls, nU, nI, cols, last_item, args, ev_state):
    from skrec.utils.py.evaluator import RankingEvaluator
    out = {}
    cfg = dict(lr=1e-3, reg=1e-3, embed_size=args.dim, batch_size=args.batch)
    for label, blk in (("dense", "1"), ("blocked", os.environ.get("SKR_ADAM_BLOCK", "32"))):
        os.environ["SKR_ADAM_BLOCK"] = blk
        m = cls.detached(nU, nI, cfg, last_item.cpu().numpy())
        ep = _Epoch(cols, args.batch, args.steps)
        ms = _time(lambda: m.train_epoch(ep)) / len(ep.bounds)
        out[f"step_ms_{label}"] = round(ms, 4)
        out[f"adam_block_{label}"] = m.adam_block
    # kernels alone
    ep = _Epoch(cols, args.batch, args.steps)
    S = _hip.SKR_LOSS_SLOTS
    loss = torch.zeros(2 * S, device=m.device)
    st = _hip.stream()
    cu, cl, cp, cn = (c.data_ptr() for c in ep.cols)
    b = args.batch
    ms = _time(lambda: [m._step_launch(cu + 4 * a, cl + 4 * a, cp + 4 * a, cn + 4 * a, b, loss.data_ptr(), st)
                        for a in range(0, b * (len(ep.bounds) - 1), b)]) / (len(ep.bounds) - 1)
    dp = m.dp
    # bytes per triple: FPMC reads 6 rows and scatters 6 rows; TransRec reads 4 rows (+T, cached) and scatters 4, + 2 biases
    rows = 6 if cls.__name__ == "FPMC" else 4
    step_bytes = b * (rows * dp * 4 * 2 + 16)
    out["step_kernel_us"] = round(ms * 1e3, 2)
    out["step_kernel_bw_frac"] = round(step_bytes / (ms * 1e-3) / HBM_PEAK, 4)
    o = m.optimizer
    n_par = o.flat.numel()

    def adam():
        o.t += 1
        _hip.check(_hip.lib().skr_adam_step(_hip.ptr(o.flat), _hip.ptr(o.grad), _hip.ptr(o.m), _hip.ptr(o.v), n_par, o.lr,
                                            o.betas[0], o.betas[1], o.eps, o.t, 1, None, st))
    ms = _time(adam, 20)
    out["n_params"] = n_par
    out["adam_dense_ms"] = round(ms, 4)
    out["adam_dense_bw_frac"] = round(32 * n_par / (ms * 1e-3) / HBM_PEAK, 4)
    # score rows alone and the whole device-score evaluation
    n_eval = min(nU, args.eval_users)
    users = torch.arange(n_eval, dtype=torch.int32, device=m.device)
    chunk = max(1, (256 << 20) // (4 * nI))
    sc = torch.empty((chunk, nI), dtype=torch.float32, device=m.device)
    ms = _time(lambda: m.score_rows(users[:chunk], sc), 5)
    n_q = 2 if cls.__name__ == "FPMC" else 1
    sbytes = chunk * nI * 4 + nI * dp * 4 * n_q * ((chunk + 15) // 16)
    out["score_rows_ms_per_chunk"] = round(ms, 4)
    out["score_chunk_users"] = chunk
    out["score_rows_users_per_s"] = round(chunk / (ms * 1e-3))
    out["score_rows_bw_frac_incl_L2"] = round(sbytes / (ms * 1e-3) / HBM_PEAK, 4)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = ev_state
    ms = _time(lambda: ev.per_user_rows(m, users.cpu().numpy()))
    out["eval_users"] = n_eval
    out["eval_users_per_s"] = round(n_eval / (ms * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--eval_users", type=int, default=65536)
    args = ap.parse_args()
    from skrec.recommender.FPMC import FPMC
    from skrec.recommender.TransRec import TransRec
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    cols, last_item = triples(ds, args.items, dev, 7)
    nU = args.users
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    ev_state = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"],
                    te_ptr=te_ptr, te_items=ds["test_item"])
    res = dict(users=nU, items=args.items, interactions=int(ds["items"].numel()), triples=int(cols[0].numel()),
               dim=args.dim, batch=args.batch, steps=args.steps)
    for cls in (FPMC, TransRec):
        res[cls.__name__] = model_leg(cls, nU, args.items, cols, last_item, args, ev_state)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
