"""Timing of the sequential recommenders (FPMC, TransRec, HGN) at bench scale on one GPU:

    python tools/seq_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --batch 1024 --steps 200]
                               [--models FPMC,TransRec,HGN --seq_L 5 --seq_T 3 --out FILE.json]

Data: bench.synth_dataset (imported, not copied); a user's interactions in their stored order stand in for time, so the
triples (u, last, pos) are consecutive pairs of a user's row, shuffled once; negatives are uniform item ids (no exclusion:
timing only).  Reported, as one JSON line: ms per training step for both models with one dense skr_adam_step per step and
with the temporally blocked Adam (SKR_ADAM_BLOCK, default 32); each kernel alone (the step, the dense Adam, the score
rows) with its bytes over time against the 8 TB/s HBM peak; evaluation users/s through the evaluator's device-score path
(skr_seq_scores -> skr_mask_train -> skr_eval_scores).

HGN (windows of seq_L consecutive items of a user's row, left-padded at the row's start, the next seq_T items as
positives): ms per step with one dense skr_adam_step_wd per step and blocked; skr_hgn_step alone; the dense _wd launch
alone next to skr_adam_step on the same buffer, the two alternated in the same session with the spread of the repeats;
evaluation users/s through the evaluator's fused top-K path with the skr_hgn_queries launch timed on its own, next to
the same fused evaluation of the same values handed over as plain factor tables (what BPRMF hands the evaluator)."""
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


def hgn_instances(ds, n_items, dev, seed, L, T, n_want):
    """n_want shuffled instances (u, window [n, L], positives [n, T], negatives [n, T]) and every user's last window"""
    rowptr, items, users = ds["rowptr"], ds["items"], ds["users"]
    n, nU = items.numel(), int(rowptr.numel()) - 1
    pos_in_row = torch.arange(n, device=dev) - rowptr[:-1][users.long()]
    row_end = rowptr[1:][users.long()]
    ok = (pos_in_row >= 1) & (torch.arange(n, device=dev) + T <= row_end)
    idx = torch.nonzero(ok).reshape(-1)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    idx = idx[torch.randperm(idx.numel(), generator=g, device=dev)[:n_want]]
    back = torch.arange(L, 0, -1, device=dev)                                  # L .. 1 items back
    win = items[(idx[:, None] - back[None]).clamp_(min=0)].int()
    win[back[None] > pos_in_row[idx][:, None]] = n_items                       # before the row's start: the padding item
    pos = items[idx[:, None] + torch.arange(T, device=dev)[None]].int()
    neg = torch.randint(0, n_items, (idx.numel(), T), generator=g, device=dev, dtype=torch.int32)
    last = rowptr[1:, None] - back[None]
    lw = items[last.clamp(0, max(n - 1, 0))].int()
    lw[last < rowptr[:-1, None]] = n_items
    lw[rowptr[1:] == rowptr[:-1]] = -1
    return [users[idx].int().contiguous(), win.contiguous(), pos.contiguous(), neg.contiguous()], lw.contiguous()


class _Factors(object):
    """plain factor tables for the evaluator's fused path: what BPRMF's predict_factors returns"""

    def __init__(self, U, V, b):
        self.f = (U, V, b)

    def predict_factors(self):
        return self.f


def _spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4))


def hgn_leg(nU, nI, ds, args, ev_state, dev):
    from skrec.recommender.HGN import HGN
    from skrec.utils.py.evaluator import RankingEvaluator
    L, T, b = args.seq_L, args.seq_T, args.batch
    cols, windows = hgn_instances(ds, nI, dev, 11, L, T, b * args.steps)
    out = dict(seq_L=L, seq_T=T, instances=int(cols[0].shape[0]))
    cfg = dict(lr=1e-3, reg=1e-3, seq_L=L, seq_T=T, embed_size=args.dim, batch_size=b)
    for label, blk in (("dense", "1"), ("blocked", os.environ.get("SKR_ADAM_BLOCK", "32"))):
        os.environ["SKR_ADAM_BLOCK"] = blk
        m = HGN.detached(nU, nI, cfg, windows.cpu().numpy())
        ep = _Epoch(cols, b, args.steps)
        runs = [_time(lambda: m.train_epoch(ep)) / len(ep.bounds) for _ in range(3)]
        out[f"step_ms_{label}"] = _spread(runs)
        out[f"adam_block_{label}"] = m.adam_block
    ep = _Epoch(cols, b, args.steps)
    S = _hip.SKR_LOSS_SLOTS
    loss = torch.zeros(2 * S, device=m.device)
    st = _hip.stream()
    cu, cl, cp, cn = (c.data_ptr() for c in ep.cols)
    nfull = len(ep.bounds) - 1
    ms = _time(lambda: [m._step_launch(cu + 4 * a, cl + 4 * L * a, cp + 4 * T * a, cn + 4 * T * a, b, loss.data_ptr(), st)
                        for a in range(0, b * nfull, b)]) / nfull
    # bytes per instance: 1 + L + 2T rows read, as many scattered (read-modify-write at the L2), ids and b2 words
    step_bytes = b * ((1 + L + 2 * T) * 256 * 2 + 4 * (1 + L + 2 * T) + 16 * T) + 2 * 256 * 4 * _hip.hgn_gate_floats(L)
    out["step_kernel_us"] = round(ms * 1e3, 2)
    out["step_kernel_bw_frac"] = round(step_bytes / (ms * 1e-3) / HBM_PEAK, 4)
    m.optimizer.grad.zero_()
    o = m.optimizer
    n_par = o.flat.numel()
    head = (_hip.ptr(o.flat), _hip.ptr(o.grad), _hip.ptr(o.m), _hip.ptr(o.v), n_par, o.lr, o.betas[0], o.betas[1], o.eps)
    lib = _hip.lib()

    def adam_plain():
        o.t += 1
        _hip.check(lib.skr_adam_step(*head, o.t, 1, None, st))

    def adam_wd():
        o.t += 1
        _hip.check(lib.skr_adam_step_wd(*head, o.weight_decay, o.t, 1, None, st))
    plain, wd = [], []
    for _ in range(5):                       # alternated: the spread of either is the margin of the comparison
        plain.append(_time(adam_plain, 20))
        wd.append(_time(adam_wd, 20))
    out["n_params"] = n_par
    out["adam_dense_ms"] = _spread(plain)
    out["adam_dense_wd_ms"] = _spread(wd)
    out["adam_dense_wd_bw_frac"] = round(32 * n_par / (_spread(wd)["median"] * 1e-3) / HBM_PEAK, 4)
    # evaluation: the fused top-K path, the query launch on its own, and plain factors of the same shapes
    n_eval = min(nU, args.eval_users)
    users = np.arange(n_eval, dtype=np.int32)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = ev_state

    def queries():
        m._q_current = False
        m.predict_factors()
    out["queries_ms_all_users"] = _spread([_time(queries, 5) for _ in range(3)])

    def evaluate():
        m._q_current = False                 # one skr_hgn_queries launch per evaluate()
        ev.per_user_rows(m, users)
    Q, W2, b2 = m.predict_factors()          # the same values as plain factor tables: the difference is the query launch
    plainf = _Factors(Q.clone(), W2, b2)
    e_h, e_p = [], []
    for _ in range(3):
        e_h.append(_time(evaluate))
        e_p.append(_time(lambda: ev.per_user_rows(plainf, users)))
    out["eval_users"] = n_eval
    out["eval_users_per_s"] = round(n_eval / (_spread(e_h)["median"] * 1e-3))
    out["eval_ms"] = _spread(e_h)
    out["eval_plain_factors_users_per_s"] = round(n_eval / (_spread(e_p)["median"] * 1e-3))
    out["eval_plain_factors_ms"] = _spread(e_p)
    # the two same-session comparisons
    sp, sw = out["adam_dense_ms"], out["adam_dense_wd_ms"]
    out["adam_wd_over_plain"] = dict(ratio_of_medians=round(sw["median"] / sp["median"], 4),
                                     plain_spread_rel=round((sp["max"] - sp["min"]) / sp["median"], 4))
    out["eval_minus_plain_factors_ms"] = round(out["eval_ms"]["median"] - out["eval_plain_factors_ms"]["median"], 4)
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
    ap.add_argument("--models", default="FPMC,TransRec,HGN")
    ap.add_argument("--seq_L", type=int, default=5)
    ap.add_argument("--seq_T", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    models = args.models.split(",")
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
        if cls.__name__ in models:
            res[cls.__name__] = model_leg(cls, nU, args.items, cols, last_item, args, ev_state)
            torch.cuda.empty_cache()
    if "HGN" in models:
        del cols, last_item
        torch.cuda.empty_cache()
        res["HGN"] = hgn_leg(nU, args.items, ds, args, ev_state, dev)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
