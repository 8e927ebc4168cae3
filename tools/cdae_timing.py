"""Timing of CDAE at bench scale on one GPU:

    python tools/cdae_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --num_neg 5 --batches 256,1024
                                 --steps 200 --repeats 3 --eval_users 65536 --out FILE.json]

Data: bench.synth_dataset (imported, not copied); a batch is a run of consecutive users of a random permutation of the
users with a training item.  Reported, as one JSON line, medians of ``--repeats`` repeats: ms per training step through
``train_epoch`` with the blocked Adam (``SKR_ADAM_BLOCK`` steps per block) and with one dense Adam launch per step -- both
include the layout preparation and the exact sampling --, the step's three launches alone by HIP events
(skr_cdae_step_timed), the layout preparation per step amortised over its block and the sampler's share of it, pairs and
distinct items per step, skr_cdae_queries over all users, and evaluation users/s through the evaluator's fused top-K path."""
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

LAUNCHES = ("user_side", "item_side", "finish")


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _median(fn, repeats):
    return float(np.median([fn() for _ in range(repeats)]))


def batch_leg(m, train_users, B, args, dev):
    out = {}
    rng = np.random.default_rng(7)
    perm = rng.permutation(train_users)[:B * args.steps].astype(np.int32)
    batches = [perm[s:s + B] for s in range(0, len(perm) - B + 1, B)]
    n = len(batches)
    out["steps"] = n
    block = m.adam_block
    m.train_epoch(batches[:block])                                    # warm-up: allocations, the side stream
    out["adam_block"] = block
    out["step_ms_blocked"] = round(_median(lambda: _time(lambda: m.train_epoch(batches)) / n, args.repeats), 4)
    m.adam_block = 1
    m.train_epoch(batches[:4])
    out["step_ms_dense"] = round(_median(lambda: _time(lambda: m.train_epoch(batches)) / n, args.repeats), 4)
    m.adam_block = block
    # the layout of a block (sampling included), amortised per step, and the sampler's share
    blk = batches[:block]

    sampler = m._sampler()
    draw = sampler.sample_epoch_exact_counts

    def prep():
        ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]

        def timed_draw(*a):
            ev[0].record()
            draw(*a)
            ev[1].record()
        sampler.sample_epoch_exact_counts = timed_draw              # shadows the method for this call only
        try:
            t = _time(lambda: m._prepare(blk))
        finally:
            del sampler.sample_epoch_exact_counts
        return t / len(blk), ev[0].elapsed_time(ev[1]) / len(blk)
    both = np.median(np.array([prep() for _ in range(args.repeats)]), axis=0)
    out["prepare_ms_per_step"], out["sampling_ms_per_step"] = round(float(both[0]), 4), round(float(both[1]), 4)
    Bk = m._prepare(blk)
    out["pairs_per_step"] = int(np.diff(Bk.pstart).mean())
    out["distinct_items_per_step"] = int(np.diff(Bk.jstart).mean())
    out["adam_blocks_per_step"] = int(Bk.per)
    # each launch of the step alone
    loss = torch.empty(2, device=dev)
    ms = np.zeros(len(LAUNCHES), np.float32)

    def timed():
        acc = np.zeros(len(LAUNCHES))
        for s in range(len(blk)):
            _hip.check(m._launch(Bk, s, _hip.ptr(loss), ms.ctypes.data))
            acc += ms
        m.optimizer.grad.zero_()
        return acc / len(blk)
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    out["launch_us"] = {k: round(float(v) * 1e3, 2) for k, v in zip(LAUNCHES, per)}
    out["step_kernels_us"] = round(float(per.sum()) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--num_neg", type=int, default=5)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    from skrec.recommender.CDAE import CDAE
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    nU, nI = args.users, args.items
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    train_users = torch.nonzero(counts > 0).view(-1).cpu().numpy()
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), dim=args.dim, num_neg=args.num_neg,
               repeats=args.repeats, device=torch.cuda.get_device_name(0))
    cfg = dict(lr=1e-3, reg=1e-3, hidden_dim=args.dim, dropout=0.5, num_neg=args.num_neg, batch_size=1024)
    m = CDAE.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]), seed=1)
    res["parameters"] = int(m._flat.numel())
    for B in (int(b) for b in args.batches.split(",")):
        res[f"batch_{B}"] = batch_leg(m, train_users, B, args, dev)
        print(json.dumps({f"batch_{B}": res[f"batch_{B}"]}), flush=True)
    # query rows of all users, and the fused evaluation
    L, st = _hip.lib(), _hip.stream()

    def queries():
        _hip.check(L.skr_cdae_queries(_hip.ptr(m._en), _hip.ptr(m._off), _hip.ptr(m._user), _hip.ptr(m._rowptr), _hip.ptr(m._items),
                                      None, nU, nU, nI, m.d, m.act, _hip.ptr(m._Q), st))
    queries()
    res["queries_all_users_ms"] = round(_median(lambda: _time(queries), args.repeats), 4)
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"], te_ptr=te_ptr,
                   te_items=ds["test_item"])
    n_eval = min(nU, args.eval_users)
    users = np.arange(n_eval, dtype=np.int32)
    m.predict_factors()
    ev.per_user_rows(m, users)
    ms = _median(lambda: _time(lambda: ev.per_user_rows(m, users)), args.repeats)
    res["eval_users"] = n_eval
    res["eval_users_per_s"] = round(n_eval / (ms * 1e-3))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
