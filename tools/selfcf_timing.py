"""Timing of SelfCF at bench scale on one GPU:

    python tools/selfcf_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --layers 2 --batch 2048
                                   --steps 20 --repeats 3 --eval_users 65536 --torch_steps 2 --out FILE.json]

Data: bench.synth_dataset (imported, not copied); a batch is a run of consecutive train pairs of a random permutation.
Reported, as one JSON line, medians of ``--repeats`` repeats: ms per training step (skr_selfcf_keeps + skr_selfcf_step + the
dense Adam launch, rates from np.random.random(), masks drawn on the device), the keeps launch alone, each launch group of
the step alone by HIP events (skr_selfcf_step_timed), one dropped run of A and of A^T at keep rates 1.0 / 0.5 / 0.1 beside
skr_spmm_plan_run_ex on the same plan (the two alternated inside every repeat, min .. max of the repeats kept as the spread),
the Adam launch against the HBM peak, the query launch, and evaluation users/s through the evaluator's fused top-K path (the
propagation of the current parameters included).

Beside it, in the same session: the reference's training step written with torch-ROCm ops (what a user of the reference gets
on this GPU): the mask over the 2 nnz entries by torch.rand, a new sparse tensor per step, torch.sparse.mm per layer, F.dropout,
nn.Linear, F.cosine_similarity, backward and torch.optim.Adam -- restated here from the model's equations
(recommender/SelfCF.py:133-168, :205-233)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "scikit-recommender_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench import synth_dataset  # noqa: E402
from skrec import _hip  # noqa: E402

HBM_PEAK = 8.0e12
GROUPS = ("forward_dropped_runs", "batch_reduce_loss", "clear_rank_seg_add", "backward_dropped_runs")


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


def _median(fn, repeats):
    return float(np.median([fn() for _ in range(repeats)]))


class TorchStep(object):
    """the reference's step on torch-ROCm ops"""

    def __init__(self, m, lr):
        nu, ni = m.num_users, m.num_items
        self.P = {k: v.clone().requires_grad_(True) for k, v in m.parameters().items()}
        rows = torch.repeat_interleave(torch.arange(nu, device=m.device), m.adj.rowptr[1:] - m.adj.rowptr[:-1])
        cols = m.adj.col.long()[:m.nnz]
        rows_t = torch.repeat_interleave(torch.arange(ni, device=m.device), m.adj_t.rowptr[1:] - m.adj_t.rowptr[:-1])
        cols_t = m.adj_t.col.long()[:m.nnz]
        self.idx = torch.cat([torch.stack([rows, cols + nu]), torch.stack([rows_t + nu, cols_t])], 1)
        self.val = torch.cat([m.adj.val[:m.nnz], m.adj_t.val[:m.nnz]])
        self.N, self.cfg = nu + ni, m.config
        self.opt = torch.optim.Adam(list(self.P.values()), lr=lr)

    def step(self, users, items):
        cfg, P, F = self.cfg, self.P, torch.nn.functional
        rate = np.random.random()
        mask = torch.floor(1 - rate + torch.rand(self.val.numel(), device=self.val.device)).bool()
        A = torch.sparse_coo_tensor(self.idx[:, mask], self.val[mask], (self.N, self.N)) * (1. / (1 - rate))
        ego = torch.cat([P["user_emb"], P["item_emb"]], 0)
        layers = [ego]
        for _ in range(cfg.n_layers):
            ego = torch.sparse.mm(A, ego)
            layers.append(ego)
        M = torch.stack(layers, 1).mean(1)
        u, i = M[users], M[self.P["user_emb"].shape[0] + items]
        with torch.no_grad():
            tu, ti = F.dropout(u.clone(), cfg.dropout), F.dropout(i.clone(), cfg.dropout)
        reg = 0.5 * (u ** 2).sum() + 0.5 * (i ** 2).sum()
        pu, pi = F.linear(u, P["predictor.weight"], P["predictor.bias"]), F.linear(i, P["predictor.weight"], P["predictor.bias"])
        loss = -F.cosine_similarity(pu, ti, dim=-1).mean() / 2 - F.cosine_similarity(pi, tu, dim=-1).mean() / 2 + cfg.reg * reg
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def _ab(run_a, run_b, repeats, reps=5):
    """a and b alternated inside every repeat -> ((median, min, max) of a, the same of b)"""
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(_time(run_a, reps))
        tb.append(_time(run_b, reps))
    f = lambda t: dict(median=round(float(np.median(t)), 4), min=round(float(min(t)), 4), max=round(float(max(t)), 4))   # noqa: E731
    return f(ta), f(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--torch_steps", type=int, default=2, help="0 skips the torch-ROCm restatement")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    from skrec.recommender.SelfCF import SelfCF
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    nU, nI, B, L = args.users, args.items, args.batch, args.layers
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), dim=args.dim, layers=L, batch=B, repeats=args.repeats,
               device=torch.cuda.get_device_name(0))
    cfg = dict(lr=1e-3, reg=1e-3, embed_dim=args.dim, n_layers=L, dropout=0.5, batch_size=B)
    torch.manual_seed(1)
    np.random.seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = SelfCF.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]), seed=2021)
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    n_pairs = int(ds["items"].numel())
    pick = torch.randperm(n_pairs, generator=g, device=dev)[:B * args.steps]
    us, ps = ds["users"][pick].int(), ds["items"][pick].int()
    batches = [(us[s:s + B].contiguous(), ps[s:s + B].contiguous()) for s in range(0, pick.numel() - B + 1, B)]

    def epoch():
        for b in batches:
            m.train_step(*b)
        m.step_losses = []
    res["steps"] = len(batches)
    res["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    print(json.dumps(dict(step_ms=res["step_ms"])), flush=True)
    res["keeps_ms"] = round(_median(lambda: _time(lambda: m.edge_keeps(0.5), 5), args.repeats), 4)
    # each launch group alone (mean rate 0.5)
    ms = (ctypes.c_float * _hip.SKR_SELFCF_GROUPS)()

    def timed():
        acc = np.zeros(len(GROUPS))
        for b in batches[:8]:
            m.gradient_step(*b, rate=0.5, h_ms=ms)
            acc += np.array(list(ms))
        return acc / min(8, len(batches))
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    res["group_ms"] = {k: round(float(v), 4) for k, v in zip(GROUPS, per)}
    res["step_kernels_ms"] = round(float(per.sum()), 4)
    # one dropped run beside the plain run on the same plan, alternated
    X = m.X0
    Y = torch.empty_like(X)
    Lb = _hip.lib()

    def run(mat, xs, ys, keep, scale):
        ep = _hip.SpmmEpilogue()
        ep.mode, ep.Y, ep.accum_scale = _hip.EPI_PLAIN, _hip.ptr(ys), 1.0
        if keep is None:
            _hip.check(Lb.skr_spmm_plan_run_ex(mat._plan_handle(), _hip.ptr(xs), 64, ctypes.byref(ep), None, None, _hip.stream()))
        else:
            _hip.check(Lb.skr_spmm_plan_run_dropped(mat._plan_handle(), _hip.ptr(xs), 64, ctypes.byref(ep), _hip.ptr(keep), scale,
                                                    _hip.stream()))
    res["dropped_run_ms"] = {}
    for keep_rate in (1.0, 0.5, 0.1):
        f = m.edge_keeps(1.0 - keep_rate, step=99).clone() if keep_rate < 1.0 else torch.ones_like(m._keeps)
        for name, mat, xs, ys, k in (("A", m.adj, X[nU:], Y[:nU], f[0]), ("At", m.adj_t, X[:nU], Y[nU:], f[1])):
            d, p = _ab(lambda: run(mat, xs, ys, k, 1.0 / keep_rate), lambda: run(mat, xs, ys, None, 1.0), args.repeats)
            res["dropped_run_ms"][f"{name}_keep_{keep_rate}"] = dict(dropped=d, plain=p, kept_share=round(float(k.float().mean()), 4))
    print(json.dumps(dict(dropped_run_ms=res["dropped_run_ms"])), flush=True)
    ms_adam = _median(lambda: _time(m.optimizer.step, 5), args.repeats)
    n_par = m.optimizer.flat.numel()
    res["adam"] = dict(n_params=n_par, ms=round(ms_adam, 4), hbm_frac=round(32 * n_par / (ms_adam * 1e-3) / HBM_PEAK, 4))
    m.propagate()

    def queries():
        _hip.check(Lb.skr_selfcf_queries(_hip.ptr(m._pred), _hip.ptr(m.pooled), nU, nI, _hip.ptr(m._Q), _hip.ptr(m._item_bias),
                                         _hip.ptr(m._user_const), _hip.stream()))
    res["queries_ms"] = round(_median(lambda: _time(queries, 5), args.repeats), 4)
    # evaluation through the fused top-K path: the propagation of the current parameters, the queries, then the ranking
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"], te_ptr=te_ptr,
                   te_items=ds["test_item"])
    n_eval = min(nU, args.eval_users)
    users = np.arange(n_eval, dtype=np.int32)
    ms_ev = _median(lambda: _time(lambda: ev.per_user_rows(m, users)), args.repeats)
    res["eval_users"] = n_eval
    res["eval_users_per_s"] = round(n_eval / (ms_ev * 1e-3))
    print(json.dumps(res), flush=True)
    # the torch-ROCm restatement of the reference's step, same session
    if args.torch_steps > 0:
        try:
            ref = TorchStep(m, 1e-3)
            bs = [tuple(t.long() for t in b) for b in batches[:args.torch_steps]]
            res["torch_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(*b) for b in bs]) / len(bs), args.repeats), 4)
            res["speedup_vs_torch"] = round(res["torch_step_ms"] / res["step_ms"], 2)
        except RuntimeError as e:        # e.g. out of memory
            res["torch_step_error"] = str(e)[:200]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
