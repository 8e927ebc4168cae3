"""Timing of BM3 at bench scale on one GPU:

    python tools/bm3_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --layers 1,2 --batch 2048
                                --img_dim 4096 --txt_dim 384 --steps 10 --repeats 3 --eval_users 65536 --torch_steps 2
                                --out profiles/bm3_timing.json]

Data: bench.synth_dataset (imported, not copied) with seeded random item features; a batch is a run of consecutive train
pairs of a random permutation.  Reported per ``--layers`` value, as one JSON line, medians of ``--repeats`` repeats: ms per
training step (skr_bm3_step + the dense Adam launch, masks drawn on the device), each launch group of the step alone by HIP
events (skr_bm3_step_timed), skr_bm3_project alone per modality, the Adam launch against the HBM peak with the feature tables'
share measured on its own (the same launch over the tables' slices of the flat buffer), skr_bm3_queries, and evaluation
users/s through the evaluator's fused top-K path (the propagation of the current parameters included).

Beside it, in the same session: the reference's training step written with torch-ROCm ops (what a user of the reference gets
on this GPU): torch.sparse.mm per layer, nn.Linear on the WHOLE feature tables, F.dropout of the four full tables,
F.cosine_similarity, torch.norm, backward and torch.optim.Adam over every tensor -- restated here from the model's equations
(recommender/BM3.py:142-204)."""
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
GROUPS = ("forward_plan_runs", "addh_sumsq", "project", "batch_reduce_loss", "project_backward", "reg_fill_seg_add", "backward_plan_runs")


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
        nnz = int(m.adj.rowptr[-1])
        self.P = {k: v.clone().requires_grad_(True) for k, v in m.parameters().items()}
        rows = torch.repeat_interleave(torch.arange(nu, device=m.device), m.adj.rowptr[1:] - m.adj.rowptr[:-1])
        cols = m.adj.col.long()[:nnz]
        rows_t = torch.repeat_interleave(torch.arange(ni, device=m.device), m.adj_t.rowptr[1:] - m.adj_t.rowptr[:-1])
        cols_t = m.adj_t.col.long()[:nnz]
        idx = torch.cat([torch.stack([rows, cols + nu]), torch.stack([rows_t + nu, cols_t])], 1)
        self.A = torch.sparse_coo_tensor(idx, torch.cat([m.adj.val[:nnz], m.adj_t.val[:nnz]]), (nu + ni, nu + ni)).coalesce()
        self.nu, self.ni, self.cfg = nu, ni, m.config
        self.opt = torch.optim.Adam(list(self.P.values()), lr=lr)

    def step(self, users, items):
        cfg, P, F = self.cfg, self.P, torch.nn.functional
        h = P["item_id_embedding.weight"]
        ego = torch.cat([P["user_embedding.weight"], h], 0)
        layers = [ego]
        for _ in range(cfg.n_layers):
            ego = torch.sparse.mm(self.A, ego)
            layers.append(ego)
        M = torch.stack(layers, 1).mean(1)
        Mu, Mi = M[:self.nu], M[self.nu:] + h
        pred = lambda x: F.linear(x, P["predictor.weight"], P["predictor.bias"])     # noqa: E731
        online = {}
        for key in ("text", "image"):
            if key + "_trs.weight" in P:
                online[key] = F.linear(P[key + "_embedding.weight"], P[key + "_trs.weight"], P[key + "_trs.bias"])
        with torch.no_grad():
            tu, ti = F.dropout(Mu.clone(), cfg.dropout), F.dropout(Mi.clone(), cfg.dropout)
            tx = {k: F.dropout(v.clone(), cfg.dropout) for k, v in online.items()}
        cos = lambda a, b: 1 - F.cosine_similarity(a, b, dim=-1).mean()              # noqa: E731
        ti_b = ti[items]
        loss = cos(pred(Mu)[users], ti_b) + cos(pred(Mi)[items], tu[users]) + cfg.reg * (torch.norm(Mu) + torch.norm(Mi)) / self.ni
        for k, v in online.items():
            p = pred(v)[items]
            loss = loss + cfg.cl_weight * (cos(p, ti_b) + cos(p, tx[k][items]))
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def run_layers(args, ds, img, txt, L, dev):
    from skrec.recommender.BM3 import BM3
    from skrec.utils.py.evaluator import RankingEvaluator
    nU, nI, B = args.users, args.items, args.batch
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    res = dict(layers=L)
    cfg = dict(lr=1e-3, reg=0.1, embed_dim=args.dim, n_layers=L, dropout=0.3, cl_weight=2.0, batch_size=B)
    torch.manual_seed(1)
    np.random.seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = BM3.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]), img=img, txt=txt, seed=2021)
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pick = torch.randperm(int(ds["items"].numel()), generator=g, device=dev)[:B * args.steps]
    us, ps = ds["users"][pick].int(), ds["items"][pick].int()
    batches = [(us[s:s + B].contiguous(), ps[s:s + B].contiguous()) for s in range(0, pick.numel() - B + 1, B)]

    def epoch():
        for b in batches:
            m.train_step(*b)
        m.step_losses = []
    res["steps"] = len(batches)
    res["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    print(json.dumps(dict(layers=L, step_ms=res["step_ms"])), flush=True)
    ms = (ctypes.c_float * _hip.SKR_BM3_GROUPS)()

    def timed():
        acc = np.zeros(len(GROUPS))
        for b in batches[:8]:
            m.gradient_step(*b, h_ms=ms)
            acc += np.array(list(ms))
        return acc / min(8, len(batches))
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    res["group_ms"] = {k: round(float(v), 4) for k, v in zip(GROUPS, per)}
    res["step_kernels_ms"] = round(float(per.sum()), 4)
    Lb = _hip.lib()
    Y = torch.empty((B, 64), device=dev)
    res["project_ms"] = {}
    for key in ("img", "txt"):
        if m.feat_dim[key]:
            t, e = m._off[key]

            def project():
                _hip.check(Lb.skr_bm3_project(_hip.ptr(m._flat[e:]), nI, m.feat_dim[key], m.feat_ld[key], _hip.ptr(m._flat[t:]),
                                              _hip.ptr(batches[0][1]), B, _hip.ptr(Y), _hip.stream()))
            res["project_ms"][key] = round(_median(lambda: _time(project, 5), args.repeats), 4)
    # the Adam launch: the whole flat buffer, and the feature tables' slices alone
    opt = m.optimizer
    ms_adam = _median(lambda: _time(opt.step, 3), args.repeats)
    n_par = opt.flat.numel()
    res["adam"] = dict(n_params=n_par, ms=round(ms_adam, 4), hbm_frac=round(32 * n_par / (ms_adam * 1e-3) / HBM_PEAK, 4))
    n_feat, ms_feat = 0, 0.0
    for key in ("img", "txt"):
        if m.feat_dim[key]:
            e, cnt = m._off[key][1], nI * m.feat_ld[key]

            def table():
                _hip.check(Lb.skr_adam_step(_hip.ptr(opt.flat[e:]), _hip.ptr(opt.grad[e:]), _hip.ptr(opt.m[e:]), _hip.ptr(opt.v[e:]), cnt, opt.lr,
                                            0.9, 0.999, opt.eps, max(opt.t, 1), 1, None, _hip.stream()))
            n_feat += cnt
            ms_feat += _median(lambda: _time(table, 3), args.repeats)
    res["adam"]["feature_tables"] = dict(n_params=n_feat, ms=round(ms_feat, 4), share_of_step=round(ms_feat / res["step_ms"], 4))
    m.propagate()

    def queries():
        _hip.check(Lb.skr_bm3_queries(_hip.ptr(m._pred), _hip.ptr(m.pooled), nU, nI, _hip.ptr(m._Qu), _hip.ptr(m._Qi), _hip.stream()))
    res["queries_ms"] = round(_median(lambda: _time(queries, 5), args.repeats), 4)
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
    if args.torch_steps > 0:
        try:
            ref = TorchStep(m, 1e-3)
            bs = [tuple(t.long() for t in b) for b in batches[:args.torch_steps]]
            res["torch_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(*b) for b in bs]) / len(bs), args.repeats), 4)
            res["speedup_vs_torch"] = round(res["torch_step_ms"] / res["step_ms"], 2)
            del ref
        except RuntimeError as e:        # e.g. out of memory
            res["torch_step_error"] = str(e)[:200]
    del m
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", default="1,2")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--img_dim", type=int, default=4096)
    ap.add_argument("--txt_dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--torch_steps", type=int, default=2, help="0 skips the torch-ROCm restatement")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    img = torch.randn((args.items, args.img_dim), generator=g, device=dev) if args.img_dim else None
    txt = torch.randn((args.items, args.txt_dim), generator=g, device=dev) if args.txt_dim else None
    res = dict(users=args.users, items=args.items, interactions=int(ds["items"].numel()), dim=args.dim, batch=args.batch, img_dim=args.img_dim,
               txt_dim=args.txt_dim, repeats=args.repeats, device=torch.cuda.get_device_name(0), runs=[])
    for L in (int(x) for x in args.layers.split(",")):
        res["runs"].append(run_layers(args, ds, img, txt, L, dev))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
