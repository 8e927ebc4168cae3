"""Timing of FREEDOM at bench scale on one GPU:

    python tools/freedom_timing.py [--users 1000000 --items 100000 --inter 48000000 --batch 2048 --img_dim 4096 --txt_dim 384
                                    --regs 0,1e-3 --steps 10 --repeats 3 --eval_users 65536 --torch_steps 2
                                    --out profiles/freedom_timing.json]

Data: bench.synth_dataset (imported, not copied) with seeded random item features, as tools/bm3_timing.py; a batch is a run of
consecutive train pairs of a random permutation with uniform negatives.  The model's defaults (n_ui_layers 2, n_mm_layers 1,
knn_k 10, dropout 0.8).  Reported per ``--regs`` value, as one JSON line, medians of ``--repeats`` repeats: construction
(kNN lists and item graph included), ms per training step (skr_freedom_step + the dense Adam launch) on a pruned graph, each
launch group of the step alone by HIP events (skr_freedom_step_timed), the Adam launch, the per-epoch pruning split into keys /
select / compaction / the two plan analyses, one plain run of a pruned plan beside one of the full plan, and evaluation
users/s through the evaluator's fused top-K path (the propagation of the current parameters included).

Beside it, in the same session: the reference's training step written with torch-ROCm ops (torch.sparse.mm on the square pruned
matrix and on the item graph, nn.Linear on the WHOLE feature tables, logsigmoid, backward, torch.optim.Adam over every tensor:
recommender/FREEDOM.py:211-252), and its pruning draw: ``torch.multinomial`` refuses more than 2^24 categories, so it is timed
on the first 2^24 edge weights -- a third of this set -- and cannot run on the whole of it."""
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
GROUPS = ("ui_forward_plan_runs", "item_graph_runs", "clear_project", "batch_loss", "clear_rank_seg_add", "project_backward",
          "backward_plan_runs")


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


def _square(A, At, nu, ni, dev):
    nnz = A.nnz
    rows = torch.repeat_interleave(torch.arange(nu, device=dev), A.rowptr[1:] - A.rowptr[:-1])
    rows_t = torch.repeat_interleave(torch.arange(ni, device=dev), At.rowptr[1:] - At.rowptr[:-1])
    idx = torch.cat([torch.stack([rows, A.col.long()[:nnz] + nu]), torch.stack([rows_t + nu, At.col.long()[:nnz]])], 1)
    return torch.sparse_coo_tensor(idx, torch.cat([A.val[:nnz], At.val[:nnz]]), (nu + ni, nu + ni)).coalesce()


class TorchStep(object):
    """the reference's step on torch-ROCm ops"""

    def __init__(self, m, lr):
        nu, ni, dev = m.num_users, m.num_items, m.device
        self.P = {k: v.clone().requires_grad_(True) for k, v in m.parameters().items()}
        self.A = _square(m.adj_train, m.adj_train_t, nu, ni, dev)
        S = m.mm_adj
        rows = torch.repeat_interleave(torch.arange(ni, device=dev), S.rowptr[1:] - S.rowptr[:-1])
        self.S = torch.sparse_coo_tensor(torch.stack([rows, S.col.long()[:S.nnz]]), S.val[:S.nnz], (ni, ni)).coalesce()
        self.nu, self.cfg = nu, m.config
        self.opt = torch.optim.Adam(list(self.P.values()), lr=lr)

    def step(self, users, pos, neg):
        cfg, P, F = self.cfg, self.P, torch.nn.functional
        h = P["item_id_embedding.weight"]
        for _ in range(cfg.n_mm_layers):
            h = torch.sparse.mm(self.S, h)
        ego = torch.cat([P["user_embedding.weight"], P["item_id_embedding.weight"]], 0)
        layers = [ego]
        for _ in range(cfg.n_ui_layers):
            ego = torch.sparse.mm(self.A, ego)
            layers.append(ego)
        M = torch.stack(layers, 1).mean(1)
        Mu, Mi = M[:self.nu], M[self.nu:] + h
        bpr = lambda u, p, q: -F.logsigmoid((u * p).sum(1) - (u * q).sum(1)).mean()      # noqa: E731
        loss = bpr(Mu[users], Mi[pos], Mi[neg])
        modal = 0.0
        for key in ("text", "image"):
            if key + "_trs.weight" in P:
                feats = F.linear(P[key + "_embedding.weight"], P[key + "_trs.weight"], P[key + "_trs.bias"])
                modal = modal + bpr(Mu[users], feats[pos], feats[neg])
        loss = loss + cfg.reg * modal
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def run_reg(args, ds, img, txt, reg, dev):
    from skrec.recommender.FREEDOM import FREEDOM
    from skrec.utils.py.evaluator import RankingEvaluator
    nU, nI, B = args.users, args.items, args.batch
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    res = dict(reg=reg)
    cfg = dict(lr=1e-3, reg=reg, batch_size=B)
    torch.manual_seed(1)
    np.random.seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = FREEDOM.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]), img=img, txt=txt, seed=2021)
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    L, st, nnz = _hip.lib(), _hip.stream, m._nnz
    # ---- the pruning of one epoch, part by part
    n_keep = int(nnz * (1. - m.config.dropout))
    keys = torch.empty(nnz, dtype=torch.float32, device=dev)
    keep = torch.empty(nnz, dtype=torch.uint8, device=dev)
    ws = int(L.skr_freedom_select_workspace(nnz))
    work = torch.empty(ws, dtype=torch.uint8, device=dev)

    def do_keys():
        _hip.check(L.skr_freedom_keys(_hip.ptr(m.edge_w), nnz, 2021, 0, _hip.ptr(keys), st()))

    def do_select():
        _hip.check(L.skr_freedom_select(_hip.ptr(keys), nnz, n_keep, _hip.ptr(keep), _hip.ptr(work), ws, st()))
    prune = dict(nnz=nnz, n_keep=n_keep)
    prune["keys_ms"] = round(_median(lambda: _time(do_keys, 3), args.repeats), 4)
    prune["select_ms"] = round(_median(lambda: _time(do_select, 3), args.repeats), 4)
    pairs = []

    def do_compact():
        pairs.append(m.pruned_pair(keep))
    prune["compaction_ms"] = round(_median(lambda: _time(do_compact), args.repeats), 4)
    A1, A1t = pairs[-1]
    del pairs[:-1]

    def analyses():
        t0 = time.perf_counter()
        A, At = m.pruned_pair(keep)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        A._plan_handle()
        At._plan_handle()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) * 1e3
    prune["plan_analyses_ms"] = round(_median(analyses, args.repeats), 4)
    t0 = time.perf_counter()
    m.prune(0)
    torch.cuda.synchronize()
    prune["prune_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["prune"] = prune
    # ---- one plain run: the pruned plan beside the full one
    from skrec.recommender._graph import run_plan
    Y = torch.empty((nU, 64), device=dev)
    res["plan_run_ms"] = dict(pruned=round(_median(lambda: _time(lambda: run_plan(m.adj_train, m.X0[nU:], Y=Y), 5), args.repeats), 4),
                              full=round(_median(lambda: _time(lambda: run_plan(m.adj, m.X0[nU:], Y=Y), 5), args.repeats), 4))
    # ---- the step
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pick = torch.randperm(int(ds["items"].numel()), generator=g, device=dev)[:B * args.steps]
    us, ps = ds["users"][pick].int(), ds["items"][pick].int()
    ns = torch.randint(0, nI, (pick.numel(),), generator=g, device=dev, dtype=torch.int32)
    batches = [(us[s:s + B].contiguous(), ps[s:s + B].contiguous(), ns[s:s + B].contiguous()) for s in range(0, pick.numel() - B + 1, B)]

    def epoch():
        for b in batches:
            m.train_step(*b)
        m.step_losses = []
    res["steps"] = len(batches)
    res["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    print(json.dumps(dict(reg=reg, step_ms=res["step_ms"], prune=prune)), flush=True)
    ms = (ctypes.c_float * _hip.SKR_FREEDOM_GROUPS)()

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
    opt = m.optimizer
    ms_adam = _median(lambda: _time(opt.step, 3), args.repeats)
    n_par = opt.flat.numel()
    res["adam"] = dict(n_params=n_par, ms=round(ms_adam, 4), hbm_frac=round(32 * n_par / (ms_adam * 1e-3) / HBM_PEAK, 4))
    # ---- evaluation
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"], te_ptr=te_ptr,
                   te_items=ds["test_item"])
    n_eval = min(nU, args.eval_users)
    users = np.arange(n_eval, dtype=np.int32)
    ms_ev = _median(lambda: _time(lambda: ev.per_user_rows(m, users)), args.repeats)
    res["eval_users"] = n_eval
    res["eval_users_per_s"] = round(n_eval / (ms_ev * 1e-3))
    res["propagate_ms"] = round(_median(lambda: _time(m.propagate, 3), args.repeats), 4)
    print(json.dumps(res), flush=True)
    # ---- the reference's ops
    if args.torch_steps > 0:
        try:
            ref = TorchStep(m, 1e-3)
            bs = [tuple(t.long() for t in b) for b in batches[:args.torch_steps]]
            res["torch_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(*b) for b in bs]) / len(bs), args.repeats), 4)
            res["speedup_vs_torch"] = round(res["torch_step_ms"] / res["step_ms"], 2)
            del ref
        except RuntimeError as e:        # e.g. out of memory
            res["torch_step_error"] = str(e)[:200]
        torch.cuda.empty_cache()
        n_slice = min(nnz, 1 << 24)
        w = m.edge_w[:n_slice]
        k_slice = int(n_slice * (1. - m.config.dropout))
        try:
            res["torch_multinomial"] = dict(categories=n_slice, drawn=k_slice,
                                            ms=round(_median(lambda: _time(lambda: torch.multinomial(w, k_slice)), args.repeats), 4))
        except RuntimeError as e:
            res["torch_multinomial"] = dict(categories=n_slice, error=str(e)[:200])
        if nnz > 1 << 24:
            try:
                torch.multinomial(m.edge_w, n_keep)
                res["torch_multinomial"]["whole_set"] = "ran"
            except RuntimeError as e:
                res["torch_multinomial"]["whole_set"] = "refused: " + str(e)[:120]
    del m, A1, A1t
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--img_dim", type=int, default=4096)
    ap.add_argument("--txt_dim", type=int, default=384)
    ap.add_argument("--regs", default="0,1e-3")
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
    res = dict(users=args.users, items=args.items, interactions=int(ds["items"].numel()), batch=args.batch, img_dim=args.img_dim,
               txt_dim=args.txt_dim, repeats=args.repeats, device=torch.cuda.get_device_name(0), runs=[])
    for reg in (float(x) for x in args.regs.split(",")):
        res["runs"].append(run_reg(args, ds, img, txt, reg, dev))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
