"""Timing of DENS at bench scale on one GPU:

    python tools/dens_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --hops 3 --n_negs 6 --batch 2048
                                 --steps 20 --repeats 3 --eval_users 65536 --torch_steps 2 --out FILE.json]

Data: bench.synth_dataset (imported, not copied); a batch is a run of consecutive train pairs of a random permutation, the
candidates uniform.  Reported, as one JSON line, medians of ``--repeats`` repeats: ms per training step (skr_dens_step + the
dense Adam launch), each launch group of the step alone by HIP events (skr_dens_step_timed), the two batch kernels against the
fp32 matrix peak (select: n (H + 1) (n_negs + 3) rows of 64 against a 64 x 64 gate; back: per (row, hop) four transposed gate
products and four 64 x 64 outer products), the Adam launch against the HBM peak, and evaluation users/s through the
evaluator's fused top-K path (the propagation of the current parameters included).

Beside it, in the same session: the reference's training step written with torch-ROCm ops (what a user of the reference gets
on this GPU): torch.sparse.mm propagations, the [B, n_negs, H + 1, d] gathers, the four nn.Linear gates evaluated for the
selection and again for the loss, backward and torch.optim.Adam -- restated here from the model's equations
(recommender/DENS.py:196-257, :318-374)."""
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
FP32_MATRIX_PEAK = 157.3e12
GROUPS = ("forward_plan_runs", "select", "pool_loss", "back_gate_reduce", "clear_rank_seg_add", "backward_plan_runs")


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
        nu, d = m.num_users, m.config.dim
        P = m.parameters()
        self.P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        self.A = torch.sparse_csr_tensor(m.adj.rowptr, m.adj.col.long(), m.adj.val, size=m.adj.shape)
        self.At = torch.sparse_csr_tensor(m.adj_t.rowptr, m.adj_t.col.long(), m.adj_t.val, size=m.adj_t.shape)
        self.cfg, self.nu, self.d = m.config, nu, d
        self.opt = torch.optim.Adam(list(self.P.values()), lr=lr)

    def _lin(self, name, x):
        return torch.nn.functional.linear(x, self.P[name + ".weight"], self.P[name + ".bias"])

    def step(self, users, pos, cand, w):
        cfg, P = self.cfg, self.P
        xu, xi = [P["user_embed"]], [P["item_embed"]]
        for _ in range(cfg.context_hops):
            xu, xi = xu + [torch.sparse.mm(self.A, xi[-1])], xi + [torch.sparse.mm(self.At, xu[-1])]
        Xu, Xi = torch.stack(xu, 1), torch.stack(xi, 1)
        s, p, c = Xu[users], Xi[pos], Xi[cand]
        # the selection (its own evaluation of the gates, as the reference has it)
        gp = torch.sigmoid(self._lin("item_gate", p) + self._lin("user_gate", s))
        gn = torch.sigmoid(self._lin("neg_gate", c) + self._lin("pos_gate", p * gp).unsqueeze(1))
        scores = (s.unsqueeze(1) * (w * c - c * gn)).sum(-1)
        idx = scores.max(1)[1].detach()
        n, H1 = idx.shape
        cs = c.gather(1, idx.view(n, 1, H1, 1).expand(n, 1, H1, c.shape[-1])).squeeze(1)
        # the loss
        u, Pm, Nm = s.mean(1), p.mean(1), cs.mean(1)
        dot = lambda a, b: (a * b).sum(-1)      # noqa: E731
        sp = torch.nn.functional.softplus
        loss = sp(dot(u, Nm) - dot(u, Pm)).mean()
        if cfg.gamma > 0:
            gp = torch.sigmoid(self._lin("item_gate", p) + self._lin("user_gate", s))
            pr = p * gp
            gs = torch.sigmoid(self._lin("neg_gate", cs) + self._lin("pos_gate", pr))
            Pr, Nr = pr.mean(1), (cs * gs).mean(1)
            Pir, Nir = Pm - Pr, Nm - Nr
            loss = loss + cfg.gamma / 4 * (sp(dot(u, Pir) - dot(u, Pr)).mean() + sp(dot(u, Nr) - dot(u, Nir)).mean()
                                           + sp(dot(u, Nr) - dot(u, Pr)).mean() + sp(dot(u, Pir) - dot(u, Nir)).mean())
        loss = loss + cfg.l2 * (s[:, 0].square().sum() + p[:, 0].square().sum() + cs[:, 0].square().sum()) / 2 / n
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--hops", type=int, default=3)
    ap.add_argument("--n_negs", type=int, default=6)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--torch_steps", type=int, default=2, help="0 skips the torch-ROCm restatement")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    from skrec.recommender.DENS import DENS
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    nU, nI, B, H, K = args.users, args.items, args.batch, args.hops, args.n_negs
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), dim=args.dim, hops=H, n_negs=K, batch=B,
               repeats=args.repeats, device=torch.cuda.get_device_name(0))
    cfg = dict(lr=1e-3, l2=1e-4, gamma=0.3, dim=args.dim, batch_size=B, context_hops=H, n_negs=K, warmup=100)
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = DENS.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]))
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    n_pairs = int(ds["items"].numel())
    pick = torch.randperm(n_pairs, generator=g, device=dev)[:B * args.steps]
    us, ps = ds["users"][pick].int(), ds["items"][pick].int()
    cs = torch.randint(0, nI, (pick.numel(), K), generator=g, device=dev, dtype=torch.int32)
    batches = [(us[s:s + B].contiguous(), ps[s:s + B].contiguous(), cs[s:s + B].contiguous())
               for s in range(0, pick.numel() - B + 1, B)]

    def epoch():
        for b in batches:
            m.train_step(*b, 1)
        m.step_losses = []
    res["steps"] = len(batches)
    res["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    print(json.dumps(dict(step_ms=res["step_ms"])), flush=True)
    # each launch group alone
    ms = (ctypes.c_float * _hip.SKR_DENS_GROUPS)()

    def timed():
        acc = np.zeros(len(GROUPS))
        for b in batches[:8]:
            m.gradient_step(*b, 1, h_ms=ms)
            acc += np.array(list(ms))
        return acc / min(8, len(batches))
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    res["group_ms"] = {k: round(float(v), 4) for k, v in zip(GROUPS, per)}
    res["step_kernels_ms"] = round(float(per.sum()), 4)
    f_sel = 2.0 * B * (H + 1) * (K + 3) * 64 * 64
    f_back = 2.0 * B * (H + 1) * 8 * 64 * 64
    res["gate_rows_per_step"] = B * (H + 1) * (K + 3)
    res["matrix_peak_frac"] = dict(select=round(f_sel / (per[1] * 1e-3) / FP32_MATRIX_PEAK, 4),
                                   back=round(f_back / (per[3] * 1e-3) / FP32_MATRIX_PEAK, 4))
    ms_adam = _median(lambda: _time(m.optimizer.step, 5), args.repeats)
    n_par = m.optimizer.flat.numel()
    res["adam"] = dict(n_params=n_par, ms=round(ms_adam, 4), hbm_frac=round(32 * n_par / (ms_adam * 1e-3) / HBM_PEAK, 4))
    # evaluation through the fused top-K path: the propagation of the current parameters, then the ranking
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
            w = m.selection_weight(1)
            bs = [tuple(t.long() for t in b) for b in batches[:args.torch_steps]]
            res["torch_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(*b, w) for b in bs]) / len(bs), args.repeats), 4)
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
