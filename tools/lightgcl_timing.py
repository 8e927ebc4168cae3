"""Timing of LightGCL at bench scale on one GPU:

    python tools/lightgcl_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --layers 2 --q 5 --batch 2048
                                     --steps 20 --repeats 3 --eval_users 65536 --torch_steps 2 --out FILE.json]

Data: bench.synth_dataset (imported, not copied); a batch is a run of consecutive train pairs of a random permutation, the
negatives uniform.  Reported, as one JSON line, medians of ``--repeats`` repeats: ms per training step (skr_lightgcl_step +
the dense Adam launch), each launch group of the step alone by HIP events (skr_lightgcl_step_timed), the two InfoNCE sides
with pass 1 and pass 2 apart against the fp32 matrix peak (pass 1: one n x N x 64 product, pass 2: three), the 4L plan runs,
the low-rank and batch kernels, the Adam launch against the HBM peak, the SVD at construction, and evaluation users/s
through the evaluator's fused top-K path.

Beside it, in the same session: the reference's training step written with torch-ROCm ops (what a user of the reference gets
on this GPU): torch.sparse.mm propagations, the per-layer SVD view, the dense [B, U] and [2B, I] logits, backward and
torch.optim.Adam -- restated here from the model's equations (recommender/LightGCL.py:117-169)."""
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
GROUPS = ("forward_plan_runs", "prep_lowrank_gather", "user_pass1", "user_pass2", "item_pass1", "item_pass2",
          "batch_dT_expand", "backward_plan_runs")


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
    """the reference's step on torch-ROCm ops: sparse propagations, dense [B, U] and [2B, I] logits"""

    def __init__(self, m, lr):
        nu, d = m.num_users, m.config.d
        self.Eu = m.E0[:nu, :d].clone().requires_grad_(True)
        self.Ei = m.E0[nu:, :d].clone().requires_grad_(True)
        self.A = torch.sparse_csr_tensor(m.adj.rowptr, m.adj.col.long(), m.adj.val, size=m.adj.shape)
        self.At = torch.sparse_csr_tensor(m.adj_t.rowptr, m.adj_t.col.long(), m.adj_t.val, size=m.adj_t.shape)
        self.f = (m.u_mul_s, m.v_mul_s, m.ut, m.vt)
        self.cfg = m.config
        self.opt = torch.optim.Adam([self.Eu, self.Ei], lr=lr)

    def step(self, uids, pos, neg):
        cfg = self.cfg
        u_mul_s, v_mul_s, ut, vt = self.f
        Eu, Ei, Gu, Gi = [self.Eu], [self.Ei], [self.Eu], [self.Ei]
        for _ in range(cfg.gnn_layer):
            zu, zi = torch.sparse.mm(self.A, Ei[-1]), torch.sparse.mm(self.At, Eu[-1])
            Gu.append(u_mul_s @ (vt @ Ei[-1]))
            Gi.append(v_mul_s @ (ut @ Eu[-1]))
            Eu.append(zu)
            Ei.append(zi)
        Eu, Ei, Gu, Gi = sum(Eu), sum(Ei), sum(Gu), sum(Gi)
        iids = torch.cat([pos, neg])
        neg_score = torch.log(torch.exp(Gu[uids] @ Eu.T / cfg.temp).sum(1) + 1e-8).mean() \
            + torch.log(torch.exp(Gi[iids] @ Ei.T / cfg.temp).sum(1) + 1e-8).mean()
        pos_score = torch.clamp((Gu[uids] * Eu[uids]).sum(1) / cfg.temp, -5.0, 5.0).mean() \
            + torch.clamp((Gi[iids] * Ei[iids]).sum(1) / cfg.temp, -5.0, 5.0).mean()
        x = (Eu[uids] * Ei[pos]).sum(-1) - (Eu[uids] * Ei[neg]).sum(-1)
        loss = -torch.nn.functional.logsigmoid(x).mean() + cfg.lambda1 * (neg_score - pos_score) \
            + cfg.lambda2 * (self.Eu.norm(2).square() + self.Ei.norm(2).square())
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--q", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--torch_steps", type=int, default=2, help="0 skips the torch-ROCm restatement")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    from skrec.recommender.LightGCL import LightGCL
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    nU, nI, B = args.users, args.items, args.batch
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), dim=args.dim, layers=args.layers, q=args.q, batch=B,
               repeats=args.repeats, device=torch.cuda.get_device_name(0))
    cfg = dict(lr=1e-3, lambda1=0.2, d=args.dim, gnn_layer=args.layers, batch_size=B, svd_q=args.q, temp=0.2, lambda2=1e-7)
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = LightGCL.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]))
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    from skrec.recommender.LightGCL import svd_lowrank_device
    R = torch.randn(min(nU, nI), args.q, device=dev)
    res["svd_ms"] = round(_median(lambda: _time(lambda: svd_lowrank_device(m.adj, m.adj_t, R)), args.repeats), 3)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    n_pairs = int(ds["items"].numel())
    pick = torch.randperm(n_pairs, generator=g, device=dev)[:B * args.steps]
    us, ps = ds["users"][pick].int(), ds["items"][pick].int()
    ns = torch.randint(0, nI, (pick.numel(),), generator=g, device=dev, dtype=torch.int32)
    batches = [(us[s:s + B].contiguous(), ps[s:s + B].contiguous(), ns[s:s + B].contiguous())
               for s in range(0, pick.numel() - B + 1, B)]

    def epoch():
        for b in batches:
            m.train_step(*b)
        m.step_losses = []
    res["steps"] = len(batches)
    res["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    print(json.dumps(dict(step_ms=res["step_ms"])), flush=True)
    # each launch group alone
    ms = (ctypes.c_float * _hip.SKR_LIGHTGCL_GROUPS)()

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
    fu, fi = 2.0 * B * nU * 64, 2.0 * 2 * B * nI * 64
    res["matrix_peak_frac"] = dict(user_pass1=round(fu / (per[2] * 1e-3) / FP32_MATRIX_PEAK, 4),
                                   user_pass2=round(3 * fu / (per[3] * 1e-3) / FP32_MATRIX_PEAK, 4),
                                   item_pass1=round(fi / (per[4] * 1e-3) / FP32_MATRIX_PEAK, 4),
                                   item_pass2=round(3 * fi / (per[5] * 1e-3) / FP32_MATRIX_PEAK, 4))
    ms_adam = _median(lambda: _time(m.optimizer.step, 5), args.repeats)
    n_par = m.optimizer.flat.numel()
    res["adam"] = dict(n_params=n_par, ms=round(ms_adam, 4), hbm_frac=round(32 * n_par / (ms_adam * 1e-3) / HBM_PEAK, 4))
    # evaluation through the fused top-K path on the kept sums
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
    # the torch-ROCm restatement of the reference's step, same session (dense [B, U] included)
    if args.torch_steps > 0:
        try:
            ref = TorchStep(m, 1e-3)
            bs = [tuple(t.long() for t in b) for b in batches[:args.torch_steps]]
            res["torch_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(*b) for b in bs]) / len(bs), args.repeats), 4)
            res["speedup_vs_torch"] = round(res["torch_step_ms"] / res["step_ms"], 2)
        except RuntimeError as e:        # e.g. out of memory for the dense logits and their autograd copies
            res["torch_step_error"] = str(e)[:200]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
