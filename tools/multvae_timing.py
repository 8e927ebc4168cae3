"""Timing of MultVAE at bench scale on one GPU:

    python tools/multvae_timing.py [--users 1000000 --items 100000 --inter 48000000 --dim 64 --batches 256,1024
                                    --steps 200 --repeats 3 --eval_users 65536 --out FILE.json]

Data: bench.synth_dataset (imported, not copied); a batch is a run of consecutive users of a random permutation.
Reported, as one JSON line, medians of ``--repeats`` repeats: ms per training step (skr_multvae_step with device draws +
the two dense Adam launches), each launch of the step alone by HIP events (skr_multvae_step_timed), the decoder
passes against the fp32 matrix peak (pass 1: one B x I x 64 product, pass 2: three), the two Adam launches against
the HBM peak, skr_multvae_queries over all users, and evaluation users/s through the evaluator's fused top-K path.

Beside it, in the same session: the reference's training step written with torch-ROCm ops on a dense [B, I] input (what
a user of the reference gets on this GPU): the batch's rows as a dense float matrix (built on the device: the
reference's host-side ``csr[users].toarray()`` and its copy are not charged), F.normalize, dropout, the two Linear
layers, log_softmax, the loss with the l2 term, backward and torch.optim.Adam -- restated here from the model's
equations (recommender/MultVAE.py:99-136,179-201)."""
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
FP32_MATRIX_PEAK = 157.3e12
LAUNCHES = ("prep", "encode", "pass1", "merge", "pass2", "reduce", "enc_bwd", "dbq")


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
    """the reference's step on torch-ROCm ops, dense [B, I] input"""

    def __init__(self, n_items, d, lr, reg, keep_prob, anneal, dev):
        import torch.nn as nn
        self.q, self.p = nn.Linear(n_items, 2 * d).to(dev), nn.Linear(d, n_items).to(dev)
        for t in (self.q.weight, self.q.bias, self.p.weight, self.p.bias):
            nn.init.normal_(t, 0.0, 0.01)
        self.opt = torch.optim.Adam(list(self.q.parameters()) + list(self.p.parameters()), lr=lr)
        self.d, self.reg, self.drop, self.anneal = d, reg, nn.Dropout(1 - keep_prob), anneal

    def step(self, x):
        import torch.nn.functional as F
        h = self.drop(F.normalize(x, p=2, dim=1))
        e = self.q(h)
        mu, logvar = e[:, :self.d], e[:, self.d:]
        std = torch.exp(0.5 * logvar)
        kl = torch.sum(0.5 * (-logvar + logvar.exp() + mu.pow(2) - 1), dim=1).mean()
        z = mu + torch.randn_like(std) * std
        logits = self.p(z)
        neg_ll = -(F.log_softmax(logits, dim=-1) * x).sum(-1).mean()
        l2 = 0.5 * (self.q.weight.pow(2).sum() + self.p.weight.pow(2).sum())
        loss = neg_ll + self.anneal * kl + 2 * self.reg * l2
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def dense_batch(rowptr, items, users, n_items):
    """float32 [B, I] binary rows of the device CSR"""
    lens = (rowptr[users + 1] - rowptr[users])
    rows = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), lens)
    start = torch.repeat_interleave(rowptr[users] - torch.cumsum(lens, 0) + lens, lens)
    cols = items[start + torch.arange(rows.numel(), device=users.device)].long()
    x = torch.zeros((users.numel(), n_items), dtype=torch.float32, device=users.device)
    x[rows, cols] = 1.0
    return x


def batch_leg(m, ds, nU, nI, B, args, dev):
    out = {}
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    perm = torch.randperm(nU, generator=g, device=dev)[:B * args.steps].int()
    batches = [perm[s:s + B].contiguous() for s in range(0, perm.numel() - B + 1, B)]
    L, st = _hip.lib(), _hip.stream()

    def epoch():
        for b in batches:
            m.train_step(b)
        m.step_losses = []
    out["steps"] = len(batches)
    out["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    # each launch alone
    du = batches[:32]
    loss = torch.empty(2, device=dev)
    ms = np.zeros(len(LAUNCHES), np.float32)

    def timed():
        acc = np.zeros(len(LAUNCHES))
        for u in du:
            rc = L.skr_multvae_step_timed(_hip.ptr(m._wqt), _hip.ptr(m._bq), _hip.ptr(m._wp), _hip.ptr(m._bp), _hip.ptr(m._rowptr),
                                          _hip.ptr(m._items), _hip.ptr(u), B, nU, nI, m.d, m.config.keep_prob, 0.2, None, None,
                                          1, 0, *[_hip.ptr(t) for t in m._grads], _hip.ptr(m._work), m._work.numel(),
                                          _hip.ptr(loss), st, ms.ctypes.data)
            _hip.check(rc)
            acc += ms
        for o in (m.opt_w, m.opt_b):
            o.grad.zero_()
        return acc / len(du)
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    out["launch_us"] = {k: round(float(v) * 1e3, 2) for k, v in zip(LAUNCHES, per)}
    out["step_kernels_us"] = round(float(per.sum()) * 1e3, 2)
    flop = 2.0 * B * nI * 64
    out["pass1_matrix_peak_frac"] = round(flop / (per[2] * 1e-3) / FP32_MATRIX_PEAK, 4)
    out["pass2_matrix_peak_frac"] = round(3 * flop / (per[4] * 1e-3) / FP32_MATRIX_PEAK, 4)
    # the torch-ROCm restatement of the reference's step, same session
    ref = TorchStep(nI, m.d, 1e-3, 1e-3, 0.5, 0.2, dev)
    xs = [dense_batch(ds["rowptr"], ds["items"], u.long(), nI) for u in du[:4]]
    out["torch_dense_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(x) for x in xs], 3) / len(xs), args.repeats), 4)
    out["torch_dense_input_ms"] = round(_median(lambda: _time(lambda: dense_batch(ds["rowptr"], ds["items"], du[0].long(), nI), 5),
                                                args.repeats), 4)
    out["speedup_vs_torch_dense"] = round(out["torch_dense_step_ms"] / out["step_ms"], 2)
    del ref, xs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    from skrec.recommender.MultVAE import MultVAE
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    nU, nI = args.users, args.items
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), dim=args.dim, repeats=args.repeats,
               device=torch.cuda.get_device_name(0))
    cfg = dict(lr=1e-3, reg=1e-3, p_dims=[args.dim], keep_prob=0.5, anneal_steps=0, anneal_cap=0.2, batch_size=1024)
    m = MultVAE.detached(nU, nI, cfg, (ds["rowptr"], ds["items"]), seed=1)
    for B in (int(b) for b in args.batches.split(",")):
        res[f"batch_{B}"] = batch_leg(m, ds, nU, nI, B, args, dev)
        print(json.dumps({f"batch_{B}": res[f"batch_{B}"]}), flush=True)
    # the two Adam launches
    st = _hip.stream()
    adam = {}
    for name, o in (("weights_wd", m.opt_w), ("biases", m.opt_b)):
        def one(o=o):
            o.step()
        ms = _median(lambda: _time(one, 10), args.repeats)
        adam[name] = dict(n_params=o.flat.numel(), ms=round(ms, 4), hbm_frac=round(32 * o.flat.numel() / (ms * 1e-3) / HBM_PEAK, 4))
    res["adam"] = adam
    # query rows of all users, and the fused evaluation
    L = _hip.lib()

    def queries():
        _hip.check(L.skr_multvae_queries(_hip.ptr(m._wqt), _hip.ptr(m._bq), _hip.ptr(m._rowptr), _hip.ptr(m._items), None, nU, nU,
                                         nI, _hip.ptr(m._Q), st))
    ms = _median(lambda: _time(queries, 3), args.repeats)
    res["queries_all_users_ms"] = round(ms, 4)
    # 256 B of a WqT row (its mu half) and 4 B of the CSR per non-zero, 256 B written per user; the 51 MB table is
    # re-read out of L2 / Infinity Cache, so this is a gather rate, not HBM traffic
    res["queries_gather_TBps"] = round((int(ds["items"].numel()) * 260 + nU * 256) / (ms * 1e-3) / 1e12, 3)
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"], te_ptr=te_ptr,
                   te_items=ds["test_item"])
    n_eval = min(nU, args.eval_users)
    users = np.arange(n_eval, dtype=np.int32)
    m.predict_factors()
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
