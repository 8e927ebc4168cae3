"""Timing of SASRec at bench scale on one GPU:

    python tools/sasrec_timing.py [--users 1000000 --items 100000 --inter 48000000 --batch 128 --steps 100 --repeats 3
                                   --eval_users 65536 --out profiles/sasrec_timing.json]

Data: bench.synth_dataset (imported, not copied); a user's interactions in their stored order stand in for time.  A training
row is a random user's last max_len + 1 items (items[:-1] against items[1:], left-padded), negatives uniform (no exclusion:
timing only).  Settings: the reference's defaults (hidden_units 64, max_len 50, 2 blocks, 1 head, batch 128, dropout 0.5 drawn
on the device).

Reported, as one JSON document: ms per training step with its dense skr_adam_step_tf; the step's launch groups one by one
(skr_sasrec_step_timed); skr_sasrec_queries over ``eval_users`` users; evaluation users/s through the fused top-K evaluator at
64 columns (the route RankingEvaluator takes).

Beside it, in the same session: the same step composed of torch-ROCm ops (embedding lookups, layer norms written out, matmul,
softmax, dropout, relu, the two log losses, backward, torch.optim.Adam(betas=(0.9, 0.98)) over every parameter) -- restated
here from the model's equations (recommender/SASRec.py:387-459)."""
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
from seq_timing import _spread, _time  # noqa: E402
from skrec import _hip  # noqa: E402

GROUPS = ("step", "reduce", "positions", "rank", "ordered_adds", "loss")


def last_items(ds, users, width, pad, dev):
    """int32 [len(users), width]: the last ``width`` items of the users' rows, ``back`` positions earlier, left-padded"""
    rowptr, items = ds["rowptr"], ds["items"]
    end = rowptr[1:][users]
    idx = end[:, None] - torch.arange(width, 0, -1, device=dev)[None]
    out = items[idx.clamp(0, max(items.numel() - 1, 0))].int()
    out[idx < rowptr[:-1][users][:, None]] = pad
    return out.contiguous()


class TorchStep(torch.nn.Module):
    """the reference's graph on torch-ROCm ops"""

    def __init__(self, nI, d, T, blocks, heads, rate, lr, dev):
        super().__init__()
        nn = torch.nn
        self.d, self.T, self.blocks, self.heads, self.rate, self.nI = d, T, blocks, heads, rate, nI
        self.E, self.P = nn.Embedding(nI, d), nn.Embedding(T, d)
        mk = lambda: nn.Linear(d, d)                                      # noqa: E731
        self.lin = nn.ModuleList([nn.ModuleList([mk() for _ in range(5)]) for _ in range(blocks)])
        self.ln = nn.ParameterList([nn.Parameter(torch.ones(d) if i % 2 == 0 else torch.zeros(d)) for i in range(4 * blocks + 2)])
        self.to(dev)
        self.opt = torch.optim.Adam(self.parameters(), lr=lr, betas=(0.9, 0.98))

    @staticmethod
    def norm(x, g, b):
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        return g * ((x - mean) / (var + 1e-8) ** 0.5) + b

    def step(self, seq, pos, neg):
        F = torch.nn.functional
        d, T, h = self.d, self.T, self.heads
        n = seq.shape[0]
        table = torch.cat([self.E.weight, torch.zeros(1, d, device=seq.device)], 0) * d ** 0.5
        x = F.dropout(table[seq] + self.P.weight[None], self.rate)
        mask = (seq != self.nI).unsqueeze(-1).float()
        x = x * mask
        tril = torch.tril(torch.ones(T, T, device=seq.device)) == 0
        for b in range(self.blocks):
            q = self.norm(x, self.ln[4 * b], self.ln[4 * b + 1])
            Q, K, V = self.lin[b][0](q), self.lin[b][1](x), self.lin[b][2](x)
            Q, K, V = (t.view(n, T, h, d // h).transpose(1, 2) for t in (Q, K, V))
            s = Q @ K.transpose(-1, -2) / (d // h) ** 0.5
            s = s.masked_fill((x.sum(-1) == 0)[:, None, None, :], -2.0 ** 32 + 1).masked_fill(tril[None, None], -2.0 ** 32 + 1)
            a = torch.softmax(s, -1) * torch.sign(q.sum(-1).abs())[:, None, :, None]
            y = (F.dropout(a, self.rate) @ V).transpose(1, 2).reshape(n, T, d) + q
            f = self.norm(y, self.ln[4 * b + 2], self.ln[4 * b + 3])
            x = (F.dropout(self.lin[b][4](F.dropout(torch.relu(self.lin[b][3](f)), self.rate)), self.rate) + f) * mask
        out = self.norm(x, self.ln[4 * self.blocks], self.ln[4 * self.blocks + 1])
        pl, nl = (table[pos] * out).sum(-1), (table[neg] * out).sum(-1)
        tgt = (pos != self.nI).float()
        loss = ((-torch.log(torch.sigmoid(pl) + 1e-24) - torch.log(1 - torch.sigmoid(nl) + 1e-24)) * tgt).sum() / tgt.sum()
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sasrec_timing.json"))
    args = ap.parse_args()
    from skrec.recommender.SASRec import SASRec
    from skrec.utils.py.evaluator import RankingEvaluator
    dev = _hip.require_gpu()
    nU, nI, b = args.users, args.items, args.batch
    d, T, blocks, heads, rate = 64, 50, 2, 1, 0.5
    ds = synth_dataset(nU, nI, args.inter, 2021, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    counts = ds["rowptr"][1:] - ds["rowptr"][:-1]
    cand = torch.nonzero(counts >= 2).reshape(-1)
    users = cand[torch.randint(0, cand.numel(), (b * args.steps,), generator=g, device=dev)]
    both = last_items(ds, users, T + 1, nI, dev)
    seq, pos = both[:, :-1].contiguous(), both[:, 1:].contiguous()
    neg = torch.randint(0, nI, pos.shape, generator=g, device=dev, dtype=torch.int32)
    neg[pos == nI] = nI
    n_eval = min(nU, args.eval_users)
    windows = torch.full((nU, T), nI, dtype=torch.int32, device=dev)
    windows[:n_eval] = last_items(ds, torch.arange(n_eval, device=dev), T, nI, dev)
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), rows=int(seq.shape[0]), batch=b, hidden_units=d, max_len=T,
               num_blocks=blocks, num_heads=heads, dropout_rate=rate, repeats=args.repeats, device=torch.cuda.get_device_name(0),
               real_positions_share=round(float((seq != nI).float().mean()), 4))
    cfg = dict(lr=1e-3, l2_emb=0.0, hidden_units=d, dropout_rate=rate, max_len=T, num_blocks=blocks, num_heads=heads, batch_size=b)
    m = SASRec.detached(nU, nI, cfg, windows=windows.cpu().numpy(), seed=1)
    res["n_params"] = m.optimizer.flat.numel()
    bounds = [(a, a + b) for a in range(0, seq.shape[0], b)]
    loss = torch.zeros(2 * _hip.SKR_LOSS_SLOTS, device=dev)

    def epoch():
        for a, z in bounds:
            m.train_step(seq[a:z], pos[a:z], neg[a:z], loss)
    res["step_ms_with_adam"] = _spread([_time(epoch) / len(bounds) for _ in range(args.repeats)])
    # the launch groups one by one, the gradients left to accumulate (timing only)
    m.timed_ms = np.zeros(_hip.SKR_SASREC_LAUNCHES, np.float32)
    st = _hip.stream()

    def timed():
        acc = np.zeros(len(GROUPS))
        for a, z in bounds[:32]:
            _hip.check(m._step_launch(seq[a:z].data_ptr(), pos[a:z].data_ptr(), neg[a:z].data_ptr(), b, loss.data_ptr(), st))
            acc += m.timed_ms
        return acc / len(bounds[:32])
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    m.timed_ms = None
    m.optimizer.grad.zero_()
    res["launch_us"] = {k: round(float(v) * 1e3, 2) for k, v in zip(GROUPS, per)}
    res["step_kernels_us"] = round(float(per.sum()) * 1e3, 2)
    # the torch-ROCm restatement of the same step, same session
    ref = TorchStep(nI, d, T, blocks, heads, rate, 1e-3, dev)
    bt = [(seq[a:z].long(), pos[a:z].long(), neg[a:z].long()) for a, z in bounds[:8]]
    res["torch_step_ms"] = _spread([_time(lambda: [ref.step(*x) for x in bt], 2) / len(bt) for _ in range(args.repeats)])
    res["speedup_vs_torch"] = round(res["torch_step_ms"]["median"] / res["step_ms_with_adam"]["median"], 2)
    del ref, bt
    torch.cuda.empty_cache()
    # query rows and the fused evaluation at 64 columns
    L = _hip.lib()
    cfgq = (d, T, blocks, heads)
    Q = torch.empty((n_eval, 64), dtype=torch.float32, device=dev)

    def queries():
        _hip.check(L.skr_sasrec_queries(_hip.ptr(m._item_rows), _hip.ptr(m._pos_rows), _hip.ptr(m._shared), None, n_eval,
                                        _hip.ptr(m._windows), nU, nI, *cfgq, _hip.ptr(Q), _hip.stream()))
    res["eval_users"] = n_eval
    res["queries_ms"] = _spread([_time(queries, 3) for _ in range(args.repeats)])
    te_ptr = torch.arange(nU + 1, dtype=torch.int64, device=dev)
    ev = RankingEvaluator({0: np.array([0])}, {0: np.array([1])}, metric=["Precision", "Recall", "NDCG"], top_k=(10, 20))
    ev._dev = dict(dev=dev, n_rows=nU, max_train=int(counts.max()), tr_ptr=ds["rowptr"], tr_items=ds["items"], te_ptr=te_ptr,
                   te_items=ds["test_item"])
    eu = np.arange(n_eval, dtype=np.int32)
    m.predict_factors()                                 # (all users' rows: outside the timed evaluation)
    ms = _spread([_time(lambda: ev.per_user_rows(m, eu)) for _ in range(args.repeats)])
    res["eval_ms"] = ms
    res["eval_users_per_s"] = round(n_eval / (ms["median"] * 1e-3))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
