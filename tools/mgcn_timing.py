"""Timing of MGCN at bench scale on one GPU:

    python tools/mgcn_timing.py [--users 1000000 --items 100000 --inter 48000000 --batch 2048 --img_dim 4096 --txt_dim 384
                                 --steps 6 --repeats 3 --torch_steps 2 --out profiles/mgcn_timing.json]

Data: bench.synth_dataset (imported, not copied) with seeded random item features, as tools/bm3_timing.py; a batch is a run of
consecutive train pairs of a random permutation with uniform negatives.  The model's defaults (n_ui_layers 2, n_layers 1,
knn_k 10).  ONE session; reported as one JSON line, medians of ``--repeats`` repeats: construction (kNN lists and item graphs
included), ms per training step (skr_mgcn_step + the dense Adam launch), each launch group of the step alone by HIP events
(skr_mgcn_step_timed) with the fraction of its floor where it has one -- the 78.6 TF fp64 matrix peak (these products add
their fp32 operands on the f64 instruction; the fp32 peak would be 157.3 TF) for the 2 I F 64
products of the projections (one forward, two backward per modality), the 8 TB/s HBM peak for the tables the projection
backward must move and for the Adam launch --, ``propagate()`` with the dense fuser, and, in the same session, the
reference's training step written with torch-ROCm ops (torch.sparse.mm on the square adjacency, on both item graphs and on R,
nn.Linear on the WHOLE feature tables, the fuser over all U + I rows, InfoNCE as two [B, B] matrices, backward,
torch.optim.Adam over every tensor: recommender/MGCN.py:250-353)."""
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

HBM_PEAK, MATRIX_PEAK = 8.0e12, 78.6e12     # the projections' products issue on v_mfma_f64_16x16x4_f64: the fp64 matrix peak
GROUPS = ("project", "ui_forward_plan_runs", "purify_item_graph_runs_R", "batch_forward_loss", "batch_backward_seg_add",
          "mean_backward_chain", "image_backward", "text_backward")


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


def _coo(csr, shape, dev):
    rows = torch.repeat_interleave(torch.arange(shape[0], device=dev), csr.rowptr[1:] - csr.rowptr[:-1])
    return torch.sparse_coo_tensor(torch.stack([rows, csr.col.long()]), csr.val, shape).coalesce()


class TorchStep(object):
    """the reference's step on torch-ROCm ops"""

    def __init__(self, m, lr):
        nu, ni, dev = m.num_users, m.num_items, m.device
        self.P = {k: v.clone().requires_grad_(True) for k, v in m.parameters().items()}
        self.R = _coo(m.adj, (nu, ni), dev)
        Rt = _coo(m.adj_t, (ni, nu), dev)
        idx = torch.cat([torch.stack([self.R.indices()[0], self.R.indices()[1] + nu]), torch.stack([Rt.indices()[0] + nu, Rt.indices()[1]])], 1)
        self.A = torch.sparse_coo_tensor(idx, torch.cat([self.R.values(), Rt.values()]), (nu + ni, nu + ni)).coalesce()
        self.S = [_coo(m.mm_adj[k], (ni, ni), dev) for k in ("img", "txt")]
        self.nu, self.ni, self.cfg = nu, ni, m.config
        self.opt = torch.optim.Adam(list(self.P.values()), lr=lr)

    def step(self, users, pos, neg):
        cfg, P, F, nu = self.cfg, self.P, torch.nn.functional, self.nu
        Ei = P["item_id_embedding.weight"]
        Z = []
        for m, (pre, gate) in enumerate((("image", "gate_v.0"), ("text", "gate_t.0"))):
            feats = F.linear(P[pre + "_embedding.weight"], P[pre + "_trs.weight"], P[pre + "_trs.bias"])
            X = Ei * torch.sigmoid(F.linear(feats, P[gate + ".weight"], P[gate + ".bias"]))
            for _ in range(cfg.n_layers):
                X = torch.sparse.mm(self.S[m], X)
            Z.append(torch.cat([torch.sparse.mm(self.R, X), X], 0))
        ego = torch.cat([P["user_embedding.weight"], Ei], 0)
        layers = [ego]
        for _ in range(cfg.n_ui_layers):
            ego = torch.sparse.mm(self.A, ego)
            layers.append(ego)
        M = torch.stack(layers, 1).mean(1)
        att = torch.cat([F.linear(torch.tanh(F.linear(z, P["query_common.0.weight"], P["query_common.0.bias"])), P["query_common.2.weight"])
                         for z in Z], -1)
        w = torch.softmax(att, -1)
        c = w[:, :1] * Z[0] + w[:, 1:] * Z[1]
        pv = torch.sigmoid(F.linear(M, P["gate_image_prefer.0.weight"], P["gate_image_prefer.0.bias"]))
        pt = torch.sigmoid(F.linear(M, P["gate_text_prefer.0.weight"], P["gate_text_prefer.0.bias"]))
        side = (pv * (Z[0] - c) + pt * (Z[1] - c) + c) / 3
        out = M + side
        ou, oi, oj = out[users], out[nu + pos], out[nu + neg]
        loss = -F.logsigmoid((ou * oi).sum(1) - (ou * oj).sum(1)).mean()
        loss = loss + cfg.reg * (0.5 * (ou ** 2).sum() + 0.5 * (oi ** 2).sum() + 0.5 * (oj ** 2).sum()) / users.numel()

        def nce(a, b):
            a, b = F.normalize(a, dim=1), F.normalize(b, dim=1)
            return -torch.log(torch.exp((a * b).sum(-1) / 0.2) / torch.exp(a @ b.T / 0.2).sum(1)).mean()
        loss = loss + cfg.cl_loss * (nce(side[nu + pos], M[nu + pos]) + nce(side[users], M[users]))
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=48_000_000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--img_dim", type=int, default=4096)
    ap.add_argument("--txt_dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch_steps", type=int, default=2, help="0 skips the torch-ROCm restatement")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    from skrec.recommender.MGCN import MGCN
    dev = _hip.require_gpu()
    nU, nI, B = args.users, args.items, args.batch
    ds = synth_dataset(nU, nI, args.inter, 2021, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    img = torch.randn((nI, args.img_dim), generator=g, device=dev)
    txt = torch.randn((nI, args.txt_dim), generator=g, device=dev)
    res = dict(matrix_peak_tf=MATRIX_PEAK / 1e12, users=nU, items=nI, interactions=int(ds["items"].numel()), batch=B, img_dim=args.img_dim, txt_dim=args.txt_dim,
               repeats=args.repeats, device=torch.cuda.get_device_name(0))
    torch.manual_seed(1)
    np.random.seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = MGCN.detached(nU, nI, dict(lr=1e-3, batch_size=B), (ds["rowptr"], ds["items"]), img=img, txt=txt)
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    del img, txt
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
    print(json.dumps(dict(step_ms=res["step_ms"])), flush=True)
    ms = (ctypes.c_float * _hip.SKR_MGCN_GROUPS)()

    def timed():
        acc = np.zeros(len(GROUPS))
        for b in batches:
            m.gradient_step(*b, h_ms=ms)
            acc += np.array(list(ms))
        return acc / len(batches)
    timed()
    per = np.median(np.stack([timed() for _ in range(args.repeats)]), axis=0)
    res["group_ms"] = {k: round(float(v), 4) for k, v in zip(GROUPS, per)}
    res["step_kernels_ms"] = round(float(per.sum()), 4)
    # the floors: one 2 I F 64 product forward, two backward (dW and dT) per modality; the backward also reads T and writes dT
    F = {"img": m.feat_ld["img"], "txt": m.feat_ld["txt"]}
    flop = lambda ld: 2.0 * nI * ld * 64           # noqa: E731
    floors = dict(project_ms=(flop(F["img"]) + flop(F["txt"])) / MATRIX_PEAK * 1e3,
                  project_hbm_ms=4.0 * nI * (F["img"] + F["txt"]) / HBM_PEAK * 1e3,
                  image_backward_ms=max(2 * flop(F["img"]) / MATRIX_PEAK, 8.0 * nI * F["img"] / HBM_PEAK) * 1e3,
                  text_backward_ms=max(2 * flop(F["txt"]) / MATRIX_PEAK, 8.0 * nI * F["txt"] / HBM_PEAK) * 1e3)
    res["floors_ms"] = {k: round(v, 4) for k, v in floors.items()}
    res["floor_frac"] = dict(project=round(max(floors["project_ms"], floors["project_hbm_ms"]) / per[0], 4),
                             image_backward=round(floors["image_backward_ms"] / per[6], 4),
                             text_backward=round(floors["text_backward_ms"] / per[7], 4))
    opt = m.optimizer
    ms_adam = _median(lambda: _time(opt.step, 3), args.repeats)
    n_par = opt.flat.numel()
    res["adam"] = dict(n_params=n_par, ms=round(ms_adam, 4), hbm_frac=round(32 * n_par / (ms_adam * 1e-3) / HBM_PEAK, 4))
    res["propagate_ms"] = round(_median(lambda: _time(m.propagate, 2), args.repeats), 4)
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
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
