"""Timing of LATTICE at bench scale on one GPU:

    python tools/lattice_timing.py [--users 1000000 --items 100000 --inter 48000000 --batch 2048 --img_dim 4096 --txt_dim 384
                                    --steps 6 --repeats 3 --torch_steps 2 --out profiles/lattice_timing.json]

Data: bench.synth_dataset (imported, not copied) with seeded random item features, as tools/mgcn_timing.py; a batch is a run
of consecutive train pairs of a random permutation with uniform negatives.  The model's defaults (weight_size [64, 64],
n_layers 1, knn_k 10, lambda_coeff 0.9).  ONE session; reported as one JSON line, medians of ``--repeats`` repeats:

  * construction (frozen kNN graphs and the square adjacency included);
  * an ordinary step: skr_lattice_step + the rows' dense Adam launch, and its launch groups by HIP events
    (skr_lattice_step_timed);
  * a build step by launch group: projection of both tables, kNN of the projected rows, the graph (skr_lattice_graph, the
    transpose and the two plan analyses), the step itself with the sampled product, the graph backward
    (skr_lattice_graph_bwd), the projection backward, the modal block's Adam launch;
  * ``rebuild_graph`` alone and ``propagate()`` (an evaluation's forward, its rebuild included);
  * in the same session, the reference's step written with torch-ROCm ops (recommender/LATTICE.py:203-294): the ORDINARY step
    with a dense ``item_adj`` at the full item count when 1.5 x 4 I^2 bytes fit in 60 % of the free memory, and the BUILD step
    (dense build_sim, topk, scatter, Laplacian, mix, backward) at ``torch_build_items``, the largest count from --items
    downward by halves at which twelve dense [I, I] matrices fit in 60 % of the free memory.  Both counts are in the JSON."""
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

GROUPS = ("ui_forward_plan_runs", "item_graph_runs", "batch_forward_loss", "clear_rank_seg_add", "ui_backward_plan_runs",
          "item_graph_backward_runs", "sampled_product")


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


def _build_sim(x):
    xn = x.div(torch.norm(x, p=2, dim=-1, keepdim=True))
    return torch.mm(xn, xn.transpose(1, 0))


def _knn(adj, k):
    val, ind = torch.topk(adj, k, dim=-1)
    return torch.zeros_like(adj).scatter_(-1, ind, val)


def _laplacian(adj):
    d = torch.pow(torch.sum(adj, -1), -0.5)
    d = torch.where(torch.isinf(d), torch.zeros_like(d), d)
    return d[:, None] * adj * d[None, :]


class TorchStep(object):
    """the reference's step on torch-ROCm ops over the first ``ni`` items: ``ordinary`` multiplies by a detached dense item_adj,
    ``build`` assembles it densely first and differentiates through it"""

    def __init__(self, m, ni, lr, cfg):
        nu, dev = m.num_users, m.device
        P = m.parameters()
        self.P = {k: (v[:ni] if k in ("item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight") else v).clone().requires_grad_(True)
                  for k, v in P.items()}
        A = _coo(m.adj, (nu + m.num_items,) * 2, dev)
        idx, val = A.indices(), A.values()
        keep = (idx[0] < nu + ni) & (idx[1] < nu + ni)
        self.A = torch.sparse_coo_tensor(idx[:, keep], val[keep], (nu + ni, nu + ni)).coalesce()
        self.nu, self.ni, self.cfg = nu, ni, cfg
        with torch.no_grad():
            self.orig = [_laplacian(_knn(_build_sim(self.P[k]), cfg.knn_k)) for k in ("image_embedding.weight", "text_embedding.weight")]
        self.item_adj = None
        self.opt = torch.optim.Adam(list(self.P.values()), lr=lr)

    def step(self, users, pos, neg, build):
        cfg, P, F, nu = self.cfg, self.P, torch.nn.functional, self.nu
        if build:
            w = torch.softmax(P["modal_weight"], 0)
            fv = F.linear(P["image_embedding.weight"], P["image_trs.weight"], P["image_trs.bias"])
            ft = F.linear(P["text_embedding.weight"], P["text_trs.weight"], P["text_trs.bias"])
            learned = w[0] * _knn(_build_sim(fv), cfg.knn_k) + w[1] * _knn(_build_sim(ft), cfg.knn_k)
            original = w[0] * self.orig[0] + w[1] * self.orig[1]
            self.item_adj = (1 - cfg.lambda_coeff) * _laplacian(learned) + cfg.lambda_coeff * original
        else:
            self.item_adj = self.item_adj.detach()
        h = P["item_id_embedding.weight"]
        for _ in range(cfg.n_layers):
            h = torch.mm(self.item_adj, h)
        ego = torch.cat([P["user_embedding.weight"], P["item_id_embedding.weight"]], 0)
        layers = [ego]
        for _ in range(len(cfg.weight_size)):
            ego = torch.sparse.mm(self.A, ego)
            layers.append(ego)
        M = torch.stack(layers, 1).mean(1)
        ou, items = M[:nu][users], M[nu:] + F.normalize(h, p=2, dim=1)
        oi, oj = items[pos], items[neg]
        loss = -F.logsigmoid((ou * oi).sum(1) - (ou * oj).sum(1)).mean()
        loss = loss + cfg.reg * (0.5 * (ou ** 2).sum() + 0.5 * (oi ** 2).sum() + 0.5 * (oj ** 2).sum()) / users.numel()
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
    from skrec.recommender.LATTICE import LATTICE, MODALITIES
    dev = _hip.require_gpu()
    L, p = _hip.lib(), _hip.ptr
    nU, nI, B = args.users, args.items, args.batch
    ds = synth_dataset(nU, nI, args.inter, 2021, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    img = torch.randn((nI, args.img_dim), generator=g, device=dev)
    txt = torch.randn((nI, args.txt_dim), generator=g, device=dev)
    res = dict(users=nU, items=nI, interactions=int(ds["items"].numel()), batch=B, img_dim=args.img_dim, txt_dim=args.txt_dim,
               repeats=args.repeats, device=torch.cuda.get_device_name(0))
    torch.manual_seed(1)
    np.random.seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = LATTICE.detached(nU, nI, dict(lr=1e-3, batch_size=B), (ds["rowptr"], ds["items"]), img=img, txt=txt)
    torch.cuda.synchronize()
    res["construction_s"] = round(time.perf_counter() - t0, 3)
    del img, txt
    pick = torch.randperm(int(ds["items"].numel()), generator=g, device=dev)[:B * args.steps]
    us, ps = ds["users"][pick].int(), ds["items"][pick].int()
    ns = torch.randint(0, nI, (pick.numel(),), generator=g, device=dev, dtype=torch.int32)
    batches = [(us[s:s + B].contiguous(), ps[s:s + B].contiguous(), ns[s:s + B].contiguous()) for s in range(0, pick.numel() - B + 1, B)]
    m.adj._plan_handle()
    m.adj_t._plan_handle()
    # ---- the graph: projection, kNN, the whole rebuild
    st = _hip.stream

    def project():
        for key, _ in MODALITIES:
            trs, tab = m._blocks(key)
            _hip.check(L.skr_mgcn_project(p(tab), nI, m.feat_dim[key], m.feat_ld[key], p(trs), p(m._F[key]), st()))

    def knn():
        from skrec.utils.item_graph import knn_topk
        for key, _ in MODALITIES:
            knn_topk(m._F[key], m.config.knn_k, feat_dim=m.config.feat_embed_dim, return_sims=True)
    build = dict(project_ms=_median(lambda: _time(project), args.repeats), knn_ms=_median(lambda: _time(knn), args.repeats))
    rebuild_ms = _median(lambda: _time(m.rebuild_graph), args.repeats)
    build["graph_ms"] = rebuild_ms - build["project_ms"] - build["knn_ms"]
    res["rebuild_graph_ms"] = round(rebuild_ms, 4)
    res["graph_nnz"] = m.graph["nnz"]
    print(json.dumps(dict(rebuild_graph_ms=res["rebuild_graph_ms"], knn_ms=round(build["knn_ms"], 4))), flush=True)

    # ---- an ordinary step
    def epoch():
        for b in batches:
            m.train_step(*b)
        m.step_losses = []
    res["steps"] = len(batches)
    res["step_ms"] = round(_median(lambda: _time(epoch) / len(batches), args.repeats), 4)
    print(json.dumps(dict(step_ms=res["step_ms"])), flush=True)
    ms = (ctypes.c_float * _hip.SKR_LATTICE_GROUPS)()

    def timed(is_build):
        acc = np.zeros(len(GROUPS))
        for b in batches:
            m.gradient_step(*b, build=is_build, h_ms=ms)
            acc += np.array(list(ms))
        return acc / len(batches)
    timed(False)
    per = np.median(np.stack([timed(False) for _ in range(args.repeats)]), axis=0)
    res["group_ms"] = {k: round(float(v), 4) for k, v in zip(GROUPS, per)}
    res["step_kernels_ms"] = round(float(per.sum()), 4)
    opt = m.optimizer
    res["adam_ms"] = round(_median(lambda: _time(opt.step, 3), args.repeats), 4)
    # ---- a build step on the installed graph (the parameters have not moved since the rebuild above's last step: the graph
    # is rebuilt once by the first call and reused by the following ones)
    per_b = np.median(np.stack([timed(True) for _ in range(args.repeats)]), axis=0)
    build["step_ms"] = float(per_b[:6].sum())
    build["sampled_product_ms"] = float(per_b[6])
    G = m.graph

    def project_bwd():
        for key, _ in MODALITIES:
            (trs, tab), (gtrs, gtab) = m._blocks(key), m._blocks(key, True)
            _hip.check(L.skr_mgcn_project_bwd(p(m._dF[key]), p(tab), nI, m.feat_dim[key], m.feat_ld[key], p(trs), p(gtrs), p(gtab),
                                              p(m._bwd_work), m._bwd_work.numel(), st()))
    whole_bwd = _median(lambda: _time(lambda: m.graph_backward(G)), args.repeats)
    build["project_backward_ms"] = _median(lambda: _time(project_bwd), args.repeats)
    build["graph_backward_ms"] = whole_bwd - build["project_backward_ms"]
    build["modal_adam_ms"] = _median(lambda: _time(m.modal_optimizer.step, 2), args.repeats)
    res["build_ms"] = {k: round(float(v), 4) for k, v in build.items()}
    res["build_step_total_ms"] = round(float(sum(build.values())) + res["adam_ms"], 4)
    res["propagate_ms"] = round(_median(lambda: _time(m.propagate, 1), args.repeats), 4)
    print(json.dumps(res), flush=True)
    if args.torch_steps > 0:
        try:
            m._mgrad.zero_()
            free = torch.cuda.mem_get_info()[0]
            bs = [tuple(t.long() for t in b) for b in batches[:args.torch_steps]]
            ni_o = nI
            while 1.5 * 4.0 * ni_o * ni_o > 0.6 * free:
                ni_o //= 2
            res["torch_ordinary_items"] = ni_o
            ref = TorchStep(m, ni_o, 1e-3, m.config)
            fit = lambda b: (b[0], b[1] % ni_o, b[2] % ni_o)       # noqa: E731
            S = _coo(m.graph["S"], (nI, nI), dev)
            ref.item_adj = S.to_dense()[:ni_o, :ni_o].contiguous()
            del S
            res["torch_step_ms"] = round(_median(lambda: _time(lambda: [ref.step(*fit(b), False) for b in bs]) / len(bs), args.repeats), 4)
            res["speedup_vs_torch"] = round(res["torch_step_ms"] / res["step_ms"], 2) if ni_o == nI else None
            del ref
            torch.cuda.empty_cache()
            free = torch.cuda.mem_get_info()[0]
            ni_b = nI
            while 12 * 4.0 * ni_b * ni_b > 0.6 * free:
                ni_b //= 2
            res["torch_build_items"] = ni_b
            ref = TorchStep(m, ni_b, 1e-3, m.config)
            fit = lambda b: (b[0], b[1] % ni_b, b[2] % ni_b)       # noqa: E731
            res["torch_build_step_ms"] = round(_median(lambda: _time(lambda: ref.step(*fit(bs[0]), True)), args.repeats), 4)
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
