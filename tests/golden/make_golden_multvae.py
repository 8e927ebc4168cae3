"""Generate the golden vectors of MultVAE by RUNNING THE REFERENCE on the tiny set of make_golden.py:

    python tests/golden/make_golden_multvae.py

Same rules as make_golden.py, whose helpers are reused: a fresh process, only data is written.  The reference draws its
dropout mask and its latent noise from torch's generator inside the step, so the fixture records them: per training
step the batch's users, one keep flag per non-zero of the batch (user after user, items ascending; from a forward hook
on ``net.dropout``: output != 0 at the non-zeros of the input), ``eps`` (from a wrapper around ``Tensor.normal_`` that
is active while the net is in training mode), ``neg_ll`` and ``kl``.  Otherwise: the four parameters before and after,
per evaluation the report and the dense ``predict(test_users)`` matrix, and the best report.

The run is then replayed in float64 from the recorded draws (torch autograd, ``torch.optim.Adam``).  ``f64_dev`` is the
largest difference between that replay and the reference, per parameter and per evaluation's scores: the reference's
own fp32 noise, from which the tests derive their tolerances.  A replay that differs by more than ten times the figures
of the first trial (F64_TRIAL) means the recording is wrong, not the tolerance: no fixture is written then.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

CONFIG = dict(lr=1e-2, reg=1e-3, p_dims=[64], keep_prob=0.5, anneal_steps=6, anneal_cap=0.2, batch_size=24, epochs=3)
PARAMS = ("Wq", "bq", "Wp", "bp")
# the first trial's replay differences: Wq, bq, Wp, bp, then the scores of the three evaluations
F64_TRIAL = dict(Wq=2.3e-6, bq=8.9e-8, Wp=4.3e-8, bp=1.7e-8, scores=(3.6e-8, 1.1e-7, 3.2e-7))


def _params(net, sfx):
    t = dict(Wq=net.layers_q[0].weight, bq=net.layers_q[0].bias, Wp=net.layers_p[0].weight, bp=net.layers_p[0].bias)
    return {k + sfx: t[k].detach().numpy().copy() for k in PARAMS}


def replay_f64(csr, init, steps, cfg, eval_every, test_users):
    """the run in float64 from recorded draws -> (final parameters, per-step (neg_ll, kl), scores per evaluation);
    ``csr``: scipy CSR of the binary train matrix, ``steps``: (users, keep flags, eps) per training step"""
    import torch
    d = cfg["p_dims"][0]
    Wq, bq, Wp, bp = (torch.tensor(init[k], dtype=torch.float64, requires_grad=True) for k in PARAMS)
    opt = torch.optim.Adam([Wq, bq, Wp, bp], lr=cfg["lr"])
    dense = lambda us: torch.tensor(csr[np.asarray(us)].toarray(), dtype=torch.float64)    # noqa: E731
    losses, scores = [], []
    for t, (users, keep, eps) in enumerate(steps):
        x = dense(users)
        mask = torch.zeros_like(x)
        mask[x != 0] = torch.tensor(keep, dtype=torch.float64)       # row-major: user after user, items ascending
        h = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) * mask / cfg["keep_prob"]
        e = h @ Wq.T + bq
        mu, logvar = e[:, :d], e[:, d:]
        kl = (0.5 * (-logvar + logvar.exp() + mu ** 2 - 1)).sum(1).mean()
        z = mu + torch.tensor(eps, dtype=torch.float64) * (0.5 * logvar).exp()
        neg_ll = -(torch.log_softmax(z @ Wp.T + bp, dim=-1) * x).sum(-1).mean()
        anneal = min(cfg["anneal_cap"], t / cfg["anneal_steps"]) if cfg["anneal_steps"] > 0 else cfg["anneal_cap"]
        loss = neg_ll + anneal * kl + 2 * cfg["reg"] * 0.5 * ((Wq ** 2).sum() + (Wp ** 2).sum())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append((neg_ll.item(), kl.item()))
        if (t + 1) % eval_every == 0:
            with torch.no_grad():
                x = dense(test_users)
                h = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
                scores.append(((h @ Wq.T + bq)[:, :d] @ Wp.T + bp).numpy())
    return {k: v.detach().numpy() for k, v in zip(PARAMS, (Wq, bq, Wp, bp))}, np.array(losses), scores


def make_multvae():
    if not os.path.exists(os.path.join(G.DATA_DIR, "tiny.train")):
        G.make_dataset()
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.MultVAE as M
    G._seed_all()
    users_rec, keep_rec, eps_rec, nll_rec, kl_rec, pred_rec = [], [], [], [], [], []
    orig_iter = M.BatchIterator

    class RecordingIterator(object):
        def __init__(self, *a, **k):
            self.it = orig_iter(*a, **k)

        def __len__(self):
            return len(self.it)

        def __iter__(self):
            for b in self.it:
                users_rec.append(np.asarray(b, np.int32).copy())
                yield b
    M.BatchIterator = RecordingIterator
    model = M.MultVAE(G._run_config(recommender="MultVAE"), dict(CONFIG))
    net = model.multvae
    out = _params(net, "0")

    def hook(mod, inp, outp):
        if net.training:
            x = inp[0]
            keep_rec.append((outp[x != 0] != 0).numpy().astype(np.uint8))
    net.dropout.register_forward_hook(hook)
    orig_normal = torch.Tensor.normal_

    def normal_(self, *a, **k):
        r = orig_normal(self, *a, **k)
        if net.training:
            eps_rec.append(self.detach().numpy().copy())
        return r
    torch.Tensor.normal_ = normal_
    orig_fwd = net.forward

    def forward(x):
        logits, kl = orig_fwd(x)
        if net.training:
            kl_rec.append(float(kl.detach()))
            nll_rec.append(float(-(torch.log_softmax(logits, dim=-1) * x).sum(-1).mean()))
        return logits, kl
    net.forward = forward
    test_users = list(model.evaluator.user_pos_test.keys())
    orig_eval = model.evaluate

    def evaluate(tu=None):
        r = orig_eval(tu)                     # puts the net into eval mode first
        pred_rec.append(model.predict(test_users).astype(np.float32))
        return r
    model.evaluate = evaluate
    reports = G._record_reports(model)
    best = model.fit()
    torch.Tensor.normal_ = orig_normal
    out.update(_params(net, "1"))
    n_steps = len(users_rec)
    assert n_steps == len(keep_rec) == len(eps_rec) == len(nll_rec) == 9 and len(pred_rec) == 3
    assert [len(u) for u in users_rec] == [24, 24, 15] * 3
    csr = model.train_csr_mat.tocsr()
    csr.sort_indices()
    for u, k in zip(users_rec, keep_rec):
        assert len(k) == csr[u].nnz
    # float64 replay from the recorded draws
    init = {k: out[k + "0"] for k in PARAMS}
    p64, l64, s64 = replay_f64(csr, init, list(zip(users_rec, keep_rec, eps_rec)), CONFIG, 3, test_users)
    dev_p = [float(np.abs(p64[k] - out[k + "1"]).max()) for k in PARAMS]
    dev_s = [float(np.abs(a - b).max()) for a, b in zip(s64, pred_rec)]
    print("f64_dev params", dict(zip(PARAMS, dev_p)), "scores", dev_s)
    print("loss dev", np.abs(l64[:, 0] / np.float64(nll_rec) - 1).max(), np.abs(l64[:, 1] / np.float64(kl_rec) - 1).max())
    for k, v in zip(PARAMS, dev_p):
        if v > 10 * F64_TRIAL[k]:
            raise SystemExit(f"float64 replay differs from the reference by {v:.3g} in {k}: fixture NOT written")
    for v, lim in zip(dev_s, F64_TRIAL["scores"]):
        if v > 10 * lim:
            raise SystemExit(f"float64 replay differs from the reference by {v:.3g} in the scores: fixture NOT written")
    # users whose 22 best scores hold a pair closer than 5e-6 (rankings of the tests leave them out)
    ev = model.evaluator
    close = []
    for sc in pred_rec:
        c = 0
        for r, u in enumerate(test_users):
            row = sc[r].astype(np.float64).copy()
            tr = ev.user_pos_train.get(u, [])
            row[np.asarray(tr, dtype=np.int64)] = -np.inf
            top = np.sort(row)[::-1][:22]
            c += int(np.min(top[:-1] - top[1:]) <= 5e-6)
        close.append(c)
    print("users with a top-22 gap <= 5e-6 per evaluation:", close)
    out.update(step_users=np.concatenate(users_rec), step_sizes=np.int32([len(u) for u in users_rec]),
               keep=np.concatenate(keep_rec), keep_sizes=np.int32([len(k) for k in keep_rec]),
               eps=np.concatenate(eps_rec, 0).astype(np.float32), neg_ll=np.float32(nll_rec), kl=np.float32(kl_rec),
               reports=np.stack(reports), names=np.array(model.evaluator.metrics_list),
               best=np.array(list(best.values()), np.float32), test_users=np.int32(test_users),
               pred=np.stack(pred_rec), f64_dev_params=np.float64(dev_p), f64_dev_scores=np.float64(dev_s),
               close_users=np.int32(close))
    print("multvae: steps", n_steps, "neg_ll", nll_rec[0], nll_rec[-1], "kl", kl_rec[0], kl_rec[-1], "NDCG@10",
          dict(best.items())["NDCG@10"], "max |score|", float(np.abs(pred_rec[-1]).max()))
    np.savez_compressed(os.path.join(HERE, "golden_multvae.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_multvae()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
