"""Float64 restatement of MultVAE's training step (reference: recommender/MultVAE.py:99-136,187-201) for the tests:
torch autograd on dense inputs, draws handed in.  Written from the model's equations, shared by the CPU and GPU tests."""
import numpy as np
import torch

PARAMS = ("Wq", "bq", "Wp", "bp")


def dense_rows(rowptr, items, users, n_items):
    """float64 [len(users), n_items] binary rows of the CSR"""
    x = np.zeros((len(users), n_items), np.float64)
    for r, u in enumerate(users):
        x[r, items[rowptr[u]:rowptr[u + 1]]] = 1.0
    return x


def keep_mask(x, keep):
    """the keep flags (one per non-zero, user after user, items ascending) as a dense mask of x's shape"""
    m = np.zeros_like(x)
    m[x != 0] = np.asarray(keep, np.float64)
    return m


def losses_f64(Wq, bq, Wp, bp, x, mask, eps, keep_prob):
    """(neg_ll, kl) of a batch; Wq [2d, I], bq [2d], Wp [I, d], bp [I] float64 tensors; x, mask [B, I], eps [B, d]"""
    d = Wp.shape[1]
    x, mask, eps = (torch.as_tensor(a, dtype=torch.float64) for a in (x, mask, eps))
    h = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) * mask / keep_prob
    e = h @ Wq.T + bq
    mu, logvar = e[:, :d], e[:, d:]
    kl = (0.5 * (-logvar + logvar.exp() + mu ** 2 - 1)).sum(1).mean()
    z = mu + eps * (0.5 * logvar).exp()
    neg_ll = -(torch.log_softmax(z @ Wp.T + bp, dim=-1) * x).sum(-1).mean()
    return neg_ll, kl


def scores_f64(Wq, bq, Wp, bp, x):
    """evaluation scores: no dropout, z = mu"""
    d = Wp.shape[1]
    x = torch.as_tensor(x, dtype=torch.float64)
    h = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return (h @ Wq.T + bq)[:, :d] @ Wp.T + bp


def anneal_at(t, anneal_steps, anneal_cap):
    return min(anneal_cap, t / anneal_steps) if anneal_steps > 0 else anneal_cap


def replay_f64(rowptr, items, n_items, init, steps, cfg, eval_every, test_users):
    """the whole run in float64 with torch.optim.Adam -> (final parameters, [(neg_ll, kl)], [scores per evaluation]);
    ``steps``: (users, keep, eps) per training step; the l2 term 2 * reg * 0.5 * (|Wq|^2 + |Wp|^2) is in the loss"""
    par = [torch.tensor(np.asarray(init[k]), dtype=torch.float64, requires_grad=True) for k in PARAMS]
    opt = torch.optim.Adam(par, lr=cfg["lr"])
    losses, scores = [], []
    for t, (users, keep, eps) in enumerate(steps):
        x = dense_rows(rowptr, items, users, n_items)
        neg_ll, kl = losses_f64(*par, x, keep_mask(x, keep), eps, cfg["keep_prob"])
        loss = neg_ll + anneal_at(t, cfg["anneal_steps"], cfg["anneal_cap"]) * kl \
            + 2 * cfg["reg"] * 0.5 * ((par[0] ** 2).sum() + (par[2] ** 2).sum())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append((neg_ll.item(), kl.item()))
        if (t + 1) % eval_every == 0:
            with torch.no_grad():
                scores.append(scores_f64(*par, dense_rows(rowptr, items, test_users, n_items)).numpy())
    return {k: p.detach().numpy() for k, p in zip(PARAMS, par)}, np.array(losses), scores


def fixture_steps(g):
    """(users, keep, eps) per step from golden_multvae.npz"""
    ub = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    kb = np.concatenate([[0], np.cumsum(g["keep_sizes"])])
    return [(g["step_users"][ub[s]:ub[s + 1]], g["keep"][kb[s]:kb[s + 1]], g["eps"][ub[s]:ub[s + 1]])
            for s in range(len(g["step_sizes"]))]


def tiny_csr(d):
    """(rowptr, items ascending) of tiny_dataset.npz's train split"""
    tr = d["train"]
    nu, ni = int(d["num_users"]), int(d["num_items"])
    rows = [[] for _ in range(nu)]
    for u, i, _ in tr:
        rows[int(u)].append(int(i))
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum([len(set(r)) for r in rows])
    items = np.concatenate([np.array(sorted(set(r)), np.int32) for r in rows])
    return rowptr, items.astype(np.int32), ni
