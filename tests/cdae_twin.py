"""Float64 restatement of CDAE's training step (reference: recommender/CDAE.py:95-130,168-206) for the tests: torch
autograd on a pair list, draws handed in.  Written from the model's equations, shared by the CPU and GPU tests and by the
fixture's generator."""
import numpy as np
import torch

from multvae_twin import tiny_csr  # noqa: F401  (the tiny set's train CSR)

PARAMS = ("en_embeddings", "en_offset", "de_embeddings", "de_bias", "user_embeddings")


def pairs(rowptr, items, users, negatives):
    """(puser, pitem, plabel) of a batch: per user pos + unique(neg), items ascending (the coalesced order of the encoder's
    input, which the keep flags follow); ``negatives``: the raw draws per user"""
    pu, pi, pl = [], [], []
    for b, u in enumerate(users):
        pos = np.asarray(items[rowptr[u]:rowptr[u + 1]], np.int64)
        neg = np.unique(np.asarray(negatives[b], np.int64))
        assert not np.intersect1d(pos, neg).size
        both = np.concatenate([pos, neg])
        o = np.argsort(both, kind="stable")
        pu.append(np.full(len(both), b, np.int64))
        pi.append(both[o])
        pl.append(np.concatenate([np.ones(len(pos)), np.zeros(len(neg))])[o])
    return np.concatenate(pu), np.concatenate(pi), np.concatenate(pl)


def _act(x, act):
    return torch.sigmoid(x) if act == "sigmoid" else x


def losses_f64(par, users, puser, pitem, plabel, keep, keep_prob, act, pair_ok=None, user_ok=None, l2_items=None, detail=None):
    """(bce sum, l2) of a batch; ``par``: float64 tensors in the reference's shapes, PARAMS order; ``keep``: one flag per
    pair.  l2 = 0.5 (|E_en[J]|^2 + |offset|^2 + |U[users]|^2 + |E_de[J]|^2 + |b[J]|^2), J the distinct items.
    The skipped entries of skr_cdae_step's contract: ``pair_ok`` (bool per pair): a pair that is not ok goes into neither
    the encoder's sum nor the BCE, whatever its item; ``user_ok`` (bool per batch position): a user that is not ok has no U
    row, in h or in l2 (its pairs are masked by the caller); J is the distinct items of the ok pairs unless ``l2_items``
    names them.  The BCE is a sum: no divisor.  ``detail`` (a dict) receives enc [n, d], h [n, d] and r [ok pairs], enc and
    r keeping their gradients, and ``rows``, the ok pairs' numbers"""
    en, off, de, b, U = par
    n = len(users)
    ok = np.ones(len(puser), bool) if pair_ok is None else np.asarray(pair_ok, bool)
    uok = np.ones(n, bool) if user_ok is None else np.asarray(user_ok, bool)
    assert uok[np.asarray(puser)[ok]].all()
    users = torch.as_tensor(np.where(uok, np.asarray(users, np.int64), 0))
    pu, pi = torch.as_tensor(np.asarray(puser, np.int64)[ok]), torch.as_tensor(np.asarray(pitem, np.int64)[ok])
    kept = torch.as_tensor(np.asarray(keep)[ok] != 0)
    enc = torch.zeros((n, en.shape[1]), dtype=torch.float64).index_add(0, pu[kept], en[pi[kept]] / keep_prob)
    urow = U[users] * torch.as_tensor(uok, dtype=torch.float64).unsqueeze(1)
    h = _act(enc + urow + off, act)
    r = (h[pu] * de[pi]).sum(1) + b[pi, 0]
    bce = torch.nn.functional.binary_cross_entropy_with_logits(r, torch.as_tensor(np.asarray(plabel, np.float64)[ok]), reduction="sum")
    J = torch.unique(pi) if l2_items is None else torch.as_tensor(np.asarray(l2_items, np.int64))
    l2 = 0.5 * sum((w ** 2).sum() for w in (en[J], off, urow, de[J], b[J]))
    if detail is not None:
        if enc.requires_grad:
            enc.retain_grad()
            r.retain_grad()
        detail.update(enc=enc, h=h, r=r, rows=np.flatnonzero(ok))
    return bce, l2


def scores_f64(par, rowptr, items, users, act):
    """evaluation scores from the train rows alone: no negatives, no dropout"""
    en, off, de, b, U = par
    enc = torch.stack([en[torch.as_tensor(np.asarray(items[rowptr[u]:rowptr[u + 1]], np.int64))].sum(0) for u in users])
    h = _act(enc + U[torch.as_tensor(np.asarray(users, np.int64))] + off, act)
    return h @ de.T + b[:, 0]


def replay_f64(rowptr, items, init, steps, cfg, eval_every, test_users):
    """the whole run in float64 with torch.optim.Adam -> (final parameters, [(bce, l2)], [scores per evaluation]);
    ``steps``: (users, raw negatives per user, keep flags) per training step"""
    par = [torch.tensor(np.asarray(init[k]), dtype=torch.float64, requires_grad=True) for k in PARAMS]
    opt = torch.optim.Adam(par, lr=cfg["lr"])
    losses, scores = [], []
    for t, (users, negs, keep) in enumerate(steps):
        pu, pi, pl = pairs(rowptr, items, users, negs)
        bce, l2 = losses_f64(par, users, pu, pi, pl, keep, 1 - cfg["dropout"], cfg["hidden_act"])
        opt.zero_grad()
        (bce + cfg["reg"] * l2).backward()
        opt.step()
        losses.append((bce.item(), l2.item()))
        if (t + 1) % eval_every == 0:
            with torch.no_grad():
                scores.append(scores_f64(par, rowptr, items, test_users, cfg["hidden_act"]).numpy())
    return {k: p.detach().numpy() for k, p in zip(PARAMS, par)}, np.array(losses), scores


def fixture_steps(g):
    """(users, raw negatives per user, keep flags, flat raw negatives) per step from golden_cdae.npz"""
    ub = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    nb = np.concatenate([[0], np.cumsum(g["neg_sizes"])])
    kb = np.concatenate([[0], np.cumsum(g["keep_sizes"])])
    out = []
    for s in range(len(g["step_sizes"])):
        negs = [g["neg_raw"][nb[i]:nb[i + 1]] for i in range(ub[s], ub[s + 1])]
        out.append((g["step_users"][ub[s]:ub[s + 1]], negs, g["keep"][kb[s]:kb[s + 1]], g["neg_raw"][nb[ub[s]]:nb[ub[s + 1]]]))
    return out
