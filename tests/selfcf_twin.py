"""Float64 restatement of SelfCF's training step and score (reference: recommender/SelfCF.py:118-168, 205-241) for the tests:
torch autograd on dense blocks of the masked adjacency [[0, R1], [R2^T, 0]], plus a numpy mirror of the keep permutation of
``skr_selfcf_keeps``.  Written from the model's equations, shared by the CPU and GPU tests and by the fixture's generator."""
import numpy as np
import torch

F64 = torch.float64
EPS = 1e-8


def t64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad)


def csr_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def normalised_values(rowptr, items, num_items):
    """float64 (rowdeg + 1e-7)^-0.5 * (coldeg + 1e-7)^-0.5 at the CSR's entries (SelfCF.py:118-123)"""
    rows = csr_rows(rowptr)
    du = np.power(np.diff(rowptr).astype(np.float64) + 1e-7, -0.5)
    di = np.power(np.bincount(items, minlength=num_items).astype(np.float64) + 1e-7, -0.5)
    return du[rows] * di[items]


def transpose_order(rowptr, items):
    """(order, perm): order[t] = the entry of R at position t of R^T's order (by item, then by user); perm = its inverse"""
    rows = csr_rows(rowptr)
    order = np.lexsort((rows, items))
    perm = np.empty(len(order), np.int64)
    perm[order] = np.arange(len(order))
    return order, perm


def mirror_keeps(perm, k1, k2):
    """the four arrays of skr_selfcf_keeps from k1 (R order) and k2 (R^T order): forward user rows, forward item rows,
    backward user rows (k2 in R order), backward item rows (k1 in R^T order)"""
    k1, k2 = np.asarray(k1, np.uint8), np.asarray(k2, np.uint8)
    bi = np.empty_like(k1)
    bi[perm] = k1
    return k1.copy(), k2.copy(), k2[perm], bi


def masked_blocks(rowptr, items, num_items, val, k1, k2, scale):
    """dense float64 (R1 [U, I], R2t [I, U]) of the masked, rescaled matrix: R1 = val * k1 * scale at R's entries, R2t the
    same values with k2 (R^T order) at the transposed entries; ``val`` in R order"""
    rows = csr_rows(rowptr)
    order, _ = transpose_order(rowptr, items)
    nu = len(rowptr) - 1
    v = np.asarray(val, np.float64)
    R1 = np.zeros((nu, num_items), np.float64)
    R1[rows, items] = v * np.asarray(k1, np.float64) * scale
    R2t = np.zeros((num_items, nu), np.float64)
    R2t[items[order], rows[order]] = v[order] * np.asarray(k2, np.float64) * scale
    return R1, R2t


def cosine(x, y):
    """<x, y> / (max(|x|, 1e-8) max(|y|, 1e-8)): each norm clamped on its own, as F.cosine_similarity does"""
    return (x * y).sum(-1) / (x.norm(dim=-1).clamp_min(EPS) * y.norm(dim=-1).clamp_min(EPS))


def forward_f64(Eu, Ei, R1, R2t, n_layers):
    """-> (M_u, M_i): the means over the layers X_0 .. X_L of X_k = A' X_(k-1) (SelfCF.py:151-159)"""
    xu, xi, su, si = Eu, Ei, Eu, Ei
    for _ in range(n_layers):
        xu, xi = R1 @ xi, R2t @ xu
        su, si = su + xu, si + xi
    return su / (n_layers + 1), si / (n_layers + 1)


def losses_f64(Eu, Ei, W, b, R1, R2t, users, items, ku, ki, n_layers, dropout, reg, n_div=None):
    """-> ((cosine part, reg part), M_u, M_i) of one step (SelfCF.py:205-233); ku / ki: [n, d] keep flags of the targets;
    ``n_div``: the divisor of the two means when it is not the number of rows handed in (rows the kernel skips leave n)"""
    Mu, Mi = forward_f64(Eu, Ei, R1, R2t, n_layers)
    users, items = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (users, items))
    u, i = Mu[users], Mi[items]
    tu = (u * torch.as_tensor(np.asarray(ku), dtype=u.dtype) / (1.0 - dropout)).detach()
    ti = (i * torch.as_tensor(np.asarray(ki), dtype=i.dtype) / (1.0 - dropout)).detach()
    pu, pi = u @ W.T + b, i @ W.T + b
    if n_div is None:
        cos = -cosine(pu, ti).mean() / 2 - cosine(pi, tu).mean() / 2
    else:
        cos = -cosine(pu, ti).sum() / n_div / 2 - cosine(pi, tu).sum() / n_div / 2
    regl = reg * 0.5 * ((u ** 2).sum() + (i ** 2).sum())
    return (cos, regl), Mu, Mi


def scores_f64(Mu, Mi, W, b, users):
    """the reference's full_sort_predict (SelfCF.py:235-241): (W u + b).i + u.(W i + b)"""
    u = Mu[np.asarray(users)]
    return (u @ W.T + b) @ Mi.T + u @ (Mi @ W.T + b).T


def folded_scores_f64(Mu, Mi, W, b, users):
    """the same score as the kernels rank it: u^T (W + W^T) i + <b, i> + <b, u>"""
    u = Mu[np.asarray(users)]
    return (u @ (W + W.T).T) @ Mi.T + (Mi @ b)[None, :] + (u @ b)[:, None]


def replay_f64(csr, val, init, steps, cfg, eval_every, test_users):
    """the whole run in float64 with torch.optim.Adam -> (parameters dict, [total loss], [scores per evaluation]).
    ``csr`` = (rowptr, items, num_items); ``steps``: dicts with users, items, rate, k1, k2, ku, ki; every evaluation
    propagates the CURRENT parameters through the un-dropped matrix"""
    rowptr, items, ni = csr
    P = {k: t64(v, True) for k, v in init.items()}
    opt = torch.optim.Adam(list(P.values()), lr=cfg["lr"])
    L, ones = cfg["n_layers"], np.ones(len(items))
    R1p, R2tp = (t64(a) for a in masked_blocks(rowptr, items, ni, val, ones, ones, 1.0))
    losses, scores = [], []
    for s, st in enumerate(steps):
        scale = float(np.float32(1.0 / (1.0 - float(st["rate"]))))
        R1, R2t = (t64(a) for a in masked_blocks(rowptr, items, ni, val, st["k1"], st["k2"], scale))
        (cos, regl), _, _ = losses_f64(P["user_emb"], P["item_emb"], P["predictor.weight"], P["predictor.bias"], R1, R2t, st["users"],
                                       st["items"], st["ku"], st["ki"], L, cfg["dropout"], cfg["reg"])
        loss = cos + regl
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if (s + 1) % eval_every == 0:
            with torch.no_grad():
                Mu, Mi = forward_f64(P["user_emb"], P["item_emb"], R1p, R2tp, L)
                scores.append(scores_f64(Mu, Mi, P["predictor.weight"], P["predictor.bias"], test_users).numpy())
    return {k: v.detach().numpy() for k, v in P.items()}, np.array(losses), scores


PARAMS = ("user_emb", "item_emb", "predictor.weight", "predictor.bias")


def fixture_steps(g):
    """per step a dict (users, items, rate, k1, k2, ku, ki) from golden_selfcf.npz (flags unpacked)"""
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    nnz, d = int(g["adj_val"].shape[0]), int(g["user_emb_0"].shape[1])
    steps = []
    for s in range(len(g["step_sizes"])):
        n = int(g["step_sizes"][s])
        steps.append(dict(users=g["step_users"][b[s]:b[s + 1]], items=g["step_items"][b[s]:b[s + 1]], rate=float(g["step_rate"][s]),
                          k1=np.unpackbits(g["step_k1"][s])[:nnz], k2=np.unpackbits(g["step_k2"][s])[:nnz],
                          ku=np.unpackbits(g["step_ku"][b[s] * d // 8:b[s + 1] * d // 8])[:n * d].reshape(n, d),
                          ki=np.unpackbits(g["step_ki"][b[s] * d // 8:b[s + 1] * d // 8])[:n * d].reshape(n, d)))
    return steps


def fixture_params(g, which):
    """the recorded parameters: which = 0 (initial) or 1 (final)"""
    return {k: g[f"{k.replace('.', '_')}_{which}"] for k in PARAMS}


def tiny_csr(d):
    """(rowptr, items ascending, num_items) of tiny_dataset.npz's train split"""
    tr = d["train"]
    nu, ni = int(d["num_users"]), int(d["num_items"])
    rows = [[] for _ in range(nu)]
    for u, i, _ in tr:
        rows[int(u)].append(int(i))
    rowptr = np.zeros(nu + 1, np.int64)
    rowptr[1:] = np.cumsum([len(set(r)) for r in rows])
    items = np.concatenate([np.array(sorted(set(r)), np.int32) for r in rows])
    return rowptr, items.astype(np.int32), ni
