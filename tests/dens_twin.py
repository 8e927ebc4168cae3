"""Float64 restatement of one DENS training step (paper: Disentangled Negative Sampling for Collaborative Filtering, WSDM 2023;
reference: recommender/DENS.py) for the tests and the fixture generator: torch autograd on a dense normalised adjacency.
Written from the model's equations.  The per-hop choice of a negative is either computed (arg-max of the gated score, the first
of equal scores) or handed in (an entry of -1 leaves that group to the arg-max)."""
import numpy as np
import torch

F64 = torch.float64
GATES = ("user_gate", "item_gate", "pos_gate", "neg_gate")
NAMES = tuple(f"{g}.{p}" for g in GATES for p in ("weight", "bias")) + ("user_embed", "item_embed")


def t64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad)


def dense_adjacency(rowptr, items, num_items):
    """float64 [U + I, U + I]: the bipartite graph's D^-1/2 A D^-1/2, zero rows for nodes without an edge"""
    nu = len(rowptr) - 1
    rows = np.repeat(np.arange(nu), np.diff(rowptr))
    N = nu + num_items
    A = np.zeros((N, N), np.float64)
    A[rows, nu + np.asarray(items)] = 1.0
    A[nu + np.asarray(items), rows] = 1.0
    deg = A.sum(1)
    dinv = np.zeros(N)
    dinv[deg > 0] = deg[deg > 0] ** -0.5
    return dinv[:, None] * A * dinv[None, :]


def hop_tables(P, A, H):
    """[N, H + 1, d]: X_0 = [user_embed; item_embed], X_h = A X_(h-1)"""
    X = [torch.cat([P["user_embed"], P["item_embed"]], 0)]
    for _ in range(H):
        X.append(A @ X[-1])
    return torch.stack(X, 1)


def _lin(P, name, x):
    return x @ P[name + ".weight"].T + P[name + ".bias"]


def gates_and_scores(P, s, p, c, w, pre=None):
    """s, p [n, H+1, d], c [n, K, H+1, d] -> (gp, p gp, gn, scores [n, K, H+1], scale [n, H+1], arg-max [n, H+1]);
    ``pre`` (a dict) receives the two gates' pre-activations ``a`` and ``z``"""
    a = _lin(P, "item_gate", p) + _lin(P, "user_gate", s)
    gp = torch.sigmoid(a)
    pr = p * gp
    z = _lin(P, "neg_gate", c) + _lin(P, "pos_gate", pr).unsqueeze(1)
    gn = torch.sigmoid(z)
    if pre is not None:
        pre["a"], pre["z"] = a.detach().numpy(), z.detach().numpy()
    with torch.no_grad():
        terms = s.unsqueeze(1) * (w * c - c * gn)
        scores = terms.sum(-1)
        scale = terms.abs().sum(-1).max(1).values
        own = scores.argmax(1)                                          # torch: the first of equal maxima
    return gp, pr, gn, scores, scale, own


def step_f64(P, A, users, pos, cand, H, w, gamma, l2, choices=None, n_div=None):
    """one step's forward on float64 tensors ``P`` (NAMES) -> dict: mf, emb, total (tensors with a graph), choices [n, H + 1]
    (candidate index), scores [n, K, H + 1], scale [n, H + 1] (the group's largest sum of |terms| of a score), x [5, n] (the
    arguments of the five softplus terms), a [n, H + 1, d] and z [n, K, H + 1, d] (the gates' pre-activations).
    A candidate outside [0, num_items) is a zero row; ``n_div``: the divisor of the batch means when it is not the number of
    rows handed in (rows skipped by the kernel leave n as the divisor)"""
    nu, ni = P["user_embed"].shape[0], P["item_embed"].shape[0]
    users, pos, cand = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (users, pos, cand))
    n, K = cand.shape
    nd = n if n_div is None else n_div
    X = hop_tables(P, A, H)
    Xz = torch.cat([X, torch.zeros_like(X[:1])], 0)                     # one more row: the zero row of a candidate out of range
    ci = torch.where((cand >= 0) & (cand < ni), nu + cand, torch.full_like(cand, X.shape[0]))
    s, p, c = X[users], X[nu + pos], Xz[ci]                             # [n, H+1, d], [n, H+1, d], [n, K, H+1, d]
    pre = {}
    gp, pr, gn, scores, scale, own = gates_and_scores(P, s, p, c, w, pre)
    if choices is None:
        choices = own
    else:                                                               # -1: the step's own choice
        choices = torch.as_tensor(np.asarray(choices), dtype=torch.int64)
        choices = torch.where(choices >= 0, choices, own)
    idx = choices.view(n, 1, H + 1, 1).expand(n, 1, H + 1, c.shape[-1])
    cs, gs = c.gather(1, idx).squeeze(1), gn.gather(1, idx).squeeze(1)  # the chosen rows and their gate values
    u, Pm, Nm = s.mean(1), p.mean(1), cs.mean(1)
    Pr, Nr = pr.mean(1), (cs * gs).mean(1)
    Pir, Nir = Pm - Pr, Nm - Nr
    dot = lambda a, b: (a * b).sum(-1)      # noqa: E731
    sp = torch.nn.functional.softplus
    x = [dot(u, Nm) - dot(u, Pm), dot(u, Pir) - dot(u, Pr), dot(u, Nr) - dot(u, Nir), dot(u, Nr) - dot(u, Pr), dot(u, Pir) - dot(u, Nir)]
    mf = sp(x[0]).sum() / nd
    if gamma > 0:
        mf = mf + gamma / 4 * (sp(x[1]).sum() / nd + sp(x[2]).sum() / nd + sp(x[3]).sum() / nd + sp(x[4]).sum() / nd)
    emb = l2 * ((s[:, 0] ** 2).sum() + (p[:, 0] ** 2).sum() + (cs[:, 0] ** 2).sum()) / 2 / nd
    return dict(mf=mf, emb=emb, total=mf + emb, choices=choices.numpy(), own=own.numpy(), scores=scores.numpy(), scale=scale.numpy(),
                x=torch.stack(x).detach().numpy(), a=pre["a"], z=pre["z"])


def margins(scores, scale, cand):
    """per (b, h): (relative margin, best item, runner-up item or -1): the best score minus the best score of a DIFFERENT item,
    over the group's largest sum of |terms|; a group whose candidates are one item has margin inf"""
    scores, cand = np.asarray(scores, np.float64), np.asarray(cand)
    n, K, H1 = scores.shape
    m = np.full((n, H1), np.inf)
    best_item, second_item = np.zeros((n, H1), np.int64), np.full((n, H1), -1, np.int64)
    for b in range(n):
        for h in range(H1):
            sc = scores[b, :, h]
            k = int(np.argmax(sc))
            best_item[b, h] = cand[b, k]
            other = cand[b] != cand[b, k]
            if other.any():
                k2 = int(np.argmax(np.where(other, sc, -np.inf)))
                second_item[b, h] = cand[b, k2]
                m[b, h] = (sc[k] - sc[k2]) / scale[b, h]
    return m, best_item, second_item


def replay_f64(A, init, steps, cfg, choices, eval_every, test_users):
    """the whole run in float64 with torch.optim.Adam and the handed-in choices -> (final parameters {name: ndarray},
    [total loss], [scores per evaluation])"""
    P = {k: t64(init[k], True) for k in NAMES}
    A = t64(A)
    opt = torch.optim.Adam(list(P.values()), lr=cfg["lr"])
    H = cfg["context_hops"]
    nu = P["user_embed"].shape[0]
    steps_per_epoch = eval_every
    losses, scores = [], []
    for t, (users, pos, cand) in enumerate(steps):
        epoch = t // steps_per_epoch
        w = 1.0 - min(1.0, epoch / cfg["warmup"])
        r = step_f64(P, A, users, pos, cand, H, w, cfg["gamma"], cfg["l2"], choices=choices[t])
        opt.zero_grad()
        r["total"].backward()
        opt.step()
        losses.append(r["total"].item())
        if (t + 1) % eval_every == 0:
            with torch.no_grad():
                pooled = hop_tables(P, A, H).mean(1)
                scores.append((pooled[:nu][np.asarray(test_users)] @ pooled[nu:].T).numpy())
    return {k: v.detach().numpy() for k, v in P.items()}, np.array(losses), scores


def fixture_steps(g):
    """(users, pos, cand [n, n_negs], chosen index [n, H + 1], chosen item, margin, runner-up item) per step from golden_dens.npz"""
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    return [tuple(g[k][b[s]:b[s + 1]] for k in ("step_users", "step_pos", "step_cand", "step_choice", "step_item", "step_margin",
                                                "step_second")) for s in range(len(g["step_sizes"]))]


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
