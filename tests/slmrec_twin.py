"""Float64 restatement of SLMRec's forward, loss, hand-derived backward, Adam and score (reference: recommender/SLMRec.py:132-177,
337-362, 366-376, 423-432, 488-533) for the tests, in numpy on dense matrices.  Written from the model's equations, shared by the
CPU and GPU tests and by the fixture's generator.

    Dv = V Wv^T + bv;  Dt = T Wt^T + bt                      V, T: the row-normalised feature tables, constants
    P(x) = mean_{k=0..L} A^k x;  Mi = P([E_u; E_i]);  Mv = P([E_u; Dv]);  Mt = P([E_u; Dt])
    user = W_ua [Mi_u | Mv_u | Mt_u] + b_ua;  item = W_ia [Mi_i | Mv_i | Mt_i] + b_ia
    main = CE(normalize(user[u]) normalize(item[i])^T / temp)
    x = g_i_iv(Mi_i[i]);  y = g_v_iv(Mv_i[i]);  v_loss = CE(x y^T / ssl_temp)
    z = g_iva_ivat(g_iv_iva(x));  w = g_t_ivat(Mt_i[i]);  t_loss = CE(z w^T / ssl_temp)
    loss = main + ssl_alpha (v_loss + t_loss)                CE: cross-entropy with the diagonal as labels, mean over the batch

A batch row with an id out of range contributes nothing: it is left out of every sum, and n stays the batch's length.
g_a_iva takes no part in the loss: its gradient is None in the reference, and Adam never touches it.
"""
import numpy as np

from mgcn_twin import Adam64, csr_rows  # noqa: F401

SEED = 2022                    # of the golden run (tests/golden/make_golden_slmrec.py says how it was chosen)
NORM_EPS = 1e-12

LINEARS = ("v_dense", "t_dense", "embedding_item_after_GCN", "embedding_user_after_GCN", "g_i_iv", "g_v_iv", "g_iv_iva", "g_a_iva",
           "g_iva_ivat", "g_t_ivat")
NAMES = ("embedding_user.weight", "embedding_item.weight") + tuple(f"{m}.{p}" for m in LINEARS for p in ("weight", "bias"))
UNTRAINED = ("g_a_iva.weight", "g_a_iva.bias")
TRAINED = tuple(k for k in NAMES if k not in UNTRAINED)
# The two biases whose gradient is ZERO in exact arithmetic: adding one vector b to every row y_k moves every logit of row r of
# x y^T by <x_r, b>, which a row's softmax does not see, so sum_k dL/dy_k = 0 (and likewise for w in z w^T).  What an fp32
# evaluation hands Adam there is rounding noise of about its eps, which the update magnifies to steps of up to lr: the
# reference's own trajectory of these two tensors is that noise.  Nothing else reads it: the loss and every other gradient are
# invariant under the shift.  The fixture's bound on f64_dev_params does not cover them; their recorded deviation (some lr) is
# what the replay's per-tensor multiple then allows.
NOISE_DRIVEN = ("g_v_iv.bias", "g_t_ivat.bias")


# ---- the graph ----------------------------------------------------------------------------------
def pre_adj_values(rowptr, items, num_items):
    """the 'pre' adjacency's values at the CSR's entries as the reference computes them (SLMRec.py:518-526): fp32 factors
    (rowsum + 1e-8) ** -0.5, multiplied left then right, each product rounded to fp32"""
    rows = csr_rows(rowptr)
    du = np.power(np.diff(rowptr).astype(np.float32) + np.float32(1e-08), np.float32(-0.5))
    di = np.power(np.bincount(items, minlength=num_items).astype(np.float32) + np.float32(1e-08), np.float32(-0.5))
    return ((du[rows] * np.float32(1.0)) * di[items]).astype(np.float32)


def dense_block(rowptr, items, num_items, values=None):
    """dense float64 R [U, I]: the user x item block of norm_adj, with recorded ``values`` (R's CSR order) or the restated ones"""
    R = np.zeros((len(rowptr) - 1, num_items), np.float64)
    R[csr_rows(rowptr), items] = np.asarray(pre_adj_values(rowptr, items, num_items) if values is None else values, np.float64)
    return R


def normalize_rows(X):
    """F.normalize(X, dim=1) in the table's own precision (SLMRec.py:448, 453)"""
    X = np.asarray(X)
    return X / np.maximum(np.sqrt((X * X).sum(1, keepdims=True)), X.dtype.type(NORM_EPS))


# ---- the model ----------------------------------------------------------------------------------
def _mean(R, xu, xi, L):
    su, si = xu, xi
    for _ in range(L):
        xu, xi = R @ xi, R.T @ xu
        su, si = su + xu, si + xi
    return su / (L + 1), si / (L + 1)


def _lin(P, name, x):
    return x @ P[name + ".weight"].T + P[name + ".bias"]


def forward_f64(P, R, V, T, L):
    """the full-table part of the forward -> cache: D (the two projected tables), M = ((Mi_u, Mi_i), (Mv_u, Mv_i), (Mt_u, Mt_i))"""
    Eu, Ei = P["embedding_user.weight"], P["embedding_item.weight"]
    D = (_lin(P, "v_dense", V), _lin(P, "t_dense", T))
    M = (_mean(R, Eu, Ei, L), _mean(R, Eu, D[0], L), _mean(R, Eu, D[1], L))
    return {"D": D, "M": M}


def fuse_f64(P, C):
    """(all_users [U, d], all_items [I, d]): the fusion over every row (SLMRec.py:174-175)"""
    M = C["M"]
    return (_lin(P, "embedding_user_after_GCN", np.hstack([M[0][0], M[1][0], M[2][0]])),
            _lin(P, "embedding_item_after_GCN", np.hstack([M[0][1], M[1][1], M[2][1]])))


def nce(a, b, inv_tau, n):
    """(sum_r [log sum_k exp(<a_r, b_k> inv_tau) - <a_r, b_r> inv_tau] / n, d / da, d / db) with the running maximum subtracted"""
    if len(a) == 0:
        return 0.0, np.zeros_like(a), np.zeros_like(b)
    Lg = a @ b.T * inv_tau
    mx = Lg.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(Lg - mx).sum(1))
    Pm = np.exp(Lg - lse[:, None])
    return (lse - np.diag(Lg)).sum() / n, (Pm @ b - b) * (inv_tau / n), (Pm.T @ a - a) * (inv_tau / n)


def _valid(users, pos, nu, ni):
    users, pos = np.asarray(users, np.int64), np.asarray(pos, np.int64)
    ok = (users >= 0) & (users < nu) & (pos >= 0) & (pos < ni)
    return users[ok], pos[ok], len(users)


def gradients_f64(P, R, V, T, users, pos, cfg, use_main=True, use_v=True, use_t=True, cache=None):
    """-> ((main, ssl_alpha v_loss, ssl_alpha t_loss), {name: gradient}, cache): the backward by hand, no autograd.  The gradient of
    g_a_iva is zero.  The three switches take a term out (the generator's sensitivity checks)"""
    L, alpha = cfg["layer_num"], cfg["ssl_alpha"]
    C = forward_f64(P, R, V, T, L) if cache is None else cache
    nu, ni = R.shape
    u, i, n = _valid(users, pos, nu, ni)
    G = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in P.items()}
    if n == 0 or len(u) == 0:
        return (0.0, 0.0, 0.0), G, C
    M = C["M"]
    cat_u = np.hstack([M[0][0][u], M[1][0][u], M[2][0][u]])
    cat_i = np.hstack([M[0][1][i], M[1][1][i], M[2][1][i]])
    d = P["embedding_user.weight"].shape[1]
    user, item = _lin(P, "embedding_user_after_GCN", cat_u), _lin(P, "embedding_item_after_GCN", cat_i)
    na = np.maximum(np.linalg.norm(user, axis=1, keepdims=True), NORM_EPS)
    nb = np.maximum(np.linalg.norm(item, axis=1, keepdims=True), NORM_EPS)
    uh, ih = user / na, item / nb
    main, duh, dih = nce(uh, ih, 1.0 / cfg["temp"], n)
    x, y = _lin(P, "g_i_iv", M[0][1][i]), _lin(P, "g_v_iv", M[1][1][i])
    v_loss, dx, dy = nce(x, y, 1.0 / cfg["ssl_temp"], n)
    x2 = _lin(P, "g_iv_iva", x)
    z, w = _lin(P, "g_iva_ivat", x2), _lin(P, "g_t_ivat", M[2][1][i])
    t_loss, dz, dw = nce(z, w, 1.0 / cfg["ssl_temp"], n)
    sm, sv, st = float(use_main), alpha * float(use_v), alpha * float(use_t)
    comps = (sm * main, sv * v_loss, st * t_loss)
    # the main term through the normalisation and the fusion
    d_user = sm * (duh - uh * (uh * duh).sum(1, keepdims=True)) / na
    d_item = sm * (dih - ih * (ih * dih).sum(1, keepdims=True)) / nb
    G["embedding_user_after_GCN.weight"], G["embedding_user_after_GCN.bias"] = d_user.T @ cat_u, d_user.sum(0)
    G["embedding_item_after_GCN.weight"], G["embedding_item_after_GCN.bias"] = d_item.T @ cat_i, d_item.sum(0)
    d_cat_u = d_user @ P["embedding_user_after_GCN.weight"]
    d_cat_i = d_item @ P["embedding_item_after_GCN.weight"]
    # the chain
    dx, dy, dz, dw = sv * dx, sv * dy, st * dz, st * dw
    G["g_iva_ivat.weight"], G["g_iva_ivat.bias"] = dz.T @ x2, dz.sum(0)
    dx2 = dz @ P["g_iva_ivat.weight"]
    G["g_iv_iva.weight"], G["g_iv_iva.bias"] = dx2.T @ x, dx2.sum(0)
    dx = dx + dx2 @ P["g_iv_iva.weight"]
    G["g_i_iv.weight"], G["g_i_iv.bias"] = dx.T @ M[0][1][i], dx.sum(0)
    G["g_v_iv.weight"], G["g_v_iv.bias"] = dy.T @ M[1][1][i], dy.sum(0)
    G["g_t_ivat.weight"], G["g_t_ivat.bias"] = dw.T @ M[2][1][i], dw.sum(0)
    fac = (dx @ P["g_i_iv.weight"], dy @ P["g_v_iv.weight"], dw @ P["g_t_ivat.weight"])
    # the three tables' gradient rows, then the mean's backward (A is symmetric: the same operator)
    back = []
    for t in range(3):
        gu, gi = np.zeros((nu, d)), np.zeros((ni, d))
        np.add.at(gu, u, d_cat_u[:, t * d:(t + 1) * d])
        np.add.at(gi, i, d_cat_i[:, t * d:(t + 1) * d] + fac[t])
        back.append(_mean(R, gu, gi, L))
    G["embedding_user.weight"] = (back[0][0] + back[1][0]) + back[2][0]
    G["embedding_item.weight"] = back[0][1]
    for name, X, dD in (("v_dense", V, back[1][1]), ("t_dense", T, back[2][1])):
        G[name + ".weight"], G[name + ".bias"] = dD.T @ X, dD.sum(0)
    return comps, G, C


def gradients_torch(P, R, V, T, users, pos, cfg, dtype="float64"):
    """the same loss and gradient by torch autograd on the CPU in ``dtype``, written with the reference's torch ops -> ((main,
    ssl_alpha v_loss, ssl_alpha t_loss), {name: gradient of the trained tensors}).  In float32 (every operand rounded first): what
    an fp32 evaluation is worth against ``gradients_f64``"""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    t_ = lambda a, grad=False: torch.tensor(np.asarray(a), dtype=dt, requires_grad=grad)      # noqa: E731
    Q = {k: t_(v, k in TRAINED) for k, v in P.items()}
    Rt, Vt, Tt = t_(R), t_(V), t_(T)
    nu, ni = R.shape
    u, i, n = _valid(users, pos, nu, ni)
    u, i = torch.as_tensor(u), torch.as_tensor(i)
    lin = lambda name, x: Fn.linear(x, Q[name + ".weight"], Q[name + ".bias"])      # noqa: E731
    A = torch.zeros((nu + ni, nu + ni), dtype=dt)
    A[:nu, nu:], A[nu:, :nu] = Rt, Rt.T

    def graph(ue, ie):
        e = torch.cat([ue, ie])
        embs = [e]
        for _ in range(cfg["layer_num"]):
            e = A @ e
            embs.append(e)
        return torch.split(torch.mean(torch.stack(embs, 1), 1), [nu, ni])
    Eu = Q["embedding_user.weight"]
    Mi, Mv, Mt = graph(Eu, Q["embedding_item.weight"]), graph(Eu, lin("v_dense", Vt)), graph(Eu, lin("t_dense", Tt))
    user = lin("embedding_user_after_GCN", torch.cat([Mi[0], Mv[0], Mt[0]], 1))[u]
    item = lin("embedding_item_after_GCN", torch.cat([Mi[1], Mv[1], Mt[1]], 1))[i]

    def ce(lg):
        return (torch.logsumexp(lg, 1) - torch.diagonal(lg)).sum() / n
    main = ce(Fn.normalize(user, dim=1) @ Fn.normalize(item, dim=1).T / cfg["temp"])
    x, y = lin("g_i_iv", Mi[1][i]), lin("g_v_iv", Mv[1][i])
    v_loss = ce(x @ y.T / cfg["ssl_temp"])
    z, w = lin("g_iva_ivat", lin("g_iv_iva", x)), lin("g_t_ivat", Mt[1][i])
    t_loss = ce(z @ w.T / cfg["ssl_temp"])
    comps = (main, cfg["ssl_alpha"] * v_loss, cfg["ssl_alpha"] * t_loss)
    (comps[0] + comps[1] + comps[2]).backward()
    return tuple(float(c.detach()) for c in comps), {k: Q[k].grad.numpy() for k in TRAINED}


def scores_f64(P, C, users):
    """the raw ranking scores all_users[users] all_items^T of a forward's cache (SLMRec.py:366-370 before the sigmoid)"""
    au, ai = fuse_f64(P, C)
    return au[np.asarray(users)] @ ai.T


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def schedule_lr(cfg, epoch, lr_scheduler=(1.0, 50)):
    """LambdaLR with the fixed lr_scheduler = [1.0, 50] (SLMRec.py:545-547): constant, the expression kept"""
    return cfg["lr"] * lr_scheduler[0] ** (epoch / lr_scheduler[1])


def replay_f64(R, V, T, init, steps, cfg, steps_per_epoch, test_users, **switches):
    """the whole run in float64 -> (parameters dict, [total loss], [raw scores per evaluation]); an evaluation after every
    ``steps_per_epoch`` steps ranks on the LAST TRAINING FORWARD, that is with the parameters before the last update"""
    P = {k: np.asarray(v, np.float64).copy() for k, v in init.items()}
    opt = Adam64({k: P[k] for k in TRAINED})
    losses, scores = [], []
    for s, st in enumerate(steps):
        comps, G, C = gradients_f64(P, R, V, T, st["users"], st["pos"], cfg, **switches)
        before = {k: P[k] for k in ("embedding_user_after_GCN.weight", "embedding_user_after_GCN.bias",
                                    "embedding_item_after_GCN.weight", "embedding_item_after_GCN.bias")}
        Q = {k: P[k] for k in TRAINED}
        opt.step(Q, {k: G[k] for k in TRAINED}, schedule_lr(cfg, s // steps_per_epoch))
        P.update(Q)
        losses.append(sum(comps))
        if (s + 1) % steps_per_epoch == 0:
            scores.append(scores_f64(before, C, test_users))
    return P, np.array(losses), scores


# ---- the fixture ----------------------------------------------------------------------------------
def _key(name, which):
    return f"{name.replace('.', '_')}_{which}"


def fixture_params(g, which):
    """the recorded parameters: which = 0 (initial) or 1 (final)"""
    return {k: g[_key(k, which)] for k in NAMES}


def fixture_steps(g):
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    return [dict(users=g["step_users"][b[s]:b[s + 1]], pos=g["step_pos"][b[s]:b[s + 1]]) for s in range(len(g["step_sizes"]))]


def fixture_config(g):
    import json
    return json.loads(str(g["config"]))


def fixture_graph(g):
    """R dense float64 from the recorded values"""
    nu, ni = int(g["shape"][0]), int(g["shape"][1])
    R = np.zeros((nu, ni), np.float64)
    R[g["adj_rows"], g["adj_cols"]] = g["adj_val"].astype(np.float64)
    return R


def fixture_features(g):
    """(V, T): the reference's normalised fp32 tables as float64"""
    return g["v_feat"].astype(np.float64), g["t_feat"].astype(np.float64)


def shapes(nu, ni, d, Fv, Ft):
    s = {"embedding_user.weight": (nu, d), "embedding_item.weight": (ni, d), "v_dense.weight": (d, Fv), "t_dense.weight": (d, Ft),
         "embedding_item_after_GCN.weight": (d, 3 * d), "embedding_user_after_GCN.weight": (d, 3 * d)}
    for m in ("g_i_iv", "g_v_iv", "g_iv_iva", "g_a_iva"):
        s[m + ".weight"] = (d, d)
    for m in ("g_iva_ivat", "g_t_ivat"):
        s[m + ".weight"] = (d // 2, d)
    for m in LINEARS:
        s[m + ".bias"] = (s[m + ".weight"][0],)
    return {k: s[k] for k in NAMES}


def random_case(seed=0, nu=5, ni=7, d=6, Fv=5, Ft=3, L=2, scale=0.5):
    """a small random model: (P, R, V, T, cfg, rowptr, items)"""
    rng = np.random.default_rng(seed)
    A = (rng.random((nu, ni)) < 0.45).astype(np.int64)
    A[np.arange(nu), rng.integers(0, ni, nu)] = 1
    rowptr = np.concatenate([[0], np.cumsum(A.sum(1))]).astype(np.int64)
    items = np.concatenate([np.nonzero(r)[0] for r in A]).astype(np.int32)
    R = dense_block(rowptr, items, ni)
    P = {k: rng.standard_normal(s) * scale for k, s in shapes(nu, ni, d, Fv, Ft).items()}
    V, T = normalize_rows(rng.standard_normal((ni, Fv))), normalize_rows(rng.standard_normal((ni, Ft)))
    cfg = dict(lr=1e-2, layer_num=L, ssl_alpha=0.5, ssl_temp=0.1, temp=0.2)
    return P, R, V, T, cfg, rowptr, items
