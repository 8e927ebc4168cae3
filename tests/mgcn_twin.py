"""Float64 restatement of MGCN's graphs, forward, loss, hand-derived backward, Adam with the learning-rate schedule and score
(reference: recommender/MGCN.py:61-110, 213-361, 372-376) for the tests, in numpy on dense matrices.  Written from the
model's equations, shared by the CPU and GPU tests and by the fixture's generator.

    F_m = T_m W_m^T + b_m;  g_m = sigmoid(F_m Wg_m^T + bg_m);  X_m = S_m^n (E_i * g_m);  Z_m = [R X_m; X_m]
    M = mean_{k=0..L} A^k [E_u; E_i]
    a_m = q . tanh(Wc z_m + bc);  w = softmax(a_v, a_t);  c = w_v z_v + w_t z_t;  s_m = z_m - c
    p_v = sigmoid(W_ip M + b_ip);  p_t = sigmoid(W_tp M + b_tp);  side = (p_v s_v + p_t s_t + c) / 3;  out = M + side
    loss = -mean logsigmoid(<o_u, o_i - o_j>) + reg (|o_u|^2 + |o_i|^2 + |o_j|^2) / (2 B)
           + cl_loss (InfoNCE(side[i], M[i]) + InfoNCE(side[u], M[u])),  temperature 0.2, F.normalize's eps 1e-12

A batch row with an id out of range contributes nothing: it is left out of every sum, and B stays the batch's length.
"""
import numpy as np

SEED = 2200                    # of the golden run (tests/golden/make_golden_mgcn.py says how it was chosen)
TAU = 0.2
NORM_EPS = 1e-12

NAMES = ("user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
         "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias",
         "query_common.0.weight", "query_common.0.bias", "query_common.2.weight",
         "gate_v.0.weight", "gate_v.0.bias", "gate_t.0.weight", "gate_t.0.bias",
         "gate_image_prefer.0.weight", "gate_image_prefer.0.bias", "gate_text_prefer.0.weight", "gate_text_prefer.0.bias")
# per modality: (feature table, projection, purifier gate, preference gate)
MODAL = (("image_embedding.weight", "image_trs", "gate_v.0", "gate_image_prefer.0"),
         ("text_embedding.weight", "text_trs", "gate_t.0", "gate_text_prefer.0"))


def csr_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def log_sigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


# ---- the graphs ---------------------------------------------------------------------------------
def norm_adj_values(rowptr, items, num_items):
    """float64 rowdeg^-0.5 * coldeg^-0.5 at the CSR's entries, inf -> 0 (MGCN.py:222-233)"""
    rows = csr_rows(rowptr)
    with np.errstate(divide="ignore"):
        du = np.power(np.diff(rowptr).astype(np.float64), -0.5)
        di = np.power(np.bincount(items, minlength=num_items).astype(np.float64), -0.5)
    du[np.isinf(du)] = 0.0
    di[np.isinf(di)] = 0.0
    return du[rows] * di[items]


def dense_block(rowptr, items, num_items, values=None):
    """dense float64 R [U, I]: the user x item block of norm_adj, with recorded ``values`` (R's CSR order) or the restated ones"""
    R = np.zeros((len(rowptr) - 1, num_items), np.float64)
    R[csr_rows(rowptr), items] = norm_adj_values(rowptr, items, num_items) if values is None else np.asarray(values, np.float64)
    return R


def knn_f64(feat, k):
    """(ids [I, k], sims [I, k]) in float64: cosine similarities of the rows, the k largest per row in descending order, equal
    similarities by ascending id (MGCN.py:61-64, 103)"""
    X = np.asarray(feat, np.float64)
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    S = Xn @ Xn.T
    ids = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return ids, np.take_along_axis(S, ids, 1)


def weighted_graph_values(ids, sims):
    """values [I, k] of the modality graph: s_ij deg_i^-0.5 deg_j^-0.5 with deg the ROW sums of the kept similarities,
    inf -> 0 (MGCN.py:67-80, 'sym')"""
    sims = np.asarray(sims, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.power(sims.sum(1), -0.5)
    r[np.isinf(r)] = 0.0
    return r[:, None] * sims * r[np.asarray(ids, np.int64)]


def dense_graph(ids, vals):
    """dense float64 S [I, I] from neighbour lists and their values"""
    ni = len(ids)
    S = np.zeros((ni, ni), np.float64)
    S[np.repeat(np.arange(ni), ids.shape[1]), np.asarray(ids, np.int64).reshape(-1)] = np.asarray(vals, np.float64).reshape(-1)
    return S


# ---- the model ----------------------------------------------------------------------------------
def forward_f64(P, R, S, Lu, Ln):
    """the full forward -> cache dict with M, Z (per modality), the fuser's intermediates, side and out, all [U + I, d].
    ``S`` = (S_v, S_t)"""
    Eu, Ei = P["user_embedding.weight"], P["item_id_embedding.weight"]
    C = {"F": [], "g": [], "Z": []}
    for m, (tab, trs, gate, _) in enumerate(MODAL):
        F = P[tab] @ P[trs + ".weight"].T + P[trs + ".bias"]
        g = sigmoid(F @ P[gate + ".weight"].T + P[gate + ".bias"])
        X = Ei * g
        for _ in range(Ln):
            X = S[m] @ X
        C["F"].append(F); C["g"].append(g); C["Z"].append(np.vstack([R @ X, X]))
    xu, xi, su, si = Eu, Ei, Eu, Ei
    for _ in range(Lu):
        xu, xi = R @ xi, R.T @ xu
        su, si = su + xu, si + xi
    M = np.vstack([su, si]) / (Lu + 1)
    Wc, bc, q = P["query_common.0.weight"], P["query_common.0.bias"], P["query_common.2.weight"].reshape(-1)
    h = [np.tanh(Z @ Wc.T + bc) for Z in C["Z"]]
    a = [hh @ q for hh in h]
    mx = np.maximum(a[0], a[1])
    e = [np.exp(a[0] - mx), np.exp(a[1] - mx)]
    w = [e[0] / (e[0] + e[1]), e[1] / (e[0] + e[1])]
    c = w[0][:, None] * C["Z"][0] + w[1][:, None] * C["Z"][1]
    s = [C["Z"][0] - c, C["Z"][1] - c]
    p = [sigmoid(M @ P[MODAL[m][3] + ".weight"].T + P[MODAL[m][3] + ".bias"]) for m in range(2)]
    side = (p[0] * s[0] + p[1] * s[1] + c) / 3.0
    C.update(M=M, h=h, w=w, c=c, s=s, p=p, side=side, out=M + side)
    return C


def info_nce(a, b, n):
    """(sum_r [-<a_r, b_r> / tau + log sum_k exp(<a_r, b_k> / tau)] / n over the normalised rows, d / da, d / db)"""
    if len(a) == 0:
        return 0.0, np.zeros_like(a), np.zeros_like(b)
    na = np.maximum(np.linalg.norm(a, axis=1, keepdims=True), NORM_EPS)
    nb = np.maximum(np.linalg.norm(b, axis=1, keepdims=True), NORM_EPS)
    ah, bh = a / na, b / nb
    L = ah @ bh.T / TAU
    mx = L.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(L - mx).sum(1))
    loss = (lse - np.diag(L)).sum() / n
    Pm = np.exp(L - lse[:, None])
    dah = (Pm @ bh - bh) / (n * TAU)
    dbh = (Pm.T @ ah - ah) / (n * TAU)
    da = (dah - ah * (ah * dah).sum(1, keepdims=True)) / na
    db = (dbh - bh * (bh * dbh).sum(1, keepdims=True)) / nb
    return loss, da, db


def _valid(users, pos, neg, nu, ni):
    users, pos, neg = (np.asarray(x, np.int64) for x in (users, pos, neg))
    ok = (users >= 0) & (users < nu) & (pos >= 0) & (pos < ni) & (neg >= 0) & (neg < ni)
    return users[ok], pos[ok], neg[ok], len(users)


def losses_f64(P, R, S, users, pos, neg, cfg, cache=None):
    """-> (bpr, regulariser, cl_loss * InfoNCE terms) of one batch"""
    C = forward_f64(P, R, S, cfg["n_ui_layers"], cfg["n_layers"]) if cache is None else cache
    nu, ni = R.shape
    u, i, j, n = _valid(users, pos, neg, nu, ni)
    if n == 0:
        return 0.0, 0.0, 0.0
    out, side, M = C["out"], C["side"], C["M"]
    ou, oi, oj = out[u], out[nu + i], out[nu + j]
    bpr = -log_sigmoid((ou * (oi - oj)).sum(1)).sum() / n
    reg = cfg["reg"] * ((ou ** 2).sum() + (oi ** 2).sum() + (oj ** 2).sum()) / (2.0 * n)
    cl = info_nce(side[nu + i], M[nu + i], n)[0] + info_nce(side[u], M[u], n)[0]
    return bpr, reg, cfg["cl_loss"] * cl


def gradients_f64(P, R, S, users, pos, neg, cfg):
    """-> ((bpr, regulariser, cl_loss * InfoNCE), {name: gradient}): the backward by hand, no autograd"""
    Lu, Ln = cfg["n_ui_layers"], cfg["n_layers"]
    C = forward_f64(P, R, S, Lu, Ln)
    comps = losses_f64(P, R, S, users, pos, neg, cfg, C)
    nu, ni = R.shape
    u, i, j, n = _valid(users, pos, neg, nu, ni)
    G = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in P.items()}
    if n == 0:
        return comps, G
    out, side, M, Z = C["out"], C["side"], C["M"], C["Z"]
    d_out, d_side, d_M = np.zeros_like(out), np.zeros_like(out), np.zeros_like(out)
    ou, oi, oj = out[u], out[nu + i], out[nu + j]
    x = (ou * (oi - oj)).sum(1)
    c = (-sigmoid(-x) / n)[:, None]
    r = cfg["reg"] / n
    np.add.at(d_out, u, c * (oi - oj) + r * ou)
    np.add.at(d_out, nu + i, c * ou + r * oi)
    np.add.at(d_out, nu + j, -c * ou + r * oj)
    for idx in (nu + i, u):
        _, da, db = info_nce(side[idx], M[idx], n)
        np.add.at(d_side, idx, cfg["cl_loss"] * da)
        np.add.at(d_M, idx, cfg["cl_loss"] * db)
    d_side += d_out
    d_M += d_out
    # the fuser
    Wc, q = P["query_common.0.weight"], P["query_common.2.weight"].reshape(-1)
    h, w, s, p = C["h"], C["w"], C["s"], C["p"]
    ds = d_side / 3.0
    d_p = [ds * s[0], ds * s[1]]
    d_s = [ds * p[0], ds * p[1]]
    d_c = ds - d_s[0] - d_s[1]
    dZ = [d_s[m] + w[m][:, None] * d_c for m in range(2)]
    d_w = [(d_c * Z[m]).sum(1) for m in range(2)]
    d_a0 = w[0] * w[1] * (d_w[0] - d_w[1])
    d_a = [d_a0, -d_a0]
    G["query_common.2.weight"] = (d_a[0][:, None] * h[0] + d_a[1][:, None] * h[1]).sum(0).reshape(P["query_common.2.weight"].shape)
    for m in range(2):
        d_pre = d_a[m][:, None] * q * (1.0 - h[m] ** 2)
        G["query_common.0.weight"] += d_pre.T @ Z[m]
        G["query_common.0.bias"] += d_pre.sum(0)
        dZ[m] = dZ[m] + d_pre @ Wc
        pref = MODAL[m][3]
        d_pp = d_p[m] * p[m] * (1.0 - p[m])
        G[pref + ".weight"] = d_pp.T @ M
        G[pref + ".bias"] = d_pp.sum(0)
        d_M = d_M + d_pp @ P[pref + ".weight"]
    # the item-item view and the purifier
    Ei = P["item_id_embedding.weight"]
    d_Ei = np.zeros_like(Ei)
    for m, (tab, trs, gate, _) in enumerate(MODAL):
        dX = dZ[m][nu:] + R.T @ dZ[m][:nu]
        for _ in range(Ln):
            dX = S[m].T @ dX
        g, F = C["g"][m], C["F"][m]
        d_Ei += dX * g
        dz = dX * Ei * g * (1.0 - g)
        G[gate + ".weight"] = dz.T @ F
        G[gate + ".bias"] = dz.sum(0)
        dF = dz @ P[gate + ".weight"]
        G[trs + ".weight"] = dF.T @ P[tab]
        G[trs + ".bias"] = dF.sum(0)
        G[tab] = dF @ P[trs + ".weight"]
    # the user-item view
    tu, ti = d_M[:nu], d_M[nu:]
    au, ai = tu, ti
    for _ in range(Lu):
        tu, ti = R @ ti, R.T @ tu
        au, ai = au + tu, ai + ti
    G["user_embedding.weight"] = au / (Lu + 1)
    G["item_id_embedding.weight"] = ai / (Lu + 1) + d_Ei
    return comps, G


def gradients_f32_torch(P, R, S, users, pos, neg, cfg):
    """the same gradient by torch autograd on the CPU in float32, every operand rounded to fp32 first: what an fp32
    evaluation of these quantities is worth against ``gradients_f64`` -- the yardstick of a tensor whose gradient is a sum of
    terms that nearly cancel -> {name: gradient}"""
    import torch
    import torch.nn.functional as Fn
    t32 = lambda a, grad=False: torch.tensor(np.asarray(a, np.float32), requires_grad=grad)      # noqa: E731
    Q = {k: t32(v, True) for k, v in P.items()}
    Rt, St = t32(R), (t32(S[0]), t32(S[1]))
    nu, ni = R.shape
    u, i, j, n = (torch.as_tensor(x) if isinstance(x, np.ndarray) else x for x in _valid(users, pos, neg, nu, ni))
    Eu, Ei = Q["user_embedding.weight"], Q["item_id_embedding.weight"]
    Z = []
    for m, (tab, trs, gate, _) in enumerate(MODAL):
        F = Fn.linear(Q[tab], Q[trs + ".weight"], Q[trs + ".bias"])
        X = Ei * torch.sigmoid(Fn.linear(F, Q[gate + ".weight"], Q[gate + ".bias"]))
        for _ in range(cfg["n_layers"]):
            X = St[m] @ X
        Z.append(torch.cat([Rt @ X, X]))
    xu, xi, su, si = Eu, Ei, Eu, Ei
    for _ in range(cfg["n_ui_layers"]):
        xu, xi = Rt @ xi, Rt.T @ xu
        su, si = su + xu, si + xi
    M = torch.cat([su, si]) / (cfg["n_ui_layers"] + 1)
    att = torch.cat([Fn.linear(torch.tanh(Fn.linear(z, Q["query_common.0.weight"], Q["query_common.0.bias"])), Q["query_common.2.weight"])
                     for z in Z], -1)
    w = torch.softmax(att, -1)
    c = w[:, :1] * Z[0] + w[:, 1:] * Z[1]
    p = [torch.sigmoid(Fn.linear(M, Q[MODAL[m][3] + ".weight"], Q[MODAL[m][3] + ".bias"])) for m in range(2)]
    side = (p[0] * (Z[0] - c) + p[1] * (Z[1] - c) + c) / 3
    out = M + side
    ou, oi, oj = out[u], out[nu + i], out[nu + j]
    loss = -Fn.logsigmoid((ou * oi).sum(1) - (ou * oj).sum(1)).sum() / n
    loss = loss + cfg["reg"] * (0.5 * (ou ** 2).sum() + 0.5 * (oi ** 2).sum() + 0.5 * (oj ** 2).sum()) / n
    for idx in (nu + i, u):
        a, b = Fn.normalize(side[idx], dim=1), Fn.normalize(M[idx], dim=1)
        loss = loss + cfg["cl_loss"] * (torch.logsumexp(a @ b.T / TAU, 1) - (a * b).sum(1) / TAU).sum() / n
    loss.backward()
    return {k: v.grad.numpy() for k, v in Q.items()}


def scores_f64(P, R, S, cfg, users):
    C = forward_f64(P, R, S, cfg["n_ui_layers"], cfg["n_layers"])
    nu = R.shape[0]
    return C["out"][:nu][np.asarray(users)] @ C["out"][nu:].T


def schedule_lr(cfg, epoch):
    """the learning rate of epoch ``epoch``: LambdaLR with lr_scheduler[0] ** (epoch / lr_scheduler[1]) (MGCN.py:373-375)"""
    g, s = cfg["lr_scheduler"]
    return cfg["lr"] * g ** (epoch / s)


class Adam64:
    """torch.optim.Adam's update (no weight decay, no amsgrad) in float64 over a dict of arrays"""

    def __init__(self, P, b1=0.9, b2=0.999, eps=1e-8):
        self.m = {k: np.zeros_like(v) for k, v in P.items()}
        self.v = {k: np.zeros_like(v) for k, v in P.items()}
        self.t, self.b1, self.b2, self.eps = 0, b1, b2, eps

    def step(self, P, G, lr):
        self.t += 1
        c1, c2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for k in P:
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * G[k]
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * G[k] * G[k]
            P[k] = P[k] - (lr / c1) * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(c2) + self.eps)


def replay_f64(R, S, init, steps, cfg, steps_per_epoch, test_users, use_cl=True, use_reg=True, use_schedule=True):
    """the whole run in float64 -> (parameters dict, [total loss], [scores per evaluation]); evaluation and the schedule's
    step after every ``steps_per_epoch`` steps.  The three switches take a term out (the generator's sensitivity checks)"""
    cfg = dict(cfg)
    if not use_cl:
        cfg["cl_loss"] = 0.0
    if not use_reg:
        cfg["reg"] = 0.0
    P = {k: np.asarray(v, np.float64).copy() for k, v in init.items()}
    opt = Adam64(P)
    losses, scores = [], []
    for s, st in enumerate(steps):
        epoch = s // steps_per_epoch
        comps, G = gradients_f64(P, R, S, st["users"], st["pos"], st["neg"], cfg)
        opt.step(P, G, schedule_lr(cfg, epoch) if use_schedule else cfg["lr"])
        losses.append(sum(comps))
        if (s + 1) % steps_per_epoch == 0:
            scores.append(scores_f64(P, R, S, cfg, test_users))
    return P, np.array(losses), scores


# ---- the fixture ----------------------------------------------------------------------------------
def _key(name, which):
    return f"{name.replace('.', '_')}_{which}"


def fixture_params(g, which):
    """the recorded parameters: which = 0 (initial) or 1 (final)"""
    return {k: g[_key(k, which)] for k in NAMES}


def fixture_steps(g):
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    return [dict(users=g["step_users"][b[s]:b[s + 1]], pos=g["step_pos"][b[s]:b[s + 1]], neg=g["step_neg"][b[s]:b[s + 1]])
            for s in range(len(g["step_sizes"]))]


def fixture_config(g):
    import json
    return json.loads(str(g["config"]))


def fixture_graphs(g):
    """(R, (S_v, S_t)) dense float64 from the recorded values"""
    nu, ni = int(g["shape"][0]), int(g["shape"][1])
    R = np.zeros((nu, ni), np.float64)
    R[g["adj_rows"], g["adj_cols"]] = g["adj_val"].astype(np.float64)
    return R, (dense_graph(g["image_knn_ids"], g["image_graph_val"]), dense_graph(g["text_knn_ids"], g["text_graph_val"]))


def tiny_case(seed=0, nu=5, ni=7, d=6, Fv=5, Ft=3, k=3):
    """a small random model for the finite-difference check: (P, R, S, cfg)"""
    rng = np.random.default_rng(seed)
    A = (rng.random((nu, ni)) < 0.45).astype(np.int64)
    A[np.arange(nu), rng.integers(0, ni, nu)] = 1
    rowptr = np.concatenate([[0], np.cumsum(A.sum(1))])
    items = np.concatenate([np.nonzero(r)[0] for r in A]).astype(np.int32)
    R = dense_block(rowptr, items, ni)
    shapes = {"user_embedding.weight": (nu, d), "item_id_embedding.weight": (ni, d), "image_embedding.weight": (ni, Fv),
              "text_embedding.weight": (ni, Ft), "image_trs.weight": (d, Fv), "image_trs.bias": (d,), "text_trs.weight": (d, Ft),
              "text_trs.bias": (d,), "query_common.0.weight": (d, d), "query_common.0.bias": (d,), "query_common.2.weight": (1, d)}
    for gate in ("gate_v.0", "gate_t.0", "gate_image_prefer.0", "gate_text_prefer.0"):
        shapes[gate + ".weight"], shapes[gate + ".bias"] = (d, d), (d,)
    P = {k_: rng.standard_normal(shapes[k_]) * 0.5 for k_ in NAMES}
    S = []
    for tab in ("image_embedding.weight", "text_embedding.weight"):
        ids, sims = knn_f64(P[tab], k)
        S.append(dense_graph(ids, weighted_graph_values(ids, sims)))
    cfg = dict(reg=0.05, cl_loss=0.3, n_ui_layers=2, n_layers=2, lr=1e-2, lr_scheduler=[0.5, 1])
    return P, R, tuple(S), cfg
