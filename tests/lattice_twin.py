"""Float64 restatement of LATTICE's learned graph, forward, loss, hand-derived backward, its two Adam blocks with the
learning-rate schedule and score (reference: recommender/LATTICE.py:67-85, 171-302, 313-338) for the tests, in numpy.  Written
from the model's equations, shared by the CPU and GPU tests.

    F_m = X_m W_m^T + b_m;  (ids_m, s_m) = the k largest cosine similarities of F_m's rows (the row itself included)
    w = softmax(modal_weight) with both modalities, 1 with one
    L = w0 s_v + w1 s_t on the union pattern;  r = row sums;  q = r^-1/2 (0 where r <= 0)
    S = (1 - lam) q_i L_ij q_j + lam (w0 O_v + w1 O_t);  h = S^n E_i;  item rows = M_i + h_i / max(|h_i|, 1e-12)
    M = mean_{k=0..L} P^k [E_u; E_i] with P = D^-1 (A + I) (lightgcn), or [E_u; E_i] (mf)
    loss = -mean logsigmoid(<u, p - q>) + reg (|u|^2 + |p|^2 + |q|^2) / (2 B)

The graph lives on its entries (``union_graph``): rows, columns, the four provenance slots -- the position of the entry in the
learned image, learned text, frozen image and frozen text list of its row, or -1 -- as the device builds it.  A batch row with
an id out of range contributes nothing: it is left out of every sum, and B stays the batch's length.
"""
import numpy as np

NORM_EPS = 1e-12
NAMES = ("modal_weight", "user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
         "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias")
MODAL = (("image_embedding.weight", "image_trs"), ("text_embedding.weight", "text_trs"))
ROWS = ("user_embedding.weight", "item_id_embedding.weight")


def csr_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def log_sigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def twin_config(lr=1e-4, reg=0.0, lambda_coeff=0.9, n_layers=1, knn_k=10, cf_model="lightgcn", weight_size=(64, 64),
                lr_scheduler=(0.96, 50), **_):
    """the twin's view of a LATTICEConfig's fields: n_ui_layers = len(weight_size)"""
    return dict(lr=lr, reg=reg, lambda_coeff=lambda_coeff, n_layers=n_layers, knn_k=knn_k, cf_model=cf_model,
                n_ui_layers=len(weight_size), lr_scheduler=list(lr_scheduler))


# ---- the graphs ---------------------------------------------------------------------------------
def norm_adj_dense(rowptr, items, num_items):
    """dense float64 P = D^-1 (A + I) on the square [U + I] adjacency: row-normalised, self loops, not symmetric
    (LATTICE.py:171-193)"""
    nu = len(rowptr) - 1
    N = nu + num_items
    A = np.eye(N)
    rows = csr_rows(rowptr)
    A[rows, nu + np.asarray(items, np.int64)] = 1.0
    A[nu + np.asarray(items, np.int64), rows] = 1.0
    return A / A.sum(1, keepdims=True)


def cosine_at(F, ids):
    """the cosine similarities of row i with the rows ids[i] (norms clamped at 1e-12)"""
    Fh = F / np.maximum(np.linalg.norm(F, axis=1, keepdims=True), NORM_EPS)
    return np.einsum("id,ikd->ik", Fh, Fh[np.asarray(ids, np.int64)])


def knn_f64(feat, k):
    """(ids [I, k], sims [I, k]): the k largest cosine similarities per row, descending, equal ones by ascending id"""
    X = np.asarray(feat, np.float64)
    Xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), NORM_EPS)
    ids = np.argsort(-(Xh @ Xh.T), axis=1, kind="stable")[:, :k]
    return ids, cosine_at(X, ids)


def frozen_lists(feat, k):
    """(ids [I, k] ascending per row, values [I, k]) of O_m = deg^-1/2 s deg^-1/2 over the kNN of the raw features, deg the
    row sums of the kept similarities, inf -> 0 (LATTICE.py:142-144): the layout of build_weighted_item_graph's CSR"""
    ids, sims = knn_f64(feat, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.power(sims.sum(1), -0.5)
    r[~np.isfinite(r)] = 0.0
    vals = r[:, None] * sims * r[ids]
    order = np.argsort(ids, axis=1, kind="stable")
    return np.take_along_axis(ids, order, 1), np.take_along_axis(vals, order, 1)


def _pick(G, t):
    """the values of list t at the entries (0 where the entry is not in the list)"""
    v = np.zeros(len(G["col"]))
    if G["lists"][t] is not None:
        m = G["slots"][:, t] >= 0
        v[m] = np.asarray(G["lists"][t][1], np.float64)[G["rows"][m], G["slots"][m, t]]
    return v


def union_graph(lists, w, lam):
    """the mixed graph on the union pattern of the up to four lists of a row (``lists``: four (ids [I, k], values [I, k]) or
    None; an id outside [0, I) is ignored, of a repeated id the first counts) -> dict(rowptr, rows, col, slots [nnz, 4], L, r,
    q, val, lists, w, lam); columns ascend inside a row"""
    first = next(x for x in lists if x is not None)
    I = len(first[0])
    rowptr, col, slots = [0], [], []
    for i in range(I):
        cand = {}
        for t, l in enumerate(lists):
            if l is None:
                continue
            for p, c in enumerate(np.asarray(l[0])[i]):
                c = int(c)
                if 0 <= c < I:
                    s = cand.setdefault(c, [-1] * 4)
                    if s[t] < 0:
                        s[t] = p
        for c in sorted(cand):
            col.append(c)
            slots.append(cand[c])
        rowptr.append(len(col))
    G = dict(rowptr=np.array(rowptr, np.int64), col=np.array(col, np.int64), slots=np.array(slots, np.int64).reshape(-1, 4),
             lists=lists, w=np.asarray(w, np.float64), lam=float(lam), n=I)
    G["rows"] = csr_rows(G["rowptr"])
    w = G["w"]
    G["L"] = w[0] * _pick(G, 0) + w[1] * _pick(G, 1)
    G["r"] = np.bincount(G["rows"], G["L"], I)
    with np.errstate(divide="ignore", invalid="ignore"):
        G["q"] = np.where(G["r"] > 0, np.power(np.where(G["r"] > 0, G["r"], 1.0), -0.5), 0.0)
    frozen = w[0] * _pick(G, 2) + w[1] * _pick(G, 3)
    G["val"] = (1.0 - lam) * G["q"][G["rows"]] * G["L"] * G["q"][G["col"]] + lam * frozen
    return G


def dense_S(G):
    S = np.zeros((G["n"], G["n"]))
    S[G["rows"], G["col"]] = G["val"]
    return S


def graph_backward(G, g, F):
    """the hand-derived backward of ``union_graph`` given g [nnz] = dLoss/dS and the projected rows F = [F_v, F_t] (None:
    absent) -> (dF list, dw [2], dtheta [2])"""
    rows, col, slots, L, q, w, lam, I = G["rows"], G["col"], G["slots"], G["L"], G["q"], G["w"], G["lam"], G["n"]
    a = (1.0 - lam) * g
    t = np.bincount(rows, a * L * q[col], I) + np.bincount(col, a * L * q[rows], I)
    rho = -0.5 * q ** 3 * t
    learned = (slots[:, 0] >= 0) | (slots[:, 1] >= 0)
    dL = np.where(learned, a * q[rows] * q[col] + rho[rows], 0.0)
    dw = np.array([(dL * _pick(G, m)).sum() + lam * (g * _pick(G, 2 + m)).sum() for m in range(2)])
    dtheta = w * (dw - (w * dw).sum())
    dF = []
    for m in range(2):
        if F[m] is None:
            dF.append(None)
            continue
        nrm = np.maximum(np.linalg.norm(F[m], axis=1, keepdims=True), NORM_EPS)
        fh = F[m] / nrm
        msk = slots[:, m] >= 0
        i, j, ds, s = rows[msk], col[msk], (w[m] * dL[msk])[:, None], _pick(G, m)[msk][:, None]
        d = np.zeros_like(F[m])
        np.add.at(d, i, ds * (fh[j] - s * fh[i]) / nrm[i])
        np.add.at(d, j, ds * (fh[i] - s * fh[j]) / nrm[j])
        dF.append(d)
    return dF, dw, dtheta


# ---- the model ----------------------------------------------------------------------------------
def modal_weights(P):
    pr = [tab in P for tab, _ in MODAL]
    if all(pr):
        t = np.asarray(P["modal_weight"], np.float64)
        e = np.exp(t - t.max())
        return e / e.sum()
    return np.array([1.0 if pr[0] else 0.0, 1.0 if pr[1] else 0.0])


def project(P):
    return [P[tab] @ P[trs + ".weight"].T + P[trs + ".bias"] if tab in P else None for tab, trs in MODAL]


def build_graph(P, frozen, cfg, knn=None):
    """the graph of the current parameters; ``frozen``: [(ids, values) or None] per modality; ``knn``: handed-in neighbour
    ids per modality (the similarities are those of the current rows)"""
    F = project(P)
    lists = [None] * 4
    for m in range(2):
        if F[m] is None:
            continue
        ids = knn_f64(F[m], cfg["knn_k"])[0] if knn is None else np.asarray(knn[m], np.int64)
        lists[m], lists[2 + m] = (ids, cosine_at(F[m], ids)), frozen[m]
    G = union_graph(lists, modal_weights(P), cfg["lambda_coeff"])
    G["F"] = F
    return G


def forward_f64(P, A, S, cfg):
    """-> cache: M [U + I, d], the layers hs of h, the normalised y and its norm, the output tables"""
    Eu, Ei = P["user_embedding.weight"], P["item_id_embedding.weight"]
    nu, Lu = len(Eu), cfg["n_ui_layers"] if cfg["cf_model"] == "lightgcn" else 0
    E = np.vstack([Eu, Ei])
    X = acc = E
    for _ in range(Lu):
        X = A @ X
        acc = acc + X
    M = acc / (Lu + 1)
    hs = [Ei]
    for _ in range(cfg["n_layers"]):
        hs.append(S @ hs[-1])
    nrm = np.maximum(np.linalg.norm(hs[-1], axis=1, keepdims=True), NORM_EPS)
    y = hs[-1] / nrm
    return dict(M=M, hs=hs, nrm=nrm, y=y, out_u=M[:nu], out_i=M[nu:] + y, Lu=Lu)


def _valid(users, pos, neg, nu, ni):
    users, pos, neg = (np.asarray(x, np.int64) for x in (users, pos, neg))
    ok = (users >= 0) & (users < nu) & (pos >= 0) & (pos < ni) & (neg >= 0) & (neg < ni)
    return users[ok], pos[ok], neg[ok], len(users)


def losses_f64(P, A, frozen, users, pos, neg, cfg, knn=None, G=None):
    """-> (bpr, regulariser) of one batch on the graph of the current parameters (``G``: on that graph instead)"""
    if G is None and cfg["n_layers"] > 0:
        G = build_graph(P, frozen, cfg, knn)
    C = forward_f64(P, A, dense_S(G) if cfg["n_layers"] > 0 else None, cfg)
    nu, ni = len(C["out_u"]), len(C["out_i"])
    u, i, j, n = _valid(users, pos, neg, nu, ni)
    if n == 0:
        return 0.0, 0.0
    ou, oi, oj = C["out_u"][u], C["out_i"][i], C["out_i"][j]
    bpr = -log_sigmoid((ou * (oi - oj)).sum(1)).sum() / n
    return bpr, cfg["reg"] * ((ou ** 2).sum() + (oi ** 2).sum() + (oj ** 2).sum()) / (2.0 * n)


def gradients_f64(P, A, frozen, users, pos, neg, cfg, build=True, knn=None, G=None):
    """-> ((bpr, regulariser), {name: gradient}, graph, g): the backward by hand.  ``build``: the graph is that of the current
    parameters and the gradient reaches the modal tensors; otherwise ``G`` is the installed graph and they get zeros"""
    Ln = cfg["n_layers"]
    if Ln > 0 and (build or G is None):
        G = build_graph(P, frozen, cfg, knn)
    S = dense_S(G) if Ln > 0 else None
    C = forward_f64(P, A, S, cfg)
    comps = losses_f64(P, A, frozen, users, pos, neg, cfg, G=G)
    Gr = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in P.items()}
    nu, ni = len(C["out_u"]), len(C["out_i"])
    u, i, j, n = _valid(users, pos, neg, nu, ni)
    if n == 0:
        return comps, Gr, G, None
    ou, oi, oj = C["out_u"][u], C["out_i"][i], C["out_i"][j]
    c = (-sigmoid(-(ou * (oi - oj)).sum(1)) / n)[:, None]
    r = cfg["reg"] / n
    d_u, d_i = np.zeros_like(C["out_u"]), np.zeros_like(C["out_i"])
    np.add.at(d_u, u, c * (oi - oj) + r * ou)
    np.add.at(d_i, i, c * ou + r * oi)
    np.add.at(d_i, j, -c * ou + r * oj)
    y, nrm = C["y"], C["nrm"]
    dh = np.where(nrm > NORM_EPS, (d_i - y * (y * d_i).sum(1, keepdims=True)) / nrm, d_i / nrm)
    g_dense = np.zeros((ni, ni))
    for l in range(Ln, 0, -1):
        g_dense += dh @ C["hs"][l - 1].T
        dh = S.T @ dh
    t = acc = np.vstack([d_u, d_i])
    for _ in range(C["Lu"]):
        t = A.T @ t
        acc = acc + t
    dE = acc / (C["Lu"] + 1)
    Gr["user_embedding.weight"] = dE[:nu]
    Gr["item_id_embedding.weight"] = dE[nu:] + dh
    g = None
    if Ln > 0:
        g = g_dense[G["rows"], G["col"]]
    if build and Ln > 0:
        dF, _, dtheta = graph_backward(G, g, G["F"])
        for m, (tab, trs) in enumerate(MODAL):
            if dF[m] is None:
                continue
            Gr[trs + ".weight"] = dF[m].T @ P[tab]
            Gr[trs + ".bias"] = dF[m].sum(0)
            Gr[tab] = dF[m] @ P[trs + ".weight"]
        if all(tab in P for tab, _ in MODAL):
            Gr["modal_weight"] = dtheta
    return comps, Gr, G, g


def scores_f64(P, A, frozen, cfg, users, knn=None):
    G = build_graph(P, frozen, cfg, knn) if cfg["n_layers"] > 0 else None
    C = forward_f64(P, A, dense_S(G) if G is not None else None, cfg)
    return C["out_u"][np.asarray(users)] @ C["out_i"].T


def schedule_lr(cfg, epoch):
    """the learning rate of epoch ``epoch``: LambdaLR with lr_scheduler[0] ** (epoch / lr_scheduler[1]) (LATTICE.py:314-316)"""
    g, s = cfg["lr_scheduler"]
    return cfg["lr"] * g ** (epoch / s)


class Adam64:
    """torch.optim.Adam's update (no weight decay, no amsgrad) in float64 over the named arrays of a dict"""

    def __init__(self, P, names, b1=0.9, b2=0.999, eps=1e-8):
        self.names = [k for k in names if k in P]
        self.m = {k: np.zeros_like(P[k]) for k in self.names}
        self.v = {k: np.zeros_like(P[k]) for k in self.names}
        self.t, self.b1, self.b2, self.eps = 0, b1, b2, eps

    def step(self, P, G, lr):
        self.t += 1
        c1, c2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for k in self.names:
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * G[k]
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * G[k] * G[k]
            P[k] = P[k] - (lr / c1) * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(c2) + self.eps)


def replay_f64(A, frozen, init, steps, cfg, steps_per_epoch, test_users, knn_builds=None, use_learned=True, use_reg=True,
               use_schedule=True, skip_modal_on_ordinary_steps=True):
    """the whole run in float64 -> (parameters, [total loss], [scores per evaluation], (t of the rows, t of the modal block)).
    The first step of an epoch builds the graph and is the only one whose gradient reaches the modal tensors; torch's Adam
    skips a tensor without a gradient, so the modal block is stepped on build steps only (``skip_modal_on_ordinary_steps``
    False: it is stepped with zeros instead, and moves by its momentum).  ``knn_builds``: per build and evaluation, in the
    order they happen, the neighbour ids to use.  ``use_learned`` False: lambda_coeff = 1, the frozen graph alone"""
    cfg = dict(cfg)
    if not use_reg:
        cfg["reg"] = 0.0
    if not use_learned:
        cfg["lambda_coeff"] = 1.0
    P = {k: np.asarray(v, np.float64).copy() for k, v in init.items()}
    rows, modal = Adam64(P, ROWS), Adam64(P, [k for k in NAMES if k not in ROWS])
    losses, scores, G, builds = [], [], None, iter(knn_builds) if knn_builds is not None else None
    nxt = (lambda: next(builds)) if builds is not None else (lambda: None)
    for s, st in enumerate(steps):
        epoch, build = s // steps_per_epoch, s % steps_per_epoch == 0
        lr = schedule_lr(cfg, epoch) if use_schedule else cfg["lr"]
        comps, Gr, G, _ = gradients_f64(P, A, frozen, st["users"], st["pos"], st["neg"], cfg, build=build, knn=nxt() if build else None, G=G)
        rows.step(P, Gr, lr)
        if (build and cfg["n_layers"] > 0) or not skip_modal_on_ordinary_steps:
            modal.step(P, Gr, lr)
        losses.append(sum(comps))
        if (s + 1) % steps_per_epoch == 0:
            scores.append(scores_f64(P, A, frozen, cfg, test_users, knn=nxt()))
    return P, np.array(losses), scores, (rows.t, modal.t)


def tiny_case(seed=0, nu=5, ni=9, d=6, Fv=5, Ft=3, k=3, fd=4, **cfg_kw):
    """a small random model for the finite-difference check: (P, A, frozen, cfg)"""
    rng = np.random.default_rng(seed)
    R = (rng.random((nu, ni)) < 0.45).astype(np.int64)
    R[np.arange(nu), rng.integers(0, ni, nu)] = 1
    rowptr = np.concatenate([[0], np.cumsum(R.sum(1))])
    items = np.concatenate([np.nonzero(r)[0] for r in R]).astype(np.int32)
    shapes = {"modal_weight": (2,), "user_embedding.weight": (nu, d), "item_id_embedding.weight": (ni, d),
              "image_embedding.weight": (ni, Fv), "text_embedding.weight": (ni, Ft), "image_trs.weight": (fd, Fv),
              "image_trs.bias": (fd,), "text_trs.weight": (fd, Ft), "text_trs.bias": (fd,)}
    P = {k_: rng.standard_normal(shapes[k_]) * 0.5 for k_ in NAMES}
    P["modal_weight"] = np.array([0.3, -0.4])
    frozen = [frozen_lists(P["image_embedding.weight"], k), frozen_lists(P["text_embedding.weight"], k)]
    cfg = twin_config(lr=1e-2, reg=0.05, lambda_coeff=0.4, n_layers=2, knn_k=k, weight_size=(d, d), lr_scheduler=(0.5, 1))
    cfg.update(cfg_kw)
    return P, norm_adj_dense(rowptr, items, ni), frozen, cfg


# ---- the fixture ----------------------------------------------------------------------------------
SEED = 2026                    # of the golden run (tests/golden/make_golden_lattice.py says how it was chosen)


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
    """the model config of the run (json) -> (the config dict, the twin's view of it)"""
    import json
    cfg = json.loads(str(g["config"]))
    return cfg, twin_config(**cfg)


def fixture_adjacency(g):
    """dense float64 norm_adj [U + I, U + I] from the recorded values"""
    N = int(g["shape"][0]) + int(g["shape"][1])
    A = np.zeros((N, N))
    A[csr_rows(g["norm_rowptr"]), g["norm_col"]] = g["norm_val"].astype(np.float64)
    return A


def fixture_frozen(g):
    """[(ids ascending, values)] per modality from the recorded frozen graphs (recorded in the top-k's order)"""
    out = []
    for m in ("image", "text"):
        ids, val = g[m + "_frozen_ids"].astype(np.int64), g[m + "_frozen_val"].astype(np.float64)
        order = np.argsort(ids, axis=1, kind="stable")
        out.append((np.take_along_axis(ids, order, 1), np.take_along_axis(val, order, 1)))
    return out


def fixture_knn(g, k):
    """the neighbour ids of every build, in the order a replay asks for them (per epoch: its build step, its evaluation):
    [[ids_image [I, k], ids_text [I, k]]]"""
    return [[b[0][:, :k].astype(np.int64), b[1][:, :k].astype(np.int64)] for b in g["knn_ids"]]
