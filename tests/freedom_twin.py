"""Float64 restatement of FREEDOM's pruned normalisation, training step, optimiser and score (reference:
recommender/FREEDOM.py:175-260) for the tests: torch autograd on the dense block R' of the epoch's adjacency [[0, R'], [R'^T, 0]]
and on the dense item graph S.  Written from the model's equations, shared by the CPU and GPU tests and by the fixture's
generator.

    M_u, M_i = mean_{k=0..Lu} A'^k X0;  h = S^Lm X0_items;  M_i += h
    x_g = <M_u[u], M_i[p] - M_i[q]>;  per present modality x_m = <M_u[u], (f[p] - f[q]) W^T>   (the bias cancels)
    loss = -mean logsigmoid(x_g) + reg * sum_m -mean logsigmoid(x_m)

The biases take no part in the loss, so they are no leaves of the replay and never move -- as on the device; the reference's
move by rounding residue, which the fixture records as ``bias_drift``.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from selfcf_twin import csr_rows, t64, tiny_csr, transpose_order  # noqa: F401

F64 = torch.float64
SEED = 2039                    # of the golden run (tests/golden/make_golden_freedom.py says how it was chosen)

BASE = ("user_embedding.weight", "item_id_embedding.weight")
IMAGE = ("image_embedding.weight", "image_trs.weight", "image_trs.bias")
TEXT = ("text_embedding.weight", "text_trs.weight", "text_trs.bias")
BIASES = ("image_trs.bias", "text_trs.bias")


def param_names(has_img, has_txt):
    """the reference's parameter names, in its registration order"""
    return BASE + (IMAGE if has_img else ()) + (TEXT if has_txt else ())


# ---- the pruning --------------------------------------------------------------------------------
def n_keep_of(nnz, dropout):
    return int(nnz * (1. - dropout))


def select_keys(keys, n_keep):
    """uint8 flags of the n_keep largest keys, equal keys ranked by ascending index (numpy's stable sort)"""
    keep = np.zeros(len(keys), np.uint8)
    keep[np.argsort(-np.asarray(keys, np.float64), kind="stable")[:n_keep]] = 1
    return keep


def sample_keep(w, n_keep, rng):
    """the sampler's law: the n_keep largest of w / Exp(1) are a draw without replacement with probabilities proportional to w"""
    return select_keys(np.asarray(w, np.float64) / rng.exponential(size=len(w)), n_keep)


def pruned_counts(rows, cols, keep, nu, ni):
    k = np.asarray(keep).astype(bool)
    return np.bincount(rows[k], minlength=nu), np.bincount(cols[k], minlength=ni)


def pruned_values_f32(rows, cols, keep, nu, ni):
    """the values of the kept entries (in R's order) as the library computes them: each factor (1e-7 + count)^-0.5 in float64
    rounded to fp32, then one fp32 product"""
    k = np.asarray(keep).astype(bool)
    cu, ci = pruned_counts(rows, cols, keep, nu, ni)
    fu = np.power(1e-7 + cu.astype(np.float64), -0.5).astype(np.float32)
    fi = np.power(1e-7 + ci.astype(np.float64), -0.5).astype(np.float32)
    return fu[rows[k]] * fi[cols[k]]


def pruned_csr(rowptr, items, ni, keep):
    """(rowptr', cols', values) and the same of the transpose for the kept entries: what skr_freedom_pruned_csr returns"""
    nu = len(rowptr) - 1
    rows = csr_rows(rowptr)
    k = np.asarray(keep).astype(bool)
    val = pruned_values_f32(rows, items, keep, nu, ni)
    r, c = rows[k], items[k]
    rp = np.zeros(nu + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(r, minlength=nu))
    order = np.lexsort((r, c))
    rpt = np.zeros(ni + 1, np.int64)
    rpt[1:] = np.cumsum(np.bincount(c, minlength=ni))
    return (rp, c.astype(np.int32), val), (rpt, r[order].astype(np.int32), val[order])


def pruned_block(rowptr, items, ni, keep, values=None):
    """dense float64 R' [U, I] of the kept entries with the fp32 values above, or with ``values`` (those of the kept entries,
    in R's order); ``keep`` None: no entry is dropped"""
    rows = csr_rows(rowptr)
    keep = np.ones(len(items), np.uint8) if keep is None else keep
    k = np.asarray(keep).astype(bool)
    R = np.zeros((len(rowptr) - 1, ni), np.float64)
    v = pruned_values_f32(rows, items, keep, len(rowptr) - 1, ni) if values is None else values
    R[rows[k], items[k]] = np.asarray(v, np.float64)
    return R


def dense_graph(row, col, val, ni):
    S = np.zeros((ni, ni), np.float64)
    S[np.asarray(row), np.asarray(col)] = np.asarray(val, np.float64)
    return S


# ---- the model ----------------------------------------------------------------------------------
def forward_f64(Eu, Ei, R, S, Lu, Lm):
    """-> (M_u, M_i + h)"""
    xu, xi, su, si = Eu, Ei, Eu, Ei
    for _ in range(Lu):
        xu, xi = R @ xi, R.T @ xu
        su, si = su + xu, si + xi
    h = Ei
    for _ in range(Lm):
        h = S @ h
    return su / (Lu + 1), si / (Lu + 1) + h


def losses_f64(P, R, S, users, pos, neg, Lu, Lm, reg, n_div=None, args=None):
    """-> ((graph term, reg * modal terms), M_u, M_i) of one step.  ``P``: {name: float64 tensor}; ``n_div``: the divisor of
    the means when it is not the number of rows handed in (rows the kernel skips leave n); ``args`` (a list) receives the
    arguments of the log-sigmoids: x_g, then x_m of the text and of the image block"""
    Mu, Mi = forward_f64(P["user_embedding.weight"], P["item_id_embedding.weight"], R, S, Lu, Lm)
    users, pos, neg = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (users, pos, neg))
    mean = (lambda v: v.mean()) if n_div is None else (lambda v: v.sum() / n_div)       # noqa: E731
    u = Mu[users]
    xs = [(u * (Mi[pos] - Mi[neg])).sum(-1)]
    graph = mean(-Fn.logsigmoid(xs[0]))
    modal = torch.zeros((), dtype=Mu.dtype)
    if reg > 0:
        for emb, w, _ in (TEXT, IMAGE):
            if emb in P:
                diff = (P[emb][pos] - P[emb][neg]) @ P[w].T
                xs.append((u * diff).sum(-1))
                modal = modal + mean(-Fn.logsigmoid(xs[-1]))
    if args is not None:
        args.extend(x.detach().numpy() for x in xs)
    return (graph, reg * modal), Mu, Mi


def gradients_f64(P, R, S, users, pos, neg, Lu, Lm, reg):
    """-> ((graph, modal), {name: gradient}) with exact zeros for what takes no part"""
    Q = {k: t64(v, True) for k, v in P.items()}
    (g, m), _, _ = losses_f64(Q, R, S, users, pos, neg, Lu, Lm, reg)
    (g + m).backward()
    return (g.item(), m.item()), {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy()) for k, v in Q.items()}


def scores_f64(Mu, Mi, users):
    return Mu[np.asarray(users)] @ Mi.T


def replay_f64(csr, keeps, S, init, steps, cfg, steps_per_epoch, test_users, keep_values=None, full_values=None):
    """the whole run in float64 with torch.optim.Adam over every tensor but the biases -> (parameters dict, [total loss],
    [scores per evaluation]).  ``csr`` = (rowptr, items, num_items); ``keeps``: per epoch the keep flags in R's order;
    ``steps``: dicts with users, pos, neg; evaluation (on the unpruned graph) after every ``steps_per_epoch`` steps;
    ``keep_values`` (per epoch, the kept entries' in R's order) / ``full_values``: recorded values instead of the restated ones"""
    rowptr, items, ni = csr
    P = {k: t64(v, k not in BIASES) for k, v in init.items()}
    opt = torch.optim.Adam([v for k, v in P.items() if k not in BIASES], lr=cfg["lr"])
    St = t64(S)
    full = t64(pruned_block(rowptr, items, ni, None, full_values))
    Lu, Lm = cfg["n_ui_layers"], cfg["n_mm_layers"]
    losses, scores = [], []
    R = None
    for s, st in enumerate(steps):
        if s % steps_per_epoch == 0:
            e = s // steps_per_epoch
            R = t64(pruned_block(rowptr, items, ni, keeps[e], None if keep_values is None else keep_values[e]))
        (g, m), _, _ = losses_f64(P, R, St, st["users"], st["pos"], st["neg"], Lu, Lm, cfg["reg"])
        loss = g + m
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if (s + 1) % steps_per_epoch == 0:
            with torch.no_grad():
                Mu, Mi = forward_f64(P["user_embedding.weight"], P["item_id_embedding.weight"], full, St, Lu, Lm)
                scores.append(scores_f64(Mu, Mi, test_users).numpy())
    return {k: v.detach().numpy() for k, v in P.items()}, np.array(losses), scores


# ---- the fixture ----------------------------------------------------------------------------------
def _key(name, which):
    return f"{name.replace('.', '_')}_{which}"


def fixture_params(g, which):
    """the recorded parameters: which = 0 (initial) or 1 (final)"""
    return {k: g[_key(k, which)] for k in BASE + IMAGE + TEXT if _key(k, which) in g.files}


def fixture_keeps(g):
    """per epoch the keep flags (uint8 [nnz], R's CSR order) of golden_freedom.npz"""
    nnz = len(g["edge_w"])
    return [np.unpackbits(row)[:nnz] for row in g["keep_bits"]]


def fixture_steps(g):
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    return [dict(users=g["step_users"][b[s]:b[s + 1]], pos=g["step_pos"][b[s]:b[s + 1]], neg=g["step_neg"][b[s]:b[s + 1]])
            for s in range(len(g["step_sizes"]))]
