"""Float64 restatement of BM3's training step, optimiser and score (reference: recommender/BM3.py:142-210) for the tests: torch
autograd on the dense block R of the normalised adjacency [[0, R], [R^T, 0]].  Written from the model's equations, shared by
the CPU and GPU tests and by the fixture's generator.

    M_u, M_i = mean_{k=0..L} A^k X0, then M_i += X0_items
    T = text_embedding text_trs.W^T + text_trs.b, V likewise from the image block (only the batch's rows are formed here)
    targets: x * keep / (1 - dropout) of M_u, M_i, T, V, detached
    graph = (1 - mean cos(P(M_u[u]), i_tgt)) + (1 - mean cos(P(M_i[i]), u_tgt)),  P(x) = predictor.W x + predictor.b
    modal = cl_weight * sum over the present modalities X in (T, V) of (1 - mean cos(P(X[i]), i_tgt)) + (1 - mean cos(P(X[i]), x_tgt))
    reg   = reg * (|M_u|_F + |M_i|_F) / num_items
"""
import numpy as np
import torch

from selfcf_twin import cosine, csr_rows, normalised_values, t64, tiny_csr  # noqa: F401

F64 = torch.float64

BASE = ("user_embedding.weight", "item_id_embedding.weight", "predictor.weight", "predictor.bias")
IMAGE = ("image_embedding.weight", "image_trs.weight", "image_trs.bias")
TEXT = ("text_embedding.weight", "text_trs.weight", "text_trs.bias")


def param_names(has_img, has_txt):
    """the reference's parameter names, in its registration order"""
    return BASE + (IMAGE if has_img else ()) + (TEXT if has_txt else ())


def dense_block(rowptr, items, num_items, val):
    """dense float64 R [U, I] with ``val`` (R order) at the CSR's entries"""
    R = np.zeros((len(rowptr) - 1, num_items), np.float64)
    R[csr_rows(rowptr), items] = np.asarray(val, np.float64)
    return R


def forward_f64(Eu, Ei, R, n_layers):
    """-> (M_u, M_i): the layer means, the item side with its ``+ h``"""
    xu, xi, su, si = Eu, Ei, Eu, Ei
    for _ in range(n_layers):
        xu, xi = R @ xi, R.T @ xu
        su, si = su + xu, si + xi
    return su / (n_layers + 1), si / (n_layers + 1) + Ei


def losses_f64(P, R, users, items, keeps, n_layers, dropout, reg, cl_weight, n_div=None):
    """-> ((graph, modal, reg part), M_u, M_i) of one step.  ``P``: {name: float64 tensor}; ``keeps``: {"u", "i", "t", "v"} ->
    [n, d] keep flags of the batch rows' targets (the entries of absent modalities are not read); ``n_div``: the divisor of
    the cosine means when it is not the number of rows handed in (rows the kernel skips leave n)"""
    Mu, Mi = forward_f64(P["user_embedding.weight"], P["item_id_embedding.weight"], R, n_layers)
    users, items = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (users, items))
    W, b = P["predictor.weight"], P["predictor.bias"]
    pred = lambda x: x @ W.T + b                                                 # noqa: E731
    tgt = lambda x, k: (x * torch.as_tensor(np.asarray(keeps[k]), dtype=x.dtype) / (1.0 - dropout)).detach()     # noqa: E731
    mean = (lambda v: v.mean()) if n_div is None else (lambda v: v.sum() / n_div)                                # noqa: E731
    u, i = Mu[users], Mi[items]
    tu, ti = tgt(u, "u"), tgt(i, "i")
    graph = (1 - mean(cosine(pred(u), ti))) + (1 - mean(cosine(pred(i), tu)))
    modal = torch.zeros((), dtype=Mu.dtype)
    for key, (emb, w, bias) in (("t", TEXT), ("v", IMAGE)):
        if emb not in P:
            continue
        x = P[emb][items] @ P[w].T + P[bias]
        tx = tgt(x, key)
        px = pred(x)
        modal = modal + (1 - mean(cosine(px, ti))) + (1 - mean(cosine(px, tx)))
    regl = reg * (Mu.norm() + Mi.norm()) / Mi.shape[0]
    return (graph, cl_weight * modal, regl), Mu, Mi


def scores_f64(Mu, Mi, W, b, users):
    """full_sort_predict: (W M_u + b) . (W M_i + b)"""
    return (Mu[np.asarray(users)] @ W.T + b) @ (Mi @ W.T + b).T


def replay_f64(csr, val, init, steps, cfg, eval_every, test_users):
    """the whole run in float64 with torch.optim.Adam over every tensor, the feature tables included (dense gradients) ->
    (parameters dict, [total loss], [scores per evaluation]).  ``csr`` = (rowptr, items, num_items); ``steps``: dicts with
    users, items and the batch rows' keep flags ku, ki, kt, kv"""
    rowptr, items, ni = csr
    P = {k: t64(v, True) for k, v in init.items()}
    opt = torch.optim.Adam(list(P.values()), lr=cfg["lr"])
    R = t64(dense_block(rowptr, items, ni, val))
    L = cfg["n_layers"]
    losses, scores = [], []
    for s, st in enumerate(steps):
        keeps = {"u": st["ku"], "i": st["ki"], "t": st.get("kt"), "v": st.get("kv")}
        (g, m, r), _, _ = losses_f64(P, R, st["users"], st["items"], keeps, L, cfg["dropout"], cfg["reg"], cfg["cl_weight"])
        loss = g + m + r
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if (s + 1) % eval_every == 0:
            with torch.no_grad():
                Mu, Mi = forward_f64(P["user_embedding.weight"], P["item_id_embedding.weight"], R, L)
                scores.append(scores_f64(Mu, Mi, P["predictor.weight"], P["predictor.bias"], test_users).numpy())
    return {k: v.detach().numpy() for k, v in P.items()}, np.array(losses), scores


def _key(name, which):
    return f"{name.replace('.', '_')}_{which}"


def fixture_params(g, which):
    """the recorded parameters: which = 0 (initial) or 1 (final)"""
    return {k: g[_key(k, which)] for k in BASE + IMAGE + TEXT if _key(k, which) in g.files}


def fixture_steps(g):
    """per step a dict (users, items, ku, ki, kt, kv) from golden_bm3.npz: the recorded full-table masks at the batch's rows"""
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    nu, ni, d = int(g["user_embedding_weight_0"].shape[0]), int(g["item_id_embedding_weight_0"].shape[0]), int(g["predictor_bias_0"].shape[0])
    steps = []
    for s in range(len(g["step_sizes"])):
        users, items = g["step_users"][b[s]:b[s + 1]], g["step_items"][b[s]:b[s + 1]]
        full = {k: np.unpackbits(g[f"step_mask_{k}"][s])[:rows * d].reshape(rows, d) for k, rows in (("u", nu), ("i", ni), ("t", ni), ("v", ni))}
        steps.append(dict(users=users, items=items, ku=full["u"][users], ki=full["i"][items], kt=full["t"][items], kv=full["v"][items]))
    return steps
