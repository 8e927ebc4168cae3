"""Float64 restatement of LightGCL's training step (reference: recommender/LightGCL.py:117-169) for the tests: torch autograd
on a dense adjacency, in the PER-LAYER form of the reference (G = sum_l u_mul_s (vt E_i^(l-1)), not the folded form the
kernels use).  Written from the model's equations, shared by the CPU and GPU tests."""
import numpy as np
import torch

F64 = torch.float64


def t64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad)


def dense_adjacency(rowptr, items, num_items, values=None):
    """float64 [U, I]: 1 / sqrt(rowdeg * coldeg) at the CSR's entries (LightGCL.py:185-196), or ``values`` there"""
    nu = len(rowptr) - 1
    rows = np.repeat(np.arange(nu), np.diff(rowptr))
    A = np.zeros((nu, num_items), np.float64)
    if values is None:
        rowdeg = np.diff(rowptr).astype(np.float64)
        coldeg = np.bincount(items, minlength=num_items).astype(np.float64)
        values = 1.0 / np.sqrt(rowdeg[rows] * coldeg[items])
    A[rows, items] = values
    return A


def forward_f64(Eu0, Ei0, A, factors, n_layers):
    """-> (E_u, E_i, G_u, G_i): the sums over the layers of the propagated and of the SVD view (LightGCL.py:117-137)"""
    u_mul_s, v_mul_s, ut, vt = factors
    Eu, Ei, Gu, Gi = [Eu0], [Ei0], [Eu0], [Ei0]
    for _ in range(n_layers):
        zu, zi = A @ Ei[-1], A.T @ Eu[-1]
        Gu.append(u_mul_s @ (vt @ Ei[-1]))
        Gi.append(v_mul_s @ (ut @ Eu[-1]))
        Eu.append(zu)
        Ei.append(zi)
    return sum(Eu), sum(Ei), sum(Gu), sum(Gi)


def _lse_eps(s):
    """log(sum_k exp(s_k) + 1e-8) per row: as written in float64 (the reference's form); with the largest term taken out in
    any narrower type, where exp(s) itself may overflow"""
    if s.dtype == F64:
        return torch.log(torch.exp(s).sum(1) + 1e-8)
    m = s.detach().max(1).values.clamp_min(float(np.log(1e-8)))
    return m + torch.log(torch.exp(s - m[:, None]).sum(1) + 1e-8 * torch.exp(-m))


def losses_f64(Eu0, Ei0, A, factors, uids, pos, neg, n_layers, temp, lambda1, lambda2, valid=None):
    """-> ((bpr, cl, reg), E_u, E_i, (positive scores of the user side, of the item side) before the clamp).
    ``valid`` = (vu, vp, vq), bool [n] each: the ids the kernel does not skip (the others are out of range and are not looked
    up).  Each id is skipped on its own: the BPR term of a pair needs its three ids, the log-sum-exp and the positive score of
    a user or an item that id alone; n and 2 n stay the divisors"""
    Eu, Ei, Gu, Gi = forward_f64(Eu0, Ei0, A, factors, n_layers)
    uids, pos, neg = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (uids, pos, neg))
    if valid is None:
        mean = lambda v, w: v.mean()                                   # noqa: E731
        wu = wi = wb = None
    else:
        vu, vp, vq = (torch.as_tensor(np.asarray(v), dtype=torch.bool) for v in valid)
        uids, pos, neg = torch.where(vu, uids, 0), torch.where(vp, pos, 0), torch.where(vq, neg, 0)
        wu, wi, wb = vu.to(Eu.dtype), torch.cat([vp, vq]).to(Eu.dtype), (vu & vp & vq).to(Eu.dtype)
        mean = lambda v, w: (v * w).sum() / len(v)                     # noqa: E731
    iids = torch.cat([pos, neg])
    cl = torch.zeros((), dtype=Eu.dtype)
    ps_u = ps_i = None
    if lambda1 > 0:
        neg_score = mean(_lse_eps(Gu[uids] @ Eu.T / temp), wu) + mean(_lse_eps(Gi[iids] @ Ei.T / temp), wi)
        ps_u, ps_i = (Gu[uids] * Eu[uids]).sum(1) / temp, (Gi[iids] * Ei[iids]).sum(1) / temp
        pos_score = mean(torch.clamp(ps_u, -5.0, 5.0), wu) + mean(torch.clamp(ps_i, -5.0, 5.0), wi)
        cl = lambda1 * (neg_score - pos_score)
    x = (Eu[uids] * Ei[pos]).sum(-1) - (Eu[uids] * Ei[neg]).sum(-1)
    bpr = mean(-torch.nn.functional.logsigmoid(x), wb)
    reg = lambda2 * ((Eu0 ** 2).sum() + (Ei0 ** 2).sum())
    return (bpr, cl, reg), Eu, Ei, (ps_u, ps_i)


def replay_f64(A, factors, init, steps, cfg, eval_every, test_users):
    """the whole run in float64 with torch.optim.Adam (the l2 term in the loss) -> (E_u_0, E_i_0, [total loss], [scores per
    evaluation]); the scores come from the sums of the LAST TRAINING FORWARD, as the reference's evaluate() ranks them"""
    Eu0, Ei0 = t64(init[0], True), t64(init[1], True)
    A, factors = t64(A), tuple(t64(f) for f in factors)
    opt = torch.optim.Adam([Eu0, Ei0], lr=cfg["lr"])
    losses, scores = [], []
    for t, (uids, pos, neg) in enumerate(steps):
        (bpr, cl, reg), Eu, Ei, _ = losses_f64(Eu0, Ei0, A, factors, uids, pos, neg, cfg["gnn_layer"], cfg["temp"], cfg["lambda1"],
                                               cfg["lambda2"])
        loss = bpr + cl + reg
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if (t + 1) % eval_every == 0:
            scores.append((Eu.detach()[np.asarray(test_users)] @ Ei.detach().T).numpy())
    return Eu0.detach().numpy(), Ei0.detach().numpy(), np.array(losses), scores


def fixture_steps(g):
    """(uids, pos, neg) per step from golden_lightgcl.npz"""
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    return [(g["step_users"][b[s]:b[s + 1]], g["step_pos"][b[s]:b[s + 1]], g["step_neg"][b[s]:b[s + 1]])
            for s in range(len(g["step_sizes"]))]


def fixture_factors(g):
    return g["u_mul_s"], g["v_mul_s"], g["ut"], g["vt"]


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
