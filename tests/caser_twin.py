"""Float64 restatement of Caser's step and query rows (torch autograd), written from the model's equations -- shared by
tests/golden/make_golden_caser.py (which checks it against the reference before it writes the fixture), the CPU suite and
the GPU suite.

Parameters are a dict of float64 tensors under the reference's names, in the reference's shapes:
    user_embeddings [U, e], item_embeddings [I + 1, e], conv_v_weight [nv, 1, L, 1], conv_v_bias [nv],
    conv_h_weight_<i> [nh, 1, i + 1, e], conv_h_bias_<i> [nh] for i < L, fc1_weight [e, nv e + nh L], fc1_bias [e],
    W2 [I + 1, 2 e], b2 [I + 1, 1]

    out_v[c, :] = bv[c] + sum_l wv[c, l] E_l                              (flattened c e + column, no activation)
    a[h, k, t]  = bh[h, k] + sum_{r < h} <Wh[h, k, r, :], E_(t + r)>      out_h[h, k] = max_t relu(a[h, k, t])
    out = [out_v, out_h] * keep / (1 - rate),  z = relu(W1 out + b1),  x = [z, p],  y_j = <W2[t_j], x> + b2[t_j]
    loss = mean over n T of (softplus(-y_pos) + softplus(y_neg))

The max takes the LOWEST position among exact ties and relu'(0) = 0: torch's max_pool1d and relu do the same
(tests/test_caser_host.py checks that on windows with equal sub-windows).
"""
import numpy as np
import torch

CONFIG = dict(lr=1e-3, l2_reg=1e-6, embed_size=64, seq_L=5, seq_T=3, nv=4, nh=16, dropout=0.5, batch_size=256, epochs=3)


def param_names(L):
    names = ["user_embeddings", "item_embeddings", "conv_v_weight", "conv_v_bias"]
    for i in range(L):
        names += [f"conv_h_weight_{i}", f"conv_h_bias_{i}"]
    return names + ["fc1_weight", "fc1_bias", "W2", "b2"]


# max |twin - golden| per parameter after the fixture's 9 steps, as tests/test_caser_host.py prints it: the reference's own
# fp32 noise against float64 on the same batches and keep flags.  The GPU replay allows twice these (two fp32 runs each lie
# that far from the float64 one).
TWIN_DEVIATION = {
    "user_embeddings": 1.6e-07,
    "item_embeddings": 1.1e-07,
    "conv_v_weight": 6.1e-08,
    "conv_v_bias": 2.3e-08,
    "conv_h_weight_0": 2.2e-08,
    "conv_h_bias_0": 7.4e-09,
    "conv_h_weight_1": 2.6e-08,
    "conv_h_bias_1": 6.2e-09,
    "conv_h_weight_2": 2.4e-08,
    "conv_h_bias_2": 1.1e-08,
    "conv_h_weight_3": 1.6e-08,
    "conv_h_bias_3": 5.1e-09,
    "conv_h_weight_4": 3.1e-08,
    "conv_h_bias_4": 5.6e-09,
    "fc1_weight": 3.6e-07,
    "fc1_bias": 8.4e-09,
    "W2": 3e-07,
    "b2": 2.6e-08,
}


def random_params(rng, nU, nI, e, L, nv, nh, scale=None):
    """float32 arrays; the filters and fc1 are scaled so that the pre-activations are O(1) for embedding rows of scale 1"""
    F = nv * e + nh * L
    p = {"user_embeddings": rng.standard_normal((nU, e)) * 0.5, "item_embeddings": rng.standard_normal((nI + 1, e)),
         "conv_v_weight": rng.standard_normal((nv, 1, L, 1)) / np.sqrt(L), "conv_v_bias": rng.standard_normal(nv) * 0.3}
    for i in range(L):
        p[f"conv_h_weight_{i}"] = rng.standard_normal((nh, 1, i + 1, e)) / np.sqrt((i + 1) * e)
        p[f"conv_h_bias_{i}"] = rng.standard_normal(nh) * 0.3
    p["fc1_weight"] = rng.standard_normal((e, F)) / np.sqrt(F)
    p["fc1_bias"] = rng.standard_normal(e) * 0.3
    p["W2"] = rng.standard_normal((nI + 1, 2 * e)) / np.sqrt(2 * e)
    p["b2"] = rng.standard_normal((nI + 1, 1)) * 0.3
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}


def to_torch(params, dtype=torch.float64, requires_grad=True):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def conv_parts(P, seq, pad=None):
    """(out_v [n, nv, e], a: list over h of [n, nh, L - h + 1]) for the windows ``seq`` [n, L]; with ``pad`` the padding
    item's row reads as zeros"""
    E = P["item_embeddings"][seq]                                   # [n, L, e]
    if pad is not None:
        E = E * (seq != pad).unsqueeze(-1).to(E.dtype)
    L = seq.shape[1]
    wv = P["conv_v_weight"].reshape(-1, L)
    out_v = torch.einsum("cl,nle->nce", wv, E) + P["conv_v_bias"].view(1, -1, 1)
    a = []
    for i in range(L):
        h = i + 1
        Wh = P[f"conv_h_weight_{i}"].reshape(-1, h, E.shape[2])      # [nh, h, e]
        win = E.unfold(1, h, 1)                                      # [n, L - h + 1, e, h]
        a.append(torch.einsum("nter,kre->nkt", win, Wh) + P[f"conv_h_bias_{i}"].view(1, -1, 1))
    return out_v, a


def first_argmax(a):
    """the lowest position of the maximum along the last axis"""
    d = a.detach()
    return (d == d.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)


def forward_x(P, u, seq, keep=None, rate=0.0, pad=None, return_parts=False):
    """x = [z, p] [n, 2 e]; ``keep`` [n, nv e + nh L] of 0 / 1 (None: eval mode)"""
    out_v, a = conv_parts(P, seq, pad)
    n = seq.shape[0]
    pooled = [torch.relu(t.gather(-1, first_argmax(t).unsqueeze(-1)).squeeze(-1)) for t in a]
    out = torch.cat([out_v.reshape(n, -1)] + pooled, 1)
    if keep is not None and rate > 0.0:
        out = out * keep.to(out.dtype) * (1.0 / (1.0 - rate))
    zp = out @ P["fc1_weight"].T + P["fc1_bias"]
    x = torch.cat([torch.relu(zp), P["user_embeddings"][u]], 1)
    return (x, a, zp) if return_parts else x


def step_losses(P, u, seq, pos, neg, keep=None, rate=0.0, pad=None, valid=None):
    """(sum of bce(y_pos, 1), sum of bce(y_neg, 0), their mean over n T); ``valid`` [n] of 0 / 1: the instances that count
    (the mean still divides by n T)"""
    x = forward_x(P, u, seq, keep, rate, pad)
    sp = torch.nn.functional.softplus
    yp = (P["W2"][pos] * x.unsqueeze(1)).sum(-1) + P["b2"][pos].squeeze(-1)
    yn = (P["W2"][neg] * x.unsqueeze(1)).sum(-1) + P["b2"][neg].squeeze(-1)
    lp, ln = sp(-yp), sp(yn)
    if valid is not None:
        lp, ln = lp * valid.unsqueeze(-1), ln * valid.unsqueeze(-1)
    lp, ln = lp.sum(), ln.sum()
    return lp, ln, (lp + ln) / (pos.shape[0] * pos.shape[1])


def decision_margins(P, u, seq, pad=None, keep=None, rate=0.0):
    """per instance, the smallest of: the gap between the best and the second-best position of every pool (positions whose
    sub-windows hold the same items tie exactly in every arithmetic and are left out), |max pre-activation| of every pool,
    |z pre-activation|"""
    with torch.no_grad():
        x, a, zp = forward_x(P, u, seq, keep, rate, pad, return_parts=True)
        m = zp.abs().min(1).values
        L = seq.shape[1]
        for i, t in enumerate(a):
            h = i + 1
            best = t.max(-1)
            m = torch.minimum(m, best.values.abs().min(1).values)
            if t.shape[-1] > 1:
                arg = first_argmax(t)                                            # [n, nh]
                sub = seq.unfold(1, h, 1)                                        # [n, L - h + 1, h]
                same = (sub.unsqueeze(1) == sub.unsqueeze(2)).all(-1)            # [n, t, t']: equal contents
                tie = same[torch.arange(seq.shape[0]).unsqueeze(-1), arg]        # [n, nh, t']: ties with the arg-max
                gap = best.values.unsqueeze(-1) - t
                gap = torch.where(tie, torch.full_like(gap, float("inf")), gap)
                m = torch.minimum(m, gap.min(-1).values.min(-1).values)
        return m


def query_rows(P, users, windows, pad=None):
    with torch.no_grad():
        return forward_x(P, users, windows, None, 0.0, pad)


# ---- the library's layouts -----------------------------------------------------------------------------------------
def caser_fp(L, nv, nh):
    return 64 * ((nv * 64 + nh * L + 63) // 64)


def shared_offsets(L, nv, nh):
    rows = nh * L * (L + 1) // 2
    o_wh = 128
    o_bh = o_wh + 64 * rows
    o_w1 = o_bh + 64 * ((L * nh + 63) // 64)
    o_b1 = o_w1 + 64 * caser_fp(L, nv, nh)
    return dict(wv=0, bv=64, wh=o_wh, bh=o_bh, w1=o_w1, b1=o_b1, total=o_b1 + 64, rows=rows)


def fc1_columns(e, L, nv, nh):
    """the padded column of every reference column of fc1.weight"""
    cols = [c * 64 + k for c in range(nv) for k in range(e)]
    return np.array(cols + [nv * 64 + j for j in range(nh * L)], np.int64)


def shared_block(params, e, L, nv, nh):
    """the shared parameters in skr_caser_step's layout (float32), from arrays in the reference's shapes"""
    o = shared_offsets(L, nv, nh)
    fp = caser_fp(L, nv, nh)
    s = np.zeros(o["total"], np.float32)
    s[:nv * L] = np.asarray(params["conv_v_weight"]).reshape(-1)
    s[64:64 + nv] = np.asarray(params["conv_v_bias"])
    row = 0
    for i in range(L):
        w = np.asarray(params[f"conv_h_weight_{i}"]).reshape(nh, i + 1, e)
        blk = np.zeros((nh * (i + 1), 64), np.float32)
        blk[:, :e] = w.reshape(-1, e)
        s[o["wh"] + 64 * row:o["wh"] + 64 * (row + len(blk))] = blk.ravel()
        row += len(blk)
        s[o["bh"] + i * nh:o["bh"] + (i + 1) * nh] = np.asarray(params[f"conv_h_bias_{i}"])
    w1 = np.zeros((64, fp), np.float32)
    w1[:e, fc1_columns(e, L, nv, nh)] = np.asarray(params["fc1_weight"])
    s[o["w1"]:o["b1"]] = w1.ravel()
    s[o["b1"]:o["b1"] + e] = np.asarray(params["fc1_bias"])
    return s


def unpack_shared(s, e, L, nv, nh):
    """(the reference-shaped arrays of a shared block or of its gradient, what lies in the padding): the inverse of
    shared_block; the second value must be all zero"""
    o = shared_offsets(L, nv, nh)
    fp = caser_fp(L, nv, nh)
    s = np.asarray(s)
    rest = s.copy()
    out = {"conv_v_weight": s[:nv * L].reshape(nv, 1, L, 1), "conv_v_bias": s[64:64 + nv]}
    rest[:nv * L] = 0
    rest[64:64 + nv] = 0
    row = 0
    for i in range(L):
        k = nh * (i + 1)
        blk = s[o["wh"] + 64 * row:o["wh"] + 64 * (row + k)].reshape(k, 64)
        out[f"conv_h_weight_{i}"] = blk[:, :e].reshape(nh, 1, i + 1, e)
        rest[o["wh"] + 64 * row:o["wh"] + 64 * (row + k)].reshape(k, 64)[:, :e] = 0
        row += k
        out[f"conv_h_bias_{i}"] = s[o["bh"] + i * nh:o["bh"] + (i + 1) * nh]
        rest[o["bh"] + i * nh:o["bh"] + (i + 1) * nh] = 0
    cols = fc1_columns(e, L, nv, nh)
    w1 = s[o["w1"]:o["b1"]].reshape(64, fp)
    out["fc1_weight"] = w1[:e][:, cols]
    r1 = rest[o["w1"]:o["b1"]].reshape(64, fp)
    r1[np.ix_(np.arange(e), cols)] = 0
    out["fc1_bias"] = s[o["b1"]:o["b1"] + e]
    rest[o["b1"]:o["b1"] + e] = 0
    return out, rest


def pad_cols(a, width):
    a = np.asarray(a, dtype=np.float32)
    out = np.zeros((a.shape[0], width), np.float32)
    out[:, :a.shape[1]] = a
    return out


def w2_rows(W2, e):
    """[I + 1, 2 e] -> [I + 1, 128]: the z half, then the p half"""
    W2 = np.asarray(W2, dtype=np.float32)
    return np.concatenate([pad_cols(W2[:, :e], 64), pad_cols(W2[:, e:], 64)], 1)


def unpack_bits(bits, shape):
    return np.unpackbits(np.asarray(bits, np.uint8))[:int(np.prod(shape))].reshape(shape)
