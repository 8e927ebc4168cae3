"""Float64 restatement of SASRec's graph (torch autograd), written LITERALLY from the reference's skrec/recommender/SASRec.py
-- shared by the CPU suite (tests/test_sasrec_host.py) and the GPU suite (tests/test_gpu_sasrec.py).  TensorFlow is not
installed where this suite runs, so parity with a run of the reference stays unpinned; this file is the yardstick.

It keeps what the kernel simplifies: the key mask by a row sum of exactly zero, the query mask, the -2^32 + 1 fill, and
``1 - sigmoid(x)``.  Parameters are a dict of tensors under the reference's names (``param_names``), in the reference's shapes:
    item_embeddings [I, d], position_embeddings [T, d], per block b: ln1_gamma_b, ln1_beta_b [d], Wq_b, Wk_b, Wv_b [d, d]
    ([in, out]), bq_b, bk_b, bv_b [d], ln2_gamma_b, ln2_beta_b [d], W1_b, W2_b [d, d], b1_b, b2_b [d]; ln_out_gamma, ln_out_beta.
The padding item is id I: its row is a constant zero and no parameter.

Keep flags (one byte per element, per sequence ``keep_bytes`` of them):
    the input [T][d] | per block: the attention weights [heads][T][T] (query, then key) | ffn site 1 [T][d] | ffn site 2 [T][d]
"""
import numpy as np
import torch

BLOCK_NAMES = ("ln1_gamma", "ln1_beta", "Wq", "bq", "Wk", "bk", "Wv", "bv", "ln2_gamma", "ln2_beta", "W1", "b1", "W2", "b2")
PAD_FILL = float(-2 ** 32 + 1)

# the fit tests' configuration (tests/test_gpu_sasrec.py) and the deviation of the twin run in fp32 from its float64 run over
# that trajectory (two epochs of the tiny sequential set, 4 steps, lr 1e-3), as ``measure_deviation`` prints it on the CPU:
# the larger of the runs at dropout 0 and 0.5, from ``random_params`` of seed 2021.  The GPU replay allows twice these.  The
# entries of 0.002 = 2 lr are single elements whose first gradient is smaller than fp32's error in it (about 1e-5 of the
# largest): Adam's first step is lr sign(g), so the two runs part by 2 lr there and stay apart; bk's gradient is zero in exact
# arithmetic (a softmax does not see a shift of its row), so its trajectory is rounding noise that Adam magnifies.
# The run starts from ``random_params`` and not from the model's initialisation: with gamma = 1 and beta = 0 a normalised
# query row sums to zero up to rounding, the reference's query mask sign(|sum|) is then 0 for whichever real rows round to
# exactly 0.0 -- more often in fp32 than in float64 -- and the two runs differ by tens of per cent from the first step on.
FIT_CONFIG = dict(lr=1e-3, l2_emb=0.0, hidden_units=40, dropout_rate=0.0, max_len=12, num_blocks=2, num_heads=2, batch_size=32,
                  epochs=2)
TWIN_DEVIATION = {
    "item_embeddings": 6.3e-05,
    "position_embeddings": 0.002,
    "ln1_gamma": 3.4e-05, "ln1_beta": 1.3e-05, "Wq": 0.002, "bq": 1.9e-05, "Wk": 0.002, "bk": 0.00026, "Wv": 0.002, "bv": 1.5e-05,
    "ln2_gamma": 1.6e-05, "ln2_beta": 1.5e-05, "W1": 0.002, "b1": 2.2e-05, "W2": 0.002, "b2": 8.1e-06,
    "ln_out_gamma": 4.4e-06, "ln_out_beta": 6e-06,
}
TWIN_LOSS_DEVIATION = 2.9e-05     # relative, of the per-step losses


def param_names(blocks):
    return ["item_embeddings", "position_embeddings"] + [f"{k}_{b}" for b in range(blocks) for k in BLOCK_NAMES] + \
        ["ln_out_gamma", "ln_out_beta"]


def deviation_of(name):
    """the TWIN_DEVIATION entry of a parameter's name (a block's parameters share one)"""
    return TWIN_DEVIATION[name if name in TWIN_DEVIATION else name.rsplit("_", 1)[0]]


def random_params(rng, I, T, d, blocks):
    """float32 arrays with O(1) pre-activations: sqrt(d) E and the kernels' products have unit scale"""
    p = {"item_embeddings": rng.standard_normal((I, d)) * 0.7 / np.sqrt(d), "position_embeddings": rng.standard_normal((T, d)) * 0.5}
    for b in range(blocks):
        for k in BLOCK_NAMES:
            if k[0] == "W":
                v = rng.standard_normal((d, d)) / np.sqrt(d)
            elif k.endswith("gamma"):
                v = 1.0 + 0.2 * rng.standard_normal(d)
            else:
                v = 0.3 * rng.standard_normal(d)
            p[f"{k}_{b}"] = v
    p["ln_out_gamma"] = 1.0 + 0.2 * rng.standard_normal(d)
    p["ln_out_beta"] = 0.3 * rng.standard_normal(d)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}


def to_torch(params, dtype=torch.float64, requires_grad=True):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def keep_bytes(d, T, blocks, heads):
    return T * d + blocks * (heads * T * T + 2 * T * d)


def split_keeps(keep, d, T, blocks, heads):
    """the flags [n, keep_bytes] as {"in": [n, T, d], ("attn", b): [n, heads, T, T], ("ffn1", b), ("ffn2", b): [n, T, d]}"""
    keep = torch.as_tensor(np.asarray(keep))
    n = keep.shape[0]
    out = {"in": keep[:, :T * d].reshape(n, T, d)}
    o = T * d
    for b in range(blocks):
        out[("attn", b)] = keep[:, o:o + heads * T * T].reshape(n, heads, T, T)
        o += heads * T * T
        out[("ffn1", b)] = keep[:, o:o + T * d].reshape(n, T, d)
        o += T * d
        out[("ffn2", b)] = keep[:, o:o + T * d].reshape(n, T, d)
        o += T * d
    assert o == keep.shape[1]
    return out


def normalize(x, gamma, beta, epsilon=1e-8):
    mean = x.mean(-1, keepdim=True)
    variance = ((x - mean) ** 2).mean(-1, keepdim=True)
    return gamma * ((x - mean) / ((variance + epsilon) ** 0.5)) + beta


def _dropout(x, keep, rate):
    if keep is None or rate <= 0.0:
        return x
    return x * keep.to(x.dtype) / (1.0 - rate)


def attention(queries, keys, P, b, heads, keep, rate, hooks):
    """multihead_attention of the reference (causality=True); ``hooks``: test switches -- "query_mask" False drops the query
    mask, "weights" collects the softmax outputs"""
    n, T, d = queries.shape
    dh = d // heads
    Q = queries @ P[f"Wq_{b}"] + P[f"bq_{b}"]
    K = keys @ P[f"Wk_{b}"] + P[f"bk_{b}"]
    V = keys @ P[f"Wv_{b}"] + P[f"bv_{b}"]
    Q_, K_, V_ = (t.reshape(n, T, heads, dh).permute(0, 2, 1, 3) for t in (Q, K, V))          # [n, h, T, dh]
    outputs = Q_ @ K_.transpose(-1, -2) / (dh ** 0.5)
    key_masks = torch.sign(torch.abs(keys.sum(-1)))                                           # [n, T_k]
    paddings = torch.full_like(outputs, PAD_FILL)
    outputs = torch.where((key_masks == 0)[:, None, None, :].expand_as(outputs), paddings, outputs)
    tril = torch.tril(torch.ones(T, T, dtype=outputs.dtype))
    outputs = torch.where((tril == 0)[None, None].expand_as(outputs), paddings, outputs)
    outputs = torch.softmax(outputs, -1)
    if hooks is not None and "weights" in hooks:
        hooks["weights"].append(outputs)
    if hooks is None or hooks.get("query_mask", True):
        query_masks = torch.sign(torch.abs(queries.sum(-1)))                                  # [n, T_q]
        outputs = outputs * query_masks[:, None, :, None]
    outputs = _dropout(outputs, keep, rate)
    outputs = outputs @ V_                                                                    # [n, h, T, dh]
    outputs = outputs.permute(0, 2, 1, 3).reshape(n, T, d)
    return outputs + queries


def feedforward(inputs, P, b, keep1, keep2, rate):
    outputs = torch.relu(inputs @ P[f"W1_{b}"] + P[f"b1_{b}"])
    outputs = _dropout(outputs, keep1, rate)
    outputs = outputs @ P[f"W2_{b}"] + P[f"b2_{b}"]
    outputs = _dropout(outputs, keep2, rate)
    return outputs + inputs


def tables(P):
    d = P["item_embeddings"].shape[1]
    E = torch.cat([P["item_embeddings"], torch.zeros(1, d, dtype=P["item_embeddings"].dtype)], 0) * (d ** 0.5)
    return E


def forward(P, seq, blocks, heads, keep=None, rate=0.0, hooks=None):
    """out [n, T, d] = the graph of _build_model up to the last normalize; ``seq`` long [n, T]; ``keep``: flags [n, keep_bytes]
    or None (no dropout); hooks["padded_queries"]: a tensor [n, T, d] ADDED to the normalised queries of padded positions in
    every block (the host suite shows that it changes nothing)"""
    I, d = P["item_embeddings"].shape
    T = seq.shape[1]
    K = split_keeps(keep, d, T, blocks, heads) if keep is not None and rate > 0.0 else None
    x = tables(P)[seq] + P["position_embeddings"][None, :T]
    x = _dropout(x, K["in"] if K else None, rate)
    mask = (seq != I).to(x.dtype).unsqueeze(-1)
    x = x * mask
    for b in range(blocks):
        q = normalize(x, P[f"ln1_gamma_{b}"], P[f"ln1_beta_{b}"])
        if hooks is not None and "padded_queries" in hooks:
            q = q + hooks["padded_queries"] * (1.0 - mask)
        x = attention(q, x, P, b, heads, K[("attn", b)] if K else None, rate, hooks)
        x = feedforward(normalize(x, P[f"ln2_gamma_{b}"], P[f"ln2_beta_{b}"]), P, b, K[("ffn1", b)] if K else None,
                        K[("ffn2", b)] if K else None, rate)
        x = x * mask
    return normalize(x, P["ln_out_gamma"], P["ln_out_beta"])


def logits(P, out, pos, neg):
    E = tables(P)
    return (E[pos] * out).sum(-1), (E[neg] * out).sum(-1)


def loss_of_logits(pos_logits, neg_logits, is_target, stable=False):
    """the reference's two log losses over the targets; ``stable``: sigmoid(-x) in place of 1 - sigmoid(x)"""
    pos_loss = -torch.log(torch.sigmoid(pos_logits) + 1e-24) * is_target
    one_minus = torch.sigmoid(-neg_logits) if stable else 1 - torch.sigmoid(neg_logits)
    neg_loss = -torch.log(one_minus + 1e-24) * is_target
    return (pos_loss + neg_loss).sum() / is_target.sum()


def step_loss(P, seq, pos, neg, blocks, heads, keep=None, rate=0.0, l2_emb=0.0, hooks=None, stable=False):
    """(mean loss, l2 term); their sum is what the reference minimises"""
    I = P["item_embeddings"].shape[0]
    out = forward(P, seq, blocks, heads, keep, rate, hooks)
    pl, nl = logits(P, out, pos, neg)
    is_target = (pos != I).to(out.dtype)
    loss = loss_of_logits(pl, nl, is_target, stable)
    l2 = 0.5 * l2_emb * ((P["item_embeddings"] ** 2).sum() + (P["position_embeddings"] ** 2).sum())
    return loss, l2


def query_rows(P, windows, blocks, heads):
    """[n, d]: sqrt(d) out[T - 1], so that <row, item_embeddings[i]> is the reference's all_logits"""
    with torch.no_grad():
        d = P["item_embeddings"].shape[1]
        return forward(P, windows, blocks, heads)[:, -1, :] * (d ** 0.5)


class TFAdam(object):
    """tf.train.AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); p -= lr_t m / (sqrt(v) + eps)"""

    def __init__(self, P, lr, beta1=0.9, beta2=0.98, eps=1e-8):
        self.P, self.lr, self.b1, self.b2, self.eps, self.t = P, lr, beta1, beta2, eps, 0
        self.m = {k: torch.zeros_like(v) for k, v in P.items()}
        self.v = {k: torch.zeros_like(v) for k, v in P.items()}

    def step(self):
        self.t += 1
        lr_t = self.lr * (1.0 - self.b2 ** self.t) ** 0.5 / (1.0 - self.b1 ** self.t)
        with torch.no_grad():
            for k, p in self.P.items():
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                self.m[k].mul_(self.b1).add_(g, alpha=1.0 - self.b1)
                self.v[k].mul_(self.b2).addcmul_(g, g, value=1.0 - self.b2)
                p.sub_(lr_t * self.m[k] / (self.v[k].sqrt() + self.eps))
                p.grad = None


def trajectory(params, batches, blocks, heads, lr, keeps=None, rate=0.0, l2_emb=0.0, dtype=torch.float64, stable=True):
    """the run over ``batches`` (a list of (seq, pos, neg) integer arrays): -> (per-step mean losses, final parameters as numpy).
    ``stable``: the kernel's sigmoid(-x); at the fit tests' logits the two forms agree to float64's rounding"""
    P = to_torch(params, dtype)
    opt = TFAdam(P, lr)
    losses = []
    for k, (seq, pos, neg) in enumerate(batches):
        seq, pos, neg = (torch.as_tensor(np.asarray(a)).long() for a in (seq, pos, neg))
        loss, l2 = step_loss(P, seq, pos, neg, blocks, heads, None if keeps is None else keeps[k], rate, l2_emb, stable=stable)
        (loss + l2).backward()
        losses.append(float(loss.detach()))
        opt.step()
    return np.array(losses), {k: v.detach().numpy().astype(np.float64) for k, v in P.items()}


# ---- the library's layouts -------------------------------------------------------------------------------------------
BLOCK_ROWS = 329
ROWS = dict(ln1_gamma=0, ln1_beta=1, Wq=2, bq=66, Wk=67, bk=131, Wv=132, bv=196, ln2_gamma=197, ln2_beta=198, W1=199, b1=263, W2=264,
            b2=328)


def shared_floats(blocks):
    return 64 * (BLOCK_ROWS * blocks + 2)


def pad_cols(a, width=64):
    a = np.asarray(a, dtype=np.float32)
    out = np.zeros((a.shape[0], width), np.float32)
    out[:, :a.shape[1]] = a
    return out


def shared_block(params, d, blocks):
    """the shared parameters in skr_sasrec_step's layout (float32): kernels transposed, [out][in]"""
    s = np.zeros((BLOCK_ROWS * blocks + 2, 64), np.float32)
    for b in range(blocks):
        for k, r in ROWS.items():
            v = np.asarray(params[f"{k}_{b}"])
            if k[0] == "W":
                s[b * BLOCK_ROWS + r:b * BLOCK_ROWS + r + d, :d] = v.T
            else:
                s[b * BLOCK_ROWS + r, :d] = v
    s[BLOCK_ROWS * blocks, :d] = np.asarray(params["ln_out_gamma"])
    s[BLOCK_ROWS * blocks + 1, :d] = np.asarray(params["ln_out_beta"])
    return s.reshape(-1)


def unpack_shared(s, d, blocks):
    """(the reference-shaped arrays of a shared block or of its gradient, what lies in the padding): the second must be zero"""
    s = np.asarray(s).reshape(BLOCK_ROWS * blocks + 2, 64)
    rest = s.copy()
    out = {}
    for b in range(blocks):
        for k, r in ROWS.items():
            r0 = b * BLOCK_ROWS + r
            if k[0] == "W":
                out[f"{k}_{b}"] = s[r0:r0 + d, :d].T.copy()
                rest[r0:r0 + d, :d] = 0
            else:
                out[f"{k}_{b}"] = s[r0, :d].copy()
                rest[r0, :d] = 0
    for j, k in enumerate(("ln_out_gamma", "ln_out_beta")):
        out[k] = s[BLOCK_ROWS * blocks + j, :d].copy()
        rest[BLOCK_ROWS * blocks + j, :d] = 0
    return out, rest


# ---- measurement (CPU): python tests/sasrec_twin.py ---------------------------------------------------------------------
def tiny_train_rows(golden_npz, max_len):
    """(user_pos_train by time, users, seq, pos) of the tiny sequential set, by a literal loop"""
    d = np.load(golden_npz)
    tr = d["train"]
    order = np.lexsort((tr[:, 2], tr[:, 0]))
    upt = {}
    for u, i, _ in tr[order]:
        upt.setdefault(int(u), []).append(int(i))
    users = list(upt.keys())
    I = int(d["num_items"])
    seq, pos = (np.full((len(users), max_len), I, np.int32) for _ in range(2))
    for r, u in enumerate(users):
        a, b = upt[u][:-1][-max_len:], upt[u][1:][-max_len:]
        if len(a):
            seq[r, max_len - len(a):] = a
            pos[r, max_len - len(b):] = b
    return upt, users, seq, pos, I


def measure_deviation(golden_npz):
    cfg = FIT_CONFIG
    d, T, nb, nh, bs = cfg["hidden_units"], cfg["max_len"], cfg["num_blocks"], cfg["num_heads"], cfg["batch_size"]
    upt, users, seq, pos, I = tiny_train_rows(golden_npz, T)
    rng = np.random.default_rng(5)
    worst, worst_loss = {}, 0.0
    for rate in (0.0, 0.5):
        batches, keeps = [], []
        for _ in range(cfg["epochs"]):
            neg = np.where(pos != I, rng.integers(0, I, pos.shape), I).astype(np.int32)
            perm = rng.permutation(len(users))
            for a in range(0, len(users), bs):
                idx = perm[a:a + bs]
                batches.append((seq[idx], pos[idx], neg[idx]))
                keeps.append((rng.random((len(idx), keep_bytes(d, T, nb, nh))) >= rate).astype(np.uint8))
        p0 = random_params(np.random.default_rng(2021), I, T, d, nb)
        l64, p64 = trajectory(p0, batches, nb, nh, cfg["lr"], keeps, rate, dtype=torch.float64)
        l32, p32 = trajectory(p0, batches, nb, nh, cfg["lr"], keeps, rate, dtype=torch.float32)
        worst_loss = max(worst_loss, float(np.abs(l32 / l64 - 1).max()))
        for k in p64:
            key = k if k in TWIN_DEVIATION else k.rsplit("_", 1)[0]
            worst[key] = max(worst.get(key, 0.0), float(np.abs(p32[k] - p64[k]).max()))
    for k, v in worst.items():
        print(f'    "{k}": {v:.2g},')
    print("TWIN_LOSS_DEVIATION =", f"{worst_loss:.2g}")


if __name__ == "__main__":
    import os
    measure_deviation(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_seq_dataset.npz"))
