"""Caser on MI355X (reference: skrec/recommender/Caser.py).

Paper: Personalized Top-N Sequential Recommendation via Convolutional Sequence Embedding (Tang and Wang).
Same config, same initialisation (the constructors of the two embeddings, conv_v, the seq_L conv_h, fc1, W2 and b2 draw
from the CPU generator in the reference's order, then reset_parameters re-draws normal(0, 0.01) user rows, item rows and W2
and zeroes b2; Caser.py:80-116), same loss (the mean over the batch and the seq_T pairs of bce(y_pos, 1) + bce(y_neg, 0),
Caser.py:199-203), same optimiser: ``torch.optim.Adam(weight_decay=l2_reg)`` over every parameter.  One training step is
``skr_caser_step`` (csrc/caser.hip) and the weight-decay Adam update of the flat buffer (skrec/recommender/_seq.py).

Like the reference, ``num_items`` counts the padding item (``pad_idx`` = the data set's item count) -- and, like the
reference, that item is an ORDINARY row: ``_Caser`` is built without ``item_pad_idx`` (Caser.py:179), so ``padding_idx`` is
None in all three embeddings, the row is normal-initialised, read in padded windows and trained.  ``predict`` returns its
column and the evaluator ranks it like any item.

Dropout: the step draws its keep flags on the device, keyed by (the run's seed, the step's number, user, column): equal
to torch's draws in law only.  ``keep_in`` (uint8 [instances of the coming steps, nv e + nh L], in the reference's column
order, consumed step by step) replays recorded flags; ``keep_out = []`` collects the flags every step used.

Scoring collapses to one query row per user, x_u = [z_u, p_u] in eval mode from the user's last seq_L training items, with
y = <x_u, W2[t]> + b2[t]: the rows are computed once per evaluation (``skr_caser_queries``) and ranked by the fused
top-K evaluator at 128 columns (``predict_factors``); ``score_rows`` stays as the dense hook (``skr_score_matrix``), which
the evaluator takes under ``SKR_FUSED_MODE=fp32`` or when K leaves too few unmasked items.

Limits: embed_size <= 64 (zero-padded to 64), 1 <= seq_L <= 8, 1 <= seq_T <= 16, 1 <= nv <= 8, 1 <= nh <= 32,
batch_size <= 2048, one GPU.

Where the reference's own code fails -- a last batch of exactly one instance, whose ``.squeeze()`` changes the rank before
``torch.split`` (Caser.py:155,199) -- the kernel computes the mathematically intended result; no parity claim there.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..io import SequentialPairwiseIterator
from ..utils.py import ModelConfig
from ..utils.torch import get_initializer
from ._seq import SeqPairwiseRecommender
from .base import DeviceRecommender, on_compute_stream

__all__ = ["Caser", "CaserConfig"]


class CaserConfig(ModelConfig):
    def __init__(self, lr=1e-3, l2_reg=1e-6, embed_size=64, seq_L=5, seq_T=3, nv=4, nh=16, dropout=0.5, batch_size=1024,
                 epochs=500, early_stop=100, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.l2_reg: float = l2_reg
        self.embed_size: int = embed_size
        self.seq_L: int = seq_L
        self.seq_T: int = seq_T
        self.nv: int = nv
        self.nh: int = nh
        self.dropout: float = dropout
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.l2_reg, float) and self.l2_reg >= 0
        assert isinstance(self.embed_size, int) and self.embed_size > 0
        assert isinstance(self.seq_L, int) and self.seq_L > 0
        assert isinstance(self.seq_T, int) and self.seq_T > 0
        assert isinstance(self.nv, int) and self.nv > 0
        assert isinstance(self.nh, int) and self.nh > 0
        assert isinstance(self.dropout, float)
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def _init_tables(num_users, num_rows, e, L, nv, nh):
    """CPU-side construction in the reference's order (_Caser.__init__ / reset_parameters, Caser.py:80-116); ``num_rows``
    counts the padding item, which is an ordinary row (padding_idx is None there).  -> dict under the reference's names"""
    ue = nn.Embedding(num_users, e)
    ie = nn.Embedding(num_rows, e)
    conv_v = nn.Conv2d(1, nv, (L, 1))
    conv_h = [nn.Conv2d(1, nh, (i + 1, e)) for i in range(L)]
    fc1 = nn.Linear(nv * e + nh * L, e)
    w2 = nn.Embedding(num_rows, 2 * e)
    b2 = nn.Embedding(num_rows, 1)
    normal, zeros = get_initializer("normal"), get_initializer("zeros")
    normal(ue.weight)
    normal(ie.weight)
    normal(w2.weight)
    zeros(b2.weight)
    t = {"user_embeddings": ue.weight, "item_embeddings": ie.weight, "conv_v_weight": conv_v.weight, "conv_v_bias": conv_v.bias,
         "fc1_weight": fc1.weight, "fc1_bias": fc1.bias, "W2": w2.weight, "b2": b2.weight}
    for i, c in enumerate(conv_h):
        t[f"conv_h_weight_{i}"], t[f"conv_h_bias_{i}"] = c.weight, c.bias
    return {k: v.detach() for k, v in t.items()}


def _fc1_columns(e, L, nv, nh):
    """the padded column of every reference column of fc1.weight: c e + col -> 64 c + col, then the nh L pooled ones"""
    v = (torch.arange(nv).view(-1, 1) * 64 + torch.arange(e).view(1, -1)).reshape(-1)
    return torch.cat([v, nv * 64 + torch.arange(nh * L)])


class _Layout(object):
    """offsets (in floats) of the flat buffer [U | E | W2 | b2 | shared], every segment on a 64-float boundary, and of the
    parts of the shared block (include/skrec_hip.h, section Caser)"""

    def __init__(self, nu, ni, L, nv, nh):
        self.nu, self.ni, self.L, self.nv, self.nh = nu, ni, L, nv, nh
        self.nb = 64 * ((ni + 63) // 64)
        self.fp = _hip.caser_fp(L, nv, nh)
        self.rows = _hip.caser_rows(L, nh)
        self.ns = _hip.caser_shared_floats(L, nv, nh)
        self.U, self.E = 0, nu * 64
        self.W2 = self.E + ni * 64
        self.b2 = self.W2 + ni * 128
        self.shared = self.b2 + self.nb
        self.total = self.shared + self.ns
        self.s_wv, self.s_bv, self.s_wh = 0, 64, 128
        self.s_bh = self.s_wh + 64 * self.rows
        self.s_w1 = self.s_bh + 64 * ((L * nh + 63) // 64)
        self.s_b1 = self.s_w1 + 64 * self.fp


def pack_parameters(tables, lay, e):
    """the flat fp32 buffer of ``lay`` from tensors in the reference's shapes (zero where padded)"""
    from ._sparse import pad_columns
    L, nv, nh = lay.L, lay.nv, lay.nh
    flat = torch.zeros(lay.total, dtype=torch.float32)
    flat[lay.U:lay.E] = pad_columns(tables["user_embeddings"], 64).reshape(-1)
    flat[lay.E:lay.W2] = pad_columns(tables["item_embeddings"], 64).reshape(-1)
    w2 = tables["W2"]
    flat[lay.W2:lay.b2] = torch.cat([pad_columns(w2[:, :e].contiguous(), 64), pad_columns(w2[:, e:].contiguous(), 64)], 1).reshape(-1)
    flat[lay.b2:lay.b2 + lay.ni] = tables["b2"].reshape(-1)
    s = flat[lay.shared:]
    s[:nv * L] = tables["conv_v_weight"].reshape(-1)
    s[lay.s_bv:lay.s_bv + nv] = tables["conv_v_bias"]
    row = 0
    for i in range(L):
        k = nh * (i + 1)
        s[lay.s_wh + 64 * row:lay.s_wh + 64 * (row + k)].view(k, 64)[:, :e] = tables[f"conv_h_weight_{i}"].reshape(k, e)
        row += k
        s[lay.s_bh + i * nh:lay.s_bh + (i + 1) * nh] = tables[f"conv_h_bias_{i}"]
    s[lay.s_w1:lay.s_b1].view(64, lay.fp)[:e, _fc1_columns(e, L, nv, nh)] = tables["fc1_weight"]
    s[lay.s_b1:lay.s_b1 + e] = tables["fc1_bias"]
    return flat


def parameter_views(flat, lay, e):
    """the reference's parameters, under its names and in its shapes, as VIEWS into the flat buffer ``flat`` -- except
    ``fc1_weight`` and ``W2`` for embed_size < 64: the reference's fc1 column c e + col lies at 64 c + col and its W2 column
    e + col at 64 + col, which no stride expresses, so those two are gathered COPIES there (write through ``flat``)"""
    L, nv, nh, ni = lay.L, lay.nv, lay.nh, lay.ni
    s = flat[lay.shared:lay.total]
    v = {"user_embeddings": flat[lay.U:lay.E].view(lay.nu, 64)[:, :e], "item_embeddings": flat[lay.E:lay.W2].view(ni, 64)[:, :e],
         "conv_v_weight": s[:nv * L].view(nv, 1, L, 1), "conv_v_bias": s[lay.s_bv:lay.s_bv + nv],
         "fc1_bias": s[lay.s_b1:lay.s_b1 + e], "b2": flat[lay.b2:lay.b2 + ni].view(ni, 1)}
    row = 0
    for i in range(L):
        k = nh * (i + 1)
        v[f"conv_h_weight_{i}"] = s[lay.s_wh + 64 * row:lay.s_wh + 64 * (row + k)].view(nh, 1, i + 1, 64)[..., :e]
        v[f"conv_h_bias_{i}"] = s[lay.s_bh + i * nh:lay.s_bh + (i + 1) * nh]
        row += k
    w1 = s[lay.s_w1:lay.s_b1].view(64, lay.fp)
    w2 = flat[lay.W2:lay.b2].view(ni, 128)
    if e == 64:
        v["fc1_weight"], v["W2"] = w1[:, :nv * 64 + nh * L], w2
    else:
        v["fc1_weight"] = w1[:e][:, _fc1_columns(e, L, nv, nh).to(flat.device)]
        v["W2"] = torch.cat([w2[:, :e], w2[:, 64:64 + e]], 1)
    return v


class Caser(SeqPairwiseRecommender):
    """limits: embed_size <= 64 (NotImplementedError beyond), 1 <= seq_L <= 8, 1 <= seq_T <= 16, 1 <= nv <= 8, 1 <= nh <= 32,
    batch_size <= 2048, 0 <= dropout < 1 (ValueError), one GPU.  ``detached``: ``num_items`` without the padding item;
    ``seed``: the key of the device draws (the run's seed otherwise)"""
    config_class = CaserConfig

    def _check_limits(self, world):
        c = self.config
        if c.embed_size > 64:
            raise NotImplementedError(f"Caser: embed_size <= 64 (got {c.embed_size}): rows are 64 floats")
        for name, hi in (("seq_L", _hip.SKR_CASER_MAX_L), ("seq_T", _hip.SKR_CASER_MAX_T), ("nv", _hip.SKR_CASER_MAX_NV),
                         ("nh", _hip.SKR_CASER_MAX_NH), ("batch_size", _hip.SKR_CASER_MAX_BATCH)):
            if not 1 <= getattr(c, name) <= hi:
                raise ValueError(f"Caser: 1 <= {name} <= {hi} (got {getattr(c, name)}): a limit of skr_caser_step")
        if not 0.0 <= c.dropout < 1.0:
            raise ValueError(f"Caser: 0 <= dropout < 1 (got {c.dropout})")
        super()._check_limits(world)

    def _build_args(self, run_config):
        kw = super()._build_args(run_config)
        Lw, pad = self.config.seq_L, self.num_items                    # the padding item: Caser.py:171-176
        self.user_truncated_seq = self.dataset.train_data.to_truncated_seq_dict(Lw, pad_value=pad, padding="pre",
                                                                                truncating="pre")
        win = np.full((self.num_users, Lw), -1, np.int32)
        for u, row in self.user_truncated_seq.items():
            win[int(u)] = row
        return dict(kw, windows=win, seed=getattr(run_config, "seed", 0) or 0)

    @property
    def _weight_decay(self):
        return self.config.l2_reg                    # Caser.py:180: the regulariser sits in the optimiser

    def _make_iterator(self):
        cfg = self.config
        return SequentialPairwiseIterator(self.dataset.train_data, num_previous=cfg.seq_L, num_next=cfg.seq_T,
                                          pad=self.pad_idx, batch_size=cfg.batch_size, shuffle=True, drop_last=False)

    def _build(self, windows=None, last_items=None, seed=0):
        """``windows``: int32 [num_users, seq_L], every user's last seq_L training items, left-padded with the padding item
        (``detached``'s default: item 0 in every position)"""
        super()._build(last_items)
        cfg = self.config
        e, Lw, T, nv, nh = cfg.embed_size, cfg.seq_L, cfg.seq_T, cfg.nv, cfg.nh
        self.pad_idx = self.num_items                 # Caser.py:171-172
        self.num_items += 1
        nu, ni = self.num_users, self.num_items
        self.dp = 64
        self.seed, self.update_count = int(seed), 0
        self.keep_in, self.keep_out, self._keep_cursor = None, None, 0
        self.timed_ms = None      # float32 numpy [SKR_CASER_LAUNCHES]: every step goes through skr_caser_step_timed (tools)
        win = np.zeros((nu, Lw), np.int32)
        if windows is not None:
            win[:] = np.asarray(windows, dtype=np.int32).reshape(nu, Lw)
        self._windows = torch.from_numpy(win).to(self.device)
        self._lay = lay = _Layout(nu, ni, Lw, nv, nh)
        self._setup(pack_parameters(_init_tables(nu, ni, e, Lw, nv, nh), lay, e).to(self.device).contiguous())
        f = self._flat
        self._user_rows, self._item_rows = f[lay.U:lay.E].view(nu, 64), f[lay.E:lay.W2].view(ni, 64)
        self._w2_rows, self._b2 = f[lay.W2:lay.b2].view(ni, 128), f[lay.b2:lay.b2 + ni]
        self._shared = f[lay.shared:lay.total]
        self._bind_views()
        opt = self.optimizer
        grads = (opt.grad_view(lay.U, (nu, 64)), opt.grad_view(lay.E, (ni, 64)), opt.grad_view(lay.W2, (ni, 128)),
                 opt.grad_view(lay.b2, (ni,)), opt.grad_view(lay.shared, (lay.ns,)))
        L = _hip.lib()
        nbytes = int(L.skr_caser_workspace(max(cfg.batch_size, 1024), Lw, nv, nh))
        self._work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._Q = torch.empty((nu, 128), dtype=torch.float32, device=self.device)
        self._q_current = False
        self._fref = nv * e + nh * Lw
        pt = [t.data_ptr() for t in (self._user_rows, self._item_rows, self._w2_rows, self._b2, self._shared)]
        pg = [t.data_ptr() for t in grads]
        pw, rate = self._work.data_ptr(), float(cfg.dropout)

        def step(pu, pl, pp, pn, n, ploss, st):
            pk = pko = None
            if rate > 0.0 and self.keep_in is not None:
                pk = self.keep_in.data_ptr() + self._keep_cursor * self._fref
                assert self._keep_cursor + n <= self.keep_in.shape[0], "keep_in holds fewer rows than the steps consume"
                self._keep_cursor += n
            if self.keep_out is not None:
                ko = torch.empty((n, self._fref), dtype=torch.uint8, device=self.device)
                self.keep_out.append(ko)
                pko = ko.data_ptr()
            self.update_count += 1
            # pad_idx = -1: the padding item is an ordinary row, as in the reference
            args = (*pt, pu, pl, pp, pn, n, nu, ni, -1, 64, e, Lw, T, nv, nh, rate, pk, pko, self.seed, self.update_count, *pg, pw,
                    nbytes, ploss, _hip.SKR_LOSS_SLOTS, st)
            if self.timed_ms is None:
                return L.skr_caser_step(*args)
            return L.skr_caser_step_timed(*args, self.timed_ms.ctypes.data)
        self._step_launch = step

    def _bind_views(self):
        """the reference's parameters as attributes (``parameter_views``); ``conv_h_weight`` / ``conv_h_bias`` are lists"""
        v = parameter_views(self._flat, self._lay, self.config.embed_size)
        for k in ("user_embeddings", "item_embeddings", "conv_v_weight", "conv_v_bias", "fc1_bias", "b2"):
            setattr(self, k, v[k])
        self.conv_h_weight = [v[f"conv_h_weight_{i}"] for i in range(self.config.seq_L)]
        self.conv_h_bias = [v[f"conv_h_bias_{i}"] for i in range(self.config.seq_L)]

    @property
    def fc1_weight(self):
        """[e, nv e + nh L]: a view at embed_size 64, a gathered copy below (see ``parameter_views``)"""
        return parameter_views(self._flat, self._lay, self.config.embed_size)["fc1_weight"]

    @property
    def W2(self):
        """[num_items, 2 e]: a view at embed_size 64, a gathered copy below (see ``parameter_views``)"""
        return parameter_views(self._flat, self._lay, self.config.embed_size)["W2"]

    def reference_parameters(self):
        """every parameter under the reference's name (conv_h_weight_<i>, conv_h_bias_<i>) in the reference's shape"""
        return parameter_views(self._flat, self._lay, self.config.embed_size)

    def _block_id_parts(self, u, seq, p, n):
        # 64-float blocks of U[u], the window's item rows (the padding item's too: it is an ordinary row), the TWO blocks
        # of every W2[p], W2[n] and the blocks of the words b2[p], b2[n]
        lay = self._lay
        bu, be, bw, bb = lay.U // 64, lay.E // 64, lay.W2 // 64, lay.b2 // 64
        return [u + bu, seq + be, 2 * p + bw, 2 * p + (bw + 1), 2 * n + bw, 2 * n + (bw + 1), (p >> 6) + bb, (n >> 6) + bb]

    def _block_ids_per_step(self):
        g0 = self._lay.shared // 64                   # the shared parameters: every batch
        return list(range(g0, g0 + self._lay.ns // 64))

    # ---- training --------------------------------------------------------------------------------
    def train_epoch(self, data_iter):
        self._q_current = False
        return super().train_epoch(data_iter)

    # ---- ranking ---------------------------------------------------------------------------------
    @on_compute_stream
    def predict_factors(self):
        """(Q [num_users, 128], W2 [num_items, 128], b2 [num_items]): score = <Q[u], W2[i]> + b2[i].  Q is computed by
        one ``skr_caser_queries`` call over all users and kept until the next training step; the row of a user without
        training history is NaN (predict / evaluate raise KeyError before they ask)"""
        if not self._q_current:
            cfg = self.config
            _hip.check(_hip.lib().skr_caser_queries(_hip.ptr(self._user_rows), _hip.ptr(self._item_rows), _hip.ptr(self._shared),
                                                    None, self.num_users, _hip.ptr(self._windows), self.num_users,
                                                    self.num_items, -1, 64, cfg.embed_size, cfg.seq_L, cfg.nv, cfg.nh,
                                                    _hip.ptr(self._work), self._work.numel(), _hip.ptr(self._Q), _hip.stream()))
            self._q_current = True
        return self._Q, self._w2_rows, self._b2

    def score_rows(self, d_users, out):
        """evaluator hook: dense score rows of the int32 device users into ``out`` [B, num_items]; the evaluator's device
        top-K ranks them (the path FPMC and TransRec rank on)"""
        Q, W2, b2 = self.predict_factors()
        _hip.check(_hip.lib().skr_score_matrix(_hip.ptr(Q), _hip.ptr(d_users), d_users.numel(), _hip.ptr(W2), _hip.ptr(b2),
                                               self.num_items, 128, _hip.ptr(out), out.stride(0), _hip.stream()))

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores, the padding item's column included (Caser.py:159-162,222-227)"""
        users = list(users)
        self._require_history(users)
        return DeviceRecommender.predict(self, users)
