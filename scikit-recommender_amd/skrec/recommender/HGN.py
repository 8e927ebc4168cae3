"""HGN on MI355X (reference: skrec/recommender/HGN.py).

Paper: Hierarchical Gating Networks for Sequential Recommendation (Ma, Kang and Liu).
Same config, same initialisation (the constructors of the two embeddings, the two Linear gates, W2 and b2 draw from the
CPU generator in the reference's order, then reset_parameters re-draws in its own: normal(0, 0.01) user and item rows,
he_uniform on the user gate then the item gate, zero biases, xavier_uniform on the two instance gates, normal W2, zero
b2, zero padding rows; HGN.py:58-99), same loss (sum over the batch and the seq_T pairs of -logsigmoid(y_pos - y_neg),
no l2 term, HGN.py:202-203), same optimiser: ``torch.optim.Adam(weight_decay=reg)`` over every parameter.  One training
step is ``skr_hgn_step`` (csrc/hgn.hip: the fused forward/backward, then the gate gradients summed in a fixed order)
and the weight-decay Adam update of the flat buffer (skrec/recommender/_seq.py, whose engine takes the iterator's
[n, seq_L] windows and [n, seq_T] targets as they come).

Like the reference, ``num_items`` counts the padding item (``pad_idx`` = the data set's item count): every item table
has that row, ``predict`` returns that column (its score is b2[pad] = 0) and the evaluator ranks it like any item.

Scoring collapses to one query row per user, q_u = p_u + union(u) + sum_l e_{s_l}, with y = <q_u, W2[t]> + b2[t]: the
rows are computed once per evaluation (``skr_hgn_queries``) and the evaluator's fused top-K path ranks them.

Limits: embed_size <= 64 (zero-padded to 64), 1 <= seq_L <= 32, 1 <= seq_T <= 16, one GPU.

Where the reference's own code fails -- a last batch of exactly one instance, or seq_T = 1, whose ``.squeeze()`` calls
change rank (HGN.py:111,128-138) -- the kernel computes the mathematically intended result; there is no parity claim
for those shapes.
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

__all__ = ["HGN", "HGNConfig"]


class HGNConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=1e-3, seq_L=5, seq_T=3, embed_size=64, batch_size=1024, epochs=1000, early_stop=100,
                 **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.seq_L: int = seq_L
        self.seq_T: int = seq_T
        self.embed_size: int = embed_size
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.seq_L, int) and self.seq_L > 0
        assert isinstance(self.seq_T, int) and self.seq_T > 0
        assert isinstance(self.embed_size, int) and self.embed_size > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def _init_tables(num_users, num_rows, dim, seq_L, pad_idx):
    """CPU-side construction in the reference's order (_HGN.__init__ / reset_parameters, HGN.py:58-99); ``num_rows``
    counts the padding row"""
    ue = nn.Embedding(num_users, dim)
    ie = nn.Embedding(num_rows, dim, padding_idx=pad_idx)
    gi, gu = nn.Linear(dim, dim), nn.Linear(dim, dim)
    igi, igu = torch.empty(dim, 1), torch.empty(dim, seq_L)      # Parameter(torch.Tensor(...)): no draw
    w2 = nn.Embedding(num_rows, dim, padding_idx=pad_idx)
    b2 = nn.Embedding(num_rows, 1, padding_idx=pad_idx)
    normal, he, xavier, zeros = (get_initializer(k) for k in ("normal", "he_uniform", "xavier_uniform", "zeros"))
    normal(ue.weight)
    normal(ie.weight)
    he(gu.weight)
    he(gi.weight)
    zeros(gu.bias)
    zeros(gi.bias)
    xavier(igi)
    xavier(igu)
    normal(w2.weight)
    zeros(b2.weight)
    with torch.no_grad():
        ie.weight[pad_idx].zero_()
        w2.weight[pad_idx].zero_()
    return tuple(t.detach() for t in (ue.weight, ie.weight, gi.weight, gi.bias, gu.weight, gu.bias, igi, igu, w2.weight,
                                      b2.weight))


class HGN(SeqPairwiseRecommender):
    """limits: embed_size <= 64 (NotImplementedError beyond), 1 <= seq_L <= 32 and 1 <= seq_T <= 16 (ValueError:
    ``skr_hgn_step`` holds an instance's window, instance gates and targets one per lane), one GPU.
    ``detached``: ``num_items`` without the padding item"""
    config_class = HGNConfig

    def _check_limits(self, world):
        e, Lw, T = self.config.embed_size, self.config.seq_L, self.config.seq_T
        if e > 64:
            raise NotImplementedError(f"HGN: embed_size <= 64 (got {e}): rows are 64 floats, the gate matrices live in LDS "
                                      f"and the fused evaluator ranks 64 columns")
        if not (1 <= Lw <= _hip.SKR_HGN_MAX_L and 1 <= T <= _hip.SKR_HGN_MAX_T):
            raise ValueError(f"HGN: 1 <= seq_L <= {_hip.SKR_HGN_MAX_L} and 1 <= seq_T <= {_hip.SKR_HGN_MAX_T} "
                             f"(got {Lw}, {T}): skr_hgn_step holds an instance's window and targets one per lane")
        super()._check_limits(world)

    def _build_args(self, run_config):
        kw = super()._build_args(run_config)
        # every user's window of the last seq_L training items; a user without history gets -1 (predict raises first)
        Lw, pad = self.config.seq_L, self.num_items                    # the padding item: HGN.py:173-174
        self.user_truncated_seq = self.dataset.train_data.to_truncated_seq_dict(Lw, pad_value=pad, padding="pre",
                                                                                truncating="pre")
        win = np.full((self.num_users, Lw), -1, np.int32)
        for u, row in self.user_truncated_seq.items():
            win[int(u)] = row
        return dict(kw, windows=win)

    @property
    def _weight_decay(self):
        return self.config.reg                       # HGN.py:182: the regulariser sits in the optimiser

    def _make_iterator(self):
        cfg = self.config
        return SequentialPairwiseIterator(self.dataset.train_data, num_previous=cfg.seq_L, num_next=cfg.seq_T,
                                          pad=self.pad_idx, batch_size=cfg.batch_size, shuffle=True, drop_last=False)

    def _build(self, windows=None, last_items=None):
        """``windows``: int32 [num_users, seq_L], every user's last seq_L training items, left-padded with the padding item
        (``detached``'s default: item 0 in every position)"""
        from ._sparse import pad_columns
        super()._build(last_items)
        cfg = self.config
        e, Lw, T = cfg.embed_size, cfg.seq_L, cfg.seq_T
        self.pad_idx = self.num_items                 # HGN.py:173-174
        self.num_items += 1
        nu, ni, d = self.num_users, self.num_items, 64
        self.dp = d
        win = np.zeros((nu, Lw), np.int32)
        if windows is not None:
            win[:] = np.asarray(windows, dtype=np.int32).reshape(nu, Lw)
        self._windows = torch.from_numpy(win).to(self.device)
        ue, ie, giw, gib, guw, gub, igi, igu, w2, b2 = _init_tables(nu, ni, e, Lw, self.pad_idx)
        nb = 64 * ((ni + 63) // 64)                   # b2, zero-padded to whole 64-float blocks
        sq = lambda w: nn.functional.pad(w, (0, d - e, 0, d - e)).reshape(-1)      # noqa: E731  [e, e] -> [64, 64]
        vec = lambda w: nn.functional.pad(w.reshape(-1), (0, d - e))               # noqa: E731
        # one flat buffer [user | item (I+1) | W2 (I+1) | b2 | gates], every segment on a 64-float boundary; the gate
        # segment in skr_hgn_step's layout (instance_gate_user transposed: one 64-float row per window position)
        flat = torch.cat([pad_columns(ue, d).reshape(-1), pad_columns(ie, d).reshape(-1), pad_columns(w2, d).reshape(-1),
                          nn.functional.pad(b2.reshape(-1), (0, nb - ni)), sq(giw), sq(guw), vec(gib), vec(gub), vec(igi),
                          pad_columns(igu.t().contiguous(), d).reshape(-1)])
        ng = _hip.hgn_gate_floats(Lw)
        self._off = o = (0, nu * d, (nu + ni) * d, (nu + 2 * ni) * d, (nu + 2 * ni) * d + nb)
        assert flat.numel() == o[4] + ng
        self._setup(flat.to(self.device).contiguous())
        f = self._flat
        self._user_rows, self._item_rows = f[o[0]:o[1]].view(nu, d), f[o[1]:o[2]].view(ni, d)
        self._w2_rows, self._b2 = f[o[2]:o[3]].view(ni, d), f[o[3]:o[3] + ni]
        self._gates = f[o[4]:o[4] + ng]
        # the reference's parameters (their first embed_size columns)
        g = self._gates
        self.user_embeddings, self.item_embeddings = self._user_rows[:, :e], self._item_rows[:, :e]
        self.W2, self.b2 = self._w2_rows[:, :e], self._b2.view(ni, 1)
        self.feature_gate_item_weight = g[:4096].view(d, d)[:e, :e]
        self.feature_gate_user_weight = g[4096:8192].view(d, d)[:e, :e]
        self.feature_gate_item_bias, self.feature_gate_user_bias = g[8192:8192 + e], g[8256:8256 + e]
        self.instance_gate_item = g[8320:8384].view(d, 1)[:e]
        self.instance_gate_user = g[8384:].view(Lw, d)[:, :e].t()
        opt = self.optimizer
        grads = (opt.grad_view(o[0], (nu, d)), opt.grad_view(o[1], (ni, d)), opt.grad_view(o[2], (ni, d)),
                 opt.grad_view(o[3], (ni,)), opt.grad_view(o[4], (ng,)))
        self._work = torch.empty(_hip.SKR_HGN_MAX_BLOCKS * ng, dtype=torch.float32, device=self.device)
        self._Q = torch.empty((nu, d), dtype=torch.float32, device=self.device)
        self._q_current = False
        L = _hip.lib()
        pt = [t.data_ptr() for t in (self._user_rows, self._item_rows, self._w2_rows, self._b2, self._gates)]
        pg = [t.data_ptr() for t in grads]
        pw, pad = self._work.data_ptr(), self.pad_idx

        def step(pu, pl, pp, pn, n, ploss, st):
            return L.skr_hgn_step(*pt, pu, pl, pp, pn, n, nu, ni, pad, d, Lw, T, *pg, pw, ploss, _hip.SKR_LOSS_SLOTS, st)
        self._step_launch = step

    def _block_id_parts(self, u, seq, p, n):
        # 64-float blocks of U[u], the window's item rows (not the padding row: it has no gradient and stays zero),
        # W2[p], W2[n] and of the words b2[p], b2[n]
        b = [o // 64 for o in self._off]
        return [u + b[0], torch.where(seq == self.pad_idx, -1, seq + b[1]).int(), p + b[2], n + b[2], (p >> 6) + b[3],
                (n >> 6) + b[3]]

    def _block_ids_per_step(self):
        g0 = self._off[4] // 64                       # the gate parameters: every batch
        return list(range(g0, g0 + self._gates.numel() // 64))

    # ---- training --------------------------------------------------------------------------------
    def train_epoch(self, data_iter):
        self._q_current = False
        return super().train_epoch(data_iter)

    # ---- ranking ---------------------------------------------------------------------------------
    @on_compute_stream
    def predict_factors(self):
        """(Q [num_users, 64], W2 [num_items, 64], b2 [num_items]): score = <Q[u], W2[i]> + b2[i].  Q is computed by
        one ``skr_hgn_queries`` launch over all users and kept until the next training step; the row of a user without
        training history is NaN (predict / evaluate raise KeyError before they ask)"""
        if not self._q_current:
            _hip.check(_hip.lib().skr_hgn_queries(_hip.ptr(self._user_rows), _hip.ptr(self._item_rows), _hip.ptr(self._gates),
                                                  None, self.num_users, _hip.ptr(self._windows), self.num_users,
                                                  self.num_items, self.pad_idx, 64, self.config.seq_L, _hip.ptr(self._Q),
                                                  _hip.stream()))
            self._q_current = True
        return self._Q, self._w2_rows, self._b2

    def score_rows(self, d_users, out):
        """evaluator hook for the cases its fused path does not take: dense score rows into ``out`` [B, num_items]"""
        Q, W2, b2 = self.predict_factors()
        _hip.check(_hip.lib().skr_score_matrix(_hip.ptr(Q), _hip.ptr(d_users), d_users.numel(), _hip.ptr(W2), _hip.ptr(b2),
                                               self.num_items, 64, _hip.ptr(out), out.stride(0), _hip.stream()))

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores, the padding item's column included (HGN.py:147-163,222-227)"""
        users = list(users)
        self._require_history(users)
        return DeviceRecommender.predict(self, users)
