"""TransRec on MI355X (reference: skrec/recommender/TransRec.py).

Paper: Translation-based Recommendation (He, Kang and McAuley).
Same config (``reg`` defaults to 0.0), same initialisation (the user, item and bias nn.Embedding constructors draw
N(0,1), the uninitialised global transition draws nothing; then zeros(user), normal(T), normal(item), zeros(bias),
TransRec.py:57-73, on the CPU in that order), same loss (sum over the batch of -log sigmoid(y_p - y_n) + reg * 0.5 * sum
of squares of U[u], T, V[l], V[p], V[n], b[p], b[n], T once per batch, TransRec.py:125-135), same dense Adam.  One
training step is ``skr_transrec_step`` (two launches: the fused triple step, then T's gradient summed over the batch in
a fixed order) and the Adam update of the flat [U | V | b | T] buffer (skrec/recommender/_seq.py).
"""
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import ModelConfig
from ..utils.torch import get_initializer
from ._seq import SeqPairwiseRecommender

__all__ = ["TransRec", "TransRecConfig"]


class TransRecConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=0.0, embed_size=64, batch_size=1024, epochs=500, early_stop=100, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_size: int = embed_size
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_size, int) and self.embed_size > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def _init_tables(num_users, num_items, dim):
    """CPU-side construction in the reference's order (_TransRec.__init__ / reset_parameters, TransRec.py:57-73)"""
    ue, ie = nn.Embedding(num_users, dim), nn.Embedding(num_items, dim)
    T = torch.empty(1, dim)                          # Parameter(torch.Tensor(1, d)): no draw
    be = nn.Embedding(num_items, 1)
    get_initializer("zeros")(ue.weight)
    get_initializer("normal")(T)
    get_initializer("normal")(ie.weight)
    get_initializer("zeros")(be.weight)
    return ue.weight.detach(), ie.weight.detach(), be.weight.detach().reshape(-1), T


class TransRec(SeqPairwiseRecommender):
    config_class = TransRecConfig

    def _build(self, last_items=None):
        super()._build(last_items)
        from ._sparse import pad_columns, padded_width
        nu, ni, e = self.num_users, self.num_items, self.config.embed_size
        self.dp = d = padded_width(e)
        U, V, b, T = _init_tables(nu, ni, e)
        nb = 64 * ((ni + 63) // 64)                   # the biases, zero-padded to whole 64-float blocks
        # one flat buffer [U | V | b | T], T in a 64-aligned block of its own
        flat = torch.cat([pad_columns(U, d).reshape(-1), pad_columns(V, d).reshape(-1),
                          nn.functional.pad(b, (0, nb - ni)), pad_columns(T, d).reshape(-1)])
        self._setup(flat.to(self.device).contiguous())
        self._off = (0, nu * d, (nu + ni) * d, (nu + ni) * d + nb)
        o = self._off
        self._user_rows = self._flat[o[0]:o[1]].view(nu, d)
        self._item_rows = self._flat[o[1]:o[2]].view(ni, d)
        self._bias = self._flat[o[2]:o[2] + ni]
        self._T = self._flat[o[3]:o[3] + d]
        g = self.optimizer
        gU, gV, gb, gT = g.grad_view(o[0], (nu, d)), g.grad_view(o[1], (ni, d)), g.grad_view(o[2], (ni,)), g.grad_view(o[3], (d,))
        # the reference's parameters (their first embed_size columns)
        self.user_embeddings, self.item_embeddings = self._user_rows[:, :e], self._item_rows[:, :e]
        self.item_biases, self.global_transition = self._bias, self._T[:e].view(1, e)
        self._work = torch.empty(_hip.SKR_TRANSREC_MAX_BLOCKS * d, dtype=torch.float32, device=self.device)
        L = _hip.lib()
        pt = [t.data_ptr() for t in (self._user_rows, self._item_rows, self._bias, self._T)]
        pg = [t.data_ptr() for t in (gU, gV, gb, gT)]
        pw, reg = self._work.data_ptr(), self.config.reg

        def step(pu, pl, pp, pn, n, ploss, st):
            return L.skr_transrec_step(*pt, pu, pl, pp, pn, n, nu, ni, d, reg, *pg, pw, ploss, _hip.SKR_LOSS_SLOTS, st)
        self._step_launch = step

    def _block_id_parts(self, u, l, p, n):
        # 64-float blocks of U[u], V[l], V[p], V[n] and of the bias words b[p], b[n]
        b = [o // 64 for o in self._off]
        return [u + b[0], l + b[1], p + b[1], n + b[1], (p >> 6) + b[2], (n >> 6) + b[2]]

    def _block_ids_per_step(self):
        return [self._off[3] // 64]                   # T's block: every batch

    def _score_launch(self, d_users, B, out, ld):
        return _hip.lib().skr_seq_scores(_hip.SKR_SEQ_TRANSREC, _hip.ptr(self._user_rows), _hip.ptr(self._item_rows),
                                         _hip.ptr(self._item_rows), None, _hip.ptr(self._T), _hip.ptr(self._bias),
                                         _hip.ptr(d_users), B, _hip.ptr(self._last), self.num_users, self.num_items,
                                         self.dp, _hip.ptr(out), ld, _hip.stream())
