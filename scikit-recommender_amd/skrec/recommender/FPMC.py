"""FPMC on MI355X (reference: skrec/recommender/FPMC.py).

Paper: Factorizing Personalized Markov Chains for Next-Basket Recommendation (Rendle et al.).
Same config, same initialisation (four nn.Embedding constructors, then normal(0, 0.01) on each, drawn on the CPU in the
reference's order, so a given ``--seed`` yields the reference's initial tables), same loss (sum over the batch of
-log sigmoid(y_p - y_n) + reg * 0.5 * sum of squares of the six gathered row sets, FPMC.py:118-128), same dense Adam.
One training step is ``skr_fpmc_step`` (gathers + both scores + loss + gradient scatter fused) and the Adam update of
the flat [UI | IU | IL | LI] buffer (skrec/recommender/_seq.py).
"""
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import ModelConfig
from ..utils.torch import get_initializer
from ._seq import SeqPairwiseRecommender

__all__ = ["FPMC", "FPMCConfig"]


class FPMCConfig(ModelConfig):
    def __init__(self, lr=0.001, reg=0.001, embed_size=64, batch_size=1024, epochs=500, early_stop=100, **kwargs):
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
    """CPU-side construction in the reference's order (_FPMC.__init__ / reset_parameters, FPMC.py:55-69): four
    nn.Embedding constructors UI, IU, IL, LI (each draws N(0,1)), then normal(0, 0.01) on each in that order"""
    tabs = [nn.Embedding(num_users, dim), nn.Embedding(num_items, dim), nn.Embedding(num_items, dim),
            nn.Embedding(num_items, dim)]
    for t in tabs:
        get_initializer("normal")(t.weight)
    return [t.weight.detach() for t in tabs]


class FPMC(SeqPairwiseRecommender):
    config_class = FPMCConfig

    def _build(self, last_items=None):
        super()._build(last_items)
        from ._sparse import pad_columns, padded_width
        nu, ni, e = self.num_users, self.num_items, self.config.embed_size
        self.dp = d = padded_width(e)
        tabs = [pad_columns(t, d) for t in _init_tables(nu, ni, e)]
        # one flat buffer [UI | IU | IL | LI] => one Adam launch per step; the tables are views into it
        self._setup(torch.cat([t.reshape(-1) for t in tabs]).to(self.device).contiguous())
        self._off = (0, nu * d, (nu + ni) * d, (nu + 2 * ni) * d)
        rows = (nu, ni, ni, ni)
        self._rows = [self._flat[o:o + n * d].view(n, d) for o, n in zip(self._off, rows)]
        self._grads = [self.optimizer.grad_view(o, (n, d)) for o, n in zip(self._off, rows)]
        # the reference's tables (their first embed_size columns)
        self.UI_embeddings, self.IU_embeddings, self.IL_embeddings, self.LI_embeddings = (r[:, :e] for r in self._rows)
        L = _hip.lib()
        p_tab, p_grad = [r.data_ptr() for r in self._rows], [g.data_ptr() for g in self._grads]
        reg = self.config.reg

        def step(pu, pl, pp, pn, n, ploss, st):
            return L.skr_fpmc_step(*p_tab, pu, pl, pp, pn, n, nu, ni, d, reg, *p_grad, ploss, _hip.SKR_LOSS_SLOTS, st)
        self._step_launch = step

    def _block_id_parts(self, u, l, p, n):
        # 64-float blocks (= rows at width 64) of UI[u], IU[p], IU[n], IL[p], IL[n], LI[l]
        b = [o // 64 for o in self._off]
        return [u + b[0], p + b[1], n + b[1], p + b[2], n + b[2], l + b[3]]

    def _score_launch(self, d_users, B, out, ld):
        UI, IU, IL, LI = self._rows
        return _hip.lib().skr_seq_scores(_hip.SKR_SEQ_FPMC, _hip.ptr(UI), _hip.ptr(LI), _hip.ptr(IU), _hip.ptr(IL), None,
                                         None, _hip.ptr(d_users), B, _hip.ptr(self._last), self.num_users, self.num_items,
                                         self.dp, _hip.ptr(out), ld, _hip.stream())
