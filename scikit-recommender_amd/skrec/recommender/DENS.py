"""DENS on MI355X (reference: skrec/recommender/DENS.py).

Paper: Disentangled Negative Sampling for Collaborative Filtering (Lai, Chen, Zhao, Chen and Han, WSDM 2023).
Same config, same initialisation, same loss (DENS.py:196-257, :318-374): H propagations of the normalised bipartite adjacency
with every hop kept, four learned d x d gates that choose, per batch row AND per hop, one of the ``n_negs`` sampled candidates
by the arg-max of a gated score, the BPR term on the hop means, the four gated terms weighted by ``gamma``, and the
regulariser on the hop-0 rows.  One training step is ``skr_dens_step`` (csrc/dens.hip: the plan runs of A and A^T, the
selection kernel with the four gates in LDS and the gate products on the fp32 matrix pipe, the backward through the gates,
the ordered segment adds into one gradient table per hop, the backward chain acc = A-hat acc + G_h through the plans' addend
epilogue) and one dense Adam launch over the flat buffer [U + I, 64] rows | four gate blocks.

The four ``nn.Linear`` are drawn first (user, item, pos, neg gate), then the two embeddings (DENS.py:163-178): a seeded model
starts with the reference's parameters bit for bit.  ``evaluate()`` propagates the CURRENT parameters (DENS.py:304-309) and
ranks the hop means through the fused top-K path.

Limits (NotImplementedError): ns == "dens", pool == "mean", K == 1, no message or edge dropout, dim <= 64,
context_hops <= 3, n_negs <= 16, batch_size <= 2048, one GPU.  warmup == 0 is a ValueError (the reference divides by zero).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..io import PairwiseIterator
from ..utils.py import ModelConfig
from ._graph import GraphRecommender, linear_block, normalized_adjacency, propagate_mean, upload_csr
from .base import DenseAdam, on_compute_stream

__all__ = ["DENS", "DENSConfig"]

MAX_BATCH, MAX_NEGS, MAX_HOPS = _hip.SKR_DENS_MAX_BATCH, _hip.SKR_DENS_MAX_NEGS, _hip.SKR_DENS_MAX_HOPS
GATE_FLOATS = _hip.SKR_DENS_GATE_FLOATS
GATES = ("user_gate", "item_gate", "pos_gate", "neg_gate")   # the order of the blocks in the flat buffer


class DENSConfig(ModelConfig):
    def __init__(self, lr=1e-3, l2=1e-4, gamma=0.3, dim=64, batch_size=2048, context_hops=3, K=1, n_negs=6, ns="dens",
                 pool="mean", warmup=100, mess_dropout=False, mess_dropout_rate=0.1, edge_dropout=False, edge_dropout_rate=0.1,
                 alpha=1.0, epochs=1000, early_stop=100, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.l2: float = l2
        self.gamma: float = gamma   # weight of the gated terms
        self.dim: int = dim
        self.batch_size: int = batch_size
        self.context_hops: int = context_hops
        self.K: int = K
        self.n_negs: int = n_negs   # candidates per positive
        self.ns: str = ns
        self.pool: str = pool
        self.warmup: int = warmup
        self.mess_dropout: bool = mess_dropout
        self.mess_dropout_rate: float = mess_dropout_rate
        self.edge_dropout: bool = edge_dropout
        self.edge_dropout_rate: float = edge_dropout_rate
        self.alpha: float = alpha
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.l2, float) and self.l2 >= 0
        assert isinstance(self.gamma, float) and self.gamma >= 0
        assert isinstance(self.dim, int) and self.dim > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.context_hops, int) and self.context_hops >= 0
        assert isinstance(self.K, int) and self.K > 0
        assert isinstance(self.n_negs, int) and self.n_negs > 0
        assert isinstance(self.ns, str) and self.ns in {"rns", "dns", "dens"}
        assert isinstance(self.warmup, int) and self.warmup >= 0
        assert isinstance(self.mess_dropout, bool)
        assert isinstance(self.mess_dropout_rate, float) and self.mess_dropout_rate >= 0
        assert isinstance(self.edge_dropout, bool)
        assert isinstance(self.edge_dropout_rate, float) and self.edge_dropout_rate >= 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config, world=1):
    """raises NotImplementedError, naming the limit, for a config this implementation does not run; ValueError for warmup == 0"""
    if config.ns != "dens":
        raise NotImplementedError(f"DENS: ns == 'dens' (got {config.ns!r}): the rns and dns samplers are not implemented")
    if config.pool != "mean":
        raise NotImplementedError(f"DENS: pool == 'mean' (got {config.pool!r}): the fused step pools the hops by their mean")
    if config.K != 1:
        raise NotImplementedError(f"DENS: K == 1 (got {config.K}): one chosen negative per positive")
    if config.mess_dropout:
        raise NotImplementedError("DENS: mess_dropout == False: message dropout is not implemented")
    if config.edge_dropout:
        raise NotImplementedError("DENS: edge_dropout == False: edge dropout is not implemented")
    if config.dim > 64:
        raise NotImplementedError(f"DENS: dim <= 64 (got {config.dim}): rows are 64 floats and the gates 64 x 64")
    if config.context_hops > MAX_HOPS:
        raise NotImplementedError(f"DENS: context_hops <= {MAX_HOPS} (got {config.context_hops})")
    if config.n_negs > MAX_NEGS:
        raise NotImplementedError(f"DENS: n_negs <= {MAX_NEGS} (got {config.n_negs})")
    if config.batch_size > MAX_BATCH:
        raise NotImplementedError(f"DENS: batch_size <= {MAX_BATCH} (got {config.batch_size}): skr_dens_step takes {MAX_BATCH} rows")
    if world > 1:
        raise NotImplementedError("DENS runs on one GPU (one rank): there is no sharded engine for it")
    if config.warmup == 0:
        raise ValueError("DENS: warmup must be positive: the selection weight is 1 - min(1, epoch / warmup)")


def init_parameters(num_users, num_items, d):
    """CPU-side draws in the reference's order (DENS.py:163-178): the four Linears, then xavier-uniform user_embed and
    item_embed -> ({gate: (W [d, d], b [d])}, user_embed, item_embed)"""
    gates = {}
    for name in GATES:
        lin = nn.Linear(d, d)
        gates[name] = (lin.weight.detach().clone(), lin.bias.detach().clone())
    eu = nn.init.xavier_uniform_(torch.empty(num_users, d))
    ei = nn.init.xavier_uniform_(torch.empty(num_items, d))
    return gates, eu, ei


class DENS(GraphRecommender):
    """limits: see ``check_limits``"""
    config_class = DENSConfig

    def _check_limits(self, world):
        check_limits(self.config, world)

    def _build(self, rowptr, items):
        cfg, dev = self.config, self.device
        nu, ni, d, H = self.num_users, self.num_items, cfg.dim, cfg.context_hops
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t = normalized_adjacency(rp, col, nu, ni)
        gates, eu, ei = init_parameters(nu, ni, d)
        flat = torch.zeros(N * 64 + 4 * GATE_FLOATS, dtype=torch.float32)
        rows = flat[:N * 64].view(N, 64)
        rows[:nu, :d], rows[nu:, :d] = eu, ei
        for name in GATES:
            W, b = self._gate_view(flat, name)
            W[:], b[:] = gates[name]
        self._flat = flat.to(dev).contiguous()
        self.X0 = self._flat[:N * 64].view(N, 64)
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)         # Adam(weight_decay=0), DENS.py:432
        self._grad = self.optimizer.grad
        z = lambda: torch.zeros((N, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self._hops = [z() for _ in range(H)]                      # X_1 .. X_H
        self._G = [z() for _ in range(H + 1)] if H > 0 else []
        self._ping = z() if H > 1 else None
        self.pooled = z()                                         # the hop means of the last propagate()
        self._work = torch.empty(int(_hip.lib().skr_dens_workspace(min(cfg.batch_size, MAX_BATCH), H)), dtype=torch.uint8, device=dev)
        self.step_losses = []          # (mf, emb, total) per training step, device tensors [3]

    def _gate_view(self, flat, name):
        k, N, d = GATES.index(name), self.num_users + self.num_items, self.config.dim
        return linear_block(flat[N * 64 + k * GATE_FLOATS:N * 64 + (k + 1) * GATE_FLOATS], d)

    def parameters(self):
        """{name: tensor} in the reference's shapes (copies): the four gates' weight and bias, user_embed, item_embed"""
        return self._named(self._flat)

    def gradients(self):
        """the gradient buffer in the shapes of ``parameters()`` (copies)"""
        return self._named(self._grad)

    def _named(self, flat):
        d, nu, N = self.config.dim, self.num_users, self.num_users + self.num_items
        out = {}
        for name in GATES:
            W, b = self._gate_view(flat, name)
            out[name + ".weight"], out[name + ".bias"] = W.contiguous(), b.contiguous()
        rows = flat[:N * 64].view(N, 64)
        out["user_embed"], out["item_embed"] = rows[:nu, :d].contiguous(), rows[nu:, :d].contiguous()
        return out

    def load_parameters(self, named):
        """sets the parameters from a dict in the shapes of ``parameters()`` (padding stays zero)"""
        d, nu, N = self.config.dim, self.num_users, self.num_users + self.num_items
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.device)    # noqa: E731
        rows = self._flat[:N * 64].view(N, 64)
        rows[:nu, :d], rows[nu:, :d] = t(named["user_embed"]), t(named["item_embed"])
        for name in GATES:
            W, b = self._gate_view(self._flat, name)
            W.copy_(t(named[name + ".weight"]))
            b.copy_(t(named[name + ".bias"]))

    # ---- training --------------------------------------------------------------------------------
    def selection_weight(self, epoch):
        """1 - min(1, epoch / warmup) (DENS.py:247)"""
        return 1.0 - min(1.0, epoch / self.config.warmup)

    def _step_args(self, du, dp, dc, dsel, sel_out, loss, epoch):
        cfg, H = self.config, self.config.context_hops
        a = _hip.DensStepArgs()
        a.plan_a, a.plan_at = (self.adj._plan_handle(), self.adj_t._plan_handle()) if H > 0 else (None, None)
        a.n_users, a.n_items, a.dim, a.n_hops, a.n_negs, a.n = self.num_users, self.num_items, cfg.dim, H, cfg.n_negs, int(du.numel())
        a.params, a.uids, a.pos, a.cand = _hip.ptr(self._flat), _hip.ptr(du), _hip.ptr(dp), _hip.ptr(dc)
        a.sel_in, a.sel_out = _hip.ptr(dsel), _hip.ptr(sel_out)
        a.w, a.gamma, a.l2 = self.selection_weight(epoch), cfg.gamma, cfg.l2
        for h in range(H):
            a.hop[h] = _hip.ptr(self._hops[h])
        for h in range(len(self._G)):
            a.G[h] = _hip.ptr(self._G[h])
        a.ping, a.grad, a.loss = _hip.ptr(self._ping), _hip.ptr(self._grad), _hip.ptr(loss)
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
        return a

    def gradient_step(self, users, pos, cand, epoch, sel_in=None, h_ms=None):
        """forward and backward of one batch without the optimiser: the gradient is left in the optimiser's gradient buffer
        -> (device tensor (mf, emb, total), device int32 [n, H + 1] of the chosen candidate index per row and hop).
        ``cand`` [n, n_negs]; ``sel_in`` [n, H + 1]: entries >= 0 force the choice, -1 leaves it to the kernel;
        ``h_ms``: a ctypes float array of SKR_DENS_GROUPS entries that receives the milliseconds of each launch group"""
        cfg = self.config
        du, dp, dc = self._ids(users), self._ids(pos), self._ids(cand)
        n, H = int(du.numel()), cfg.context_hops
        if n > MAX_BATCH:
            raise NotImplementedError(f"DENS: a batch holds at most {MAX_BATCH} rows (got {n})")
        assert dp.numel() == n and dc.numel() == n * cfg.n_negs
        loss = torch.zeros(3, dtype=torch.float32, device=self.device)
        sel_out = torch.empty((n, H + 1), dtype=torch.int32, device=self.device)
        if n == 0:                     # skr_dens_step launches nothing for an empty batch: a zero loss, a zero gradient
            self._grad.zero_()
            return loss, sel_out
        self._grow_work(int(_hip.lib().skr_dens_workspace(n, H)))
        dsel = None
        if sel_in is not None:
            dsel = self._ids(sel_in)
            assert dsel.numel() == n * (H + 1)
        a = self._step_args(du, dp, dc, dsel, sel_out, loss, epoch)
        if h_ms is None:
            _hip.check(_hip.lib().skr_dens_step(ctypes.byref(a), _hip.stream()))
        else:
            _hip.check(_hip.lib().skr_dens_step_timed(ctypes.byref(a), _hip.stream(), h_ms))
        return loss, sel_out

    @on_compute_stream
    def train_step(self, users, pos, cand, epoch, sel_in=None):
        """one step on (users [n], pos [n], cand [n, n_negs]) at ``epoch`` (sequences or int32 device tensors) -> device
        tensor of the loss components (mf, emb, their sum)"""
        loss, self.last_selection = self.gradient_step(users, pos, cand, epoch, sel_in=sel_in)
        self.optimizer.step()
        self.step_losses.append(loss)
        return loss

    def _make_iterator(self):
        cfg = self.config
        return PairwiseIterator(self.dataset.train_data, num_neg=cfg.K * cfg.n_negs, batch_size=cfg.batch_size, shuffle=True,
                                drop_last=False, sampler_mode=self.sampler_mode)

    def _batches(self, data_iter, epoch):
        for u, i, j in data_iter.iter_device():
            yield u, i, j.reshape(-1, self.config.n_negs), epoch

    # ---- ranking: the base class's, on the hop means (DENS.py:469-472) ------------------------------
    def propagate(self):
        """the forward propagation of the CURRENT parameters and the hop means (DENS.py:304-309): pooled = mean_h X_h"""
        return propagate_mean(self.adj, self.adj_t, self.X0, self.num_users, self.config.context_hops, self.pooled, hops=self._hops)
