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
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..io import PairwiseIterator
from ..run_config import RunConfig
from ..utils.py import EarlyStopping, ModelConfig
from .base import AbstractRecommender, DenseAdam, on_compute_stream
from .LightGCL import DeviceCSR, normalized_adjacency  # noqa: F401

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


def _run_plan(mat, X, Y=None, accum=None, accum_base=None, accum_scale=1.0):
    ep = _hip.SpmmEpilogue()
    ep.mode = _hip.EPI_PLAIN
    ep.Y, ep.accum, ep.accum_base = _hip.ptr(Y), _hip.ptr(accum), _hip.ptr(accum_base)
    ep.accum_scale = accum_scale
    _hip.check(_hip.lib().skr_spmm_plan_run_ex(mat._plan_handle(), _hip.ptr(X), 64, ctypes.byref(ep), None, None, _hip.stream()))


class DENS(AbstractRecommender):
    config_class = DENSConfig

    def __init__(self, run_config: RunConfig, model_config: Dict):
        """limits: see ``check_limits``"""
        self.config = DENSConfig(**model_config)
        from ..parallel import init_from_env
        self.dist = init_from_env()
        check_limits(self.config, self.dist.world)
        super().__init__(run_config, self.config)
        self.num_users, self.num_items = self.dataset.num_users, self.dataset.num_items
        self.device = _hip.require_gpu()
        self.sampler_mode = getattr(run_config, "sampler_mode", None)
        csr = self.dataset.train_data.to_csr_matrix().tocsr()
        csr.sum_duplicates()
        csr.sort_indices()
        self._build(csr.indptr, csr.indices)

    @classmethod
    def detached(cls, num_users, num_items, model_config, csr):
        """the model's parameters, training step and scoring without a data set, logger or evaluator (tests, timing tools);
        ``csr``: (rowptr [num_users + 1], items) of the binary train matrix, items ascending inside a row (numpy arrays or
        device tensors)"""
        self = cls.__new__(cls)
        self.config = cls.config_class(**model_config)
        check_limits(self.config)
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.device = _hip.require_gpu()
        self._build(csr[0], csr[1])
        return self

    def _build(self, rowptr, items):
        cfg, dev = self.config, self.device
        nu, ni, d, H = self.num_users, self.num_items, cfg.dim, cfg.context_hops
        N = nu + ni
        if torch.is_tensor(rowptr):
            rp, col = rowptr.to(dev, torch.int64).contiguous(), items.to(dev, torch.int32).contiguous()
        else:
            rp = torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).to(dev)
            col = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32)).to(dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t = normalized_adjacency(rp, col, nu, ni)
        gates, eu, ei = init_parameters(nu, ni, d)
        flat = torch.zeros(N * 64 + 4 * GATE_FLOATS, dtype=torch.float32)
        rows = flat[:N * 64].view(N, 64)
        rows[:nu, :d], rows[nu:, :d] = eu, ei
        for k, name in enumerate(GATES):
            blk = flat[N * 64 + k * GATE_FLOATS:N * 64 + (k + 1) * GATE_FLOATS]
            blk[:4096].view(64, 64)[:d, :d] = gates[name][0]
            blk[4096:4096 + d] = gates[name][1]
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
        blk = flat[N * 64 + k * GATE_FLOATS:N * 64 + (k + 1) * GATE_FLOATS]
        return blk[:4096].view(64, 64)[:d, :d], blk[4096:4096 + d]

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

    def _ids(self, t):
        if torch.is_tensor(t):
            return t.to(self.device, torch.int32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(self.device)

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
        need = int(_hip.lib().skr_dens_workspace(n, H))
        if need > self._work.numel():
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        sel_out = torch.empty((n, H + 1), dtype=torch.int32, device=self.device)
        dsel = None
        if sel_in is not None:
            dsel = self._ids(sel_in)
            assert dsel.numel() == n * (H + 1)
        a = _hip.DensStepArgs()
        a.plan_a, a.plan_at = (self.adj._plan_handle(), self.adj_t._plan_handle()) if H > 0 else (None, None)
        a.n_users, a.n_items, a.dim, a.n_hops, a.n_negs, a.n = self.num_users, self.num_items, cfg.dim, H, cfg.n_negs, n
        a.params, a.uids, a.pos, a.cand = _hip.ptr(self._flat), _hip.ptr(du), _hip.ptr(dp), _hip.ptr(dc)
        a.sel_in, a.sel_out = _hip.ptr(dsel), _hip.ptr(sel_out)
        a.w, a.gamma, a.l2 = self.selection_weight(epoch), cfg.gamma, cfg.l2
        for h in range(H):
            a.hop[h] = _hip.ptr(self._hops[h])
        for h in range(len(self._G)):
            a.G[h] = _hip.ptr(self._G[h])
        a.ping, a.grad, a.loss = _hip.ptr(self._ping), _hip.ptr(self._grad), _hip.ptr(loss)
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
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

    @on_compute_stream
    def fit(self):
        cfg = self.config
        data_iter = PairwiseIterator(self.dataset.train_data, num_neg=cfg.K * cfg.n_negs, batch_size=cfg.batch_size, shuffle=True,
                                     drop_last=False, sampler_mode=self.sampler_mode)
        self.logger.info("metrics:".ljust(12) + f"\t{self.evaluator.metrics_str}")
        early_stopping = EarlyStopping(metric="NDCG@10", patience=cfg.early_stop)
        for epoch in range(cfg.epochs):
            self.step_losses = []
            for u, i, j in data_iter.iter_device():
                self.train_step(u, i, j.reshape(-1, cfg.n_negs), epoch)
            result = self.evaluate()
            self.logger.info(f"epoch {epoch}:".ljust(12) + f"\t{result.values_str}")
            if early_stopping(result):
                self.logger.info("early stop")
                break
        self.logger.info("best:".ljust(12) + f"\t{early_stopping.best_result.values_str}")
        return early_stopping.best_result

    # ---- ranking ---------------------------------------------------------------------------------
    def propagate(self):
        """the forward propagation of the CURRENT parameters and the hop means (DENS.py:304-309): pooled = mean_h X_h"""
        nu, H = self.num_users, self.config.context_hops
        if H == 0:
            self.pooled.copy_(self.X0)
            return self.pooled
        s = 1.0 / (H + 1)
        X = self.X0
        for h in range(1, H + 1):
            Y = self._hops[h - 1]
            base = self.X0 if h == 1 else None          # pooled = s X_0 + s X_1, then pooled += s X_h
            _run_plan(self.adj, X[nu:], Y=Y[:nu], accum=self.pooled[:nu], accum_base=None if base is None else base[:nu], accum_scale=s)
            _run_plan(self.adj_t, X[:nu], Y=Y[nu:], accum=self.pooled[nu:], accum_base=None if base is None else base[nu:], accum_scale=s)
            X = Y
        return self.pooled

    @on_compute_stream
    def evaluate(self, test_users=None):
        self.propagate()
        self._pooled_current = True
        try:
            return self.evaluator.evaluate(self, test_users)
        finally:
            self._pooled_current = False

    def predict_factors(self):
        """(user table [U, 64], item table [I, 64], None): the hop means of the current parameters"""
        if not getattr(self, "_pooled_current", False):
            self.propagate()
        return self.pooled[:self.num_users], self.pooled[self.num_users:], None

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores (DENS.py:469-472)"""
        uf, vf, _ = self.predict_factors()
        return _hip.score_matrix(uf, list(users), vf, None).cpu().numpy()
