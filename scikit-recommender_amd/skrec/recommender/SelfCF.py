"""SelfCF on MI355X (reference: skrec/recommender/SelfCF.py).

Paper: SelfCF: A Simple Framework for Self-supervised Collaborative Filtering (Zhou, Sun, Liu, Zhang and Miao, TORS 2023), the
embedding-dropout variant SELFCF_ed on a LightGCN encoder.  Same config, same initialisation, same loss (SelfCF.py:133-168,
:205-233): every step draws a fresh dropout rate and a fresh mask over the 2 nnz entries of the square normalised adjacency,
propagates ``n_layers`` times through the masked, rescaled matrix, takes the mean of the layers at the batch's users and
items, and minimises the negative cosine between the 64 x 64 predictor of one side and a dropped-out, detached copy of the
other, plus ``reg`` times half the squared norms of the batch rows.  There are no negatives.

One training step is ``skr_selfcf_keeps`` (the four keep arrays of the step's plan runs: the masked matrix is not symmetric,
so the backward runs need the two halves of the mask in each other's entry order), ``skr_selfcf_step`` (csrc/selfcf.hip:
2 n_layers dropped plan runs forward -- a dropped entry's row is not gathered --, the batch kernel with the predictor on the
fp32 matrix pipe, the ordered segment add, 2 n_layers dropped runs backward) and one dense Adam launch over the flat buffer
[U + I, 64] rows | W 64 x 64 | b 64 with ``weight_decay = 0``.  The reference's ``LambdaLR`` factor is
``1.0 ** (epoch / 50) = 1``: the learning rate is constant, and no scheduler is kept.

The dropout rate of a step comes from ``np.random.random()``, once per step, as the reference draws it (SelfCF.py:148).  The
edge mask and the two target masks are drawn on the device (``draws = "device"``, the only mode: not a reference option),
keyed by (seed, step): equal to the reference's torch draws in law only.  ``gradient_step(..., rate, edge_keep, target_keep)``
takes recorded values instead and replays a recorded run.

``evaluate()`` propagates the CURRENT parameters through the plain, un-dropped adjacency (SelfCF.py:170-187) and ranks
``(W u + b).i + u.(W i + b) = u^T (W + W^T) i + <b, i> + <b, u>`` through the fused top-K path: query rows
``(W + W^T) M_u``, the item bias ``<b, M_i>``; the per-user constant does not move a ranking and is added in ``predict()``.

Limits (NotImplementedError): embed_dim <= 64, n_layers <= 4, batch_size <= 2048, one GPU.
"""
import ctypes
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..io import InteractionIterator
from ..run_config import RunConfig
from ..utils.py import EarlyStopping, ModelConfig
from .base import AbstractRecommender, DenseAdam, on_compute_stream
from .LightGCL import selfcf_adjacency

__all__ = ["SelfCF", "SelfCFConfig"]

MAX_BATCH, MAX_LAYERS = _hip.SKR_SELFCF_MAX_BATCH, _hip.SKR_SELFCF_MAX_LAYERS
PRED_FLOATS = _hip.SKR_SELFCF_PRED_FLOATS


class SelfCFConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=0.0, embed_dim=64, n_layers=2, dropout=0.5, batch_size=2048, epochs=1000, early_stop=200,
                 draws="device", **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_dim: int = embed_dim
        self.n_layers: int = n_layers
        self.dropout: float = dropout
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop
        # how the edge and target masks are made (not a reference option): "device"
        self.draws: str = draws

    @classmethod
    def param_space(cls):
        return {"n_layers": [2], "reg": [0.0], "dropout": [0.5]}

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_dim, int) and self.embed_dim > 0
        assert isinstance(self.n_layers, int) and self.n_layers >= 0
        assert isinstance(self.dropout, float) and 0 <= self.dropout < 1
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)
        assert self.draws == "device"


def check_limits(config, world=1):
    """raises NotImplementedError, naming the limit, for a config this implementation does not run"""
    if config.embed_dim > 64:
        raise NotImplementedError(f"SelfCF: embed_dim <= 64 (got {config.embed_dim}): rows are 64 floats and the predictor 64 x 64")
    if config.n_layers > MAX_LAYERS:
        raise NotImplementedError(f"SelfCF: n_layers <= {MAX_LAYERS} (got {config.n_layers})")
    if config.batch_size > MAX_BATCH:
        raise NotImplementedError(f"SelfCF: batch_size <= {MAX_BATCH} (got {config.batch_size}): skr_selfcf_step takes {MAX_BATCH} rows")
    if world > 1:
        raise NotImplementedError("SelfCF runs on one GPU (one rank): there is no sharded engine for it")


def init_parameters(num_users, num_items, d):
    """CPU-side draws in the reference's order (SelfCF.py:86-93, :201-202): xavier-uniform user_emb, xavier-uniform item_emb,
    then nn.Linear(d, d) -> (user_emb, item_emb, W [d, d], b [d])"""
    eu = nn.init.xavier_uniform_(torch.empty(num_users, d))
    ei = nn.init.xavier_uniform_(torch.empty(num_items, d))
    lin = nn.Linear(d, d)
    return eu, ei, lin.weight.detach().clone(), lin.bias.detach().clone()


def _epilogue(Y=None, accum=None, accum_base=None, accum_scale=1.0):
    ep = _hip.SpmmEpilogue()
    ep.mode = _hip.EPI_PLAIN
    ep.Y, ep.accum, ep.accum_base = _hip.ptr(Y), _hip.ptr(accum), _hip.ptr(accum_base)
    ep.accum_scale = accum_scale
    return ep


class SelfCF(AbstractRecommender):
    config_class = SelfCFConfig

    def __init__(self, run_config: RunConfig, model_config: Dict):
        """limits: see ``check_limits``"""
        self.config = SelfCFConfig(**model_config)
        from ..parallel import init_from_env
        self.dist = init_from_env()
        check_limits(self.config, self.dist.world)
        super().__init__(run_config, self.config)
        self.num_users, self.num_items = self.dataset.num_users, self.dataset.num_items
        self.device = _hip.require_gpu()
        csr = self.dataset.train_data.to_csr_matrix().tocsr()
        csr.sum_duplicates()
        csr.sort_indices()
        self._build(csr.indptr, csr.indices, int(getattr(run_config, "seed", 0) or 0))

    @classmethod
    def detached(cls, num_users, num_items, model_config, csr, seed=0):
        """the model's parameters, training step and scoring without a data set, logger or evaluator (tests, timing tools);
        ``csr``: (rowptr [num_users + 1], items) of the binary train matrix, items ascending inside a row (numpy arrays or
        device tensors); ``seed``: the key of the device draws"""
        self = cls.__new__(cls)
        self.config = cls.config_class(**model_config)
        check_limits(self.config)
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.device = _hip.require_gpu()
        self._build(csr[0], csr[1], int(seed))
        return self

    def _build(self, rowptr, items, seed):
        cfg, dev = self.config, self.device
        nu, ni, d, L = self.num_users, self.num_items, cfg.embed_dim, cfg.n_layers
        N = nu + ni
        if torch.is_tensor(rowptr):
            rp, col = rowptr.to(dev, torch.int64).contiguous(), items.to(dev, torch.int32).contiguous()
        else:
            rp = torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).to(dev)
            col = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32)).to(dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t, self.perm = selfcf_adjacency(rp, col, nu, ni)
        self.nnz = int(col.numel())
        eu, ei, W, b = init_parameters(nu, ni, d)
        flat = torch.zeros(N * 64 + PRED_FLOATS, dtype=torch.float32)
        rows = flat[:N * 64].view(N, 64)
        rows[:nu, :d], rows[nu:, :d] = eu, ei
        flat[N * 64:N * 64 + 4096].view(64, 64)[:d, :d] = W
        flat[N * 64 + 4096:N * 64 + 4096 + d] = b
        self._flat = flat.to(dev).contiguous()
        self.X0 = self._flat[:N * 64].view(N, 64)
        self._pred = self._flat[N * 64:]
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)         # Adam(weight_decay=0), a constant learning rate (SelfCF.py:252-255)
        self._grad = self.optimizer.grad
        z = lambda: torch.zeros((N, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self.M = z()                                              # the layer means of the last step's masked forward
        self.pooled = z()                                         # the layer means of the last propagate() (un-dropped)
        self._ping = (z(), z()) if L > 1 else (None, None)
        self._G = z() if L > 0 else None
        nk = max(self.nnz, 1)
        self._keeps = torch.zeros((4, nk), dtype=torch.uint8, device=dev)         # fu, fi, bu, bi
        self._Q = torch.zeros((nu, 64), dtype=torch.float32, device=dev)
        self._item_bias = torch.zeros(ni, dtype=torch.float32, device=dev)
        self._user_const = torch.zeros(nu, dtype=torch.float32, device=dev)
        self._work = torch.empty(int(_hip.lib().skr_selfcf_workspace(min(cfg.batch_size, MAX_BATCH), L)), dtype=torch.uint8, device=dev)
        self._seed, self._step = seed, 0
        self.step_losses = []          # (cosine, reg, total) per training step, device tensors [3]

    def _pred_view(self, flat):
        N, d = self.num_users + self.num_items, self.config.embed_dim
        blk = flat[N * 64:]
        return blk[:4096].view(64, 64)[:d, :d], blk[4096:4096 + d]

    def parameters(self):
        """{name: tensor} in the reference's shapes (copies): user_emb, item_emb, predictor.weight, predictor.bias"""
        return self._named(self._flat)

    def gradients(self):
        """the gradient buffer in the shapes of ``parameters()`` (copies)"""
        return self._named(self._grad)

    def _named(self, flat):
        d, nu, N = self.config.embed_dim, self.num_users, self.num_users + self.num_items
        rows = flat[:N * 64].view(N, 64)
        W, b = self._pred_view(flat)
        return {"user_emb": rows[:nu, :d].contiguous(), "item_emb": rows[nu:, :d].contiguous(),
                "predictor.weight": W.contiguous(), "predictor.bias": b.contiguous()}

    def load_parameters(self, named):
        """sets the parameters from a dict in the shapes of ``parameters()`` (padding stays zero)"""
        d, nu, N = self.config.embed_dim, self.num_users, self.num_users + self.num_items
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.device)    # noqa: E731
        rows = self._flat[:N * 64].view(N, 64)
        rows[:nu, :d], rows[nu:, :d] = t(named["user_emb"]), t(named["item_emb"])
        W, b = self._pred_view(self._flat)
        W.copy_(t(named["predictor.weight"]))
        b.copy_(t(named["predictor.bias"]))

    # ---- training --------------------------------------------------------------------------------
    def _ids(self, t):
        if torch.is_tensor(t):
            return t.to(self.device, torch.int32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(self.device)

    def _flags(self, t, shape):
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(t).astype(np.uint8))
        t = t.to(self.device, torch.uint8).contiguous()
        assert tuple(t.shape) == tuple(shape), f"keep flags of shape {tuple(t.shape)}, expected {tuple(shape)}"
        return t

    def edge_keeps(self, rate, edge_keep=None, step=None):
        """the four keep arrays of one step (``skr_selfcf_keeps``) -> uint8 [4, nnz]: forward user rows, forward item rows,
        backward user rows, backward item rows.  ``edge_keep`` = (k1, k2): the user-row half in the train CSR's order and the
        item-row half in the transpose's order; None: drawn on the device at ``rate``, keyed by (seed, step)"""
        k1 = k2 = None
        if edge_keep is not None:
            k1, k2 = (self._flags(k, (self.nnz,)) for k in edge_keep)
        f = self._keeps
        _hip.check(_hip.lib().skr_selfcf_keeps(_hip.ptr(self.perm), self.nnz, _hip.ptr(k1), _hip.ptr(k2), float(rate), self._seed,
                                               self._step if step is None else int(step), _hip.ptr(f[0]), _hip.ptr(f[1]),
                                               _hip.ptr(f[2]), _hip.ptr(f[3]), _hip.stream()))
        return f

    def gradient_step(self, users, items, rate=None, edge_keep=None, target_keep=None, h_ms=None):
        """forward and backward of one batch without the optimiser: the gradient is left in the optimiser's gradient buffer,
        the masked layer means in ``self.M`` -> device tensor (cosine, reg, total).
        ``rate``: the step's edge-dropout rate (None: ``np.random.random()``, SelfCF.py:148); ``edge_keep`` = (k1 [nnz],
        k2 [nnz]) and ``target_keep`` = (ku [n, 64], ki [n, 64]): recorded flags instead of the device draws;
        ``h_ms``: a ctypes float array of SKR_SELFCF_GROUPS entries that receives the milliseconds of each launch group"""
        cfg = self.config
        du, di = self._ids(users), self._ids(items)
        n, L = int(du.numel()), cfg.n_layers
        if n > MAX_BATCH:
            raise NotImplementedError(f"SelfCF: a batch holds at most {MAX_BATCH} rows (got {n})")
        assert di.numel() == n
        if rate is None:
            rate = np.random.random()
        rate = float(rate)
        assert 0.0 <= rate < 1.0
        need = int(_hip.lib().skr_selfcf_workspace(n, L))
        if need > self._work.numel():
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        ku = ki = None
        if target_keep is not None:
            ku, ki = (self._flags(k, (n, 64)) for k in target_keep)
        a = _hip.SelfCFStepArgs()
        if L > 0:
            f = self.edge_keeps(rate, edge_keep)
            a.plan_a, a.plan_at = self.adj._plan_handle(), self.adj_t._plan_handle()
            a.keep_fu, a.keep_fi, a.keep_bu, a.keep_bi = (_hip.ptr(f[k]) for k in range(4))
        a.edge_scale = float(np.float32(1.0 / (1.0 - rate)))
        a.n_users, a.n_items, a.dim, a.n_layers, a.n = self.num_users, self.num_items, cfg.embed_dim, L, n
        a.params, a.users, a.items = _hip.ptr(self._flat), _hip.ptr(du), _hip.ptr(di)
        a.ku, a.ki = _hip.ptr(ku), _hip.ptr(ki)
        a.dropout, a.reg, a.seed, a.step = cfg.dropout, cfg.reg, self._seed, self._step
        a.M, a.G, a.grad, a.loss = _hip.ptr(self.M), _hip.ptr(self._G), _hip.ptr(self._grad), _hip.ptr(loss)
        a.ping[0], a.ping[1] = _hip.ptr(self._ping[0]), _hip.ptr(self._ping[1])
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
        if h_ms is None:
            _hip.check(_hip.lib().skr_selfcf_step(ctypes.byref(a), _hip.stream()))
        else:
            _hip.check(_hip.lib().skr_selfcf_step_timed(ctypes.byref(a), _hip.stream(), h_ms))
        self._step += 1
        return loss

    @on_compute_stream
    def train_step(self, users, items, rate=None, edge_keep=None, target_keep=None):
        """one step on the pairs (users [n], items [n]) (sequences or int32 device tensors) -> device tensor of the loss
        components (cosine, reg, their sum)"""
        loss = self.gradient_step(users, items, rate=rate, edge_keep=edge_keep, target_keep=target_keep)
        self.optimizer.step()
        self.step_losses.append(loss)
        return loss

    @on_compute_stream
    def fit(self):
        cfg = self.config
        data_iter = InteractionIterator(self.dataset.train_data, batch_size=cfg.batch_size, shuffle=True, drop_last=False)
        self.logger.info("metrics:".ljust(12) + f"\t{self.evaluator.metrics_str}")
        early_stopping = EarlyStopping(metric="NDCG@10", patience=cfg.early_stop)
        for epoch in range(cfg.epochs):
            self.step_losses = []
            for users, items in data_iter:
                self.train_step(users, items)
            result = self.evaluate()
            self.logger.info(f"epoch {epoch}:".ljust(12) + f"\t{result.values_str}")
            if early_stopping(result):
                self.logger.info("early stop")
                break
        self.logger.info("best:".ljust(12) + f"\t{early_stopping.best_result.values_str}")
        return early_stopping.best_result

    # ---- ranking ---------------------------------------------------------------------------------
    def propagate(self):
        """the plain, un-dropped propagation of the CURRENT parameters and the layer means (SelfCF.py:170-187), then the
        query rows, the item bias and the per-user constant of the folded score (``skr_selfcf_queries``) -> pooled"""
        nu, L = self.num_users, self.config.n_layers
        L_ = _hip.lib()
        if L == 0:
            self.pooled.copy_(self.X0)
        else:
            s = 1.0 / (L + 1)
            X = self.X0
            for k in range(1, L + 1):
                Y = None if k == L else self._ping[(k - 1) & 1]
                base = self.X0 if k == 1 else None          # pooled = s X_0 + s X_1, then pooled += s X_k
                for mat, lo, hi, xs in ((self.adj, 0, nu, X[nu:]), (self.adj_t, nu, None, X[:nu])):
                    ep = _epilogue(Y=None if Y is None else Y[lo:hi], accum=self.pooled[lo:hi],
                                   accum_base=None if base is None else base[lo:hi], accum_scale=s)
                    _hip.check(L_.skr_spmm_plan_run_ex(mat._plan_handle(), _hip.ptr(xs), 64, ctypes.byref(ep), None, None, _hip.stream()))
                X = Y
        _hip.check(L_.skr_selfcf_queries(_hip.ptr(self._pred), _hip.ptr(self.pooled), nu, self.num_items, _hip.ptr(self._Q),
                                         _hip.ptr(self._item_bias), _hip.ptr(self._user_const), _hip.stream()))
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
        """(query rows (W + W^T) M_u [U, 64], item table M_i [I, 64], item bias <b, M_i> [I]) of the current parameters"""
        if not getattr(self, "_pooled_current", False):
            self.propagate()
        return self._Q, self.pooled[self.num_users:], self._item_bias

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores (SelfCF.py:235-241), the per-user constant <b, M_u> included"""
        uf, vf, bias = self.predict_factors()
        users = list(users)
        scores = _hip.score_matrix(uf, users, vf, bias)
        const = self._user_const[torch.as_tensor(np.asarray(users, dtype=np.int64)).to(self.device)]
        return (scores + const[:, None]).cpu().numpy()
