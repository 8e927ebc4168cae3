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

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import ModelConfig
from ._graph import GraphRecommender, linear_block, propagate_mean, selfcf_adjacency, upload_csr
from .base import DenseAdam, on_compute_stream

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


class SelfCF(GraphRecommender):
    """limits: see ``check_limits``; ``seed`` (``detached``; the run's seed otherwise): the key of the device draws"""
    config_class = SelfCFConfig

    def _check_limits(self, world):
        check_limits(self.config, world)

    def _build_args(self, run_config):
        return {"seed": getattr(run_config, "seed", 0) or 0}

    def _build(self, rowptr, items, seed=0):
        cfg, dev = self.config, self.device
        nu, ni, d, L = self.num_users, self.num_items, cfg.embed_dim, cfg.n_layers
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t, self.perm = selfcf_adjacency(rp, col, nu, ni)
        self.nnz = int(col.numel())
        eu, ei, W, b = init_parameters(nu, ni, d)
        flat = torch.zeros(N * 64 + PRED_FLOATS, dtype=torch.float32)
        rows = flat[:N * 64].view(N, 64)
        rows[:nu, :d], rows[nu:, :d] = eu, ei
        Wv, bv = self._pred_view(flat)
        Wv[:], bv[:] = W, b
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
        self._seed, self._step = int(seed), 0
        self.step_losses = []          # (cosine, reg, total) per training step, device tensors [3]

    def _pred_view(self, flat):
        return linear_block(flat[(self.num_users + self.num_items) * 64:], self.config.embed_dim)

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

    def _step_args(self, du, di, rate, edge_keep, ku, ki, loss):
        cfg, L = self.config, self.config.n_layers
        a = _hip.SelfCFStepArgs()
        if L > 0:
            f = self.edge_keeps(rate, edge_keep)
            a.plan_a, a.plan_at = self.adj._plan_handle(), self.adj_t._plan_handle()
            a.keep_fu, a.keep_fi, a.keep_bu, a.keep_bi = (_hip.ptr(f[k]) for k in range(4))
        a.edge_scale = float(np.float32(1.0 / (1.0 - rate)))
        a.n_users, a.n_items, a.dim, a.n_layers, a.n = self.num_users, self.num_items, cfg.embed_dim, L, int(du.numel())
        a.params, a.users, a.items = _hip.ptr(self._flat), _hip.ptr(du), _hip.ptr(di)
        a.ku, a.ki = _hip.ptr(ku), _hip.ptr(ki)
        a.dropout, a.reg, a.seed, a.step = cfg.dropout, cfg.reg, self._seed, self._step
        a.M, a.G, a.grad, a.loss = _hip.ptr(self.M), _hip.ptr(self._G), _hip.ptr(self._grad), _hip.ptr(loss)
        a.ping[0], a.ping[1] = _hip.ptr(self._ping[0]), _hip.ptr(self._ping[1])
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
        return a

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
        loss = torch.zeros(3, dtype=torch.float32, device=self.device)
        if n == 0:                     # skr_selfcf_step launches nothing for an empty batch: a zero loss, a zero gradient
            self._grad.zero_()
            return loss
        if rate is None:
            rate = np.random.random()
        rate = float(rate)
        assert 0.0 <= rate < 1.0
        self._grow_work(int(_hip.lib().skr_selfcf_workspace(n, L)))
        ku = ki = None
        if target_keep is not None:
            ku, ki = (self._flags(k, (n, 64)) for k in target_keep)
        a = self._step_args(du, di, rate, edge_keep, ku, ki, loss)
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

    # ---- ranking ---------------------------------------------------------------------------------
    def propagate(self):
        """the plain, un-dropped propagation of the CURRENT parameters and the layer means (SelfCF.py:170-187), then the
        query rows, the item bias and the per-user constant of the folded score (``skr_selfcf_queries``) -> pooled"""
        nu = self.num_users
        propagate_mean(self.adj, self.adj_t, self.X0, nu, self.config.n_layers, self.pooled, ping=self._ping)
        _hip.check(_hip.lib().skr_selfcf_queries(_hip.ptr(self._pred), _hip.ptr(self.pooled), nu, self.num_items, _hip.ptr(self._Q),
                                                 _hip.ptr(self._item_bias), _hip.ptr(self._user_const), _hip.stream()))
        return self.pooled

    def _factors(self):
        """(query rows (W + W^T) M_u [U, 64], item table M_i [I, 64], item bias <b, M_i> [I]) of the current parameters"""
        return self._Q, self.pooled[self.num_users:], self._item_bias

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores (SelfCF.py:235-241), the per-user constant <b, M_u> included"""
        uf, vf, bias = self.predict_factors()
        users = list(users)
        scores = _hip.score_matrix(uf, users, vf, bias)
        const = self._user_const[torch.as_tensor(np.asarray(users, dtype=np.int64)).to(self.device)]
        return (scores + const[:, None]).cpu().numpy()
