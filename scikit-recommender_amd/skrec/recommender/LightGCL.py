"""LightGCL on MI355X (reference: skrec/recommender/LightGCL.py).

Paper: LightGCL: Simple Yet Effective Graph Contrastive Learning for Recommendation (Cai, Huang, Xia and Ren, ICLR 2023).
Same config, same initialisation, same loss (LightGCL.py:139-169): the InfoNCE term between the SVD view G and the
propagated sums E over ALL users and ALL items, the clamped positive scores, BPR on the sums, and lambda2 |E_0|^2, whose
gradient 2 lambda2 E_0 is ``weight_decay = 2 * lambda2`` of the dense Adam.  One training step is ``skr_lightgcl_step``
(csrc/lightgcl.hip: 4L plan runs of A and A^T, the folded low-rank view, the two-pass online log-sum-exp on the fp32 matrix
pipe with no [B, U] or [2B, I] array, the batch kernel) and one dense Adam launch over the flat [U + I, 64] buffer.

Two behaviours of the reference are kept.  ``evaluate()`` ranks with the sums E_u, E_i left by the LAST TRAINING FORWARD --
computed from the parameters before that step's update (LightGCL.py:110, :136-137); before any training step it runs one
forward propagation (the reference would fail there).  And ``torch.svd_lowrank`` draws one ``torch.randn(min(U, I), q)`` from
the CPU generator before the embeddings are initialised (LightGCL.py:202 runs before :208): the same tensor is drawn at the
same place, so a seeded model has the reference's E_u_0 and E_i_0 bit for bit.

The SVD (LightGCL.py:202-204) is ``torch.svd_lowrank``'s subspace iteration (niter = 2) on the device: the sparse products go
through the SpMM plans of A and A^T, the small QR and SVD through ``torch.linalg``; the interaction matrix never visits the
host.  ``svd_factors=(u_mul_s, v_mul_s, ut, vt)`` injects recorded factors instead (an SVD is only defined up to signs and
its algorithm).

Limits: dropout == 0, d <= 64, svd_q <= 16, batch_size <= 2048 (NotImplementedError), one GPU.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..io import PairwiseIterator
from ..utils.py import ModelConfig
from ._graph import GraphRecommender, _device_csr, normalized_adjacency, run_plan, selfcf_adjacency, upload_csr  # noqa: F401
from .base import DenseAdam, on_compute_stream
from .LightGCN import DeviceCSR  # noqa: F401

__all__ = ["LightGCL", "LightGCLConfig"]

MAX_BATCH = _hip.SKR_LIGHTGCL_MAX_QUERIES // 2
MAX_Q = _hip.SKR_LIGHTGCL_MAX_Q


class LightGCLConfig(ModelConfig):
    def __init__(self, lr=1e-3, lambda1=0.2, d=64, gnn_layer=2, batch_size=2048, svd_q=5, dropout=0.0, temp=0.2, lambda2=1e-7,
                 epochs=500, early_stop=100, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.lambda1: float = lambda1  # weight of cl loss
        self.d: int = d  # embedding size
        self.gnn_layer: int = gnn_layer
        self.batch_size: int = batch_size
        self.svd_q: int = svd_q  # rank
        self.dropout: float = dropout
        self.temp: float = temp  # temperature in cl loss
        self.lambda2: float = lambda2  # l2 reg weight
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.lambda1, float) and self.lambda1 >= 0
        assert isinstance(self.d, int) and self.d > 0
        assert isinstance(self.gnn_layer, int) and self.gnn_layer > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.svd_q, int) and self.svd_q > 0
        assert isinstance(self.dropout, float) and self.dropout >= 0
        assert isinstance(self.temp, float) and self.temp > 0
        assert isinstance(self.lambda2, float) and self.lambda2 >= 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config):
    """raises NotImplementedError, naming the limit, for a config this implementation does not run"""
    if config.dropout > 0:
        raise NotImplementedError(f"LightGCL: dropout == 0 (got {config.dropout}): edge dropout is not implemented")
    if config.d > 64:
        raise NotImplementedError(f"LightGCL: d <= 64 (got {config.d}): rows are 64 floats and the fused kernels take 64 columns")
    if config.svd_q > MAX_Q:
        raise NotImplementedError(f"LightGCL: svd_q <= {MAX_Q} (got {config.svd_q}): a node's factors are one 64-byte row")
    if config.batch_size > MAX_BATCH:
        raise NotImplementedError(f"LightGCL: batch_size <= {MAX_BATCH} (got {config.batch_size}): skr_lightgcl_step takes "
                                  f"{2 * MAX_BATCH} query rows")


def init_tables(num_users, num_items, d, q):
    """CPU-side draws in the reference's order: svd_lowrank's test matrix (LightGCL.py:202, torch transposes a wide matrix, so
    it has min(U, I) rows), then xavier-uniform E_u_0 and E_i_0 (LightGCL.py:76-77) -> (R [min(U, I), q], E_u_0, E_i_0)"""
    R = torch.randn(min(num_users, num_items), q, dtype=torch.float32)
    eu = nn.init.xavier_uniform_(torch.empty(num_users, d))
    ei = nn.init.xavier_uniform_(torch.empty(num_items, d))
    return R, eu, ei


def _times(mat, X):
    """mat @ X for a narrow X [n_cols, q <= 64] through the matrix's plan (64-column rows, zero-padded)"""
    q = X.shape[1]
    Xp = torch.zeros((mat.shape[1], 64), dtype=torch.float32, device=X.device)
    Xp[:, :q] = X
    Y = torch.empty((mat.shape[0], 64), dtype=torch.float32, device=X.device)
    run_plan(mat, Xp, Y=Y)
    return Y[:, :q].contiguous()


def svd_lowrank_device(A, At, R, niter=2):
    """``torch.svd_lowrank(A, q)`` (Halko et al., algorithm 5.1 with ``niter`` subspace iterations) for the sparse A
    [U, I] held as the DeviceCSR pair (A, A^T); ``R``: the [min(U, I), q] test matrix -> (U [U, q], S [q], V [I, q])"""
    wide = A.shape[0] < A.shape[1]
    tall, tall_t = (At, A) if wide else (A, At)
    Q = torch.linalg.qr(_times(tall, R)).Q
    for _ in range(niter):
        Q = torch.linalg.qr(_times(tall_t, Q)).Q
        Q = torch.linalg.qr(_times(tall, Q)).Q
    B = _times(tall_t, Q).t()                                 # Q^T A
    Ub, S, Vh = torch.linalg.svd(B, full_matrices=False)
    Uf, V = Q @ Ub, Vh.t()
    if wide:
        Uf, V = V, Uf
    return Uf.contiguous(), S, V.contiguous()


class LightGCL(GraphRecommender):
    """limits: dropout == 0, d <= 64, svd_q <= 16, batch_size <= 2048 (NotImplementedError), one GPU.
    ``svd_factors`` (constructor and ``detached``): (u_mul_s [U, q], v_mul_s [I, q], ut [q, U], vt [q, I]) used instead of
    the model's own SVD"""
    config_class = LightGCLConfig

    def _check_limits(self, world):
        check_limits(self.config)
        if world > 1:
            raise NotImplementedError("LightGCL runs on one GPU: there is no sharded engine for it")

    def _build(self, rowptr, items, svd_factors=None):
        cfg, dev = self.config, self.device
        nu, ni, d, q = self.num_users, self.num_items, cfg.d, cfg.svd_q
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t = normalized_adjacency(rp, col, nu, ni)
        R, eu, ei = init_tables(nu, ni, d, q)
        flat = torch.zeros((N, 64), dtype=torch.float32)
        flat[:nu, :d], flat[nu:, :d] = eu, ei
        self._flat = flat.to(dev).reshape(-1).contiguous()
        self.E0 = self._flat.view(N, 64)
        # lambda2 * sum |p|^2 over the two parameters (LightGCL.py:162-165) as the optimiser's weight decay
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr, weight_decay=2.0 * cfg.lambda2)
        self._grad = self.optimizer.grad.view(N, 64)
        if svd_factors is None:
            Uf, S, V = svd_lowrank_device(self.adj, self.adj_t, R.to(dev))
            factors = (Uf * S, V * S, Uf.t(), V.t())          # LightGCL.py:203-204, :208
        else:
            factors = tuple(torch.as_tensor(np.asarray(f.cpu() if torch.is_tensor(f) else f), dtype=torch.float32).to(dev)
                            for f in svd_factors)
            assert factors[0].shape == (nu, q) and factors[1].shape == (ni, q) and factors[2].shape == (q, nu) \
                and factors[3].shape == (q, ni), "svd_factors = (u_mul_s [U, q], v_mul_s [I, q], ut [q, U], vt [q, I])"
        self.u_mul_s, self.v_mul_s, self.ut, self.vt = (f.contiguous() for f in factors)

        def table(f):                                         # [N, q] -> the kernels' [N, 16]
            t = torch.zeros((f.shape[0], MAX_Q), dtype=torch.float32, device=dev)
            t[:, :q] = f
            return t
        self._fac = (table(self.u_mul_s), table(self.v_mul_s), table(self.ut.t()), table(self.vt.t()))
        z = lambda: torch.zeros((N, 64), dtype=torch.float32, device=dev)        # noqa: E731
        L = cfg.gnn_layer
        self.sums = z()                                       # E_u | E_i of the last forward
        self._below = z() if L > 1 else None
        self._ping = (z(), z()) if L > 1 else (None, None)
        self._gsum = z()
        self._addend = z() if cfg.lambda1 > 0 else None
        self._work = torch.empty(int(_hip.lib().skr_lightgcl_workspace(min(cfg.batch_size, MAX_BATCH), nu, ni)), dtype=torch.uint8,
                                 device=dev)
        self._sums_current = False
        self.step_losses = []          # (bpr, cl, reg, total) per training step, device tensors [4]

    def parameters(self):
        """(E_u_0 [U, d], E_i_0 [I, d]) in the reference's shapes (copies)"""
        d, nu = self.config.d, self.num_users
        return self.E0[:nu, :d].contiguous(), self.E0[nu:, :d].contiguous()

    # ---- training --------------------------------------------------------------------------------
    def _step_args(self, du, dp, dn, loss):
        cfg = self.config
        a = _hip.LightGCLStepArgs()
        a.plan_a, a.plan_at = self.adj._plan_handle(), self.adj_t._plan_handle()
        a.n_users, a.n_items, a.dim, a.n_layers, a.q, a.n = self.num_users, self.num_items, cfg.d, cfg.gnn_layer, cfg.svd_q, int(du.numel())
        a.E0 = _hip.ptr(self.E0)
        a.fac_us, a.fac_vs, a.fac_ut, a.fac_vt = (_hip.ptr(f) for f in self._fac)
        a.uids, a.pos, a.neg = _hip.ptr(du), _hip.ptr(dp), _hip.ptr(dn)
        a.inv_temp, a.lambda1, a.lambda2 = 1.0 / cfg.temp, cfg.lambda1, cfg.lambda2
        a.sum, a.below = _hip.ptr(self.sums), _hip.ptr(self._below)
        a.ping[0], a.ping[1] = _hip.ptr(self._ping[0]), _hip.ptr(self._ping[1])
        a.gsum, a.addend, a.grad, a.loss = _hip.ptr(self._gsum), _hip.ptr(self._addend), _hip.ptr(self._grad), _hip.ptr(loss)
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
        return a

    def gradient_step(self, uids, pos, neg, h_ms=None):
        """forward and backward of one batch without the optimiser: the gradient of E_0 is left in the optimiser's gradient
        buffer, the sums in ``self.sums`` -> device tensor (bpr, cl, reg, total).  ``h_ms``: a ctypes float array of
        SKR_LIGHTGCL_GROUPS entries that receives the milliseconds of each launch group (synchronises)"""
        du, dp, dn = self._ids(uids), self._ids(pos), self._ids(neg)
        n = int(du.numel())
        if n > MAX_BATCH:
            raise NotImplementedError(f"LightGCL: a batch holds at most {MAX_BATCH} pairs (got {n})")
        assert dp.numel() == n and dn.numel() == n
        loss = torch.zeros(4, dtype=torch.float32, device=self.device)
        if n == 0:                     # skr_lightgcl_step launches nothing for an empty batch: a zero loss, a zero gradient, and
            self._grad.zero_()         # the sums are not those of the current parameters
            return loss
        self._grow_work(int(_hip.lib().skr_lightgcl_workspace(n, self.num_users, self.num_items)))
        a = self._step_args(du, dp, dn, loss)
        if h_ms is None:
            _hip.check(_hip.lib().skr_lightgcl_step(ctypes.byref(a), _hip.stream()))
        else:
            _hip.check(_hip.lib().skr_lightgcl_step_timed(ctypes.byref(a), _hip.stream(), h_ms))
        self._sums_current = True
        return loss

    @on_compute_stream
    def train_step(self, uids, pos, neg):
        """one step on the pairs (uids, pos, neg) (sequences or int32 device tensors) -> device tensor of the loss
        components (bpr, lambda1 * (neg_score - pos_score), lambda2 * |E_0|^2, their sum)"""
        loss = self.gradient_step(uids, pos, neg)
        self.optimizer.step()
        self.step_losses.append(loss)
        return loss

    def _make_iterator(self):
        return PairwiseIterator(self.dataset.train_data, batch_size=self.config.batch_size, shuffle=True, drop_last=False,
                                sampler_mode=self.sampler_mode)

    def _batches(self, data_iter, epoch):
        return data_iter.iter_device()

    # ---- ranking ---------------------------------------------------------------------------------
    def propagate(self):
        """the forward propagation alone: sums = sum_{l=0..L} E^(l) from the CURRENT parameters (LightGCL.py:117-137)"""
        nu, L = self.num_users, self.config.gnn_layer
        X = self.E0
        for l in range(1, L + 1):
            last = l == L
            Y = None if last else self._ping[(l - 1) & 1]
            acc = self.sums if last else self._below
            base = (self.E0 if L == 1 else self._below) if last else (self.E0 if l == 1 else None)
            run_plan(self.adj, X[nu:], Y=None if Y is None else Y[:nu], accum=acc[:nu], accum_base=None if base is None else base[:nu])
            run_plan(self.adj_t, X[:nu], Y=None if Y is None else Y[nu:], accum=acc[nu:], accum_base=None if base is None else base[nu:])
            X = Y
        self._sums_current = True
        return self.sums

    @on_compute_stream
    def evaluate(self, test_users=None):
        return self.evaluator.evaluate(self, test_users)

    def predict_factors(self):
        """(E_u [U, 64], E_i [I, 64], None): the sums of the last training forward (the reference ranks with those,
        LightGCL.py:110); one forward propagation when no step has run yet"""
        if not self._sums_current:
            self.propagate()
        return self.sums[:self.num_users], self.sums[self.num_users:], None
