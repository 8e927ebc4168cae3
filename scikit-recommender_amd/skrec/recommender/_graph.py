"""Shared half of the graph recommenders on the bipartite train matrix (LightGCL, DENS, SelfCF, BM3): the normalised
adjacency pair (A, A^T) built in HBM, the plain run of a SpMM plan, the layer-mean propagation, the ``W | b`` view of a
linear block of the flat parameter buffer, and ``GraphRecommender`` -- the constructor and ``detached`` scaffold, the fit
loop and the ranking half.  A model keeps its config, its limits, its draws, ``_build``, ``gradient_step``, ``train_step``
and what is its own in ``propagate``.
"""
import ctypes

import numpy as np
import torch

from .. import _hip
from ..io import InteractionIterator
from ..utils.py import EarlyStopping
from .base import AbstractRecommender, on_compute_stream
from .LightGCN import DeviceCSR

__all__ = ["GraphRecommender", "normalized_adjacency", "selfcf_adjacency", "train_csr", "upload_csr", "run_plan",
           "propagate_mean", "linear_block"]


# ---- the train matrix and its normalised adjacency --------------------------------------------------
def train_csr(dataset):
    """(indptr, indices) of the canonical binary train matrix: duplicates summed, items ascending inside a row"""
    csr = dataset.train_data.to_csr_matrix().tocsr()
    csr.sum_duplicates()
    csr.sort_indices()
    return csr.indptr, csr.indices


def upload_csr(rowptr, items, device):
    """(rowptr int64, items int32) on ``device`` from numpy arrays or tensors"""
    if torch.is_tensor(rowptr):
        return rowptr.to(device, torch.int64).contiguous(), items.to(device, torch.int32).contiguous()
    return (torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).to(device),
            torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32)).to(device))


def _device_csr(shape, rowptr, col, val):
    """a DeviceCSR around arrays that are already in HBM"""
    m = DeviceCSR.__new__(DeviceCSR)
    m.shape, m.nnz = shape, int(col.numel())
    m.rowptr, m.col, m.val = rowptr.contiguous(), col.contiguous(), val.contiguous()
    if m.nnz == 0:
        m.col = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
        m.val = torch.zeros(1, dtype=torch.float32, device=rowptr.device)
    return m


def _adjacency(rowptr, col, num_users, num_items, value, want_perm):
    """(A, A^T, perm or None) from the binary train CSR in HBM, computed on the device -- no loop over the non-zeros, no
    copy to the host; ``value(rowdeg, coldeg, rows, cols)``: the float32 value of every entry"""
    dev = rowptr.device
    rowdeg = (rowptr[1:] - rowptr[:-1])
    rows = torch.repeat_interleave(torch.arange(num_users, dtype=torch.int64, device=dev), rowdeg)
    cols = col.to(torch.int64)
    coldeg = torch.bincount(cols, minlength=num_items)
    val = value(rowdeg, coldeg, rows, cols)
    A = _device_csr((num_users, num_items), rowptr, col, val)
    order = torch.argsort(cols * num_users + rows)           # the transpose: by column, then by row
    rp_t = torch.zeros(num_items + 1, dtype=torch.int64, device=dev)
    rp_t[1:] = torch.cumsum(coldeg, 0)
    At = _device_csr((num_items, num_users), rp_t, rows[order].to(torch.int32), val[order])
    perm = None
    if want_perm:
        perm = torch.empty(order.numel(), dtype=torch.int32, device=dev)
        perm[order] = torch.arange(order.numel(), dtype=torch.int32, device=dev)
    return A, At, perm


def normalized_adjacency(rowptr, col, num_users, num_items):
    """(A, A^T) as DeviceCSR from the binary train CSR in HBM: values 1 / sqrt(rowdeg * coldeg) (LightGCL.py:185-196)"""
    def value(rowdeg, coldeg, rows, cols):
        return 1.0 / (rowdeg[rows].to(torch.float32) * coldeg[cols].to(torch.float32)).sqrt()
    return _adjacency(rowptr, col, num_users, num_items, value, False)[:2]


def selfcf_adjacency(rowptr, col, num_users, num_items):
    """(A, A^T, perm) from the binary train CSR in HBM with SelfCF's normalisation (SelfCF.py:118-123): the float32 of
    (rowdeg + 1e-7)^-0.5 * (coldeg + 1e-7)^-0.5, powers and product in float64.  ``perm`` (int32 [nnz]): the position in
    A^T's entry order of entry e of A's -- the inverse of the sort that builds the transpose"""
    def value(rowdeg, coldeg, rows, cols):
        du = (rowdeg.to(torch.float64) + 1e-7).pow(-0.5)
        di = (coldeg.to(torch.float64) + 1e-7).pow(-0.5)
        return (du[rows] * di[cols]).to(torch.float32)
    return _adjacency(rowptr, col, num_users, num_items, value, True)


# ---- plan runs ---------------------------------------------------------------------------------------
def run_plan(mat, X, Y=None, addend=None, accum=None, accum_base=None, accum_scale=1.0):
    """one product of ``mat``'s plan with 64-column rows of X and the plain epilogue (skr_spmm_epilogue): Y = mat X
    (+ addend); accum = accum_scale * (accum_base + Y) with a base, accum += accum_scale * Y without"""
    ep = _hip.SpmmEpilogue()
    ep.mode = _hip.EPI_PLAIN
    ep.addend, ep.Y, ep.accum, ep.accum_base = _hip.ptr(addend), _hip.ptr(Y), _hip.ptr(accum), _hip.ptr(accum_base)
    ep.accum_scale = accum_scale
    _hip.check(_hip.lib().skr_spmm_plan_run_ex(mat._plan_handle(), _hip.ptr(X), 64, ctypes.byref(ep), None, None, _hip.stream()))


def propagate_mean(adj, adj_t, X0, num_users, L, pooled, ping=None, hops=None):
    """pooled = mean_{k=0..L} X_k with X_k = A-hat X_(k-1) over the [U + I, 64] tables: pooled = s X_0 + s X_1, then
    pooled += s X_k, s = 1 / (L + 1).  ``hops``: X_k is written to hops[k - 1], the last included; otherwise X_k for
    k < L goes to ping[(k - 1) & 1] and X_L is not stored"""
    nu = num_users
    if L == 0:
        pooled.copy_(X0)
        return pooled
    s = 1.0 / (L + 1)
    X = X0
    for k in range(1, L + 1):
        Y = hops[k - 1] if hops is not None else None if k == L else ping[(k - 1) & 1]
        Yu, Yi = (None, None) if Y is None else (Y[:nu], Y[nu:])
        bu, bi = (X0[:nu], X0[nu:]) if k == 1 else (None, None)
        run_plan(adj, X[nu:], Y=Yu, accum=pooled[:nu], accum_base=bu, accum_scale=s)
        run_plan(adj_t, X[:nu], Y=Yi, accum=pooled[nu:], accum_base=bi, accum_scale=s)
        X = Y
    return pooled


def linear_block(block, d):
    """(W [:d, :d], b [:d]) views of a 4160-float block ``W [64][64] | b [64]`` of a flat buffer"""
    return block[:4096].view(64, 64)[:d, :d], block[4096:4096 + d]


# ---- the recommender ---------------------------------------------------------------------------------
class GraphRecommender(AbstractRecommender):
    """Subclasses name their ``config_class`` and provide ``_check_limits(world)`` (raises for a config that does not run),
    ``_build(rowptr, items, **build_kw)`` (whose keywords and defaults are ``detached``'s), ``gradient_step``,
    ``train_step`` and ``propagate``.  Optional: ``_build_args(run_config)`` (the keywords a data set supplies),
    ``_check_data(**build_kw)`` (limits that need them), ``_make_iterator`` / ``_batches`` (the fit loop's batches) and
    ``_factors`` (what ``propagate`` left for the ranking)."""

    def __init__(self, run_config, model_config, **build_kw):
        """limits: see the model's ``check_limits``; raises before it touches the data set or the GPU"""
        self.config = self.config_class(**model_config)
        from ..parallel import init_from_env
        self.dist = init_from_env()
        self._check_limits(self.dist.world)
        AbstractRecommender.__init__(self, run_config, self.config)
        self.num_users, self.num_items = self.dataset.num_users, self.dataset.num_items
        build_kw = dict(self._build_args(run_config), **build_kw)
        self._check_data(**build_kw)
        self.device = _hip.require_gpu()
        self.sampler_mode = getattr(run_config, "sampler_mode", None)
        rowptr, items = train_csr(self.dataset)
        self._build(rowptr, items, **build_kw)

    @classmethod
    def detached(cls, num_users, num_items, model_config, csr, **build_kw):
        """the model's parameters, training step and scoring without a data set, logger or evaluator (tests, timing tools);
        ``csr``: (rowptr [num_users + 1], items) of the binary train matrix, items ascending inside a row (numpy arrays or
        device tensors); ``build_kw``: the keywords of the model's ``_build``"""
        self = cls.__new__(cls)
        self.config = cls.config_class(**model_config)
        self._check_limits(1)
        self._check_data(**build_kw)
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.device = _hip.require_gpu()
        self._build(csr[0], csr[1], **build_kw)
        return self

    def _build_args(self, run_config):
        return {}

    def _check_data(self, **build_kw):
        pass

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

    def _grow_work(self, need):
        if need > self._work.numel():
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)

    # ---- training --------------------------------------------------------------------------------
    def _make_iterator(self):
        return InteractionIterator(self.dataset.train_data, batch_size=self.config.batch_size, shuffle=True, drop_last=False)

    def _batches(self, data_iter, epoch):
        """the argument tuples of ``train_step`` for one epoch"""
        return data_iter

    @on_compute_stream
    def fit(self):
        data_iter = self._make_iterator()
        self.logger.info("metrics:".ljust(12) + f"\t{self.evaluator.metrics_str}")
        early_stopping = EarlyStopping(metric="NDCG@10", patience=self.config.early_stop)
        for epoch in range(self.config.epochs):
            self.step_losses = []
            for batch in self._batches(data_iter, epoch):
                self.train_step(*batch)
            result = self.evaluate()
            self.logger.info(f"epoch {epoch}:".ljust(12) + f"\t{result.values_str}")
            if early_stopping(result):
                self.logger.info("early stop")
                break
        self.logger.info("best:".ljust(12) + f"\t{early_stopping.best_result.values_str}")
        return early_stopping.best_result

    # ---- ranking ---------------------------------------------------------------------------------
    def _factors(self):
        """(user table [U, 64], item table [I, 64], item bias [I] or None) as the last ``propagate()`` left them"""
        return self.pooled[:self.num_users], self.pooled[self.num_users:], None

    @on_compute_stream
    def evaluate(self, test_users=None):
        self.propagate()
        self._pooled_current = True
        try:
            return self.evaluator.evaluate(self, test_users)
        finally:
            self._pooled_current = False

    def predict_factors(self):
        """``_factors()`` of the current parameters"""
        if not getattr(self, "_pooled_current", False):
            self.propagate()
        return self._factors()

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores"""
        uf, vf, bias = self.predict_factors()
        return _hip.score_matrix(uf, list(users), vf, bias).cpu().numpy()
