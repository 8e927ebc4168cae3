"""Shared half of the graph recommenders on the bipartite train matrix (LightGCL, DENS, SelfCF, BM3): the normalised
adjacency pair (A, A^T) built in HBM, the plain run of a SpMM plan, the layer-mean propagation, the ``W | b`` view of a
linear block of the flat parameter buffer, and ``GraphRecommender`` -- the epoch of steps and the propagate-then-rank
half on ``DeviceRecommender`` (base.py).  A model keeps its config, its limits, its draws, ``_build``, ``gradient_step``,
``train_step`` and what is its own in ``propagate``.

Which model sits on which base: LightGCL, DENS and SelfCF on ``GraphRecommender`` directly; BM3, FREEDOM, MGCN, LATTICE and
SLMRec on ``MultimodalRecommender`` (_multimodal.py), which adds the feature tables, the modal blocks' layout, the parameter
dictionaries and the frame of the step; LightGCN and LayerGCN on ``FullGraphBPR`` (_fullgraph.py), beside this module.
"""
import numpy as np
import torch

from .. import _hip
from ..io import InteractionIterator
from .base import DeviceRecommender, on_compute_stream
from ._sparse import DeviceCSR

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


_device_csr = DeviceCSR.from_arrays     # (shape, rowptr, col, val): a DeviceCSR around arrays that are already in HBM


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
    (+ addend); accum = accum_scale * (accum_base + Y) with a base, accum += accum_scale * Y without.  Always the plan,
    whatever the matrix's size; the epilogue itself is filled by ``DeviceCSR._run_epilogue``"""
    mat._run_epilogue(_hip.ptr(X), None, None, _hip.EPI_PLAIN, 0, _hip.ptr(addend), _hip.ptr(Y), _hip.ptr(accum), _hip.ptr(accum_base),
                      accum_scale)


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
class GraphRecommender(DeviceRecommender):
    """``DeviceRecommender`` on the train CSR: ``_build(rowptr, items, **build_kw)``; subclasses also provide
    ``gradient_step``, ``train_step`` and ``propagate``.  Optional: ``_make_iterator`` / ``_batches`` (the fit loop's
    batches) and ``_factors`` (what ``propagate`` left for the ranking)."""

    def _train_inputs(self):
        return train_csr(self.dataset)

    def _flags(self, t, shape):
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(t).astype(np.uint8))
        t = t.to(self.device, torch.uint8).contiguous()
        assert tuple(t.shape) == tuple(shape), f"keep flags of shape {tuple(t.shape)}, expected {tuple(shape)}"
        return t

    # ---- training --------------------------------------------------------------------------------
    def _make_iterator(self):
        return InteractionIterator(self.dataset.train_data, batch_size=self.config.batch_size, shuffle=True, drop_last=False)

    def _batches(self, data_iter, epoch):
        """the argument tuples of ``train_step`` for one epoch"""
        return data_iter

    def _run_epoch(self, data_iter, epoch):
        self.step_losses = []
        for batch in self._batches(data_iter, epoch):
            self.train_step(*batch)

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
