"""LightGCN on MI355X (reference: skrec/recommender/LightGCN.py).

Paper: LightGCN: Simplifying and Powering Graph Convolution Network for Recommendation (He et al.).
Reference semantics are kept: the full-graph K-layer propagation runs forward AND backward on every
mini-batch (LightGCN.py:89-100, :180-199), the BPR loss is a mean, the L2 term uses the ego rows and
is divided by the CONFIGURED batch size (:191-196), Adam is dense.  Each propagation is
``skr_csr_spmm`` (CSR, one wavefront per 512 non-zeros, 64 lanes = 64 dims) with the layer mean
fused into its epilogue; the backward pass reuses the same kernel because the normalised adjacency
of every ``adj_type`` used here is applied as A^T = A for 'pre'/'plain' and explicitly transposed
otherwise.
"""
import os
from typing import Dict

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from .. import _hip
from ..run_config import RunConfig
from ..utils.common import make_sure_dirs, normalize_adj_matrix
from ..utils.py import ModelConfig
from ..utils.torch import get_initializer
from ._fullgraph import FullGraphBPR
from ._sparse import DeviceCSR, pad_columns, padded_width  # noqa: F401  (padded_width: the name other modules import from here)

__all__ = ["LightGCN", "LightGCNConfig", "DeviceCSR"]


class LightGCNConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=1e-3, embed_size=64, n_layers=3, adj_type="pre", batch_size=1024, epochs=1000,
                 early_stop=100, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_size: int = embed_size
        self.n_layers: int = n_layers
        self.adj_type: str = adj_type  # plain, norm, gcmc, pre
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_size, int) and self.embed_size > 0
        assert isinstance(self.n_layers, int) and self.n_layers > 0
        assert self.adj_type in {"plain", "norm", "gcmc", "pre"}
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def build_adjacency(users_np, items_np, num_users, num_items, adj_type):
    """LightGCN._create_adj_mat (LightGCN.py:142-169)"""
    n_nodes = num_users + num_items
    ones = np.ones_like(users_np, dtype=np.float32)
    upper = sp.csr_matrix((ones, (users_np, items_np + num_users)), shape=(n_nodes, n_nodes))
    adj = upper + upper.T
    if adj_type == "plain":
        return adj
    if adj_type == "norm":
        return normalize_adj_matrix(adj + sp.eye(adj.shape[0]), norm_method="left")
    if adj_type == "gcmc":
        return normalize_adj_matrix(adj, norm_method="left")
    if adj_type == "pre":
        return normalize_adj_matrix(adj, norm_method="symmetric")
    mean_adj = normalize_adj_matrix(adj, norm_method="left")
    return mean_adj + sp.eye(mean_adj.shape[0])


def build_adjacency_device(users, items, num_users, num_items, adj_type, dev):
    """The same matrices as ``build_adjacency`` without the host: (adj, adj_transposed) as DeviceCSR, built
    from the train pairs with device sorts.  Used for large graphs, where scipy needs about a minute for 10^8
    non-zeros; values agree with the scipy build to 1 ulp (numpy's and the device's pow differ in the last bit)."""
    n = num_users + num_items
    u = torch.as_tensor(users, dtype=torch.int64).to(dev)
    i = torch.as_tensor(items, dtype=torch.int64).to(dev) + num_users
    key, counts = torch.unique(torch.cat([u * n + i, i * n + u]), return_counts=True)   # duplicate pairs sum (csr_matrix)
    rows, cols, vals = torch.div(key, n, rounding_mode="floor"), key % n, counts.float()
    eye = torch.arange(n, dtype=torch.int64, device=dev)

    def with_identity(r, c, v):
        k = torch.cat([r * n + c, eye * n + eye])
        v = torch.cat([v, torch.ones(n, dtype=torch.float32, device=dev)])
        k, inv = torch.unique(k, return_inverse=True)
        return torch.div(k, n, rounding_mode="floor"), k % n, torch.zeros(k.numel(), device=dev).index_add_(0, inv, v)

    def inv_pow(deg, p):
        s = deg.pow(p)
        return torch.where(torch.isinf(s), torch.zeros_like(s), s)

    if adj_type == "norm":
        rows, cols, vals = with_identity(rows, cols, vals)
    deg = torch.zeros(n, dtype=torch.float32, device=dev).index_add_(0, rows, vals)
    if adj_type == "pre":
        s_ = inv_pow(deg, -0.5)
        vals = (s_[rows] * vals) * s_[cols]
    elif adj_type != "plain":
        vals = inv_pow(deg, -1.0)[rows] * vals
        if adj_type not in ("norm", "gcmc"):
            rows, cols, vals = with_identity(rows, cols, vals)
    adj = DeviceCSR.from_coo(rows, cols, vals, n)
    adj_t = adj if adj_type in ("pre", "plain") else DeviceCSR.from_coo(cols, rows, vals, n)
    return adj, adj_t


# graphs with at least this many train pairs are built on the device (no scipy pass, no .npz cache file)
DEVICE_ADJ_MIN_PAIRS = 1 << 21


class LightGCN(FullGraphBPR):
    width_field = "embed_size"

    def __init__(self, run_config: RunConfig, model_config: Dict):
        self.config = LightGCNConfig(**model_config)
        self._open(run_config)
        cfg = self.config
        self._connect(run_config)
        n_pairs = len(self.dataset.train_data)
        on_device = (not self.dist.active) and n_pairs >= DEVICE_ADJ_MIN_PAIRS
        adj = None if on_device else self._load_adj_mat(cfg.adj_type)
        self._final_is_current = False
        self._refuse_wide_shards()
        if self.dist.active:
            from ..parallel import ShardedLightGCN
            ue, ie = self._draw_tables()
            # narrower embeddings live in zero-padded 64-float rows, as on one GPU (padded_width)
            self.engine = ShardedLightGCN(self.dist, adj, pad_columns(ue, 64), pad_columns(ie, 64), cfg.n_layers, cfg.lr, cfg.reg,
                                          cfg.batch_size, self.device)
            self._full_user_final = None
            return
        if on_device:
            pairs = self.dataset.train_data.to_user_item_pairs()
            self.adj, self.adj_t = build_adjacency_device(pairs[:, 0], pairs[:, 1], self.num_users, self.num_items,
                                                          cfg.adj_type, self.device)
        else:
            self.adj = DeviceCSR(adj, self.device)
            # backward needs A^T; 'pre' and 'plain' are symmetric, 'norm'/'gcmc' are not
            self.adj_t = self.adj if cfg.adj_type in ("pre", "plain") else DeviceCSR(sp.csr_matrix(adj).T, self.device)
        z = self._one_gpu_parameters(*self._draw_tables())      # E0
        self.final = z()          # layer mean, E-bar
        self._x = [z(), z()]      # propagation ping-pong
        self._g_final = z()       # dL/dE-bar, then H = dL/dE-bar / (K+1)
        self._g = [z(), z()]      # backward ping-pong

    def _draw_tables(self):
        """xavier_uniform init in the reference's order (_LightGCN.__init__, LightGCN.py:71-80)"""
        cfg = self.config
        ue, ie = nn.Embedding(self.num_users, cfg.embed_size), nn.Embedding(self.num_items, cfg.embed_size)
        get_initializer("xavier_uniform")(ue.weight)
        get_initializer("xavier_uniform")(ie.weight)
        return ue.weight.detach(), ie.weight.detach()

    def _load_adj_mat(self, adj_type):
        out_dir = os.path.join(self.dataset.data_dir, f"_{self.__class__.__name__}_data")
        make_sure_dirs(out_dir)
        path = os.path.join(out_dir, f"{adj_type}_adj.npz")
        if self.dist.active and self.dist.rank != 0:
            self.dist.barrier()        # rank 0 writes the cache file, the others read it
            return sp.load_npz(path)
        if os.path.exists(path):   # same cache side file as the reference (LightGCN.py:130-140)
            adj = sp.load_npz(path)
        else:
            adj = self._create_adj_mat(adj_type)
            sp.save_npz(path, adj)
        self.dist.barrier()
        return adj

    def _create_adj_mat(self, adj_type):
        pairs = self.dataset.train_data.to_user_item_pairs()
        return build_adjacency(pairs[:, 0], pairs[:, 1], self.num_users, self.num_items, adj_type)

    # propagation -----------------------------------------------------------------------------------
    def propagate(self, last_rows=None):
        """E-bar = mean(E0, A E0, ..., A^K E0)  (_forward_gcn, LightGCN.py:89-100).
        ``last_rows`` (uint8 [N], training only): the rows of E-bar that will be read.  The LAST layer's product is then
        computed for those rows only -- every earlier layer feeds the next one and stays whole -- and E-bar is valid on
        those rows only."""
        K = self.config.n_layers
        scale = 1.0 / (K + 1)
        x = self.ego
        for k in range(K):
            y = self._x[k & 1]
            # the mean's E0 term rides in the first product's row epilogue: E-bar = scale * E0 + scale * A E0, then += per layer
            self.adj.spmm(x, y, accum=self.final, accum_scale=scale, accum_base=self.ego if k == 0 else None,
                          row_mask=last_rows if k == K - 1 else None, accum_mask=last_rows)
            x = y
        return self.final

    def train_step(self, users, pos, neg, loss_slot):
        cfg, nu = self.config, self.num_users
        K = cfg.n_layers
        n = users.numel()
        # the product A x dense is the reference's; what is skipped is arithmetic whose result is never read (rows of the
        # last forward layer outside the batch) or is a sum of zeros (the first backward hop reads dL/dE-bar, which is zero
        # outside the batch's rows).  SKR_LIGHTGCN_DENSE=1 computes everything.
        gF, gE = self._g_final, self._g_ego
        rows = self._step_rows(gF, users, pos, neg)
        self.propagate(last_rows=rows)
        self._final_is_current = False
        # the score part of the gradient is written already divided by K + 1: gF holds H = dL/dE-bar / (K + 1)
        _hip.check(_hip.lib().skr_bpr_step_dim(
            _hip.ptr(self.final[:nu]), _hip.ptr(self.final[nu:]), None, _hip.ptr(self.ego[:nu]), _hip.ptr(self.ego[nu:]),
            _hip.ptr(users), _hip.ptr(pos), _hip.ptr(neg), n, self.dp, 1.0 / n, cfg.reg, 1.0 / cfg.batch_size,
            _hip.ptr(gF[:nu]), _hip.ptr(gF[nu:]), None, _hip.ptr(gE[:nu]), _hip.ptr(gE[nu:]), _hip.ptr(loss_slot), 1,
            None, None, 1.0 / (K + 1), _hip.stream()))
        # backward through the mean and the K propagations: dL/dE0 += sum_k (A^T)^k H
        x = gF
        for k in range(K):
            y = self._g[k & 1]
            last = (k == K - 1)
            self.adj_t.spmm(x, y, addend=gF, accum=gE if last else None, accum_scale=1.0, col_mask=rows if k == 0 else None,
                            addend_mask=rows)
            x = y
        self.optimizer.step()

    def eval(self):
        """recompute and cache the final embeddings (_LightGCN.eval, LightGCN.py:109-111)"""
        if self.engine is not None:
            e = self.engine
            e.propagate()
            self._full_user_final = e.gather_user_rows(e.whole_final()[:e.n_local])    # every rank can rank any user
        else:
            self.propagate()
        self._final_is_current = True

    def _refresh_outputs(self):
        self.eval()

    def predict_factors(self):
        if not self._final_is_current:
            raise ValueError("Please first switch to 'eval' mode.")
        if self.engine is not None:
            return self._full_user_final, self.engine.whole_final()[self.engine.n_local:], None
        return self.final[:self.num_users], self.final[self.num_users:], None

    def predict(self, users):
        uf, vf, _ = self.predict_factors()
        return _hip.score_matrix(uf, users, vf, None).cpu().numpy()
