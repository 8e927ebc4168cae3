"""Shared half of the two full-graph BPR models (LightGCN, LayerGCN): every mini-batch propagates over the whole
[users ; items] graph forward and backward, on one GPU through tables of the model's own or, one process per GPU, through
a sharded engine (skrec/parallel.py).  ``FullGraphBPR`` holds what does not depend on the propagation: the start of the
constructor, the embedding views, the batch's row marks and the head of a step, the epoch of steps and the evaluation.
A model keeps its config, its adjacency, its draws, its propagation, the body of ``train_step`` and its ``predict``.
"""
import os

import torch

from .. import _hip
from ..io import PairwiseIterator
from .base import AbstractRecommender, DenseAdam, DeviceRecommender, on_compute_stream
from ._sparse import pad_columns, padded_width

__all__ = ["FullGraphBPR"]


class FullGraphBPR(DeviceRecommender):
    """Subclasses name ``width_field`` (the config's name of the embedding width) and provide ``_refresh_outputs()`` (one
    unmasked propagation that leaves what ``predict_factors`` hands out), ``train_step`` and ``predict_factors``.  Their
    constructors run ``_open``, their own checks, ``_connect``, and on one GPU ``_one_gpu_parameters``."""

    width_field = None

    @property
    def _width(self):
        return getattr(self.config, self.width_field)

    # ---- the constructor's common steps, in the order the models run them -----------------------------
    def _open(self, run_config):
        """the data set and the row width of the tables in HBM (zero-padded to a multiple of 64)"""
        AbstractRecommender.__init__(self, run_config, self.config)
        self.num_users, self.num_items = self.dataset.num_users, self.dataset.num_items
        self.dp = padded_width(self._width)

    def _connect(self, run_config):
        """the GPU and the process group: one process per GPU under torchrun (user-sharded rows, skrec/parallel.py); world
        1 otherwise"""
        from ..parallel import init_from_env
        self.device = _hip.require_gpu()
        self.dist = init_from_env()
        self.sampler_mode = getattr(run_config, "sampler_mode", None)
        self.step_losses = None
        self.engine = None
        self._row_mask = None

    def _refuse_wide_shards(self):
        if self.dist.active and self.dp != 64:
            raise NotImplementedError(f"one process per GPU: the sharded engines take {self.width_field} <= 64 (rows of 64 floats)")

    def _one_gpu_parameters(self, user0, item0):
        """E0 = [user0 ; item0] in zero-padded rows, its dense Adam and the gradient view; returns a maker of zeroed
        [N, dp] work tables"""
        N, dp = self.num_users + self.num_items, self.dp
        self.ego = pad_columns(torch.cat([user0, item0], dim=0), dp).to(self.device).contiguous()
        self.optimizer = DenseAdam(self.ego.view(-1), lr=self.config.lr)
        self._g_ego = self.optimizer.grad.view(N, dp)
        return lambda: torch.zeros((N, dp), dtype=torch.float32, device=self.device)

    # ---- views -----------------------------------------------------------------------------------
    @property
    def user_embeddings(self):
        if self.engine is not None:
            return self.engine.gather_user_table()[:, :self._width]
        return self.ego[:self.num_users, :self._width]

    @property
    def item_embeddings(self):
        if self.engine is not None:
            return self.engine.item_rows[:, :self._width]
        return self.ego[self.num_users:, :self._width]

    # ---- training --------------------------------------------------------------------------------
    def _batch_rows(self, users, pos, neg):
        """uint8 [N]: 1 on the rows of [U; V] a batch touches -- the only rows of the propagation's output its loss reads,
        and the only non-zero rows of the gradient with respect to that output (reference: the gathers of
        _LightGCN.forward, LightGCN.py:82-87, and of calculate_loss, LayerGCN.py:245-253)"""
        m, L, st, nu = self._row_mask, _hip.lib(), _hip.stream(), self.num_users
        _hip.check(L.skr_mark_ids(_hip.ptr(users), users.numel(), 0, _hip.ptr(m), st))
        _hip.check(L.skr_mark_ids(_hip.ptr(pos), pos.numel(), nu, _hip.ptr(m), st))
        _hip.check(L.skr_mark_ids(_hip.ptr(neg), neg.numel(), nu, _hip.ptr(m), st))
        return m

    def _step_rows(self, grad, users, pos, neg):
        """The head of a step.  ``grad`` ([N, dp]) is the buffer the BPR kernel scatters the gradient of the propagation's
        output into: it is zero outside the previous batch's rows, so those rows are cleared (and their marks with them)
        instead of filling the whole buffer.  Returns the marks of this batch's rows, or None under SKR_LIGHTGCN_DENSE=1,
        which computes everything."""
        if os.environ.get("SKR_LIGHTGCN_DENSE") == "1":
            grad.zero_()
            self._row_mask = None
            return None
        if self._row_mask is None:
            self._row_mask = torch.zeros(self.num_users + self.num_items, dtype=torch.uint8, device=self.device)
            grad.zero_()
        else:
            _hip.check(_hip.lib().skr_clear_marked_rows(_hip.ptr(self._row_mask), self._row_mask.numel(), 1, _hip.ptr(grad), self.dp,
                                                        _hip.stream()))
        return self._batch_rows(users, pos, neg)

    @on_compute_stream
    def train_epoch(self, data_iter):
        self.step_losses = torch.zeros((len(data_iter), 2), dtype=torch.float32, device=self.device)
        for k, (u, i, j) in enumerate(data_iter.iter_device()):
            if self.engine is not None:      # every rank walks the same global batches and keeps its users
                self.engine.train_step(u, i, j)
                self.step_losses[k] = self.engine.loss
            else:
                self.train_step(u.contiguous(), i.contiguous(), j.contiguous(), self.step_losses[k])

    def _make_iterator(self):
        return PairwiseIterator(self.dataset.train_data, batch_size=self.config.batch_size, shuffle=True,
                                drop_last=False, sampler_mode=self.sampler_mode)

    # ---- ranking ---------------------------------------------------------------------------------
    @on_compute_stream
    def evaluate(self, test_users=None):
        self._refresh_outputs()
        if self.engine is None:
            return self.evaluator.evaluate(self, test_users)
        from ..parallel import sharded_evaluate
        return sharded_evaluate(self.dist, self.evaluator, self, test_users, self.device)
