"""Shared half of the multimodal recommenders (BM3, FREEDOM, MGCN, LATTICE, SLMRec): the intake of the ``img`` / ``txt`` feature
tables, the limit clauses the five ``check_limits`` have in common, the layout of a modality's two blocks in a flat buffer
(``ModalLayout``), and ``MultimodalRecommender`` -- ``parameters()`` / ``gradients()`` / ``load_parameters()`` over the model's
``_views``, the frame of ``gradient_step`` around the model's args struct, ``train_step``, the pairwise iterator and the
``LambdaLR`` learning rate on ``GraphRecommender`` (_graph.py).  A model keeps its config, its ``check_limits``, its
``init_parameters`` and adjacency, its ``_build``, its ``_views`` outside the modal blocks, ``_step_args``, ``propagate`` and
``_factors``.
"""
import ctypes

import numpy as np
import torch

from .. import _hip
from ..io import PairwiseIterator
from ._graph import GraphRecommender
from .base import on_compute_stream

__all__ = ["MODALITIES", "MultimodalRecommender", "ModalLayout", "features", "feature_dims", "limit_batch", "limit_features",
           "limit_world", "lambda_lr"]

# (key, the reference's prefix): the reference registers the image block first
MODALITIES = (("img", "image"), ("txt", "text"))


# ---- the feature tables ------------------------------------------------------------------------------
def features(a, num_items, model, name, required=False):
    """float32 [num_items, F] tensor of an ``img`` / ``txt`` argument (numpy array or tensor), None for a missing table
    unless the model requires it; ``name``: "image" / "text", for the message"""
    if a is None:
        if required:
            raise ValueError(f"{model}: the {name} feature table is missing -- the model's forward uses both modalities")
        return None
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dim() != 2 or a.shape[0] != num_items:
        raise ValueError(f"{model}: the {name} feature table has shape {tuple(a.shape)}, the data set has {num_items} items")
    return a.to(torch.float32)


def feature_dims(feats):
    """(feat_dim, feat_ld, present) of {"img": table or None, "txt": ...}: the widths F (0: absent), the row strides (F
    rounded up to a multiple of 4) and, in the order of ``MODALITIES``, whether the table is there"""
    feat_dim = {k: 0 if v is None else int(v.shape[1]) for k, v in feats.items()}
    feat_ld = {k: (F + 3) // 4 * 4 for k, F in feat_dim.items()}
    return feat_dim, feat_ld, [bool(feat_dim[key]) for key, _ in MODALITIES]


# ---- the limit clauses the five check_limits share, each called in the model's own order -----------------
def limit_batch(model, config, max_batch):
    if config.batch_size > max_batch:
        raise NotImplementedError(f"{model}: batch_size <= {max_batch} (got {config.batch_size}): skr_{model.lower()}_step takes "
                                  f"{max_batch} rows")


def limit_features(model, max_feat, img_dim, txt_dim):
    for name, F in (("image", img_dim), ("text", txt_dim)):
        if F is not None and not 1 <= F <= max_feat:
            raise NotImplementedError(f"{model}: 1 <= feature width <= {max_feat} (the {name} table has {F} columns)")


def limit_world(model, world):
    if world > 1:
        raise NotImplementedError(f"{model} runs on one GPU (one rank): there is no sharded engine for it")


def lambda_lr(lr, scheduler, epoch):
    """LambdaLR's lr * scheduler[0] ** (epoch / scheduler[1]), the reference's Python-float expression"""
    g, s = scheduler
    return lr * g ** (epoch / s)


# ---- a modality's blocks in a flat buffer ---------------------------------------------------------------
class ModalLayout:
    """Per present modality, image first, from float offset ``start``: the projection block ``W [64, ld] | b [64]`` and, with
    ``tables``, the feature table ``[num_items, ld]`` behind it.  ``off[key] = (projection, table or None)``, ``total`` = the
    offset behind the last block.  Host arithmetic only; ``present``: the keys that get blocks (default: every F > 0)."""

    def __init__(self, num_items, feat_dim, start, present=None, tables=True):
        self.num_items, self.feat_dim = int(num_items), dict(feat_dim)
        self.feat_ld = {k: (F + 3) // 4 * 4 for k, F in self.feat_dim.items()}
        if present is None:
            present = [k for k, F in self.feat_dim.items() if F]
        self.off, o = {}, int(start)
        for key, _ in MODALITIES:
            if key in present:
                trs = 64 * self.feat_ld[key] + 64
                self.off[key] = (o, o + trs if tables else None)
                o += trs + (self.num_items * self.feat_ld[key] if tables else 0)
        self.total = o

    def blocks(self, buf, key):
        """(projection block, feature table or None) of ``key`` as flat slices of ``buf``"""
        t, e = self.off[key]
        ld = self.feat_ld[key]
        return buf[t:t + 64 * ld + 64], None if e is None else buf[e:e + self.num_items * ld]

    def linear(self, trs, key, d_out):
        """(W [:d_out, :F], b [:d_out]) views of a projection block"""
        F, ld = self.feat_dim[key], self.feat_ld[key]
        return trs[:64 * ld].view(64, ld)[:d_out, :F], trs[64 * ld:64 * ld + d_out]

    def views(self, buf, key, prefix, d_out):
        """the three views of ``key`` in the reference's names: <prefix>_embedding.weight [I, F], _trs.weight, _trs.bias; None
        each for ``buf`` None (blocks without a gradient buffer)"""
        if buf is None:
            return dict.fromkeys(prefix + s for s in ("_embedding.weight", "_trs.weight", "_trs.bias"))
        trs, tab = self.blocks(buf, key)
        W, b = self.linear(trs, key, d_out)
        return {prefix + "_embedding.weight": tab.view(self.num_items, self.feat_ld[key])[:, :self.feat_dim[key]],
                prefix + "_trs.weight": W, prefix + "_trs.bias": b}


# ---- the recommender ---------------------------------------------------------------------------------
class MultimodalRecommender(GraphRecommender):
    """``GraphRecommender`` with ``img`` / ``txt`` feature tables.  A model names ``check_limits`` (its module's, as a
    staticmethod), ``MAX_BATCH``, ``LOSS_LEN`` and provides ``_build``, ``_views(grad)``, ``_workspace(n)`` (the bytes
    ``skr_<model>_step`` needs for n rows) and ``_step_args(*ids, loss)``; ``_modal`` is the ``ModalLayout`` of its modal
    blocks.  Class switches: ``required`` (both tables), ``seeded`` (``_build`` takes the run's ``seed``), ``pairwise`` (the
    fit loop samples negatives), ``lr_scheduler`` (a fixed schedule; otherwise the config's, if it has one)."""
    required = seeded = pairwise = False
    lr_scheduler = None
    _prev_items = None      # BM3, FREEDOM: the item ids whose feature-gradient rows the previous step wrote

    @property
    def _name(self):
        return type(self).__name__

    # ---- construction ------------------------------------------------------------------------------
    def _check_limits(self, world):
        self.check_limits(self.config, world)

    def _build_args(self, run_config):
        kw = {"img": self.dataset.img_features, "txt": self.dataset.txt_features}
        if self.seeded:
            kw["seed"] = getattr(run_config, "seed", 0) or 0
        return kw

    def _check_data(self, img=None, txt=None, seed=0):
        for name, a in (("image", img), ("text", txt)):
            if a is None:
                features(a, 0, self._name, name, self.required)
        self.check_limits(self.config, 1, None if img is None else int(img.shape[1]), None if txt is None else int(txt.shape[1]))
        self._check_modalities(img, txt)

    def _check_modalities(self, img, txt):
        """the model's own ValueErrors on the tables it got"""

    def _features(self, img, txt):
        """{"img": table or None, "txt": ...} as float32 tensors; sets ``feat_dim``, ``feat_ld`` and ``present``"""
        feats = {"img": features(img, self.num_items, self._name, "image", self.required),
                 "txt": features(txt, self.num_items, self._name, "text", self.required)}
        self.feat_dim, self.feat_ld, self.present = feature_dims(feats)
        return feats

    def _entry(self, suffix):
        return getattr(_hip.lib(), f"skr_{self._name.lower()}_{suffix}")

    def _new_work(self):
        return torch.empty(self._workspace(min(self.config.batch_size, self.MAX_BATCH)), dtype=torch.uint8, device=self.device)

    # ---- the blocks --------------------------------------------------------------------------------
    def _buffer(self, grad=False):
        return self._grad if grad else self._flat

    _modal_buffer = _buffer     # the buffer the modal blocks lie in

    def _blocks(self, key, grad=False):
        """(projection block W [64, ld] | b [64], feature table [I, ld]) of a present modality as flat slices of the parameter
        (``grad``: gradient) buffer"""
        return self._modal.blocks(self._modal_buffer(grad), key)

    def _modal_views(self, grad, d_out):
        """the modal blocks' {name: view} in the reference's names, image first; None where the buffer is (FREEDOM)"""
        out = {}
        for key, prefix in MODALITIES:
            if key in self._modal.off:
                out.update(self._modal.views(self._modal_buffer(grad), key, prefix, d_out))
        return out

    def _to_reference(self, v):
        return v.contiguous().clone()

    def _from_reference(self, t, view):
        return t

    def _loaded(self):
        """after ``load_parameters``"""

    def parameters(self):
        """{name: tensor} in the reference's ``named_parameters()`` names, order and shapes (copies)"""
        return {k: self._to_reference(v) for k, v in self._views(False).items()}

    def gradients(self):
        """the gradient in the shapes of ``parameters()`` (copies); zeros where ``_views`` has None"""
        P = self._views(False)
        return {k: torch.zeros_like(P[k]).contiguous() if v is None else self._to_reference(v) for k, v in self._views(True).items()}

    def load_parameters(self, named):
        """sets the parameters from a dict in the names and shapes of ``parameters()`` (padding stays zero)"""
        views = self._views(False)
        assert set(named) == set(views), sorted(set(named) ^ set(views))
        for k, v in named.items():
            t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
            views[k].copy_(self._from_reference(t.detach().to(self.device, torch.float32), views[k]))
        self._loaded()

    # ---- training --------------------------------------------------------------------------------
    def _clear_args(self, a):
        """hands the step the feature-gradient rows the previous one wrote"""
        prev = self._prev_items
        if prev is not None:
            a.clear_items, a.n_clear = _hip.ptr(prev), int(prev.numel())

    def _before_step(self):
        pass

    def _make_args(self, ids, loss, **kw):
        """the args struct of one step; ``kw``: what the model's ``gradient_step`` takes beside the lists"""
        return self._step_args(*ids, loss)

    def _after_step(self, ids):
        pass

    def _gradient_step(self, lists, h_ms=None, **kw):
        """the frame of ``gradient_step``: ``lists`` (sequences or device tensors) to int32 device ids, the batch limit, the
        zero loss, the empty batch (a zero loss, a zero gradient, no launch), the workspace, ``skr_<model>_step`` -- with
        ``h_ms`` the ``_timed`` entry -- on ``_make_args(ids, loss, **kw)``, then ``_after_step(ids)`` -> the loss tensor"""
        ids = tuple(self._ids(t) for t in lists)
        n = int(ids[0].numel())
        if n > self.MAX_BATCH:
            raise NotImplementedError(f"{self._name}: a batch holds at most {self.MAX_BATCH} rows (got {n})")
        assert all(t.numel() == n for t in ids[1:])
        self._before_step()
        loss = torch.zeros(self.LOSS_LEN, dtype=torch.float32, device=self.device)
        if n == 0:
            self._grad.zero_()
            self._prev_items = None    # no feature-gradient row is left to clear
            return loss
        self._grow_work(self._workspace(n))
        a = self._make_args(ids, loss, **kw)
        if h_ms is None:
            _hip.check(self._entry("step")(ctypes.byref(a), _hip.stream()))
        else:
            _hip.check(self._entry("step_timed")(ctypes.byref(a), _hip.stream(), h_ms))
        self._keep = ids               # alive across the launches
        self._after_step(ids)
        return loss

    def _after_optimizer(self, **kw):
        self._prev_items = None        # the Adam launch zeroes the gradient it has read: nothing is left to clear

    @on_compute_stream
    def train_step(self, *batch, **kw):
        """one step on a batch of ``gradient_step``'s lists (sequences or int32 device tensors), the optimiser included ->
        device tensor of the loss components"""
        loss = self.gradient_step(*batch, **kw)
        self.optimizer.step()
        self._after_optimizer(**kw)
        self.step_losses.append(loss)
        return loss

    def _make_iterator(self):
        if not self.pairwise:
            return GraphRecommender._make_iterator(self)
        return PairwiseIterator(self.dataset.train_data, batch_size=self.config.batch_size, shuffle=True, drop_last=False,
                                sampler_mode=self.sampler_mode)

    def _batches(self, data_iter, epoch):
        return data_iter.iter_device() if self.pairwise else data_iter

    def _optimizers(self):
        return (self.optimizer,)

    def set_epoch(self, epoch):
        """installs the learning rate of epoch ``epoch`` (the reference steps its LambdaLR after each epoch)"""
        lr = float(lambda_lr(self.config.lr, self.lr_scheduler or self.config.lr_scheduler, epoch))
        for opt in self._optimizers():
            opt.lr = lr
        return lr

    def _begin_epoch(self, epoch):
        if self.lr_scheduler or hasattr(self.config, "lr_scheduler"):
            self.set_epoch(epoch)

    def _run_epoch(self, data_iter, epoch):
        self._begin_epoch(epoch)
        GraphRecommender._run_epoch(self, data_iter, epoch)
