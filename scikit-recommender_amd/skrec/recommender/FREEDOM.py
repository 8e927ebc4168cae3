"""FREEDOM on MI355X (reference: skrec/recommender/FREEDOM.py).

Paper: A Tale of Two Graphs: Freezing and Denoising Graph Structures for Multimodal Recommendation (Zhou and Shen, ACM MM
2023).  Same config, same initialisation, same loss (FREEDOM.py:211-252): a LightGCN encoder of ``n_ui_layers`` over the
user-item graph, whose item rows get ``h = S^n_mm_layers X0_items`` added -- ``S`` the FROZEN item-item kNN graph built once
from the initial feature tables (``knn_topk`` + ``build_item_graph``, no cache file) --, and three BPR terms that share the user
row: the graph term and, weighted by ``reg``, one per present modality against ``nn.Linear(F, feat_dim)`` of the item's feature
row.  ``lambda_coeff`` is accepted and unused, as in the reference.

The user-item graph of training changes every epoch (FREEDOM.py:175-190): ``int(nnz * (1 - dropout))`` interactions are drawn
without replacement with probabilities proportional to their normalised value, and what is left is renormalised.  Here that is
``prune(epoch)``: ``skr_freedom_keys`` (w / Exp(1) per entry, keyed by (seed, epoch, entry)), ``skr_freedom_select`` (the
n_keep largest keys) and ``skr_freedom_pruned_csr`` (the compacted CSR pair with the renormalised values), wrapped in two new
``DeviceCSR`` whose SpMM plans are analysed once per epoch.  The draw (``draws = "device"``, the only mode: not a reference
option) equals the reference's ``torch.multinomial`` in law only; it has no limit of 2^24 categories.  ``prune(epoch, keep)``
takes recorded flags instead and replays a recorded run.  ``evaluate()`` uses the unpruned graph.

One training step is ``skr_freedom_step`` (csrc/freedom.hip) and one dense Adam launch over the flat buffer

    [U + I, 64] rows            | and, at reg > 0 only, image first per present modality: W [64, ld] | b 64 | table [I, ld]

(``ld`` = the feature width rounded up to a multiple of 4).  The bias cancels in ``x_m``: its gradient is written as an exact
zero and it never moves (the reference's moves by the rounding residue of a sum of +a / -a pairs).  At ``reg == 0``, the
reference's default, every modal gradient is an exact zero, which leaves a parameter bit-unchanged under ``torch.optim.Adam``:
the projections and the feature tables are then constant tensors outside the optimiser's buffer -- still reported by
``parameters()`` -- and the step launches nothing for them.  The reference's ``LambdaLR`` factor is ``1.0 ** (epoch / 50) =
1``: no scheduler is kept.

Ranking: ``M`` from the unpruned graph plus ``h``, score ``<M_u, M_i>`` -- two plain factor tables for the fused top-K path.

Limits (NotImplementedError): embed_dim <= 64, n_ui_layers <= 4, n_mm_layers <= 4, batch_size <= 2048, knn_k <= 32,
1 <= F <= 4096 per modality, one GPU.  ValueError: no modality at all; a modality with feat_dim != embed_dim (the reference
fails there on a shape mismatch).
"""
import torch
import torch.nn as nn

from .. import _hip
from ..utils.item_graph import build_item_graph, knn_topk
from ..utils.py import ModelConfig
from ._graph import propagate_mean, run_plan, selfcf_adjacency, upload_csr
from ._multimodal import MODALITIES, ModalLayout, MultimodalRecommender, limit_batch, limit_features, limit_world
from ._sparse import DeviceCSR
from .base import DenseAdam

__all__ = ["FREEDOM", "FREEDOMConfig"]

MAX_BATCH, MAX_LAYERS, MAX_FEAT = _hip.SKR_FREEDOM_MAX_BATCH, _hip.SKR_FREEDOM_MAX_LAYERS, _hip.SKR_FREEDOM_MAX_FEAT
MAX_KNN = _hip.SKR_KNN_MAX_K


class FREEDOMConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=0.0, embed_dim=64, feat_dim=64, lambda_coeff=0.9, n_mm_layers=1, n_ui_layers=2, knn_k=10,
                 mm_image_weight=0.1, dropout=0.8, batch_size=2048, epochs=1000, early_stop=200, draws="device", **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_dim: int = embed_dim
        self.feat_dim: int = feat_dim
        self.lambda_coeff: float = lambda_coeff      # accepted and unused, as in the reference (FREEDOM.py:71)
        self.n_mm_layers: int = n_mm_layers
        self.n_ui_layers: int = n_ui_layers
        self.knn_k: int = knn_k
        self.mm_image_weight: float = mm_image_weight
        self.dropout: float = dropout
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop
        # how an epoch's kept interactions are drawn (not a reference option): "device"
        self.draws: str = draws

    @classmethod
    def param_space(cls):
        return {"reg": [0.0, 1e-05, 1e-04, 1e-03], "dropout": [0.8, 0.9]}

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_dim, int) and self.embed_dim > 0
        assert isinstance(self.feat_dim, int) and self.feat_dim > 0
        assert isinstance(self.lambda_coeff, float)
        assert isinstance(self.n_mm_layers, int) and self.n_mm_layers >= 0
        assert isinstance(self.n_ui_layers, int) and self.n_ui_layers >= 0
        assert isinstance(self.knn_k, int) and self.knn_k > 0
        assert isinstance(self.mm_image_weight, float) and 0 <= self.mm_image_weight <= 1
        assert isinstance(self.dropout, float) and self.dropout < 1
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)
        assert self.draws == "device"


def check_limits(config, world=1, img_dim=None, txt_dim=None):
    """raises NotImplementedError, naming the limit, for a config or a feature width this implementation does not run"""
    if config.embed_dim > 64:
        raise NotImplementedError(f"FREEDOM: embed_dim <= 64 (got {config.embed_dim}): rows are 64 floats")
    if config.n_ui_layers > MAX_LAYERS:
        raise NotImplementedError(f"FREEDOM: n_ui_layers <= {MAX_LAYERS} (got {config.n_ui_layers})")
    if config.n_mm_layers > MAX_LAYERS:
        raise NotImplementedError(f"FREEDOM: n_mm_layers <= {MAX_LAYERS} (got {config.n_mm_layers})")
    limit_batch("FREEDOM", config, MAX_BATCH)
    if config.knn_k > MAX_KNN:
        raise NotImplementedError(f"FREEDOM: knn_k <= {MAX_KNN} (got {config.knn_k}): skr_knn_topk keeps {MAX_KNN} neighbours per row")
    limit_features("FREEDOM", MAX_FEAT, img_dim, txt_dim)
    limit_world("FREEDOM", world)


def init_parameters(num_users, num_items, d, feat_dim, img_dim=None, txt_dim=None):
    """CPU-side draws in the reference's order (FREEDOM.py:94-109): the two nn.Embedding tables (whose own normal draws are
    consumed and overwritten), xavier-uniform user table, xavier-uniform item table, then per present modality -- image first
    -- nn.Linear(F, feat_dim) with its default initialisation (``from_pretrained`` draws nothing) -> {name: tensor} in the
    reference's names, without the feature tables"""
    eu, ei = nn.Embedding(num_users, d), nn.Embedding(num_items, d)
    nn.init.xavier_uniform_(eu.weight)
    nn.init.xavier_uniform_(ei.weight)
    P = {"user_embedding.weight": eu.weight.detach().clone(), "item_id_embedding.weight": ei.weight.detach().clone()}
    for prefix, F in (("image", img_dim), ("text", txt_dim)):
        if F is not None:
            lin = nn.Linear(F, feat_dim)
            P[prefix + "_trs.weight"], P[prefix + "_trs.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return P


def edge_weights(rowptr, col, num_items):
    """w [nnz] in R's CSR order, the reference's ``_normalize_adj_m`` on the full graph in fp32 (FREEDOM.py:192-209):
    pow(1e-7 + rowcount, -0.5) * pow(1e-7 + colcount, -0.5)"""
    rowdeg = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(rowdeg.numel(), dtype=torch.int64, device=rowptr.device), rowdeg)
    cols = col.to(torch.int64)
    coldeg = torch.bincount(cols, minlength=num_items)
    r = torch.pow(1e-7 + rowdeg.to(torch.float32), -0.5)
    c = torch.pow(1e-7 + coldeg.to(torch.float32), -0.5)
    return (r[rows] * c[cols]).contiguous()


class FREEDOM(MultimodalRecommender):
    """limits: see ``check_limits``; ``img`` / ``txt`` (``detached``; the data set's otherwise): [num_items, F] feature tables
    or None; ``seed`` (the run's): the key of the device draws"""
    config_class = FREEDOMConfig
    check_limits = staticmethod(check_limits)
    MAX_BATCH, LOSS_LEN, seeded, pairwise = MAX_BATCH, 3, True, True

    def _check_modalities(self, img, txt):
        cfg = self.config
        if img is None and txt is None:
            raise ValueError("FREEDOM: no modality at all -- the item graph needs an image or a text feature table")
        if cfg.feat_dim != cfg.embed_dim:
            raise ValueError(f"FREEDOM: feat_dim = {cfg.feat_dim} must equal embed_dim = {cfg.embed_dim}: the projected feature rows "
                             f"meet the user rows in a dot product")

    def _build(self, rowptr, items, img=None, txt=None, seed=0):
        cfg, dev = self.config, self.device
        nu, ni, d = self.num_users, self.num_items, cfg.embed_dim
        Lu, Lm = cfg.n_ui_layers, cfg.n_mm_layers
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self._rp, self._col = rp, col
        self.adj, self.adj_t, self._perm = selfcf_adjacency(rp, col, nu, ni)     # FREEDOM.py:149-173 normalises as BM3 does
        self._nnz = int(col.numel())
        self.edge_w = edge_weights(rp, col, ni)
        self.adj_train, self.adj_train_t = self.adj, self.adj_t
        self._retired = []             # (event, the matrices of an earlier epoch): kept until the stream has passed the event
        feats = self._features(img, txt)
        P = init_parameters(nu, ni, d, cfg.feat_dim, self.feat_dim["img"] or None, self.feat_dim["txt"] or None)
        # the flat buffer: the rows and, at reg > 0, the modal blocks; at reg == 0 those are constants of their own
        self._modal_trained = cfg.reg > 0
        self._modal = ModalLayout(ni, self.feat_dim, N * 64 if self._modal_trained else 0)
        self._off = self._modal.off if self._modal_trained else {}
        self._flat = torch.zeros(self._modal.total if self._modal_trained else N * 64, dtype=torch.float32, device=dev)
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)         # Adam(weight_decay=0), a constant learning rate (FREEDOM.py:271-275)
        self._grad = self.optimizer.grad
        self.X0 = self._flat[:N * 64].view(N, 64)
        self._const = None if self._modal_trained else torch.zeros(self._modal.total, dtype=torch.float32, device=dev)
        for key, prefix in MODALITIES:
            if feats[key] is not None:
                P[prefix + "_embedding.weight"] = feats[key]
        self.load_parameters(P)
        # the frozen item graph, from the initial feature tables (FREEDOM.py:111-124)
        knn = {}
        for key, _ in MODALITIES:
            F = self.feat_dim[key]
            knn[key] = knn_topk(self._blocks(key)[1].view(ni, self.feat_ld[key]), cfg.knn_k, feat_dim=F) if F else None
        S, St = build_item_graph(knn["img"], knn["txt"], cfg.knn_k, cfg.mm_image_weight)
        self.mm_adj, self.mm_adj_t = DeviceCSR.from_arrays((ni, ni), *S), DeviceCSR.from_arrays((ni, ni), *St)
        z = lambda: torch.zeros((N, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self.M = z()                                              # the layer means (+ h) of the last step's forward
        self.pooled = z()                                         # the layer means (+ h) of the last propagate()
        self._ping = (z(), z()) if max(Lu, Lm) > 1 else (None, None)
        self._G = z()
        self._work = self._new_work()
        self._seed = int(seed)
        self.step_losses = []          # (graph term, reg * modal terms, total) per training step, device tensors [3]

    # ---- the blocks ------------------------------------------------------------------------------
    def _modal_buffer(self, grad=False):
        """the buffer of the modal blocks: the flat (``grad``: gradient) buffer at reg > 0, the constants otherwise (``grad``:
        None)"""
        if self._modal_trained:
            return self._buffer(grad)
        return None if grad else self._const

    def _blocks(self, key, grad=False):
        """(projection block W [64, ld] | b [64], feature table [I, ld]) of a present modality as flat slices of
        ``_modal_buffer(grad)``; (None, None) where that is None"""
        return (None, None) if self._modal_buffer(grad) is None else MultimodalRecommender._blocks(self, key, grad)

    def _views(self, grad=False):
        """{name: view} in the reference's names, order and shapes: user_embedding.weight, item_id_embedding.weight and, per
        present modality, image_ / text_embedding.weight, _trs.weight, _trs.bias; the gradient of a constant block is None,
        which ``gradients()`` reports as exact zeros"""
        d, nu, ni = self.config.embed_dim, self.num_users, self.num_items
        rows = self._buffer(grad)[:(nu + ni) * 64].view(nu + ni, 64)
        return {"user_embedding.weight": rows[:nu, :d], "item_id_embedding.weight": rows[nu:, :d], **self._modal_views(grad, d)}

    # ---- the epoch's graph -----------------------------------------------------------------------
    def prune(self, epoch, keep=None):
        """installs the user-item graph of one epoch's steps (FREEDOM.py:175-190) as ``adj_train`` / ``adj_train_t`` -> the keep
        flags (uint8 [nnz], R's CSR order), or None with ``dropout <= 0``, where the unpruned pair is installed.
        ``keep`` None: int(nnz * (1 - dropout)) entries drawn on the device, keyed by (seed, epoch, entry) -- the reference's
        ``torch.multinomial`` in law only; otherwise handed-in flags (a recorded run)"""
        cfg, L, st = self.config, _hip.lib(), _hip.stream()
        nu, ni, nnz, dev = self.num_users, self.num_items, self._nnz, self.device
        old = (self.adj_train, self.adj_train_t)
        if old[0] is not self.adj:     # the steps that used the old pair may still be running: keep it until they have passed
            ev = torch.cuda.Event()
            ev.record()
            self._retired.append((ev, old))
        self._retired = [r for r in self._retired if not r[0].query()]
        if cfg.dropout <= 0:
            self.adj_train, self.adj_train_t = self.adj, self.adj_t
            return None
        if keep is None:
            n_keep = int(nnz * (1. - cfg.dropout))
            keys = torch.empty(nnz, dtype=torch.float32, device=dev)
            _hip.check(L.skr_freedom_keys(_hip.ptr(self.edge_w), nnz, self._seed, int(epoch), _hip.ptr(keys), st))
            keep = torch.empty(nnz, dtype=torch.uint8, device=dev)
            ws = int(L.skr_freedom_select_workspace(nnz))
            work = torch.empty(ws, dtype=torch.uint8, device=dev)
            _hip.check(L.skr_freedom_select(_hip.ptr(keys), nnz, n_keep, _hip.ptr(keep), _hip.ptr(work), ws, st))
        else:
            keep = self._flags(keep, (nnz,))
        self.adj_train, self.adj_train_t = self.pruned_pair(keep)
        self.adj_train._plan_handle()          # the two analyses belong to the epoch's prologue, not to its first step
        self.adj_train_t._plan_handle()
        return keep

    def pruned_pair(self, keep):
        """(R', R'^T) as DeviceCSR from keep flags (uint8 [nnz], device): ``skr_freedom_pruned_csr``"""
        L, dev, nu, ni, nnz = _hip.lib(), self.device, self.num_users, self.num_items, self._nnz
        i64, i32, f32 = torch.int64, torch.int32, torch.float32
        rp, rpt = torch.empty(nu + 1, dtype=i64, device=dev), torch.empty(ni + 1, dtype=i64, device=dev)
        col, colt = torch.empty(nnz, dtype=i32, device=dev), torch.empty(nnz, dtype=i32, device=dev)
        val, valt = torch.empty(nnz, dtype=f32, device=dev), torch.empty(nnz, dtype=f32, device=dev)
        kept = torch.empty(1, dtype=i64, device=dev)
        ws = int(L.skr_freedom_pruned_workspace(nu, ni, nnz))
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        p = _hip.ptr
        _hip.check(L.skr_freedom_pruned_csr(nu, ni, nnz, p(self._rp), p(self._col), p(self.adj_t.rowptr), p(self.adj_t.col), p(self._perm),
                                            p(keep), p(rp), p(col), p(val), p(rpt), p(colt), p(valt), p(kept), p(work), ws, _hip.stream()))
        k = int(kept.item())
        return DeviceCSR.from_arrays((nu, ni), rp, col[:k], val[:k]), DeviceCSR.from_arrays((ni, nu), rpt, colt[:k], valt[:k])

    # ---- training --------------------------------------------------------------------------------
    def _workspace(self, n):
        return int(_hip.lib().skr_freedom_workspace(n))

    def _step_args(self, du, dp, dn, loss):
        cfg = self.config
        Lu, Lm = cfg.n_ui_layers, cfg.n_mm_layers
        a = _hip.FreedomStepArgs()
        if Lu > 0:
            a.plan_a, a.plan_at = self.adj_train._plan_handle(), self.adj_train_t._plan_handle()
        if Lm > 0:
            a.plan_s, a.plan_st = self.mm_adj._plan_handle(), self.mm_adj_t._plan_handle()
        a.n_users, a.n_items, a.dim, a.n_ui_layers, a.n_mm_layers, a.n = self.num_users, self.num_items, cfg.embed_dim, Lu, Lm, int(du.numel())
        a.params, a.users, a.pos, a.neg = _hip.ptr(self._flat), _hip.ptr(du), _hip.ptr(dp), _hip.ptr(dn)
        a.grad, a.reg = _hip.ptr(self._grad), cfg.reg
        if self._modal_trained:
            for m, (key, _) in enumerate(MODALITIES):
                if not self.feat_dim[key]:
                    continue
                (trs, tab), (gtrs, gtab) = self._blocks(key), self._blocks(key, True)
                a.feat_dim[m], a.feat_ld[m] = self.feat_dim[key], self.feat_ld[key]
                a.trs[m], a.feat[m], a.trs_grad[m], a.feat_grad[m] = _hip.ptr(trs), _hip.ptr(tab), _hip.ptr(gtrs), _hip.ptr(gtab)
            self._clear_args(a)
        a.M, a.G, a.loss = _hip.ptr(self.M), _hip.ptr(self._G), _hip.ptr(loss)
        a.ping[0], a.ping[1] = _hip.ptr(self._ping[0]), _hip.ptr(self._ping[1])
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
        return a

    def gradient_step(self, users, pos, neg, h_ms=None):
        """forward and backward of one batch on the installed graph without the optimiser: the gradient is left in the
        optimiser's gradient buffer, the layer means (+ h) in ``self.M`` -> device tensor (graph term, reg * modal terms,
        total).  ``h_ms``: a ctypes float array of SKR_FREEDOM_GROUPS entries that receives the milliseconds of each launch group"""
        return self._gradient_step((users, pos, neg), h_ms)

    def _after_step(self, ids):
        if self._modal_trained:
            self._prev_items = torch.cat(ids[1:])

    def _begin_epoch(self, epoch):
        self.prune(epoch)              # FREEDOM.py:285 pre_epoch_processing

    # ---- ranking: the base class's, on the two factor tables (FREEDOM.py:254-260) ------------------
    def propagate(self):
        """the propagation of the CURRENT parameters over the UNPRUNED graph, the layer means, then the item rows' + h
        (FREEDOM.py:211-225 with norm_adj) -> pooled"""
        nu, ni, Lm = self.num_users, self.num_items, self.config.n_mm_layers
        propagate_mean(self.adj, self.adj_t, self.X0, nu, self.config.n_ui_layers, self.pooled, ping=self._ping)
        X = self.X0[nu:]
        if Lm == 0:
            _hip.check(_hip.lib().skr_axpy(1.0, _hip.ptr(X), _hip.ptr(self.pooled[nu:]), ni * 64, _hip.stream()))
        for k in range(1, Lm + 1):
            if k == Lm:
                run_plan(self.mm_adj, X, accum=self.pooled[nu:])
            else:
                Y = self._ping[(k - 1) & 1][:ni]
                run_plan(self.mm_adj, X, Y=Y)
                X = Y
        return self.pooled

    def _factors(self):
        """(M_u [U, 64], M_i + h [I, 64], None) of the last ``propagate()``"""
        return self.pooled[:self.num_users], self.pooled[self.num_users:], None
