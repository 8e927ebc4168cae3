"""BM3 on MI355X (reference: skrec/recommender/BM3.py).

Paper: Bootstrap Latent Representations for Multi-modal Recommendation (Zhou, Zhou, Liu, Zeng, Miao, Wang, You and Jiang, WWW
2023).  Same config, same initialisation, same loss (BM3.py:142-204): a LightGCN encoder over the normalised square adjacency
(no dropout on the graph) whose item rows get their own embedding added once more (``+ h``); per present modality a TRAINABLE
item feature table, initialised from ``<prefix>.img.npz`` / ``<prefix>.txt.npz``, and an ``nn.Linear(F, embed_dim)``; one shared
64 x 64 predictor; six cosine terms between the predictor of one row set and a dropped-out, detached copy of another; and
``reg`` times the Frobenius norms of the WHOLE propagated tables divided by the number of items.  There are no negatives.
``feat_dim`` is accepted and ignored, as in the reference: the projections are ``embed_dim`` wide.

One training step is ``skr_bm3_step`` (csrc/bm3.hip: 2 n_layers plan runs forward, the norms, the gather-and-project product
of the batch's items -- the reference's [I, d] projected tables are never formed --, the batch kernel with the predictor on
the fp32 matrix pipe, the projection backward, the ordered segment adds, the dense regulariser gradient, 2 n_layers plan runs
backward) and one dense Adam launch over the flat buffer

    [U + I, 64] rows | W 64 x 64 | b 64 | image: trs W [64, ld] | trs b 64 | table [I, ld] | text: the same three

with ``weight_decay = 0`` (``ld`` = the feature width rounded up to a multiple of 4, zero beyond it).  The feature tables
receive a dense gradient that is zero outside the batch's items; their other rows still move by leftover momentum, as under
``torch.optim.Adam``.  The step zeroes only the gradient rows the previous step wrote.  The reference's ``LambdaLR`` factor is
``1.0 ** (epoch / 50) = 1``: the learning rate is constant, and no scheduler is kept.

The four target masks are drawn on the device (``draws = "device"``, the only mode: not a reference option), keyed by (seed,
step, table, node id): equal to the reference's ``F.dropout`` draws in law only; a node that occurs twice in a batch has one
mask.  ``gradient_step(..., target_keep)`` takes recorded flags instead and replays a recorded run.

``evaluate()`` propagates the CURRENT parameters and ranks ``(W M_u + b) . (W M_i + b)`` (BM3.py:206-210) through the fused
top-K path: the two factor tables come from ``skr_bm3_queries``.

Limits (NotImplementedError): embed_dim <= 64, n_layers <= 4, batch_size <= 2048, 1 <= F <= 4096 per modality, one GPU.
"""
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import ModelConfig
from ._graph import linear_block, propagate_mean, selfcf_adjacency, upload_csr
from ._multimodal import MODALITIES, ModalLayout, MultimodalRecommender, limit_batch, limit_features, limit_world
from .base import DenseAdam

__all__ = ["BM3", "BM3Config"]

MAX_BATCH, MAX_LAYERS, MAX_FEAT = _hip.SKR_BM3_MAX_BATCH, _hip.SKR_BM3_MAX_LAYERS, _hip.SKR_BM3_MAX_FEAT
PRED_FLOATS = _hip.SKR_BM3_PRED_FLOATS


class BM3Config(ModelConfig):
    def __init__(self, lr=1e-3, reg=0.1, embed_dim=64, feat_dim=64, n_layers=1, dropout=0.3, cl_weight=2.0, batch_size=2048,
                 epochs=1000, early_stop=200, draws="device", **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_dim: int = embed_dim
        self.feat_dim: int = feat_dim          # accepted and ignored, as in the reference (BM3.py:79)
        self.n_layers: int = n_layers
        self.cl_weight: float = cl_weight
        self.dropout: float = dropout
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop
        # how the target masks are made (not a reference option): "device"
        self.draws: str = draws

    @classmethod
    def param_space(cls):
        return {"n_layers": [1, 2], "reg": [0.1, 0.01], "dropout": [0.3, 0.5]}

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_dim, int) and self.embed_dim > 0
        assert isinstance(self.feat_dim, int)
        assert isinstance(self.n_layers, int) and self.n_layers >= 0
        assert isinstance(self.cl_weight, float) and self.cl_weight >= 0
        assert isinstance(self.dropout, float) and 0 <= self.dropout < 1
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)
        assert self.draws == "device"


def check_limits(config, world=1, img_dim=None, txt_dim=None):
    """raises NotImplementedError, naming the limit, for a config or a feature width this implementation does not run"""
    if config.embed_dim > 64:
        raise NotImplementedError(f"BM3: embed_dim <= 64 (got {config.embed_dim}): rows are 64 floats and the predictor 64 x 64")
    if config.n_layers > MAX_LAYERS:
        raise NotImplementedError(f"BM3: n_layers <= {MAX_LAYERS} (got {config.n_layers})")
    limit_batch("BM3", config, MAX_BATCH)
    limit_features("BM3", MAX_FEAT, img_dim, txt_dim)
    limit_world("BM3", world)


def _linear_xavier(fan_in, d):
    lin = nn.Linear(fan_in, d)
    nn.init.xavier_normal_(lin.weight)
    return lin.weight.detach().clone(), lin.bias.detach().clone()


def init_parameters(num_users, num_items, d, img_dim=None, txt_dim=None):
    """CPU-side draws in the reference's order (BM3.py:95-114): the two nn.Embedding tables (whose own normal draws are
    consumed and overwritten), xavier-uniform user table, xavier-uniform item table, nn.Linear(d, d) then xavier_normal_ on
    its weight, then per present modality -- image first -- nn.Linear(F, d) then xavier_normal_ -> {name: tensor} in the
    reference's names, without the feature tables"""
    eu, ei = nn.Embedding(num_users, d), nn.Embedding(num_items, d)
    nn.init.xavier_uniform_(eu.weight)
    nn.init.xavier_uniform_(ei.weight)
    P = {"user_embedding.weight": eu.weight.detach().clone(), "item_id_embedding.weight": ei.weight.detach().clone()}
    P["predictor.weight"], P["predictor.bias"] = _linear_xavier(d, d)
    for prefix, F in (("image", img_dim), ("text", txt_dim)):
        if F is not None:
            P[prefix + "_trs.weight"], P[prefix + "_trs.bias"] = _linear_xavier(F, d)
    return P


class BM3(MultimodalRecommender):
    """limits: see ``check_limits``; ``img`` / ``txt`` (``detached``; the data set's otherwise): [num_items, F] feature tables
    or None; ``seed`` (the run's): the key of the device draws"""
    config_class = BM3Config
    check_limits = staticmethod(check_limits)
    MAX_BATCH, LOSS_LEN, seeded = MAX_BATCH, 4, True

    def _build(self, rowptr, items, img=None, txt=None, seed=0):
        cfg, dev = self.config, self.device
        nu, ni, d, L = self.num_users, self.num_items, cfg.embed_dim, cfg.n_layers
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t, _ = selfcf_adjacency(rp, col, nu, ni)      # BM3.py:116-140 normalises as SelfCF does
        feats = self._features(img, txt)
        P = init_parameters(nu, ni, d, self.feat_dim["img"] or None, self.feat_dim["txt"] or None)
        # float offsets of the blocks of the flat buffer: the predictor, then the modal blocks (key: (projection, table))
        self._modal = ModalLayout(ni, self.feat_dim, N * 64 + PRED_FLOATS)
        self._off = {"pred": N * 64, **self._modal.off}
        self._total = self._modal.total
        self._flat = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)         # Adam(weight_decay=0), a constant learning rate (BM3.py:221-225)
        self._grad = self.optimizer.grad
        self.X0 = self._flat[:N * 64].view(N, 64)
        self._pred = self._flat[N * 64:N * 64 + PRED_FLOATS]
        for key, prefix in MODALITIES:
            if feats[key] is not None:
                P[prefix + "_embedding.weight"] = feats[key]
        self.load_parameters(P)
        z = lambda: torch.zeros((N, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self.M = z()                                              # the layer means (+ h) of the last step's forward
        self.pooled = z()                                         # the layer means (+ h) of the last propagate()
        self._ping = (z(), z()) if L > 1 else (None, None)
        self._G = z() if L > 0 else None
        self._Qu = torch.zeros((nu, 64), dtype=torch.float32, device=dev)
        self._Qi = torch.zeros((ni, 64), dtype=torch.float32, device=dev)
        self._work = self._new_work()
        self._seed, self._step = int(seed), 0
        self.step_losses = []          # (graph cosines, modal cosines, reg, total) per training step, device tensors [4]

    # ---- the flat buffer's blocks ----------------------------------------------------------------
    def _views(self, flat=False):
        """{name: view} of ``flat`` (a buffer; False / True: the parameter / gradient buffer) in the reference's names and
        shapes: user_embedding.weight, item_id_embedding.weight, predictor.weight, predictor.bias and, per present modality,
        image_ / text_embedding.weight, _trs.weight, _trs.bias"""
        d, nu, ni = self.config.embed_dim, self.num_users, self.num_items
        N = nu + ni
        flat = self._buffer(flat) if isinstance(flat, bool) else flat
        rows = flat[:N * 64].view(N, 64)
        W, b = linear_block(flat[N * 64:N * 64 + PRED_FLOATS], d)
        out = {"user_embedding.weight": rows[:nu, :d], "item_id_embedding.weight": rows[nu:, :d], "predictor.weight": W, "predictor.bias": b}
        for key, prefix in MODALITIES:
            if key in self._modal.off:
                out.update(self._modal.views(flat, key, prefix, d))
        return out

    # ---- training --------------------------------------------------------------------------------
    def target_draws(self, ids, table, step=None):
        """the device draws of one target table at the nodes ``ids`` (``skr_bm3_draws``) -> uint8 [n, 64]; ``table``: one of
        _hip.SKR_BM3_DRAW_*; keyed by (seed, step, table, node id), ``step`` None: the coming step"""
        d_ids = self._ids(ids)
        out = torch.empty((int(d_ids.numel()), 64), dtype=torch.uint8, device=self.device)
        _hip.check(_hip.lib().skr_bm3_draws(_hip.ptr(d_ids), int(d_ids.numel()), int(table), self.config.dropout, self._seed,
                                            self._step if step is None else int(step), _hip.ptr(out), _hip.stream()))
        return out

    def _workspace(self, n):
        return int(_hip.lib().skr_bm3_workspace(n))

    def _make_args(self, ids, loss, target_keep=None):
        n, keeps = int(ids[0].numel()), None
        if target_keep is not None:
            ones = None
            keeps = []
            for k in target_keep:
                if k is None:      # an absent modality: the kernel wants all four or none, and does not read this one
                    ones = torch.ones((n, 64), dtype=torch.uint8, device=self.device) if ones is None else ones
                    k = ones
                keeps.append(self._flags(k, (n, 64)))
        self._keeps = keeps            # alive across the launches
        return self._step_args(*ids, keeps, loss)

    def _step_args(self, du, di, keeps, loss):
        """``keeps``: None or the four [n, 64] uint8 device tensors of SKR_BM3_DRAW_*"""
        cfg, L = self.config, self.config.n_layers
        a = _hip.BM3StepArgs()
        if keeps is not None:
            for t in range(4):
                a.keep[t] = _hip.ptr(keeps[t])
        if L > 0:
            a.plan_a, a.plan_at = self.adj._plan_handle(), self.adj_t._plan_handle()
        a.n_users, a.n_items, a.dim, a.n_layers, a.n = self.num_users, self.num_items, cfg.embed_dim, L, int(du.numel())
        a.params, a.users, a.items = _hip.ptr(self._flat), _hip.ptr(du), _hip.ptr(di)
        a.grad = _hip.ptr(self._grad)
        for m, (key, _) in enumerate(MODALITIES):
            if not self.feat_dim[key]:
                continue
            (trs, tab), (gtrs, gtab) = self._blocks(key), self._blocks(key, True)
            a.feat_dim[m], a.feat_ld[m] = self.feat_dim[key], self.feat_ld[key]
            a.trs[m], a.feat[m], a.trs_grad[m], a.feat_grad[m] = _hip.ptr(trs), _hip.ptr(tab), _hip.ptr(gtrs), _hip.ptr(gtab)
        self._clear_args(a)
        a.dropout, a.reg, a.cl_weight, a.seed, a.step = cfg.dropout, cfg.reg, cfg.cl_weight, self._seed, self._step
        a.M, a.G, a.loss = _hip.ptr(self.M), _hip.ptr(self._G), _hip.ptr(loss)
        a.ping[0], a.ping[1] = _hip.ptr(self._ping[0]), _hip.ptr(self._ping[1])
        a.work, a.work_bytes = _hip.ptr(self._work), self._work.numel()
        return a

    def gradient_step(self, users, items, target_keep=None, h_ms=None):
        """forward and backward of one batch without the optimiser: the gradient is left in the optimiser's gradient buffer,
        the layer means (+ h) in ``self.M`` -> device tensor (graph cosines, modal cosines, reg, total).
        ``target_keep`` = (ku, ki, kt, kv), [n, 64] each -- the flags of the user, item, text and image targets at the
        batch's rows (the entries of an absent modality may be None) -- instead of the device draws;
        ``h_ms``: a ctypes float array of SKR_BM3_GROUPS entries that receives the milliseconds of each launch group"""
        return self._gradient_step((users, items), h_ms, target_keep=target_keep)

    def _after_step(self, ids):
        self._prev_items = ids[1]
        self._step += 1

    # ---- ranking: the base class's, on the two factor tables (BM3.py:206-210) -----------------------
    def propagate(self):
        """the propagation of the CURRENT parameters, the layer means and the item rows' + h (BM3.py:142-153), then the two
        factor tables W M + b (``skr_bm3_queries``) -> pooled"""
        nu, ni = self.num_users, self.num_items
        L_ = _hip.lib()
        propagate_mean(self.adj, self.adj_t, self.X0, nu, self.config.n_layers, self.pooled, ping=self._ping)
        _hip.check(L_.skr_axpy(1.0, _hip.ptr(self.X0[nu:]), _hip.ptr(self.pooled[nu:]), ni * 64, _hip.stream()))     # + h
        _hip.check(L_.skr_bm3_queries(_hip.ptr(self._pred), _hip.ptr(self.pooled), nu, ni, _hip.ptr(self._Qu), _hip.ptr(self._Qi),
                                      _hip.stream()))
        return self.pooled

    def _factors(self):
        """(W M_u + b [U, 64], W M_i + b [I, 64], None) of the current parameters"""
        return self._Qu, self._Qi, None
