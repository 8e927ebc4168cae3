"""MGCN on MI355X (reference: skrec/recommender/MGCN.py).

Paper: Multi-View Graph Convolutional Network for Multimedia Recommendation (Yu, Tan, Lu and Bao, ACM MM 2023).  Same config,
same initialisation, same loss (MGCN.py:250-353): both TRAINABLE feature tables are projected to ``embed_dim`` columns over
all items, a sigmoid gate of the projected rows purifies the item embeddings per modality, each purified table is propagated
``n_layers`` times over its own weighted item-item kNN graph (built once from the initial features: ``knn_topk`` with
similarities + ``build_weighted_item_graph``, no cache file) and carried to the users by ``R``; a LightGCN encoder of
``n_ui_layers`` gives the user-item view ``M``; a row-local attention fuser turns the two modality views and ``M`` into ``side``
and ``out = M + side``.  The loss is BPR on ``out``, an L2 term on the batch's ``out`` rows and ``cl_loss`` times two InfoNCE
terms between ``side`` and ``M`` (temperature the literal 0.2).  ``lambda_coeff`` is accepted and unused, as in the reference.

One training step is ``skr_mgcn_step`` (csrc/mgcn.hip) and one dense Adam launch over the flat buffer

    [U + I, 64] rows | image: W [64, ld] | b 64 | table [I, ld] | text: the same | gate_v | gate_t | query_common W | b | q
    | gate_image_prefer | gate_text_prefer          (gate blocks: W [64, 64] | b 64; ld = the feature width rounded up to 4)

The fuser runs at the batch's 3 n rows only in training; ``propagate()`` runs it over all rows for ranking.  The learning rate
follows the reference's ``LambdaLR``: ``lr * lr_scheduler[0] ** (epoch / lr_scheduler[1])``, set before each epoch's steps.

Ranking: ``<out_u, out_i>`` of a full forward -- two plain factor tables for the fused top-K path.

Limits (NotImplementedError): embed_dim <= 64, n_ui_layers <= 4, n_layers <= 4, batch_size <= 2048, knn_k <= 32,
1 <= F <= 4096 per modality, one GPU.  ValueError: a missing modality (the reference's forward uses both unconditionally).
"""
import torch
import torch.nn as nn

from .. import _hip
from ..utils.item_graph import build_weighted_item_graph, knn_topk
from ..utils.py import ModelConfig
from ._graph import _adjacency, propagate_mean, run_plan, upload_csr
from ._multimodal import ModalLayout, MultimodalRecommender, lambda_lr, limit_batch, limit_features, limit_world
from ._sparse import DeviceCSR
from .base import DenseAdam

__all__ = ["MGCN", "MGCNConfig"]

MAX_BATCH, MAX_LAYERS, MAX_FEAT = _hip.SKR_MGCN_MAX_BATCH, _hip.SKR_MGCN_MAX_LAYERS, _hip.SKR_MGCN_MAX_FEAT
MAX_KNN = _hip.SKR_KNN_MAX_K
GATE, QUERY = _hip.SKR_MGCN_GATE_FLOATS, _hip.SKR_MGCN_QUERY_FLOATS
# (key, the reference's prefix, the purifier gate, the preference gate): the reference registers the image block first
MODALITIES = (("img", "image", "gate_v.0", "gate_image_prefer.0"), ("txt", "text", "gate_t.0", "gate_text_prefer.0"))
NAMES = ("user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
         "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias",
         "query_common.0.weight", "query_common.0.bias", "query_common.2.weight",
         "gate_v.0.weight", "gate_v.0.bias", "gate_t.0.weight", "gate_t.0.bias",
         "gate_image_prefer.0.weight", "gate_image_prefer.0.bias", "gate_text_prefer.0.weight", "gate_text_prefer.0.bias")


class MGCNConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=1e-4, embed_dim=64, n_ui_layers=2, n_layers=1, lambda_coeff=0.9, knn_k=10, cl_loss=0.001,
                 lr_scheduler=(0.96, 50), batch_size=2048, epochs=1000, early_stop=200, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_dim: int = embed_dim
        self.n_ui_layers: int = n_ui_layers
        self.n_layers: int = n_layers
        self.lambda_coeff: float = lambda_coeff      # accepted and unused, as in the reference (MGCN.py:31)
        self.knn_k: int = knn_k
        self.cl_loss: float = cl_loss
        self.lr_scheduler = list(lr_scheduler)
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    @classmethod
    def param_space(cls):
        return {"cl_loss": [0.001, 0.01, 0.1]}

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_dim, int) and self.embed_dim > 0
        assert isinstance(self.n_ui_layers, int) and self.n_ui_layers >= 0
        assert isinstance(self.n_layers, int) and self.n_layers >= 0
        assert isinstance(self.lambda_coeff, float)
        assert isinstance(self.knn_k, int) and self.knn_k > 0
        assert isinstance(self.cl_loss, float) and self.cl_loss >= 0
        assert len(self.lr_scheduler) == 2 and self.lr_scheduler[0] > 0 and self.lr_scheduler[1] > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config, world=1, img_dim=None, txt_dim=None):
    """raises NotImplementedError, naming the limit, for a config or a feature width this implementation does not run"""
    if config.embed_dim > 64:
        raise NotImplementedError(f"MGCN: embed_dim <= 64 (got {config.embed_dim}): rows are 64 floats")
    if config.n_ui_layers > MAX_LAYERS:
        raise NotImplementedError(f"MGCN: n_ui_layers <= {MAX_LAYERS} (got {config.n_ui_layers})")
    if config.n_layers > MAX_LAYERS:
        raise NotImplementedError(f"MGCN: n_layers <= {MAX_LAYERS} (got {config.n_layers})")
    limit_batch("MGCN", config, MAX_BATCH)
    if config.knn_k > MAX_KNN:
        raise NotImplementedError(f"MGCN: knn_k <= {MAX_KNN} (got {config.knn_k}): skr_knn_topk keeps {MAX_KNN} neighbours per row")
    limit_features("MGCN", MAX_FEAT, img_dim, txt_dim)
    limit_world("MGCN", world)


def learning_rate(config, epoch):
    """the learning rate of epoch ``epoch``: LambdaLR's lr * lr_scheduler[0] ** (epoch / lr_scheduler[1]) (MGCN.py:373-375), the
    reference's Python-float expression"""
    return lambda_lr(config.lr, config.lr_scheduler, epoch)


def init_parameters(num_users, num_items, d, img_dim, txt_dim):
    """CPU-side draws in the reference's module order (MGCN.py:138-206): the two nn.Embedding tables (whose own normal draws are
    consumed and overwritten by xavier-uniform), image_trs, text_trs, query_common (Linear(d, d), Linear(d, 1, bias=False)),
    gate_v, gate_t, gate_image_prefer, gate_text_prefer with nn.Linear's default initialisation (``from_pretrained`` draws
    nothing) -> {name: tensor} in the reference's names, without the feature tables"""
    eu, ei = nn.Embedding(num_users, d), nn.Embedding(num_items, d)
    nn.init.xavier_uniform_(eu.weight)
    nn.init.xavier_uniform_(ei.weight)
    P = {"user_embedding.weight": eu.weight, "item_id_embedding.weight": ei.weight}
    for prefix, F in (("image", img_dim), ("text", txt_dim)):
        lin = nn.Linear(F, d)
        P[prefix + "_trs.weight"], P[prefix + "_trs.bias"] = lin.weight, lin.bias
    q0, q2 = nn.Linear(d, d), nn.Linear(d, 1, bias=False)
    P["query_common.0.weight"], P["query_common.0.bias"], P["query_common.2.weight"] = q0.weight, q0.bias, q2.weight
    for gate in ("gate_v.0", "gate_t.0", "gate_image_prefer.0", "gate_text_prefer.0"):
        lin = nn.Linear(d, d)
        P[gate + ".weight"], P[gate + ".bias"] = lin.weight, lin.bias
    return {k: v.detach().clone() for k, v in P.items()}


def mgcn_adjacency(rowptr, col, num_users, num_items):
    """(R, R^T) as DeviceCSR from the binary train CSR in HBM: rowdeg^-0.5 * coldeg^-0.5 in fp32, no self loops, no epsilon
    (MGCN.py:213-240; an entry's row and column have a degree of at least 1, so the reference's inf -> 0 never applies to one)"""
    def value(rowdeg, coldeg, rows, cols):
        return rowdeg.to(torch.float32).pow(-0.5)[rows] * coldeg.to(torch.float32).pow(-0.5)[cols]
    return _adjacency(rowptr, col, num_users, num_items, value, False)[:2]


class MGCN(MultimodalRecommender):
    """limits: see ``check_limits``; ``img`` / ``txt`` (``detached``; the data set's otherwise): [num_items, F] feature tables,
    both required"""
    config_class = MGCNConfig
    check_limits = staticmethod(check_limits)
    MAX_BATCH, LOSS_LEN, required, pairwise = MAX_BATCH, 4, True, True

    def _build(self, rowptr, items, img=None, txt=None):
        cfg, dev = self.config, self.device
        nu, ni, d = self.num_users, self.num_items, cfg.embed_dim
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t = mgcn_adjacency(rp, col, nu, ni)
        feats = self._features(img, txt)
        P = init_parameters(nu, ni, d, self.feat_dim["img"], self.feat_dim["txt"])
        # the flat buffer
        self._modal = ModalLayout(ni, self.feat_dim, N * 64)
        self._off, o = dict(self._modal.off), self._modal.total        # key: (the projection block, the table)
        for name, size in (("gate_v.0", GATE), ("gate_t.0", GATE), ("query", QUERY), ("gate_image_prefer.0", GATE),
                           ("gate_text_prefer.0", GATE)):
            self._off[name] = o
            o += size
        self._flat = torch.zeros(o, dtype=torch.float32, device=dev)
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)           # Adam(lr) over every parameter (MGCN.py:372)
        self._grad = self.optimizer.grad
        self.X0 = self._flat[:N * 64].view(N, 64)
        P["image_embedding.weight"], P["text_embedding.weight"] = feats["img"], feats["txt"]
        self.load_parameters(P)
        # the two weighted item graphs, from the initial feature tables (MGCN.py:152-173)
        self.knn, self.mm_adj, self.mm_adj_t = {}, {}, {}
        for key, _, _, _ in MODALITIES:
            tab = self._blocks(key)[1].view(ni, self.feat_ld[key])
            ids, sims = knn_topk(tab, cfg.knn_k, feat_dim=self.feat_dim[key], return_sims=True)
            self.knn[key] = (ids, sims)
            S, St = build_weighted_item_graph(ids, sims)
            self.mm_adj[key], self.mm_adj_t[key] = DeviceCSR.from_arrays((ni, ni), *S), DeviceCSR.from_arrays((ni, ni), *St)
        z = lambda rows: torch.zeros((rows, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self.M, self.pooled = z(N), z(N)
        self._F, self._gout = (z(ni), z(ni)), (z(ni), z(ni))
        self._Z, self._G, self._ping = (z(N), z(N)), (z(N), z(N), z(N)), (z(N), z(N))
        self._ld_max = max(self.feat_ld.values())
        self._work = self._new_work()
        self.step_losses = []          # (BPR, regulariser, cl_loss * InfoNCE, total) per training step, device tensors [4]

    # ---- the blocks ------------------------------------------------------------------------------
    def _block(self, name, grad=False):
        o = self._off[name]
        return self._buffer(grad)[o:o + (QUERY if name == "query" else GATE)]

    def _views(self, grad=False):
        """{name: view} in the reference's ``named_parameters()`` names, order and shapes"""
        d, nu, ni = self.config.embed_dim, self.num_users, self.num_items
        rows = self._buffer(grad)[:(nu + ni) * 64].view(nu + ni, 64)
        out = {"user_embedding.weight": rows[:nu, :d], "item_id_embedding.weight": rows[nu:, :d], **self._modal_views(grad, d)}
        q = self._block("query", grad)
        out["query_common.0.weight"], out["query_common.0.bias"] = q[:4096].view(64, 64)[:d, :d], q[4096:4096 + d]
        out["query_common.2.weight"] = q[GATE:GATE + d].view(1, d)
        for name in ("gate_v.0", "gate_t.0", "gate_image_prefer.0", "gate_text_prefer.0"):
            b = self._block(name, grad)
            out[name + ".weight"], out[name + ".bias"] = b[:4096].view(64, 64)[:d, :d], b[4096:4096 + d]
        return {k: out[k] for k in NAMES}

    # ---- training --------------------------------------------------------------------------------
    def gradient_step(self, users, pos, neg, h_ms=None):
        """forward and backward of one batch without the optimiser: the gradient is left in the optimiser's gradient buffer,
        every element written -> device tensor (BPR, regulariser, cl_loss * InfoNCE, total).  ``h_ms``: a ctypes float array of
        SKR_MGCN_GROUPS entries that receives the milliseconds of each launch group"""
        return self._gradient_step((users, pos, neg), h_ms)

    def _workspace(self, n):
        return int(_hip.lib().skr_mgcn_workspace(n, self.num_items, self._ld_max))

    def _step_args(self, du, dp, dn, loss):
        cfg, n = self.config, int(du.numel())
        a, p = _hip.MGCNStepArgs(), _hip.ptr
        a.plan_a, a.plan_at = self.adj._plan_handle(), self.adj_t._plan_handle()
        a.n_users, a.n_items, a.dim, a.n_ui_layers, a.n_layers, a.n = self.num_users, self.num_items, cfg.embed_dim, cfg.n_ui_layers, cfg.n_layers, n
        a.params, a.grad = p(self._flat), p(self._grad)
        for m, (key, _, gate, pref) in enumerate(MODALITIES):
            if cfg.n_layers > 0:
                a.plan_s[m], a.plan_st[m] = self.mm_adj[key]._plan_handle(), self.mm_adj_t[key]._plan_handle()
            (trs, tab), (gtrs, gtab) = self._blocks(key), self._blocks(key, True)
            a.feat_dim[m], a.feat_ld[m] = self.feat_dim[key], self.feat_ld[key]
            a.trs[m], a.feat[m], a.trs_grad[m], a.feat_grad[m] = p(trs), p(tab), p(gtrs), p(gtab)
            a.gate[m], a.gate_grad[m] = p(self._block(gate)), p(self._block(gate, True))
            a.prefer[m], a.prefer_grad[m] = p(self._block(pref)), p(self._block(pref, True))
            a.F[m], a.gate_out[m], a.Z[m], a.ping[m] = p(self._F[m]), p(self._gout[m]), p(self._Z[m]), p(self._ping[m])
        a.query, a.query_grad = p(self._block("query")), p(self._block("query", True))
        a.users, a.pos, a.neg = p(du), p(dp), p(dn)
        a.reg, a.cl_loss = cfg.reg, cfg.cl_loss
        a.M, a.loss = p(self.M), p(loss)
        for t in range(3):
            a.G[t] = p(self._G[t])
        a.work, a.work_bytes = p(self._work), self._work.numel()
        return a

    # ---- ranking: the base class's, on the two factor tables (MGCN.py:355-361) ----------------------
    def propagate(self):
        """the full forward of the CURRENT parameters with the dense fuser over all U + I rows (MGCN.py:250-312) -> pooled = out"""
        cfg, L, st, p = self.config, _hip.lib(), _hip.stream(), _hip.ptr
        nu, ni, Ln = self.num_users, self.num_items, cfg.n_layers
        propagate_mean(self.adj, self.adj_t, self.X0, nu, cfg.n_ui_layers, self.M, ping=self._ping)
        for m, (key, _, gate, _) in enumerate(MODALITIES):
            trs, tab = self._blocks(key)
            _hip.check(L.skr_mgcn_project(p(tab), ni, self.feat_dim[key], self.feat_ld[key], p(trs), p(self._F[m]), st))
            Z = self._Z[m]
            X = Z[nu:] if Ln == 0 else self._ping[0][:ni]
            _hip.check(L.skr_mgcn_purify(p(self._F[m]), p(self.X0[nu:]), p(self._block(gate)), ni, cfg.embed_dim, p(self._gout[m]), p(X), st))
            for k in range(1, Ln + 1):
                Y = Z[nu:] if k == Ln else self._ping[k & 1][:ni]
                run_plan(self.mm_adj[key], X, Y=Y)
                X = Y
            run_plan(self.adj, Z[nu:], Y=Z[:nu])
        _hip.check(L.skr_mgcn_fuse(p(self.M), p(self._Z[0]), p(self._Z[1]), p(self._block("query")), p(self._block("gate_image_prefer.0")),
                                   p(self._block("gate_text_prefer.0")), nu + ni, cfg.embed_dim, p(self.pooled), None, st))
        return self.pooled

    def _factors(self):
        """(out_u [U, 64], out_i [I, 64], None) of the last ``propagate()``"""
        return self.pooled[:self.num_users], self.pooled[self.num_users:], None
