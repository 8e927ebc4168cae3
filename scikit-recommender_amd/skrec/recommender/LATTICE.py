"""LATTICE on MI355X (reference: skrec/recommender/LATTICE.py).

Paper: Mining Latent Structures for Multimedia Recommendation (Zhang, Zhu, Liu, Wu, Wang and Wang, ACM MM 2021).  Same config,
same initialisation, same loss (LATTICE.py:203-294): both TRAINABLE feature tables are projected to ``feat_embed_dim`` columns
over all items; at the first step of every epoch, and at every evaluation, the kNN of the PROJECTED rows is taken, normalised,
and mixed with the frozen graph of the raw features into ``item_adj``; ``h = item_adj^n_layers E_items`` is normalised row by
row and added to the item rows of a LightGCN encoder over ``D^-1 (A + I)`` (``cf_model = "lightgcn"``) or of the raw tables
(``"mf"``).  The loss is BPR plus an L2 term, both on the propagated batch rows.  At a build step the loss differentiates
through the mixed graph: through the similarities that survived the top-k, the Laplacian normalisation and the two softmax
modal weights, down to the projections and the feature tables.

Nothing here is a dense [I, I] matrix.  ``item_adj`` is a CSR matrix over the union pattern of the four neighbour lists of a
row (``skr_lattice_graph``), multiplied through the SpMM plans; ``dLoss/d item_adj`` is a sampled product over its entries
(inside ``skr_lattice_step``), and ``skr_lattice_graph_bwd`` carries it by hand to the projected rows, from where
``skr_mgcn_project_bwd`` reaches the parameters.

Two flat buffers, two ``DenseAdam``: the [U + I, 64] rows, stepped every step, and

    modal_weight 2 (+ 2 padding) | image first per present modality: W [64, ld] | b 64 | table [I, ld]

(``ld`` = the feature width rounded up to a multiple of 4), stepped on build steps only: on every other step the reference's
``item_adj`` is detached, the modal tensors have no gradient and ``torch.optim.Adam`` skips them -- they do not move by
leftover momentum and their step counter does not advance.  Both follow the reference's ``LambdaLR``:
``lr * lr_scheduler[0] ** (epoch / lr_scheduler[1])``.  With one modality ``modal_weight`` is reported and never moves; with
``n_layers == 0`` the graph is unused and no modal tensor ever moves.

The square adjacency ``D^-1 (A + I)`` is ONE CSR pair with the diagonal inside (DESIGN.md section 8 says why).

Ranking: the graph is rebuilt from the current parameters once per ``evaluate()`` (the reference rebuilds it in every
``predict()`` call, from the same parameters) -- two plain factor tables for the fused top-K path.  The graph of an evaluation
is reused by the next epoch's build step when no parameter has changed in between: the build is bit-reproducible.

``q_i = r_i^-1/2`` is 0 where the row sum ``r_i <= 0``: the reference gives 0 at r = 0 and NaN below.

Limits (NotImplementedError): embed_dim, feat_embed_dim <= 64, len(weight_size) <= 4, n_layers <= 4, batch_size <= 2048,
knn_k <= 32, 1 <= F <= 4096 per modality, one GPU, cf_model in {"lightgcn", "mf"} ("ngcf" is dense layers with dropout, a
different model).  ``mess_dropout`` is accepted and unused outside ngcf, as in the reference.  ValueError: no modality at all
(the reference fails there on an unbound name).
"""
import torch
import torch.nn as nn

from .. import _hip
from ..utils.item_graph import build_weighted_item_graph, knn_topk
from ..utils.py import ModelConfig
from ._graph import run_plan, upload_csr
from ._multimodal import MODALITIES, ModalLayout, MultimodalRecommender, lambda_lr, limit_batch, limit_features, limit_world
from ._sparse import DeviceCSR
from .base import DenseAdam

__all__ = ["LATTICE", "LATTICEConfig"]

MAX_BATCH, MAX_LAYERS, MAX_FEAT = _hip.SKR_LATTICE_MAX_BATCH, _hip.SKR_LATTICE_MAX_LAYERS, _hip.SKR_MGCN_MAX_FEAT
MAX_KNN = _hip.SKR_KNN_MAX_K
CF_MODELS = {"lightgcn": _hip.SKR_LATTICE_CF_LIGHTGCN, "mf": _hip.SKR_LATTICE_CF_MF}
NAMES = ("modal_weight", "user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
         "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias")


class LATTICEConfig(ModelConfig):
    def __init__(self, lr=1e-4, reg=0.0, embed_dim=64, feat_embed_dim=64, weight_size=(64, 64), lambda_coeff=0.9,
                 mess_dropout=(0.1, 0.1), n_layers=1, knn_k=10, cf_model="lightgcn", lr_scheduler=(0.96, 50), batch_size=2048,
                 epochs=1000, early_stop=200, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.embed_dim: int = embed_dim
        self.feat_embed_dim: int = feat_embed_dim
        self.weight_size = list(weight_size)         # only its length counts outside ngcf: n_ui_layers
        self.lambda_coeff: float = lambda_coeff
        self.mess_dropout = list(mess_dropout)       # accepted and unused outside ngcf, as in the reference
        self.n_layers: int = n_layers
        self.knn_k: int = knn_k
        self.cf_model: str = cf_model
        self.lr_scheduler = list(lr_scheduler)
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    @classmethod
    def param_space(cls):
        return {"lr": [0.0001, 0.0005, 0.001, 0.005], "reg": [0.0, 1e-05, 1e-04, 1e-03]}

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.embed_dim, int) and self.embed_dim > 0
        assert isinstance(self.feat_embed_dim, int) and self.feat_embed_dim > 0
        assert all(isinstance(w, int) and w > 0 for w in self.weight_size)
        assert isinstance(self.lambda_coeff, float) and 0 <= self.lambda_coeff <= 1
        assert isinstance(self.n_layers, int) and self.n_layers >= 0
        assert isinstance(self.knn_k, int) and self.knn_k > 0
        assert self.cf_model in ("lightgcn", "mf", "ngcf")
        assert len(self.lr_scheduler) == 2 and self.lr_scheduler[0] > 0 and self.lr_scheduler[1] > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config, world=1, img_dim=None, txt_dim=None):
    """raises NotImplementedError, naming the limit, for a config or a feature width this implementation does not run"""
    if config.cf_model not in CF_MODELS:
        raise NotImplementedError(f"LATTICE: cf_model in {sorted(CF_MODELS)} (got {config.cf_model!r}): ngcf is dense layers with "
                                  f"dropout, a different model")
    if config.embed_dim > 64:
        raise NotImplementedError(f"LATTICE: embed_dim <= 64 (got {config.embed_dim}): rows are 64 floats")
    if config.feat_embed_dim > 64:
        raise NotImplementedError(f"LATTICE: feat_embed_dim <= 64 (got {config.feat_embed_dim}): projected rows are 64 floats")
    if len(config.weight_size) > MAX_LAYERS:
        raise NotImplementedError(f"LATTICE: len(weight_size) <= {MAX_LAYERS} (got {len(config.weight_size)})")
    if config.n_layers > MAX_LAYERS:
        raise NotImplementedError(f"LATTICE: n_layers <= {MAX_LAYERS} (got {config.n_layers})")
    limit_batch("LATTICE", config, MAX_BATCH)
    if config.knn_k > MAX_KNN:
        raise NotImplementedError(f"LATTICE: knn_k <= {MAX_KNN} (got {config.knn_k}): skr_knn_topk keeps {MAX_KNN} neighbours per row")
    limit_features("LATTICE", MAX_FEAT, img_dim, txt_dim)
    limit_world("LATTICE", world)


def learning_rate(config, epoch):
    """the learning rate of epoch ``epoch``: LambdaLR's lr * lr_scheduler[0] ** (epoch / lr_scheduler[1]) (LATTICE.py:314-316),
    the reference's Python-float expression"""
    return lambda_lr(config.lr, config.lr_scheduler, epoch)


def init_parameters(num_users, num_items, d, feat_embed_dim, img_dim=None, txt_dim=None):
    """CPU-side draws in the reference's module order (LATTICE.py:116-165): the two nn.Embedding tables (whose own normal
    draws are consumed and overwritten by xavier-uniform), then per present modality -- image first -- nn.Linear(F,
    feat_embed_dim) with its default initialisation (``from_pretrained`` draws nothing); modal_weight = (0.5, 0.5)
    -> {name: tensor} in the reference's names, without the feature tables"""
    eu, ei = nn.Embedding(num_users, d), nn.Embedding(num_items, d)
    nn.init.xavier_uniform_(eu.weight)
    nn.init.xavier_uniform_(ei.weight)
    P = {"modal_weight": torch.tensor([0.5, 0.5]), "user_embedding.weight": eu.weight.detach().clone(),
         "item_id_embedding.weight": ei.weight.detach().clone()}
    for prefix, F in (("image", img_dim), ("text", txt_dim)):
        if F is not None:
            lin = nn.Linear(F, feat_embed_dim)
            P[prefix + "_trs.weight"], P[prefix + "_trs.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return P


def square_adjacency(rowptr, col, num_users, num_items):
    """(P, P^T) as DeviceCSR [N, N], N = U + I, from the binary train CSR in HBM: P = D^-1 (A + I), the fp32 of
    1 / (degree + 1) on every entry of a row, the diagonal included (LATTICE.py:171-193).  P is not symmetric: P^T has the
    same pattern and other values"""
    dev, nu, ni = rowptr.device, num_users, num_items
    N = nu + ni
    rowdeg = rowptr[1:] - rowptr[:-1]
    u = torch.repeat_interleave(torch.arange(nu, dtype=torch.int64, device=dev), rowdeg)
    i = col.to(torch.int64) + nu
    deg = torch.cat([rowdeg, torch.bincount(col.to(torch.int64), minlength=ni)]).to(torch.float32) + 1.0
    diag = torch.arange(N, dtype=torch.int64, device=dev)
    rows, cols = torch.cat([u, i, diag]), torch.cat([i, u, diag])
    vals = (1.0 / deg)[rows]
    return DeviceCSR.from_coo(rows, cols, vals, N), DeviceCSR.from_coo(cols, rows, vals, N)


def transpose_pattern(rowptr, col, n):
    """(rowptr_t int64, col_t int32, perm_t int32) of a square CSR pattern: the transpose by the device sort the other models
    use; perm_t[e] = the entry of the matrix that entry e of the transpose is"""
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=col.device), rowptr[1:] - rowptr[:-1])
    cols = col.to(torch.int64)
    order = torch.argsort(cols * n + rows)          # the keys are distinct: any sort gives the one order
    rowptr_t = torch.zeros(n + 1, dtype=torch.int64, device=col.device)
    rowptr_t[1:] = torch.cumsum(torch.bincount(cols, minlength=n), 0)
    return rowptr_t, rows[order].to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


class LATTICE(MultimodalRecommender):
    """limits: see ``check_limits``; ``img`` / ``txt`` (``detached``; the data set's otherwise): [num_items, F] feature tables
    or None"""
    config_class = LATTICEConfig
    check_limits = staticmethod(check_limits)
    MAX_BATCH, LOSS_LEN, pairwise = MAX_BATCH, 3, True

    def _check_modalities(self, img, txt):
        if img is None and txt is None:
            raise ValueError("LATTICE: no modality at all -- the item graph needs an image or a text feature table")

    def _build(self, rowptr, items, img=None, txt=None):
        cfg, dev = self.config, self.device
        nu, ni, d = self.num_users, self.num_items, cfg.embed_dim
        N, Ln = nu + ni, cfg.n_layers
        if cfg.knn_k > ni:
            raise ValueError(f"LATTICE: knn_k = {cfg.knn_k} neighbours of {ni} items")
        self.n_ui_layers = len(cfg.weight_size)
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t = square_adjacency(rp, col, nu, ni)
        feats = self._features(img, txt)
        P = init_parameters(nu, ni, d, cfg.feat_embed_dim, self.feat_dim["img"] or None, self.feat_dim["txt"] or None)
        # the two flat buffers
        self._flat = torch.zeros(N * 64, dtype=torch.float32, device=dev)
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)
        self._grad = self.optimizer.grad
        self.X0 = self._flat.view(N, 64)
        self._modal = ModalLayout(ni, self.feat_dim, 4)          # behind modal_weight and its padding
        self._off = self._modal.off
        self._mflat = torch.zeros(self._modal.total, dtype=torch.float32, device=dev)
        self.modal_optimizer = DenseAdam(self._mflat, lr=cfg.lr)     # one Adam in the reference; see the module's docstring
        self._mgrad = self.modal_optimizer.grad
        self._modal_grad_dirty = False
        self._version = 0              # bumped whenever a parameter may have changed
        for key, prefix in MODALITIES:
            if feats[key] is not None:
                P[prefix + "_embedding.weight"] = feats[key]
        self.load_parameters(P)
        # the frozen graphs O_m, from the initial feature tables (LATTICE.py:136-158): k entries per row, columns ascending
        self.frozen = {}
        for key, _ in MODALITIES:
            if not self.feat_dim[key]:
                continue
            tab = self._blocks(key)[1].view(ni, self.feat_ld[key])
            ids, sims = knn_topk(tab, cfg.knn_k, feat_dim=self.feat_dim[key], return_sims=True)
            (_, ocol, oval), _ = build_weighted_item_graph(ids, sims)
            self.frozen[key] = (ocol.view(ni, cfg.knn_k).contiguous(), oval.view(ni, cfg.knn_k).contiguous())
        z = lambda rows: torch.zeros((rows, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self.M, self.pooled, self._G, self._ping = z(N), z(N), z(N), (z(N), z(N))
        self._DH = torch.zeros((max(Ln, 1), ni, 64), dtype=torch.float32, device=dev)
        self._H = torch.zeros((Ln, ni, 64), dtype=torch.float32, device=dev) if Ln > 0 else None
        self._F = {key: z(ni) for key, _ in MODALITIES if self.feat_dim[key]}
        self._dF = {key: z(ni) for key, _ in MODALITIES if self.feat_dim[key]}
        cap = 4 * cfg.knn_k * ni
        self._g = torch.zeros(cap, dtype=torch.float32, device=dev)
        self._dw = torch.zeros(4, dtype=torch.float32, device=dev)
        self._work = self._new_work()
        self._bwd_work = torch.empty(0, dtype=torch.uint8, device=dev)
        self.graph = None              # the installed item graph: see rebuild_graph
        self._graph_version = None
        self._retired = []             # (event, the graph of an earlier epoch): kept until the stream has passed the event
        self.step_losses = []          # (BPR, regulariser, total) per training step, device tensors [3]

    # ---- the blocks ------------------------------------------------------------------------------
    def _modal_buffer(self, grad=False):
        """the modal blocks lie in the second buffer"""
        return self._mgrad if grad else self._mflat

    def _views(self, grad=False):
        """{name: view} in the reference's ``named_parameters()`` names, order and shapes; in the gradient, a modal tensor the
        last ``gradient_step`` did not reach reads as zeros"""
        d, fd, nu, ni = self.config.embed_dim, self.config.feat_embed_dim, self.num_users, self.num_items
        rows = self._buffer(grad).view(nu + ni, 64)
        out = {"modal_weight": self._modal_buffer(grad)[:2], "user_embedding.weight": rows[:nu, :d],
               "item_id_embedding.weight": rows[nu:, :d], **self._modal_views(grad, fd)}
        return {k: out[k] for k in NAMES if k in out}

    def _loaded(self):
        self._version += 1

    # ---- the learned graph -----------------------------------------------------------------------
    def _lists(self, learned):
        """the HOST arrays of the four lists' device addresses: (ids, values)"""
        ids, vals = (_hip.vp * 4)(), (_hip.vp * 4)()
        for m, (key, _) in enumerate(MODALITIES):
            if self.feat_dim[key]:
                ids[m], vals[m] = learned[key][0].data_ptr(), learned[key][1].data_ptr()
                ids[2 + m], vals[2 + m] = self.frozen[key][0].data_ptr(), self.frozen[key][1].data_ptr()
        return ids, vals

    def _similarities(self, F, ids):
        """the cosine similarities of row i of ``F`` with the rows ids[i] (norms clamped at 1e-12, as skr_knn_topk): the dot
        products by ``skr_lattice_sddmm`` over the pattern of the handed-in lists"""
        ni, k = ids.shape
        rowptr = torch.arange(ni + 1, dtype=torch.int64, device=self.device) * k
        dots = torch.empty(ni * k, dtype=torch.float32, device=self.device)
        _hip.check(_hip.lib().skr_lattice_sddmm(ni, ni, _hip.ptr(rowptr), _hip.ptr(ids), _hip.ptr(F), 0, _hip.ptr(F), 0, 1, None, 0,
                                                _hip.ptr(dots), _hip.stream()))
        norm = torch.linalg.vector_norm(F, dim=1).clamp_min(1e-12)
        return (dots.view(ni, k) / (norm[:, None] * norm[ids.long()])).contiguous()

    def rebuild_graph(self, knn_in=None, knn_out=None):
        """installs ``item_adj`` of the CURRENT parameters (LATTICE.py:204-228) as ``graph``: projects both tables, takes the kNN
        of the projected rows, assembles the CSR of S with ``skr_lattice_graph`` and wraps S and S^T in two new ``DeviceCSR``
        whose plans are analysed here.  ``knn_out``: a dict that receives the neighbour ids per modality ("img" / "txt", host
        arrays [I, knn_k]); ``knn_in``: such a dict whose lists are used instead of the device's own kNN, with the similarities of
        the current projected rows -- for the replay of a recorded run where an exact kNN could tie (as DENS's sel_in /
        sel_out)"""
        cfg, L, st, p = self.config, _hip.lib(), _hip.stream(), _hip.ptr
        ni, k, dev = self.num_items, cfg.knn_k, self.device
        if self.graph is not None:       # the steps that used the old pair may still be running: keep it until they have passed
            ev = torch.cuda.Event()
            ev.record()
            self._retired.append((ev, self.graph))
        self._retired = [r for r in self._retired if not r[0].query()]
        learned = {}
        for key, _ in MODALITIES:
            if not self.feat_dim[key]:
                continue
            trs, tab = self._blocks(key)
            _hip.check(L.skr_mgcn_project(p(tab), ni, self.feat_dim[key], self.feat_ld[key], p(trs), p(self._F[key]), st))
            if knn_in is not None:
                ids = self._ids(knn_in[key]).view(ni, k)
                if int(ids.min()) < 0 or int(ids.max()) >= ni:
                    raise ValueError("LATTICE: a handed-in neighbour id is outside [0, num_items)")
                learned[key] = (ids, self._similarities(self._F[key], ids))
            else:
                learned[key] = knn_topk(self._F[key], k, feat_dim=cfg.feat_embed_dim, return_sims=True)
            if knn_out is not None:
                knn_out[key] = learned[key][0].cpu().numpy()
        if all(self.present):
            w = torch.softmax(self._mflat[:2], 0).contiguous()
        else:
            w = torch.tensor([1.0 if self.present[0] else 0.0, 1.0 if self.present[1] else 0.0], dtype=torch.float32, device=dev)
        cap = 4 * k * ni
        rowptr = torch.empty(ni + 1, dtype=torch.int64, device=dev)
        col, val = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float32, device=dev)
        slots = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        r, q = torch.empty(ni, dtype=torch.float32, device=dev), torch.empty(ni, dtype=torch.float32, device=dev)
        ws = int(L.skr_lattice_graph_workspace(ni))
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        ids, vals = self._lists(learned)
        _hip.check(L.skr_lattice_graph(ni, k, ids, vals, p(w), float(cfg.lambda_coeff), p(rowptr), p(col), p(val), p(slots), p(r), p(q),
                                       p(work), ws, st))
        nnz = int(rowptr[-1].item())
        rowptr_t, col_t, perm_t = transpose_pattern(rowptr, col[:nnz], ni)
        S = DeviceCSR.from_arrays((ni, ni), rowptr, col[:nnz], val[:nnz])
        St = DeviceCSR.from_arrays((ni, ni), rowptr_t, col_t, val[:nnz][perm_t.to(torch.int64)])
        S._plan_handle()                   # the two analyses belong to the build, not to the step
        St._plan_handle()
        self.graph = dict(S=S, St=St, nnz=nnz, slots=slots, r=r, q=q, w=w, learned=learned, perm_t=perm_t, val=val)
        self._graph_version = self._version
        return self.graph

    def _current_graph(self, knn_in=None, knn_out=None):
        """the graph of the current parameters: the installed one when no parameter has changed since it was built (an
        evaluation's graph serves the next epoch's build step: the build is bit-reproducible), a new one otherwise, and
        whenever neighbour lists are handed in or asked for"""
        if self.graph is None or self._graph_version != self._version or knn_in is not None or knn_out is not None:
            self.rebuild_graph(knn_in, knn_out)
        return self.graph

    # ---- training --------------------------------------------------------------------------------
    def gradient_step(self, users, pos, neg, build=False, h_ms=None, knn_in=None, knn_out=None):
        """forward and backward of one batch without the optimisers: the rows' gradient is left in the first optimiser's
        gradient buffer, every element written.  ``build``: the item graph is that of the current parameters and the gradient
        reaches the modal tensors, written into the second optimiser's gradient buffer; otherwise the installed graph is a
        constant and that buffer reads as zeros -> device tensor (BPR, regulariser, total).  ``h_ms``: a ctypes float array of
        SKR_LATTICE_GROUPS entries that receives the milliseconds of each launch group of the step; ``knn_in`` / ``knn_out``
        (build steps): see ``rebuild_graph``"""
        return self._gradient_step((users, pos, neg), h_ms, build=build, knn_in=knn_in, knn_out=knn_out)

    def _before_step(self):
        if self._modal_grad_dirty:
            self._mgrad.zero_()
            self._modal_grad_dirty = False

    def _workspace(self, n):
        return int(_hip.lib().skr_lattice_workspace(n, self.num_items))

    def _make_args(self, ids, loss, build=False, knn_in=None, knn_out=None):
        cfg, p, (du, dp, dn) = self.config, _hip.ptr, ids
        n, Ln, ni = int(du.numel()), cfg.n_layers, self.num_items
        build = bool(build) and Ln > 0
        G = None
        if Ln > 0:
            G = self._current_graph(knn_in, knn_out) if build or self.graph is None else self.graph
        self._built = G if build else None         # the graph that ``_after_step`` carries the gradient through
        a = _hip.LatticeStepArgs()
        if self.n_ui_layers > 0 and cfg.cf_model == "lightgcn":
            a.plan_p, a.plan_pt = self.adj._plan_handle(), self.adj_t._plan_handle()
        if Ln > 0:
            a.plan_s, a.plan_st = G["S"]._plan_handle(), G["St"]._plan_handle()
        a.n_users, a.n_items, a.dim, a.n_ui_layers, a.n_layers = self.num_users, ni, cfg.embed_dim, self.n_ui_layers, Ln
        a.cf_model, a.n, a.reg = CF_MODELS[cfg.cf_model], n, cfg.reg
        a.params, a.users, a.pos, a.neg = p(self._flat), p(du), p(dp), p(dn)
        a.M, a.G, a.DH, a.grad, a.loss = p(self.M), p(self._G), p(self._DH), p(self._grad), p(loss)
        a.ping[0], a.ping[1] = p(self._ping[0]), p(self._ping[1])
        if build:
            a.H, a.g_out, a.s_rowptr, a.s_col = p(self._H), p(self._g), p(G["S"].rowptr), p(G["S"].col)
        a.work, a.work_bytes = p(self._work), self._work.numel()
        return a

    def _after_step(self, ids):
        if self._built is not None:
            self.graph_backward(self._built)

    def graph_backward(self, G):
        """from ``dLoss/dS`` (left in ``_g`` by a build step) to the modal gradient buffer: ``skr_lattice_graph_bwd`` to the
        projected rows and the two softmax logits, ``skr_mgcn_project_bwd`` to the projections and the feature tables"""
        cfg, L, st, p = self.config, _hip.lib(), _hip.stream(), _hip.ptr
        ni, k, nnz = self.num_items, cfg.knn_k, G["nnz"]
        ws = int(L.skr_lattice_graph_bwd_workspace(ni, nnz))
        if ws > self._bwd_work.numel():
            self._bwd_work = torch.empty(ws, dtype=torch.uint8, device=self.device)
        ids, vals = self._lists(G["learned"])
        F, dF = (_hip.vp * 2)(), (_hip.vp * 2)()
        for m, (key, _) in enumerate(MODALITIES):
            if self.feat_dim[key]:
                F[m], dF[m] = self._F[key].data_ptr(), self._dF[key].data_ptr()
        S, St = G["S"], G["St"]
        _hip.check(L.skr_lattice_graph_bwd(ni, k, nnz, p(self._g), p(S.rowptr), p(S.col), p(G["slots"]), p(St.rowptr), p(St.col),
                                           p(G["perm_t"]), ids, vals, p(G["w"]), float(cfg.lambda_coeff), p(G["q"]), F, dF, p(self._dw),
                                           p(self._bwd_work), self._bwd_work.numel(), st))
        if all(self.present):
            self._mgrad[:2].copy_(self._dw[2:])
        for key, _ in MODALITIES:
            if not self.feat_dim[key]:
                continue
            (trs, tab), (gtrs, gtab) = self._blocks(key), self._blocks(key, True)
            ld = self.feat_ld[key]
            ws = int(L.skr_mgcn_project_bwd_workspace(ni, ld))
            if ws > self._bwd_work.numel():
                self._bwd_work = torch.empty(ws, dtype=torch.uint8, device=self.device)
            _hip.check(L.skr_mgcn_project_bwd(p(self._dF[key]), p(tab), ni, self.feat_dim[key], ld, p(trs), p(gtrs), p(gtab),
                                              p(self._bwd_work), self._bwd_work.numel(), st))
        self._modal_grad_dirty = True

    def _after_optimizer(self, build=False, **kw):
        """``train_step(..., build=True)``: the first step of an epoch (LATTICE.py:168-169, 285-286)"""
        if build and self.config.n_layers > 0:     # torch's Adam skips a tensor without a gradient: the modal block moves on build steps only
            self.modal_optimizer.step()
            self._modal_grad_dirty = False     # the Adam launch zeroes the gradient it has read
        self._version += 1

    def _optimizers(self):
        return self.optimizer, self.modal_optimizer

    def _run_epoch(self, data_iter, epoch):
        self.set_epoch(epoch)
        self.step_losses = []
        for s, batch in enumerate(self._batches(data_iter, epoch)):
            self.train_step(*batch, build=s == 0)

    # ---- ranking: the base class's, on the two factor tables (LATTICE.py:296-302) -------------------
    def propagate(self):
        """the full forward of the CURRENT parameters, the graph rebuilt from them (LATTICE.py:297) -> pooled"""
        cfg, nu, ni, Ln = self.config, self.num_users, self.num_items, self.config.n_layers
        Lu = self.n_ui_layers if cfg.cf_model == "lightgcn" else 0
        if Lu == 0:
            self.pooled.copy_(self.X0)
        X, s = self.X0, 1.0 / (Lu + 1)
        for k in range(1, Lu + 1):
            Y = None if k == Lu else self._ping[(k - 1) & 1]
            run_plan(self.adj, X, Y=Y, accum=self.pooled, accum_base=self.X0 if k == 1 else None, accum_scale=s)
            X = Y
        h = self.X0[nu:]
        if Ln > 0:
            G = self._current_graph()
            for k in range(1, Ln + 1):
                Y = self._ping[(k - 1) & 1][:ni]
                run_plan(G["S"], h, Y=Y)
                h = Y
        _hip.check(_hip.lib().skr_lattice_add_normalized(_hip.ptr(h), ni, _hip.ptr(self.pooled[nu:]), _hip.stream()))
        return self.pooled

    def _factors(self):
        """(out_u [U, 64], out_i [I, 64], None) of the last ``propagate()``"""
        return self.pooled[:self.num_users], self.pooled[self.num_users:], None
