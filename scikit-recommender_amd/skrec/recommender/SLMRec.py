"""SLMRec on MI355X (reference: skrec/recommender/SLMRec.py).

Paper: Self-supervised Learning for Multimedia Recommendation (Tao, Liu, Xia, Wang, Yang, Huang and Chua, TMM 2022).  Same
config, same initialisation, same loss, in the one configuration in which the reference itself runs: ``ssl_task="FAC"``,
``mm_fusion_mode="concat"``, ``adj_type="pre"``, ``init="xavier"``, both modalities (SLMRec.py:132-177, 337-362, 423-432).  The
two feature tables are CONSTANTS, row-normalised once at construction; ``v_dense`` / ``t_dense`` project them to ``rec_dim``
columns over all items; the id table and the two projected tables are each propagated ``layer_num`` times over the user-item
graph with the user embeddings on top, and the layer mean is kept; two ``Linear(3 d, d)`` layers fuse the three means into the
user and the item representation.  The loss is a cosine InfoNCE between the batch's users and items (``temp``) plus
``ssl_alpha`` times two un-normalised InfoNCE terms (``ssl_temp``) through the five ``g_*`` layers of the "fine and coarse"
task.  ``g_a_iva`` is drawn and kept and never gets a gradient; ``reg``, ``weight_decay`` and ``dropout_rate`` are accepted
and unused, as in the reference.

One training step is ``skr_slmrec_step`` (csrc/slmrec.hip) and one dense Adam launch over the trained part of the flat buffer

    [U + I, 64] rows | v_dense: W [64, ld] | b 64 | t_dense: the same | embedding_item_after_GCN: W [64, 192] | b 64
    | embedding_user_after_GCN | g_i_iv | g_v_iv | g_iv_iva | g_iva_ivat | g_t_ivat    || g_a_iva (outside the optimiser)

(chain blocks: W [64, 64] | b 64; ld = the feature width rounded up to 4).  The fusion runs at the batch's rows only in
training.  The learning rate follows the reference's ``LambdaLR`` with its fixed ``lr_scheduler = [1.0, 50]``: constant, the
expression kept.

Ranking: the reference ranks on the ``all_users`` / ``all_items`` of the LAST TRAINING FORWARD, that is with the parameters
before the last Adam update (SLMRec.py:366-376).  The step leaves the three propagated tables; the two fusion blocks are copied
to a snapshot before each Adam launch; ``propagate()`` fuses the kept tables with the snapshot over all rows
(``skr_slmrec_fuse``) into two plain factor tables for the fused top-K path.  Before any step it runs a forward of the current
parameters.  ``predict()`` returns the sigmoid of the scores, as the reference does; the fused path ranks on the raw products.

Limits (NotImplementedError): the branches the reference itself cannot run (``check_limits`` names each), rec_dim <= 64,
layer_num <= 4, batch_size <= 2048, 1 <= F <= 4096 per modality, one GPU.  ValueError: a missing modality.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import ModelConfig
from ._graph import _adjacency, run_plan, upload_csr
from ._multimodal import ModalLayout, MultimodalRecommender, lambda_lr, limit_batch, limit_features, limit_world
from .base import DenseAdam

__all__ = ["SLMRec", "SLMRecConfig"]

MAX_BATCH, MAX_LAYERS, MAX_FEAT = _hip.SKR_SLMREC_MAX_BATCH, _hip.SKR_SLMREC_MAX_LAYERS, _hip.SKR_SLMREC_MAX_FEAT
GATE, FUSION = _hip.SKR_SLMREC_GATE_FLOATS, _hip.SKR_SLMREC_FUSION_FLOATS
MODALITIES = (("img", "v_dense", "image"), ("txt", "t_dense", "text"))
FUSIONS = ("embedding_item_after_GCN", "embedding_user_after_GCN")          # adjacent in the buffer: one snapshot copy
CHAIN = ("g_i_iv", "g_v_iv", "g_iv_iva", "g_iva_ivat", "g_t_ivat")          # the order of skr_slmrec_step_args.chain
HALF = ("g_iva_ivat", "g_t_ivat")                                          # Linear(d, d // 2)
LINEARS = ("v_dense", "t_dense") + FUSIONS + ("g_i_iv", "g_v_iv", "g_iv_iva", "g_a_iva", "g_iva_ivat", "g_t_ivat")
NAMES = ("embedding_user.weight", "embedding_item.weight") + tuple(f"{m}.{p}" for m in LINEARS for p in ("weight", "bias"))
UNTRAINED = ("g_a_iva.weight", "g_a_iva.bias")
LR_SCHEDULER = (1.0, 50)       # SLMRec.py:545


class SLMRecConfig(ModelConfig):
    def __init__(self, lr=1e-4, reg=1e-4, rec_dim=64, layer_num=3, ssl_alpha=0.01, ssl_temp=0.1, dropout_rate=0.3, temp=0.2,
                 weight_decay=1e-4, mm_fusion_mode="concat", adj_type="pre", ssl_task="FAC", init="xavier", batch_size=2048, epochs=1000,
                 early_stop=200, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg                        # accepted and unused, as in the reference
        self.rec_dim: int = rec_dim
        self.layer_num: int = layer_num
        self.ssl_alpha: float = ssl_alpha
        self.ssl_temp: float = ssl_temp
        self.dropout_rate: float = dropout_rate      # of the FD / FM tasks, which the reference cannot run
        self.temp: float = temp
        self.weight_decay: float = weight_decay      # accepted and unused, as in the reference
        self.mm_fusion_mode: str = mm_fusion_mode
        self.adj_type: str = adj_type
        self.ssl_task: str = ssl_task
        self.init: str = init
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    @classmethod
    def param_space(cls):
        return {"lr": [0.0001, 0.001, 0.01, 0.1], "ssl_temp": [0.1, 0.2, 0.5, 1.0], "ssl_alpha": [0.01, 0.05, 0.1, 0.5, 1.0],
                "reg": [0.0001, 0.001, 0.01, 0.1]}

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.rec_dim, int) and self.rec_dim > 0
        assert isinstance(self.layer_num, int) and self.layer_num >= 0
        assert isinstance(self.ssl_alpha, float) and self.ssl_alpha >= 0
        assert isinstance(self.ssl_temp, float) and self.ssl_temp > 0
        assert isinstance(self.temp, float) and self.temp > 0
        assert isinstance(self.weight_decay, float) and self.weight_decay >= 0
        assert all(isinstance(s, str) for s in (self.mm_fusion_mode, self.adj_type, self.ssl_task, self.init))
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config, world=1, img_dim=None, txt_dim=None, data_name=None):
    """raises NotImplementedError, naming the field and the reason, for a config, a data set or a feature width this
    implementation does not run; the first four are the branches that fail inside the reference itself"""
    if config.ssl_task != "FAC":
        raise NotImplementedError(f"SLMRec: ssl_task = {config.ssl_task!r}: only 'FAC' runs -- the reference's FD / FM / FD+FM tasks read "
                                  f"self.a_dense_emb, which never exists (SLMRec.py:185)")
    if config.mm_fusion_mode != "concat":
        raise NotImplementedError(f"SLMRec: mm_fusion_mode = {config.mm_fusion_mode!r}: only 'concat' runs -- the reference's 'mean' feeds "
                                  f"d columns into Linear(3 d, d) (SLMRec.py:420, 483)")
    if config.init != "xavier":
        raise NotImplementedError(f"SLMRec: init = {config.init!r}: only 'xavier' runs -- the reference's 'normal' names embedding_item_ID, "
                                  f"which does not exist (SLMRec.py:443)")
    if config.adj_type != "pre":
        raise NotImplementedError(f"SLMRec: adj_type = {config.adj_type!r}: only the 'pre' adjacency D^-1/2 A D^-1/2 is built")
    if data_name == "kwai":
        raise NotImplementedError("SLMRec: the data set 'kwai' selects the reference's two-table branch (no text features), which is not built")
    if config.rec_dim > 64:
        raise NotImplementedError(f"SLMRec: rec_dim <= 64 (got {config.rec_dim}): rows are 64 floats")
    if config.layer_num > MAX_LAYERS:
        raise NotImplementedError(f"SLMRec: layer_num <= {MAX_LAYERS} (got {config.layer_num})")
    limit_batch("SLMRec", config, MAX_BATCH)
    limit_features("SLMRec", MAX_FEAT, img_dim, txt_dim)
    limit_world("SLMRec", world)


def learning_rate(config, epoch):
    """the learning rate of epoch ``epoch``: LambdaLR's lr * lr_scheduler[0] ** (epoch / lr_scheduler[1]) with the reference's
    fixed lr_scheduler = [1.0, 50] (SLMRec.py:545-547) -- constant; the reference's Python-float expression"""
    return lambda_lr(config.lr, LR_SCHEDULER, epoch)


def init_parameters(num_users, num_items, d, img_dim, txt_dim):
    """CPU-side draws in the reference's module order (SLMRec.py:106-119, 434-486): the two nn.Embedding tables (both drawn, then
    both overwritten by xavier-uniform), v_dense, t_dense (each: nn.Linear's draws, then xavier on the weight), the two fusion
    layers (item first; both drawn, then xavier item, xavier user), the six g_* layers (all drawn, then six xaviers) ->
    {name: tensor} in the reference's names; g_a_iva among them"""
    eu, ei = nn.Embedding(num_users, d), nn.Embedding(num_items, d)
    nn.init.xavier_uniform_(eu.weight, gain=1)
    nn.init.xavier_uniform_(ei.weight, gain=1)
    mods = {}
    for name, F in (("v_dense", img_dim), ("t_dense", txt_dim)):
        mods[name] = nn.Linear(F, d)
        nn.init.xavier_uniform_(mods[name].weight)
    mods["embedding_item_after_GCN"], mods["embedding_user_after_GCN"] = nn.Linear(3 * d, d), nn.Linear(3 * d, d)
    nn.init.xavier_uniform_(mods["embedding_item_after_GCN"].weight)
    nn.init.xavier_uniform_(mods["embedding_user_after_GCN"].weight)
    chain = ("g_i_iv", "g_v_iv", "g_iv_iva", "g_a_iva", "g_iva_ivat", "g_t_ivat")
    for name in chain:
        mods[name] = nn.Linear(d, d // 2 if name in HALF else d)
    for name in chain:
        nn.init.xavier_uniform_(mods[name].weight)
    P = {"embedding_user.weight": eu.weight, "embedding_item.weight": ei.weight}
    for name in LINEARS:
        P[name + ".weight"], P[name + ".bias"] = mods[name].weight, mods[name].bias
    return {k: P[k].detach().clone() for k in NAMES}


def inverse_root_degrees(deg):
    """(deg + 1e-8) ** -0.5 in fp32 on the host, the reference's numpy expression (SLMRec.py:520-521): a node without an entry
    gets 1e4, never inf"""
    return np.power(np.asarray(deg).astype(np.float32) + np.float32(1e-08), np.float32(-0.5))


def adjacency_values(rowptr, items, num_items):
    """the 'pre' adjacency's values at the binary train CSR's entries, on the host, bit for bit the reference's: the fp32 factors
    of ``inverse_root_degrees`` multiplied left then right (SLMRec.py:525-526)"""
    rowptr, items = np.asarray(rowptr, np.int64), np.asarray(items, np.int64)
    du, di = inverse_root_degrees(np.diff(rowptr)), inverse_root_degrees(np.bincount(items, minlength=num_items))
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return (du[rows] * di[items]).astype(np.float32)


def slmrec_adjacency(rowptr, col, num_users, num_items):
    """(R, R^T) as DeviceCSR from the binary train CSR in HBM with ``adjacency_values``' values: the two factor tables are
    computed on the host (U + I floats) so that they are the reference's bits; the fp32 product is the same anywhere"""
    def value(rowdeg, coldeg, rows, cols):
        du, di = (torch.from_numpy(inverse_root_degrees(x.cpu().numpy())).to(rows.device) for x in (rowdeg, coldeg))
        return du[rows] * di[cols]
    return _adjacency(rowptr, col, num_users, num_items, value, False)[:2]


class SLMRec(MultimodalRecommender):
    """limits: see ``check_limits``; ``img`` / ``txt`` (``detached``; the data set's otherwise): [num_items, F] feature tables,
    both required, normalised here"""
    config_class = SLMRecConfig
    check_limits = staticmethod(check_limits)
    MAX_BATCH, LOSS_LEN, required, lr_scheduler = MAX_BATCH, 4, True, LR_SCHEDULER

    def _build_args(self, run_config):
        check_limits(self.config, 1, data_name=getattr(self.dataset, "data_name", None))
        return MultimodalRecommender._build_args(self, run_config)

    def _build(self, rowptr, items, img=None, txt=None):
        cfg, dev = self.config, self.device
        nu, ni, d = self.num_users, self.num_items, cfg.rec_dim
        N = nu + ni
        rp, col = upload_csr(rowptr, items, dev)
        assert rp.numel() == nu + 1
        self.adj, self.adj_t = slmrec_adjacency(rp, col, nu, ni)
        feats = self._features(img, txt)
        self.feat = {}
        for key, v in feats.items():           # the constant tables [I, ld], row-normalised once (SLMRec.py:448, 453: eps 1e-12), zero beyond F
            tab = torch.zeros((ni, self.feat_ld[key]), dtype=torch.float32, device=dev)
            tab[:, :self.feat_dim[key]] = torch.nn.functional.normalize(v, dim=1).to(dev)
            self.feat[key] = tab
        # the flat buffer: the trained part, then g_a_iva
        self._modal = ModalLayout(ni, self.feat_dim, N * 64, tables=False)
        self._off, o = {name: (self._modal.off[key][0], 64 * self.feat_ld[key] + 64) for key, name, _ in MODALITIES}, self._modal.total
        for name in FUSIONS:
            self._off[name] = (o, FUSION)
            o += FUSION
        for name in CHAIN:
            self._off[name] = (o, GATE)
            o += GATE
        self._trained = o
        self._off["g_a_iva"] = (o, GATE)
        self._flat = torch.zeros(o + GATE, dtype=torch.float32, device=dev)
        self.optimizer = DenseAdam(self._flat[:self._trained], lr=cfg.lr)          # Adam(lr) skips g_a_iva: it has no gradient
        self._grad = self.optimizer.grad
        self.X0 = self._flat[:N * 64].view(N, 64)
        fo = self._off[FUSIONS[0]][0]
        self._fusion = self._flat[fo:fo + 2 * FUSION]
        self._fusion_snapshot = torch.zeros_like(self._fusion)          # the fusion blocks of the last training forward
        self.load_parameters(init_parameters(nu, ni, d, self.feat_dim["img"], self.feat_dim["txt"]))
        z = lambda rows: torch.zeros((rows, 64), dtype=torch.float32, device=dev)        # noqa: E731
        self.M, self.pooled = (z(N), z(N), z(N)), z(N)
        self._D, self._dD = (z(ni), z(ni)), z(ni)
        self._G, self._ping = (z(N), z(N), z(N)), (z(N), z(N))
        self._ld_max = max(self.feat_ld.values())
        self._work = self._new_work()
        self.step_losses = []          # (main, ssl_alpha v_loss, ssl_alpha t_loss, total) per training step, device tensors [4]

    # ---- the blocks ------------------------------------------------------------------------------
    def _block(self, name, grad=False):
        o, size = self._off[name]
        assert not (grad and name == "g_a_iva"), "g_a_iva has no gradient"
        return self._buffer(grad)[o:o + size]

    def _views(self, grad=False):
        """{name: view}: the reference's names and order; a fusion weight as [d, 3, d] (the reference's [d, 3 d] split by table)"""
        d, nu, ni = self.config.rec_dim, self.num_users, self.num_items
        rows = self._buffer(grad)[:(nu + ni) * 64].view(nu + ni, 64)
        out = {"embedding_user.weight": rows[:nu, :d], "embedding_item.weight": rows[nu:, :d]}
        for key, name, _ in MODALITIES:
            out[name + ".weight"], out[name + ".bias"] = self._modal.linear(self._block(name, grad), key, d)
        for name in FUSIONS:
            b = self._block(name, grad)
            out[name + ".weight"], out[name + ".bias"] = b[:64 * 192].view(64, 3, 64)[:d, :, :d], b[64 * 192:64 * 192 + d]
        for name in CHAIN + (() if grad else ("g_a_iva",)):
            b, do = self._block(name, grad), d // 2 if name in HALF else d
            out[name + ".weight"], out[name + ".bias"] = b[:4096].view(64, 64)[:do, :d], b[4096:4096 + do]
        return {k: out[k] for k in NAMES if k in out}

    def _to_reference(self, v):
        """a fusion weight as the reference's [d, 3 d]; ``gradients()`` has no g_a_iva"""
        d = self.config.rec_dim
        return (v.reshape(d, 3 * d) if v.dim() == 3 else v.contiguous()).clone()

    def _from_reference(self, t, view):
        return t.reshape(view.shape)

    def _loaded(self):
        self._forward_current = False

    # ---- training --------------------------------------------------------------------------------
    def _workspace(self, n):
        return int(_hip.lib().skr_slmrec_workspace(n, self.num_items, self._ld_max))

    def _step_args(self, du, dp, loss):
        """skr_slmrec_step_args of one batch (int32 device tensors) on this model's buffers"""
        cfg = self.config
        a, p = _hip.SLMRecStepArgs(), _hip.ptr
        a.plan_a, a.plan_at = self.adj._plan_handle(), self.adj_t._plan_handle()
        a.n_users, a.n_items, a.dim, a.n_layers, a.n = self.num_users, self.num_items, cfg.rec_dim, cfg.layer_num, int(du.numel())
        a.temp, a.ssl_temp, a.ssl_alpha = cfg.temp, cfg.ssl_temp, cfg.ssl_alpha
        a.params, a.grad = p(self._flat), p(self._grad)
        for m, (key, name, _) in enumerate(MODALITIES):
            a.feat_dim[m], a.feat_ld[m] = self.feat_dim[key], self.feat_ld[key]
            a.dense[m], a.dense_grad[m], a.feat[m], a.D[m] = p(self._block(name)), p(self._block(name, True)), p(self.feat[key]), p(self._D[m])
            a.ping[m] = p(self._ping[m])
        a.fusion_item, a.fusion_item_grad = p(self._block(FUSIONS[0])), p(self._block(FUSIONS[0], True))
        a.fusion_user, a.fusion_user_grad = p(self._block(FUSIONS[1])), p(self._block(FUSIONS[1], True))
        for c, name in enumerate(CHAIN):
            a.chain[c], a.chain_grad[c] = p(self._block(name)), p(self._block(name, True))
        a.users, a.pos = p(du), p(dp)
        for t in range(3):
            a.M[t], a.G[t] = p(self.M[t]), p(self._G[t])
        a.dD, a.loss = p(self._dD), p(loss)
        a.work, a.work_bytes = p(self._work), self._work.numel()
        return a

    def gradient_step(self, users, pos, h_ms=None):
        """forward and backward of one batch without the optimiser: the gradient is left in the optimiser's gradient buffer,
        every element written, the three propagated tables in ``self.M`` -> device tensor (main, ssl_alpha v_loss, ssl_alpha
        t_loss, total).  ``h_ms``: a ctypes float array of SKR_SLMREC_GROUPS entries that receives the milliseconds of each
        launch group"""
        return self._gradient_step((users, pos), h_ms)

    def _after_step(self, ids):
        """the fusion blocks are copied to the snapshot before the Adam launch of ``train_step``"""
        self._fusion_snapshot.copy_(self._fusion)          # M and the snapshot: the forward the reference ranks on
        self._forward_current = True

    # ---- ranking (SLMRec.py:366-376) ----------------------------------------------------------------
    def _mean(self, Xi0, M):
        """M = mean_{k=0..L} A^k [E_u; Xi0]: ``propagate_mean`` with the item rows in a buffer of their own"""
        nu, L = self.num_users, self.config.layer_num
        Xu0 = self.X0[:nu]
        if L == 0:
            M[:nu].copy_(Xu0)
            M[nu:].copy_(Xi0)
            return
        s, Xu, Xi = 1.0 / (L + 1), Xu0, Xi0
        for k in range(1, L + 1):
            Y = None if k == L else self._ping[(k - 1) & 1]
            Yu, Yi = (None, None) if Y is None else (Y[:nu], Y[nu:])
            run_plan(self.adj, Xi, Y=Yu, accum=M[:nu], accum_base=Xu0 if k == 1 else None, accum_scale=s)
            run_plan(self.adj_t, Xu, Y=Yi, accum=M[nu:], accum_base=Xi0 if k == 1 else None, accum_scale=s)
            Xu, Xi = Yu, Yi

    def forward_tables(self):
        """the forward of the CURRENT parameters over all rows (SLMRec.py:132-165): the three propagated tables into ``self.M``,
        the current fusion blocks into the snapshot"""
        L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
        for m, (key, name, _) in enumerate(MODALITIES):
            _hip.check(L.skr_mgcn_project(p(self.feat[key]), self.num_items, self.feat_dim[key], self.feat_ld[key], p(self._block(name)),
                                          p(self._D[m]), st))
        self._mean(self.X0[self.num_users:], self.M[0])
        self._mean(self._D[0], self.M[1])
        self._mean(self._D[1], self.M[2])
        self._fusion_snapshot.copy_(self._fusion)
        self._forward_current = True

    def propagate(self):
        """all_users | all_items of the last training forward: the kept tables fused with the snapshot's blocks over all rows ->
        pooled; before any step (or after ``load_parameters``) a forward of the current parameters first"""
        if not getattr(self, "_forward_current", False):
            self.forward_tables()
        L, st, p, nu, ni = _hip.lib(), _hip.stream(), _hip.ptr, self.num_users, self.num_items
        for rows, blk in ((slice(nu, nu + ni), self._fusion_snapshot[:FUSION]), (slice(0, nu), self._fusion_snapshot[FUSION:])):
            _hip.check(L.skr_slmrec_fuse(p(self.M[0][rows]), p(self.M[1][rows]), p(self.M[2][rows]), p(blk), rows.stop - rows.start,
                                         self.config.rec_dim, p(self.pooled[rows]), st))
        return self.pooled

    def raw_scores(self, users):
        """dense [len(users), num_items] scores before the sigmoid"""
        uf, vf, bias = self.predict_factors()
        return _hip.score_matrix(uf, list(users), vf, bias)

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] sigmoid(scores), as the reference returns them (SLMRec.py:370); the fused top-K path ranks
        on the raw products, which order the items alike wherever fp32's sigmoid keeps two scores apart"""
        return torch.sigmoid(self.raw_scores(users)).cpu().numpy()
