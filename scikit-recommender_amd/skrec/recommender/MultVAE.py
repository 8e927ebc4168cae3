"""MultVAE on MI355X (reference: skrec/recommender/MultVAE.py).

Paper: Variational Autoencoders for Collaborative Filtering (Liang, Krishnan, Hoffman and Jebara).
Same config, same initialisation (the two ``nn.Linear`` constructors draw from the CPU generator, then
``reset_parameters`` re-draws normal(0, 0.01) in the order encoder weight, encoder bias, decoder weight, decoder bias;
MultVAE.py:64-97), same loss (multinomial log-likelihood over the whole catalogue + anneal * KL + 2 * reg * l2_loss of
the two weights, MultVAE.py:187-197), same optimiser: the reference's dense ``torch.optim.Adam`` over the four
parameters, where the l2 term's gradient 2 * reg * W is ``weight_decay = 2 * reg`` on the weights and nothing on the
biases.  One training step is ``skr_multvae_step`` (csrc/multvae.hip: the decoder's logits, softmax and three gradient
products tile by tile on the fp32 matrix pipe, no [B, I] array) and one dense Adam launch per flat buffer:
[WqT | Wp] with the weight decay, [bq | bp] plain.

Layout: the encoder weight is kept transposed, WqT [I, 128] (an item's row: 64 mu columns then 64 logvar columns, each
half zero-padded beyond d); Wp [I, 64] lies as the evaluator's fused top-K path ranks it.  Padded columns stay exactly
zero through training.

Scoring collapses to one query row per user, Q[u] = mu_u (no dropout, z = mu): score = <Q[u], Wp[i]> + bp[i].  The rows
are computed once per evaluation (``skr_multvae_queries``) and kept until the next training step.  A user without a
training item gets mu = bq and is ranked like anyone else, as in the reference.

Draws: ``train_step`` takes the dropout keep flags and the latent noise when handed them (the tests replay the
reference's); otherwise the step draws on the device from a generator keyed by (seed, step, user, item) and (seed,
step, user, column) -- the splitmix / xoshiro pieces of the fast sampler -- so a user's draws do not depend on the rest
of the batch.  Device draws equal the reference's torch draws in law only.

Limits: p_dims == [d] with d <= 64, q_dims None or [d], batch_size <= 1024, one GPU.
"""
from typing import List

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import BatchIterator, ModelConfig
from ..utils.torch import get_initializer
from ._graph import train_csr, upload_csr
from .base import DenseAdam, DeviceRecommender, on_compute_stream

__all__ = ["MultVAE", "MultVAEConfig"]


class MultVAEConfig(ModelConfig):
    def __init__(self, lr=1e-3, reg=0.0, p_dims=[64], q_dims=None, keep_prob=0.5, anneal_steps=200000, anneal_cap=0.2,
                 batch_size=256, epochs=1000, early_stop=200, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.p_dims: List[int] = p_dims
        self.q_dims: List[int] = q_dims
        self.keep_prob: float = keep_prob
        self.anneal_steps: int = anneal_steps
        self.anneal_cap: float = anneal_cap
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.p_dims, list)
        assert self.q_dims is None or isinstance(self.q_dims, list)
        assert isinstance(self.keep_prob, float) and self.keep_prob >= 0
        assert isinstance(self.anneal_steps, int) and self.anneal_steps >= 0
        assert isinstance(self.anneal_cap, float) and self.anneal_cap >= 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config):
    """the latent width d of a config this implementation runs; raises outside the limits"""
    p, q = config.p_dims, config.q_dims
    if len(p) != 1:
        raise NotImplementedError(f"MultVAE: p_dims == [d] (got {p}): one decoder layer, the fused step has no hidden layer")
    d = int(p[0])
    if not 1 <= d <= 64:
        raise NotImplementedError(f"MultVAE: p_dims == [d] with d <= 64 (got {d}): rows are 64 floats and the fused "
                                  f"evaluator ranks 64 columns")
    if q is not None and [int(x) for x in q] != [d]:
        raise NotImplementedError(f"MultVAE: q_dims in (None, [{d}]) (got {q}): one encoder layer")
    if config.batch_size > _hip.SKR_MULTVAE_MAX_BATCH:
        raise ValueError(f"MultVAE: batch_size <= {_hip.SKR_MULTVAE_MAX_BATCH} (got {config.batch_size}): skr_multvae_step "
                         f"takes that many users")
    if not 0.0 < config.keep_prob <= 1.0:
        raise ValueError(f"MultVAE: 0 < keep_prob <= 1 (got {config.keep_prob})")
    return d


def _init_tables(num_items, d):
    """CPU-side construction in the reference's order (_MultVAE.__init__ / reset_parameters, MultVAE.py:64-97):
    -> Wq [2d, I], bq [2d], Wp [I, d], bp [I]"""
    lq = nn.Linear(num_items, 2 * d, bias=True)
    lp = nn.Linear(d, num_items, bias=True)
    normal = get_initializer("normal")
    normal(lq.weight)
    normal(lq.bias)
    normal(lp.weight)
    normal(lp.bias)
    return tuple(t.detach() for t in (lq.weight, lq.bias, lp.weight, lp.bias))


class MultVAE(DeviceRecommender):
    """limits: p_dims == [d] with d <= 64 and q_dims in (None, [d]) (NotImplementedError), batch_size <= 1024 (ValueError),
    one GPU.  ``seed`` (``detached``; the run's seed otherwise): the key of the device draws"""
    config_class = MultVAEConfig

    def _check_limits(self, world):
        check_limits(self.config)
        if world > 1:
            raise NotImplementedError("MultVAE runs on one GPU: there is no sharded engine for it")

    def _train_inputs(self):
        return train_csr(self.dataset)

    def _build_args(self, run_config):
        return {"seed": getattr(run_config, "seed", 0) or 0}

    def _build(self, rowptr, items, seed=0):
        cfg = self.config
        d, nu, ni = check_limits(cfg), self.num_users, self.num_items
        self.d = d
        self.seed = int(seed)
        self._rowptr, self._items = upload_csr(rowptr, items, self.device)
        self._rowptr_host = self._rowptr.cpu().numpy() if torch.is_tensor(rowptr) else np.ascontiguousarray(rowptr, dtype=np.int64)
        assert self._rowptr_host.shape[0] == nu + 1
        Wq, bq, Wp, bp = _init_tables(ni, d)
        pad = lambda t: nn.functional.pad(t, (0, 64 - d))              # noqa: E731
        WqT = Wq.t().contiguous()                                      # [I, 2d]
        wqt = torch.cat([pad(WqT[:, :d]), pad(WqT[:, d:])], dim=1)     # [I, 128]
        nb = 64 * ((ni + 63) // 64)                                    # bp, zero-padded to whole 64-float blocks
        weights = torch.cat([wqt.reshape(-1), pad(Wp).reshape(-1)])
        biases = torch.cat([pad(bq[:d]), pad(bq[d:]), nn.functional.pad(bp, (0, nb - ni))])
        self._weights = weights.to(self.device).contiguous()
        self._biases = biases.to(self.device).contiguous()
        # the l2 term 2 * reg * 0.5 * sum(W^2) of the two weights (MultVAE.py:192-197) as the optimiser's weight decay
        self.opt_w = DenseAdam(self._weights, lr=cfg.lr, weight_decay=2.0 * cfg.reg)
        self.opt_b = DenseAdam(self._biases, lr=cfg.lr)
        w, b = self._weights, self._biases
        self._wqt, self._wp = w[:ni * 128].view(ni, 128), w[ni * 128:].view(ni, 64)
        self._bq, self._bp = b[:128], b[128:128 + ni]
        self._grads = (self.opt_w.grad_view(0, (ni, 128)), self.opt_b.grad_view(0, (128,)),
                       self.opt_w.grad_view(ni * 128, (ni, 64)), self.opt_b.grad_view(128, (ni,)))
        self._work_bytes = int(_hip.lib().skr_multvae_workspace(min(cfg.batch_size, _hip.SKR_MULTVAE_MAX_BATCH), ni))
        self._work = torch.empty(self._work_bytes, dtype=torch.uint8, device=self.device)
        self._Q = torch.empty((nu, 64), dtype=torch.float32, device=self.device)
        self._q_current = False
        self.update_count = 0
        self.step_losses = []          # (neg_ll, kl) per training step, device tensors [2]

    def parameters(self):
        """(Wq [2d, I], bq [2d], Wp [I, d], bp [I]) in the reference's shapes (copies)"""
        d = self.d
        wq = torch.cat([self._wqt[:, :d], self._wqt[:, 64:64 + d]], dim=1).t().contiguous()
        bq = torch.cat([self._bq[:d], self._bq[64:64 + d]])
        return wq, bq, self._wp[:, :d].contiguous(), self._bp.clone()

    # ---- training --------------------------------------------------------------------------------
    def _anneal(self):
        cfg = self.config
        if cfg.anneal_steps > 0:                                       # MultVAE.py:180-183
            return min(cfg.anneal_cap, 1.0 * self.update_count / cfg.anneal_steps)
        return cfg.anneal_cap

    @on_compute_stream
    def train_step(self, users, keep=None, eps=None):
        """one step on the batch ``users`` (a sequence, or an int32 device tensor).  ``keep``: uint8, one flag per non-zero of the batch's train rows (user
        after user, items ascending) and ``eps``: float32 [len(users), d] replay recorded draws; without them the step
        draws on the device (equal to the reference in law only).  -> device tensor (neg_ll, kl)"""
        cfg, L, st = self.config, _hip.lib(), _hip.stream()
        du = None
        if torch.is_tensor(users):                                     # an int32 device tensor as it is
            du = users.to(self.device, torch.int32).contiguous()
            if keep is not None:
                users = du.cpu().numpy()
        else:
            users = np.ascontiguousarray(users, dtype=np.int32)
        n = int(users.shape[0])
        if n > _hip.SKR_MULTVAE_MAX_BATCH:
            raise ValueError(f"MultVAE: a batch holds at most {_hip.SKR_MULTVAE_MAX_BATCH} users (got {n})")
        if n == 0:
            # the empty batch is no step: a zero loss pair (what skr_multvae_step writes for n == 0), and neither
            # optimiser runs -- opt_w's weight decay would move the weights on a zero gradient -- nor does the annealing
            return torch.zeros(2, dtype=torch.float32, device=self.device)
        need = int(L.skr_multvae_workspace(n, self.num_items))
        if need > self._work.numel():
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        if du is None:
            du = torch.from_numpy(users).to(self.device)
        dk = de = None
        if (keep is None) != (eps is None):
            raise ValueError("MultVAE.train_step: keep and eps come together or not at all")
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            nnz = int((self._rowptr_host[users.astype(np.int64) + 1] - self._rowptr_host[users.astype(np.int64)]).sum())
            if keep.shape[0] != nnz:
                raise ValueError(f"MultVAE.train_step: {keep.shape[0]} keep flags for {nnz} non-zeros")
            e = np.zeros((n, 64), np.float32)
            e[:, :self.d] = np.asarray(eps, dtype=np.float32).reshape(n, self.d)
            dk, de = torch.from_numpy(keep).to(self.device), torch.from_numpy(e).to(self.device)
        loss = torch.empty(2, dtype=torch.float32, device=self.device)
        self._q_current = False
        _hip.check(L.skr_multvae_step(
            _hip.ptr(self._wqt), _hip.ptr(self._bq), _hip.ptr(self._wp), _hip.ptr(self._bp), _hip.ptr(self._rowptr),
            _hip.ptr(self._items), _hip.ptr(du), n, self.num_users, self.num_items, self.d, cfg.keep_prob, self._anneal(),
            _hip.ptr(dk), _hip.ptr(de), self.seed, self.update_count, *[_hip.ptr(g) for g in self._grads],
            _hip.ptr(self._work), self._work.numel(), _hip.ptr(loss), st))
        self.opt_w.step()
        self.opt_b.step()
        self.update_count += 1
        self.step_losses.append(loss)
        return loss

    def _make_iterator(self):
        self.update_count = 0          # every fit() starts the annealing over (MultVAE.py:175)
        train_users = [u for u in range(self.num_users) if self._rowptr_host[u + 1] > self._rowptr_host[u]]
        return BatchIterator(train_users, batch_size=self.config.batch_size, shuffle=True, drop_last=False)

    def _run_epoch(self, data_iter, epoch):
        self.step_losses = []
        for bat_users in data_iter:
            self.train_step(bat_users)

    # ---- ranking ---------------------------------------------------------------------------------
    @on_compute_stream
    def predict_factors(self):
        """(Q [num_users, 64], Wp [num_items, 64], bp [num_items]): score = <Q[u], Wp[i]> + bp[i].  Q is computed by one
        ``skr_multvae_queries`` launch over all users and kept until the next training step; the row of a user without
        a training item is bq"""
        if not self._q_current:
            _hip.check(_hip.lib().skr_multvae_queries(_hip.ptr(self._wqt), _hip.ptr(self._bq), _hip.ptr(self._rowptr),
                                                      _hip.ptr(self._items), None, self.num_users, self.num_users,
                                                      self.num_items, _hip.ptr(self._Q), _hip.stream()))
            self._q_current = True
        return self._Q, self._wp, self._bp
