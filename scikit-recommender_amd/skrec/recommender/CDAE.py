"""CDAE on MI355X (reference: skrec/recommender/CDAE.py).

Paper: Collaborative Denoising Auto-Encoder for Top-N Recommender Systems (Wu, DuBois, Zheng and Ester).
Same config, same initialisation (the four ``nn.Embedding`` constructors draw from the CPU generator, then
``reset_parameters`` re-draws normal(0, 0.01) for the encoder, decoder and user tables and zeroes the offset and the bias;
CDAE.py:66-93), same step (CDAE.py:168-206), quirks included: a user's negatives -- ``np.unique`` of
``len(pos) * num_neg`` draws of the process-global MT19937 stream -- are written into the encoder's INPUT, so the input of
a user is pos + neg, every entry 1, under dropout; the l2 term takes the DISTINCT items of the batch; the optimiser is the
reference's dense ``torch.optim.Adam`` over all five parameters.

One training step is ``skr_cdae_step`` (csrc/cdae.hip: user side, item side, finish; no floating-point atomic) on a pair
list, and one Adam step.  All parameters live in ONE flat buffer of 64-float rows,
[E_en | E_de | bias, 64 per block | offset | U], stepped by one ``DenseAdam``: temporally blocked over ``SKR_ADAM_BLOCK``
steps (default 32; the blocks a step names are its users' rows, the E_en / E_de rows and bias blocks of its distinct items
and the offset block), or one dense launch per step with ``SKR_ADAM_BLOCK=1`` -- bit-identical.

Layout granularity: the pair lists of a whole Adam block of k steps (32 steps when the Adam is dense) are prepared at once
on the device -- one ``skr_sample_epoch_exact_counts`` call on the CSR of the block's users in visit order, the per-row
``np.unique`` and the grouping by item as one ``torch.unique`` and one stable sort.  A block has four points where the
host waits for the device -- ``torch.unique`` and ``torch.unique_consecutive`` each wait for their output's size, and the
steps' pair and distinct-item offsets are read back -- and a step has none.  ``batch_layout`` is the same layout on the host: its specification, and the path of recorded draws.

Scoring collapses to one query row per user, Q[u] = act(sum E_en[train(u)] + U[u] + offset) (``skr_cdae_queries``), kept
until the next training step: score = <Q[u], E_de[i]> + bias[i], ranked by the evaluator's fused top-K path.

Draws: ``train_step`` replays recorded negatives and keep flags when handed them; otherwise the negatives come from the
exact sampler (the reference's stream bit for bit) and the keep flags from a device generator keyed by (seed, step, user,
item), equal to the reference's torch draws in law only.

Limits: hidden_dim <= 64 (NotImplementedError), batch_size <= 1024, loss_func sigmoid_cross_entropy, one GPU.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..utils.py import BatchIterator, ModelConfig
from ..utils.torch import get_initializer
from ._graph import train_csr, upload_csr
from .base import DenseAdam, DeviceRecommender, on_compute_stream

__all__ = ["CDAE", "CDAEConfig"]

PARAMS = ("en_embeddings", "en_offset", "de_embeddings", "de_bias", "user_embeddings")
LAYOUT_STEPS = 32          # steps prepared at once when the Adam is not blocked


class CDAEConfig(ModelConfig):
    def __init__(self, lr=0.001, reg=0.001, hidden_dim=64, dropout=0.5, num_neg=5, hidden_act="sigmoid",
                 loss_func="sigmoid_cross_entropy", batch_size=256, epochs=1000, early_stop=200, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.reg: float = reg
        self.hidden_dim: int = hidden_dim
        self.dropout: float = dropout
        self.num_neg: int = num_neg
        self.hidden_act: str = hidden_act  # hidden_act = identity, sigmoid
        self.loss_func: str = loss_func  # loss_func = sigmoid_cross_entropy, square
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.reg, float) and self.reg >= 0
        assert isinstance(self.hidden_dim, int) and self.hidden_dim > 0
        assert isinstance(self.dropout, float) and self.dropout < 1.0
        assert isinstance(self.num_neg, int) and self.num_neg >= 0
        assert isinstance(self.hidden_act, str) and self.hidden_act in {"identity", "sigmoid"}
        assert isinstance(self.loss_func, str) and self.loss_func in {"sigmoid_cross_entropy", "square"}
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


def check_limits(config):
    """the hidden width d of a config this implementation runs; raises outside the limits and where the reference does"""
    if config.hidden_act not in ("identity", "sigmoid"):
        raise ValueError(f"hidden activate function '{config.hidden_act}' is invalid.")
    if config.loss_func != "sigmoid_cross_entropy":                   # "square" passes _validate and is refused (CDAE.py:150-155)
        raise ValueError(f"loss function '{config.loss_func}' is invalid.")
    keep_prob = 1 - config.dropout
    if keep_prob <= 0.0 or keep_prob > 1.0:                            # dropout_sparse (utils/torch.py:41)
        raise ValueError(f"'keep_prob' must be a float in the range (0, 1], got {keep_prob}")
    d = int(config.hidden_dim)
    if not 1 <= d <= 64:
        raise NotImplementedError(f"CDAE: hidden_dim <= 64 (got {d}): rows are 64 floats and the fused evaluator ranks "
                                  f"64 columns")
    if config.batch_size > _hip.SKR_CDAE_MAX_BATCH:
        raise ValueError(f"CDAE: batch_size <= {_hip.SKR_CDAE_MAX_BATCH} (got {config.batch_size}): skr_cdae_step takes "
                         f"that many users")
    return d


def _init_tables(num_users, num_items, d):
    """CPU-side construction in the reference's order (_CDAE.__init__ / reset_parameters, CDAE.py:66-93):
    -> en_embeddings [I, d], en_offset [d], de_embeddings [I, d], de_bias [I, 1], user_embeddings [U, d]"""
    en = nn.Embedding(num_items, d)
    de = nn.Embedding(num_items, d)
    bias = nn.Embedding(num_items, 1)
    user = nn.Embedding(num_users, d)
    normal = get_initializer("normal")
    normal(en.weight)
    normal(de.weight)
    normal(user.weight)
    return (en.weight.detach(), torch.zeros(d), de.weight.detach(), torch.zeros(num_items, 1), user.weight.detach())


def batch_layout(rowptr, items, users, negatives):
    """The pair list of one batch on the host -- the specification of what the device prepares.
    ``rowptr`` / ``items``: train CSR, items ascending inside a row; ``users``: the batch; ``negatives``: per user of the
    batch its raw draws (before ``np.unique``).  ->  dict of
      bat_items, bat_labels, bat_idx   the reference's arrays: per user its positives, then its unique negatives
      uptr [n + 1], pitem, plabel, puser   the pair list: per user pos + neg merged, items ascending (the coalesced order
                                       of the encoder's input, which the keep flags follow)
      ditems [J], iptr [J + 1], ipair  the item-major view: distinct items ascending, each with its pairs ascending"""
    rowptr, items = np.asarray(rowptr), np.asarray(items)
    bat_items, bat_labels, bat_idx, pitem, plabel, uptr = [], [], [], [], [], [0]
    for idx, u in enumerate(users):
        pos = items[rowptr[u]:rowptr[u + 1]].astype(np.int32)
        neg = np.unique(np.asarray(negatives[idx], dtype=np.int32))
        bat_items += [pos, neg]
        bat_labels += [np.ones(len(pos), np.float32), np.zeros(len(neg), np.float32)]
        bat_idx.append(np.full(len(pos) + len(neg), idx, np.int32))
        both = np.concatenate([pos, neg])
        order = np.argsort(both, kind="stable")
        pitem.append(both[order])
        plabel.append(np.concatenate([np.ones(len(pos), np.uint8), np.zeros(len(neg), np.uint8)])[order])
        uptr.append(uptr[-1] + len(both))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)       # noqa: E731
    pitem, plabel, puser = cat(pitem, np.int32), cat(plabel, np.uint8), cat(bat_idx, np.int32)
    ipair = np.argsort(pitem, kind="stable").astype(np.int32)
    ditems, counts = np.unique(pitem, return_counts=True)
    iptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dict(bat_items=cat(bat_items, np.int32), bat_labels=cat(bat_labels, np.float32), bat_idx=puser.copy(),
                uptr=np.asarray(uptr, np.int32), pitem=pitem, plabel=plabel, puser=puser, ditems=ditems.astype(np.int32),
                iptr=iptr, ipair=ipair)


class _Block(object):
    """the device layout of consecutive steps (see ``batch_layout``; the pair arrays are shared by the block's steps)"""
    __slots__ = ("users", "uptr", "pitem", "plabel", "pkeep", "puser", "ditems", "iptr", "ipair", "ustart", "pstart", "jstart",
                 "ids", "per")


class CDAE(DeviceRecommender):
    """limits: hidden_dim <= 64 (NotImplementedError), batch_size <= 1024 and the reference's own refusals (ValueError),
    one GPU.  ``seed`` (``detached``; the run's seed otherwise): the key of the device's keep flags"""
    config_class = CDAEConfig

    def _check_limits(self, world):
        check_limits(self.config)
        if world > 1:
            raise NotImplementedError("CDAE runs on one GPU: there is no sharded engine for it")

    def _train_inputs(self):
        return train_csr(self.dataset)

    def _build_args(self, run_config):
        return {"seed": getattr(run_config, "seed", 0) or 0}

    def _build(self, rowptr, items, seed=0):
        cfg = self.config
        d, nu, ni = check_limits(cfg), self.num_users, self.num_items
        self.d = d
        self.seed = int(seed)
        self.keep_prob = 1 - cfg.dropout
        self.act = _hip.SKR_CDAE_SIGMOID if cfg.hidden_act == "sigmoid" else _hip.SKR_CDAE_IDENTITY
        self._rowptr, self._items = upload_csr(rowptr, items, self.device)
        self._rowptr_host = self._rowptr.cpu().numpy() if torch.is_tensor(rowptr) else np.ascontiguousarray(rowptr, dtype=np.int64)
        assert self._rowptr_host.shape[0] == nu + 1
        en, off, de, bias, user = _init_tables(nu, ni, d)
        pad = lambda t: nn.functional.pad(t, (0, 64 - d))              # noqa: E731
        nb = (ni + 63) // 64                                           # bias blocks, the last zero-padded
        flat = torch.cat([pad(en).reshape(-1), pad(de).reshape(-1), nn.functional.pad(bias.reshape(-1), (0, 64 * nb - ni)),
                          pad(off), pad(user).reshape(-1)])
        self._flat = flat.to(self.device).contiguous()
        # block (64-float row) numbers of the five tables in the flat buffer
        self._blk_de, self._blk_bias, self._blk_off, self._blk_user = ni, 2 * ni, 2 * ni + nb, 2 * ni + nb + 1
        self.adam_block = max(1, min(64, int(os.environ.get("SKR_ADAM_BLOCK", "32"))))
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr)
        f, g = self._flat, self.optimizer.grad
        views = lambda t: (t[:ni * 64].view(ni, 64), t[ni * 64:2 * ni * 64].view(ni, 64),                     # noqa: E731
                           t[2 * ni * 64:2 * ni * 64 + ni], t[self._blk_off * 64:self._blk_off * 64 + 64],
                           t[self._blk_user * 64:].view(nu, 64))
        self._en, self._de, self._bias, self._off, self._user = views(f)
        self._grads = views(g)                                         # (gE_en, gE_de, gbias, goffset, gU)
        self._work = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._Q = torch.empty((nu, 64), dtype=torch.float32, device=self.device)
        self._q_current = False
        self.update_count = 0
        self.sampler = None            # the process-global MT19937(2020) stream unless a test hands in its own
        self.step_losses = None        # device [n_steps, 2]: (bce sum, l2) per step of the last epoch

    def parameters(self):
        """(en_embeddings [I, d], en_offset [d], de_embeddings [I, d], de_bias [I, 1], user_embeddings [U, d]) in the
        reference's shapes (copies)"""
        d = self.d
        return (self._en[:, :d].contiguous(), self._off[:d].clone(), self._de[:, :d].contiguous(),
                self._bias.clone().view(-1, 1), self._user[:, :d].contiguous())

    # ---- batch layout on the device ---------------------------------------------------------------
    def _sampler(self):
        if self.sampler is None:
            from ..utils.py.random import global_sampler
            self.sampler = global_sampler()
        return self.sampler

    def _row_lengths(self, users):
        u = np.asarray(users, dtype=np.int64)
        if u.size and (u.min() < 0 or u.max() >= self.num_users):
            raise ValueError("CDAE: a user of the batch is out of range")
        if np.unique(u).size != u.size:
            raise ValueError("CDAE: the users of a batch must be distinct")
        return self._rowptr_host[u + 1] - self._rowptr_host[u]

    def _prepare(self, batches, negatives=None, keep=None):
        """the layout of consecutive steps, ``batches`` a list of int32 arrays of users.  ``negatives``: raw draws, flat,
        user after user (len(pos) * num_neg each) instead of the sampler's; ``keep``: flags in pair order instead of the
        device's draws"""
        cfg, dev, I = self.config, self.device, self.num_items
        if cfg.num_neg <= 0:                                           # randint_choice(size=0) (pyx_random.pyx:34-54)
            raise ValueError("'size' must be a positive integer.")
        k = len(batches)
        sizes = np.array([len(b) for b in batches], np.int64)
        if sizes.max() > _hip.SKR_CDAE_MAX_BATCH:
            raise ValueError(f"CDAE: a batch holds at most {_hip.SKR_CDAE_MAX_BATCH} users (got {sizes.max()})")
        us = np.concatenate(batches).astype(np.int32)
        lens_h = np.concatenate([self._row_lengths(b) for b in batches])
        if (lens_h <= 0).any():
            raise ValueError("'size' must be a positive integer.")    # a user without a training item draws nothing
        N, total = len(us), int(lens_h.sum())
        ustart_h = np.concatenate([[0], np.cumsum(sizes)])
        d_us = torch.from_numpy(us).to(dev)
        lens = torch.from_numpy(lens_h).to(dev)
        rp = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(lens, 0)
        slots = torch.arange(N, device=dev)
        pos_slot = torch.repeat_interleave(slots, lens, output_size=total)
        src = self._rowptr[d_us.long()][pos_slot] + (torch.arange(total, device=dev) - rp[pos_slot])
        pos_items = self._items[src].contiguous()
        n_draws = total * cfg.num_neg
        if negatives is None:
            negs = torch.empty(n_draws, dtype=torch.int32, device=dev)
            drawptr = (rp * cfg.num_neg).contiguous()
            self._sampler().sample_epoch_exact_counts(I, N, rp, pos_items, total, drawptr, n_draws, negs)
        else:
            negs = torch.from_numpy(np.ascontiguousarray(negatives, dtype=np.int32)).to(dev)
            if negs.numel() != n_draws:
                raise ValueError(f"CDAE: {negs.numel()} recorded negatives for {n_draws} draws")
        neg_slot = torch.repeat_interleave(slots, lens * cfg.num_neg, output_size=n_draws)
        # np.unique per row and the merge with the positives: one sort of (slot, item, label) keys
        keys = torch.unique(torch.cat([(pos_slot * I + pos_items.long()) * 2 + 1, (neg_slot * I + negs.long()) * 2]), sorted=True)
        pk = keys >> 1
        slot = torch.div(pk, I, rounding_mode="floor")
        item = (pk - slot * I).to(torch.int32)
        P = int(keys.numel())
        B = _Block()
        B.users, B.pitem, B.plabel = d_us, item.contiguous(), (keys & 1).to(torch.uint8).contiguous()
        B.uptr = torch.searchsorted(slot, torch.arange(N + 1, device=dev)).to(torch.int32).contiguous()
        ustart = torch.from_numpy(ustart_h).to(dev)
        step_of_slot = torch.repeat_interleave(torch.arange(k, device=dev), torch.from_numpy(sizes).to(dev), output_size=N)
        pstep = step_of_slot[slot]
        pstart = B.uptr[ustart].long()
        B.puser = (slot - ustart[pstep]).to(torch.int32).contiguous()
        # item-major: a stable sort by (step, item) keeps a distinct item's pairs in ascending pair order
        skey, order = torch.sort(pstep * I + item.long(), stable=True)
        B.ipair = (order - pstart[pstep[order]]).to(torch.int32).contiguous()
        dk, counts = torch.unique_consecutive(skey, return_counts=True)
        dstep = torch.div(dk, I, rounding_mode="floor")
        B.ditems = (dk - dstep * I).to(torch.int32).contiguous()
        J = int(dk.numel())
        iptr = torch.zeros(J + 1, dtype=torch.int64, device=dev)
        iptr[1:] = torch.cumsum(counts, 0)
        B.iptr = iptr.to(torch.int32).contiguous()
        jstart = torch.searchsorted(dstep, torch.arange(k + 1, device=dev))
        if keep is not None:
            kp = np.ascontiguousarray(keep, dtype=np.uint8)
            if kp.shape[0] != P:
                raise ValueError(f"CDAE: {kp.shape[0]} keep flags for {P} pairs")
            B.pkeep = torch.from_numpy(kp).to(dev)
        elif self.keep_prob < 1:
            B.pkeep = torch.empty(P, dtype=torch.uint8, device=dev)
            # named, so that both live until the launch is queued: a temporary's storage goes back to the allocator at once
            slot32, pstep32 = slot.to(torch.int32).contiguous(), pstep.to(torch.int32).contiguous()
            _hip.check(_hip.lib().skr_cdae_draws(_hip.ptr(d_us), _hip.ptr(slot32), _hip.ptr(B.pitem), _hip.ptr(pstep32), P, N,
                                                 self.keep_prob, self.seed, self.update_count, _hip.ptr(B.pkeep), _hip.stream()))
        else:
            B.pkeep = torch.ones(P, dtype=torch.uint8, device=dev)
        B.ustart = ustart_h
        B.pstart, B.jstart = pstart.cpu().numpy(), jstart.cpu().numpy()      # read back; with the two uniques above, the block's four host waits
        # the 64-float blocks every step names for the blocked Adam, -1 where a step has fewer than the longest
        nmax, jmax = int(sizes.max()), int(np.diff(B.jstart).max())
        B.per = nmax + 3 * jmax + 1
        ids = torch.full((k, B.per), -1, dtype=torch.int32, device=dev)
        ids[step_of_slot, slots - ustart[step_of_slot]] = self._blk_user + d_us
        jl = torch.arange(J, device=dev) - jstart[dstep]
        ids[dstep, nmax + jl] = B.ditems
        ids[dstep, nmax + jmax + jl] = self._blk_de + B.ditems
        ids[dstep, nmax + 2 * jmax + jl] = self._blk_bias + torch.div(B.ditems, 64, rounding_mode="floor")
        ids[:, -1] = self._blk_off
        B.ids = ids.view(-1)
        need = int(_hip.lib().skr_cdae_workspace(nmax, int(np.diff(B.pstart).max())))
        if need > self._work.numel():
            self._work = torch.empty(need, dtype=torch.uint8, device=dev)
        return B

    def _launch(self, B, s, loss_ptr, h_ms=None):
        """step ``s`` of block ``B``: the step kernel alone -> return code"""
        L = _hip.lib()
        u0, j0 = int(B.ustart[s]), int(B.jstart[s])
        n, P, J = int(B.ustart[s + 1]) - u0, int(B.pstart[s + 1] - B.pstart[s]), int(B.jstart[s + 1]) - j0
        args = (_hip.ptr(self._en), _hip.ptr(self._de), _hip.ptr(self._bias), _hip.ptr(self._off), _hip.ptr(self._user),
                B.users.data_ptr() + 4 * u0, B.uptr.data_ptr() + 4 * u0, B.pitem.data_ptr(), B.plabel.data_ptr(),
                B.pkeep.data_ptr(), B.puser.data_ptr(), B.ditems.data_ptr() + 4 * j0, B.iptr.data_ptr() + 4 * j0,
                B.ipair.data_ptr(), n, P, J, self.num_users, self.num_items, self.d, self.act, self.keep_prob, self.config.reg,
                *[_hip.ptr(g) for g in self._grads], _hip.ptr(self._work), self._work.numel(), loss_ptr, _hip.stream())
        if h_ms is not None:
            return L.skr_cdae_step_timed(*args, h_ms)
        return L.skr_cdae_step(*args)

    # ---- training --------------------------------------------------------------------------------
    @on_compute_stream
    def train_step(self, users, negatives=None, keep=None):
        """one step on the batch ``users`` (distinct, each with a training item).  ``negatives``: the raw draws, flat, user
        after user, len(pos) * num_neg each (default: the exact sampler's); ``keep``: uint8, one flag per pair of the batch
        (user after user, items ascending over pos + unique(neg); default: device draws).  Recorded negatives and flags
        replay a reference run.  -> device tensor (bce sum, l2)"""
        users = np.ascontiguousarray(users.cpu().numpy() if torch.is_tensor(users) else users, dtype=np.int32)
        self._q_current = False
        if users.size == 0:
            # the empty batch: a zero loss pair and the zero gradient through Adam (nothing moves while the moments are
            # zero); there is nothing to lay out, and skr_cdae_step would write the same pair
            self.optimizer.step()
            self.update_count += 1
            return torch.zeros(2, dtype=torch.float32, device=self.device)
        B = self._prepare([users], negatives, keep)
        loss = torch.empty(2, dtype=torch.float32, device=self.device)
        _hip.check(self._launch(B, 0, _hip.ptr(loss)))
        self.optimizer.step()
        self.update_count += 1
        return loss

    @on_compute_stream
    def train_epoch(self, batches):
        """the steps of ``batches`` (a list of user arrays); the layout of ``SKR_ADAM_BLOCK`` steps is prepared at once"""
        opt = self.optimizer
        batches = [np.ascontiguousarray(b, dtype=np.int32) for b in batches]
        losses = torch.zeros((len(batches), 2), dtype=torch.float32, device=self.device)
        ploss = losses.data_ptr()
        kblk = self.adam_block
        span = kblk if kblk > 1 else LAYOUT_STEPS
        self._q_current = False
        for s0 in range(0, len(batches), span):
            B = self._prepare(batches[s0:s0 + span])
            k = len(B.ustart) - 1
            if kblk > 1:
                opt.begin_block(B.ids, k, per_step=B.per)
            for s in range(k):
                _hip.check(self._launch(B, s, ploss + 8 * (s0 + s)))
                if kblk > 1:
                    opt.hot_step()
                else:
                    opt.step()
            self.update_count += k
        if kblk > 1:
            opt.end_blocks()
        self.step_losses = losses
        return losses

    def _make_iterator(self):
        train_users = [u for u in range(self.num_users) if self._rowptr_host[u + 1] > self._rowptr_host[u]]
        return BatchIterator(train_users, batch_size=self.config.batch_size, shuffle=True, drop_last=False)

    def _run_epoch(self, data_iter, epoch):
        self.train_epoch([np.asarray(b, dtype=np.int32) for b in data_iter])      # one pass of the iterator: one shuffle

    # ---- ranking ---------------------------------------------------------------------------------
    @on_compute_stream
    def predict_factors(self):
        """(Q [num_users, 64], E_de [num_items, 64], bias [num_items]): score = <Q[u], E_de[i]> + bias[i].  Q is computed by
        one ``skr_cdae_queries`` launch over all users and kept until the next training step; the row of a user without a
        training item is act(U[u] + offset)"""
        if not self._q_current:
            _hip.check(_hip.lib().skr_cdae_queries(_hip.ptr(self._en), _hip.ptr(self._off), _hip.ptr(self._user),
                                                   _hip.ptr(self._rowptr), _hip.ptr(self._items), None, self.num_users,
                                                   self.num_users, self.num_items, self.d, self.act, _hip.ptr(self._Q),
                                                   _hip.stream()))
            self._q_current = True
        return self._Q, self._de, self._bias
