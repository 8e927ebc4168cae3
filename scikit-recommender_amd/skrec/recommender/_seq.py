"""Shared engine of the sequential pairwise recommenders (FPMC, TransRec, HGN): the reference's training loop over
``SequentialPairwiseIterator`` batches of (user, previous items, positives, negatives) -- one previous and one next item
for FPMC and TransRec, a window [n, L] and [n, T] targets for HGN: the columns are taken as the iterator hands them
over -- one fused step launch per batch (csrc/seq.hip, csrc/hgn.hip) on ONE flat fp32 parameter buffer stepped by
``DenseAdam`` -- the reference's dense ``torch.optim.Adam`` over every parameter, with ``_weight_decay`` where the
reference passes one -- and ``skr_seq_scores`` for predict() and the evaluator (HGN overrides the ranking half).

Optimiser stepping, as BPRMF's: at row width 64 the temporally blocked Adam (``SKR_ADAM_BLOCK`` batches per block,
default 32; bit-identical to one dense ``skr_adam_step`` per batch); ``SKR_ADAM_BLOCK=1`` or wider rows: one dense launch
per batch.
"""
import os

import numpy as np
import torch

from .. import _hip
from ..io import SequentialPairwiseIterator
from .base import DenseAdam, DeviceRecommender, on_compute_stream

__all__ = ["SeqPairwiseRecommender"]


class SeqPairwiseRecommender(DeviceRecommender):
    """Subclasses name their ``config_class`` and provide ``_build`` (calls this class's first, sets ``self.dp``, hands the
    flat parameter buffer to ``_setup`` and sets ``_step_launch``, one batch of the step kernel on cached addresses),
    ``_block_id_parts`` (the 64-float blocks of the flat buffer a batch touches: int32 tensors [n] or [n, w], negative
    entries are skipped) and ``_score_launch`` (skr_seq_scores).  ``_make_iterator`` names the iterator's shape,
    ``_weight_decay`` the optimiser's."""

    _weight_decay = 0.0

    def _check_limits(self, world):
        if world > 1:
            raise NotImplementedError(f"{type(self).__name__} runs on one GPU: there is no sharded engine for it")

    def _build_args(self, run_config):
        self.user_pos_dict = self.dataset.train_data.to_user_dict_by_time()
        last = np.full(self.num_users, -1, np.int32)
        for u, items in self.user_pos_dict.items():
            if len(items):
                last[int(u)] = int(items[-1])
        return {"last_items": last}

    def _build(self, last_items=None):
        """``last_items``: int32 [num_users], every user's last training item, -1 without one (``detached``'s default:
        item 0)"""
        last = np.zeros(self.num_users, np.int32) if last_items is None else last_items
        self._last_host = np.ascontiguousarray(last, dtype=np.int32)
        self._last = torch.from_numpy(self._last_host).to(self.device)
        self.step_losses = None  # device [n_steps, 2]: (bpr sum, l2) per step of the last epoch

    def _setup(self, flat):
        """``flat``: the model's parameters, one contiguous device buffer"""
        self._flat = flat
        # SKR_ADAM_BLOCK = k: the dense Adam blocked over k batches (1: one dense launch per batch); rows wider than one
        # 64-float block take the dense launch per batch (the blocked forms name rows by their 64-float block)
        self.adam_block = max(1, min(64, int(os.environ.get("SKR_ADAM_BLOCK", "32")))) if self.dp == 64 else 1
        self.optimizer = DenseAdam(flat, lr=self.config.lr, weight_decay=self._weight_decay)

    # ---- training --------------------------------------------------------------------------------
    def _block_ids(self, cols, n_steps, bsz):
        """int32 [n_steps * per_step]: step-major, the blocks of every batch; a short last batch is padded with -1 (an
        id the blocked Adam skips), so every step has the same number of entries"""
        parts = []
        for p in self._block_id_parts(*cols):
            parts.extend(p.unbind(1) if p.dim() == 2 else [p])
        n = cols[0].shape[0]
        ids = torch.full((len(parts), n_steps * bsz), -1, dtype=torch.int32, device=self.device)
        for r, p in enumerate(parts):
            ids[r, :n] = p
        ids = ids.view(len(parts), n_steps, bsz).permute(1, 0, 2).reshape(n_steps, -1)
        extra = self._block_ids_per_step()
        if extra:
            ids = torch.cat([ids, torch.tensor(extra, dtype=torch.int32, device=self.device).expand(n_steps, -1)], dim=1)
        return ids.contiguous().view(-1), ids.shape[1]

    def _block_ids_per_step(self):
        return []

    @on_compute_stream
    def train_epoch(self, data_iter):
        """one epoch; the per-step host work is one or two ctypes calls on cached integer addresses"""
        L, opt, st = _hip.lib(), self.optimizer, _hip.stream()
        S = _hip.SKR_LOSS_SLOTS
        (cu, cl, cp, cn), bounds = data_iter.epoch_columns()
        spread = torch.zeros((len(bounds), S, 2), dtype=torch.float32, device=self.device)
        ploss = spread.data_ptr()
        pcu, pcl, pcp, pcn = (c.data_ptr() for c in (cu, cl, cp, cn))
        n_all = max(cu.shape[0], 1)
        bl, bp, bn = (4 * (c.numel() // n_all) for c in (cl, cp, cn))      # bytes per instance of the three item columns
        step = self._step_launch
        kblk = self.adam_block
        if kblk <= 1:
            pflat, pgrad, pm, pv = (t.data_ptr() for t in (opt.flat, opt.grad, opt.m, opt.v))
            n_par = opt.flat.numel()
            head = (pflat, pgrad, pm, pv, n_par, opt.lr, opt.betas[0], opt.betas[1], opt.eps)
            dense = opt._entry("step")
            for k, (a, b) in enumerate(bounds):
                rc = step(pcu + 4 * a, pcl + bl * a, pcp + bp * a, pcn + bn * a, b - a, ploss + 8 * S * k, st)
                opt.t += 1
                rc |= dense(*head, opt.t, 1, None, st)
                if rc:
                    _hip.check(rc)
            self.step_losses = spread.sum(1)
            return
        # temporally blocked dense Adam (DenseAdam.begin_block): the rows no batch of a block touches get their k
        # zero-gradient updates in one pass, the touched rows are stepped batch by batch -- the same updates in the same
        # arithmetic as the loop above
        ids, per = self._block_ids((cu, cl, cp, cn), len(bounds), data_iter.batch_size)
        for s0 in range(0, len(bounds), kblk):
            blk = bounds[s0:s0 + kblk]
            opt.begin_block(ids[s0 * per:(s0 + len(blk)) * per], len(blk), per_step=per)
            rc = 0
            for k, (a, b) in enumerate(blk, start=s0):
                rc |= step(pcu + 4 * a, pcl + bl * a, pcp + bp * a, pcn + bn * a, b - a, ploss + 8 * S * k, st)
                opt.hot_step()
            if rc:
                _hip.check(rc)
        opt.end_blocks()
        self.step_losses = spread.sum(1)

    def _make_iterator(self):
        return SequentialPairwiseIterator(self.dataset.train_data, num_previous=1, num_next=1,
                                          batch_size=self.config.batch_size, shuffle=True, drop_last=False)

    # ---- ranking ---------------------------------------------------------------------------------
    def _require_history(self, users):
        """the reference looks every user's last training item up and raises KeyError(user) for a user without one
        (FPMC.py:147): the first such user, before anything is launched"""
        u = np.asarray(users, dtype=np.int64).reshape(-1)
        bad = (u < 0) | (u >= self.num_users)
        bad[~bad] = self._last_host[u[~bad]] < 0
        if bad.any():
            raise KeyError(int(u[np.argmax(bad)]))

    @on_compute_stream
    def evaluate(self, test_users=None):
        ev = self.evaluator
        users = ev.user_pos_test.keys() if test_users is None else [u for u in test_users if u in ev.user_pos_test]
        self._require_history(np.fromiter(users, dtype=np.int64))
        return ev.evaluate(self, test_users)

    def score_rows(self, d_users, out):
        """evaluator hook: dense score rows of the int32 device users into ``out`` [B, num_items] (fp32, device)"""
        _hip.check(self._score_launch(d_users, d_users.numel(), out, out.stride(0)))

    def predict(self, users) -> np.ndarray:
        """dense [len(users), num_items] scores (the reference's predict: FPMC.py:145-149, TransRec.py:156-160)"""
        users = list(users)
        self._require_history(users)
        du = torch.as_tensor(np.asarray(users, dtype=np.int32)).to(self.device)
        out = torch.empty((len(users), self.num_items), dtype=torch.float32, device=self.device)
        _hip.check(self._score_launch(du, len(users), out, self.num_items))
        return out.cpu().numpy()
