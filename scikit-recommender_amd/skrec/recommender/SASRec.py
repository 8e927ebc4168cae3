"""SASRec on MI355X (reference: skrec/recommender/SASRec.py, a TensorFlow-1.14 graph).

Paper: Self-Attentive Sequential Recommendation (Kang and McAuley).
Same config, same graph: item rows times sqrt(d) plus position rows, dropout, the padding mask; ``num_blocks`` blocks of causal
multi-head self-attention on LayerNorm'ed queries and un-normalised keys (residual: the normalised queries) and a two-layer
point-wise feed-forward part on LayerNorm'ed inputs (residual: the normalised inputs); a last LayerNorm; the two log losses of
every real target against one sampled negative; ``l2_emb / 2`` times the squared norms of the two tables; and
``tf.train.AdamOptimizer(lr, beta2=0.98)`` over every parameter, dense.  One training step is ``skr_sasrec_step``
(csrc/sasrec.hip) and one ``skr_adam_step_tf`` launch over the flat buffer [item rows | position rows | shared block].

TensorFlow is not installed where this library is built and tested, so parity with a RUN of the reference is not pinned: the
yardstick is a float64 restatement of the reference's graph (tests/sasrec_twin.py).  Initialisation follows TensorFlow's
defaults (Glorot-uniform tables and kernels, zero biases, gamma 1, beta 0) from the run's seed: equal in law, TensorFlow's
stream cannot be replayed.  Two deviations from the reference's arithmetic, both stated in DESIGN.md: a key is masked when its
item is the padding id (the reference: when its input row sums to exactly 0.0), and ``1 - sigmoid(x)`` is evaluated as
``sigmoid(-x)`` (the reference's fp32 chain rounds it to 0 beyond logits of about 17).

Training data exactly as the reference's ``_generate_train_data`` / ``_sample_negative``: a row per user, ``items[:-1]``
against ``items[1:]``, left-padded and left-truncated to ``max_len`` with the padding id ``num_items``; negatives per epoch
from ``batch_randint_choice`` in chunks of 1 024 users with the user's items excluded; ``BatchIterator(shuffle=True)``'s
permutation.  The epoch's three id tables are uploaded once and permuted on the device; a batch is a slice.

Dropout: the step draws its keep flags on the device, keyed by (the run's seed, the step's number, the sequence's number in
the batch, the element): equal to TensorFlow's draws in law only.  ``keep_in`` (uint8 [sequences of the coming steps,
``_hip.sasrec_keep_bytes``], consumed step by step) replays recorded flags; ``keep_out = []`` collects every step's flags;
``record_batches = []`` collects every step's (seq, pos, neg).

Ranking: ``score(u, i) = <out_u[max_len - 1], sqrt(d) E[i]>``: one query row per user (``skr_sasrec_queries``, kept until the
next training step) ranked by the fused top-K evaluator at 64 columns against the raw item rows.  A user without training
items is ranked on ``ln_out_beta``, as in the reference.

Limits: hidden_units <= 64 (zero-padded to 64), max_len <= 64, num_blocks <= 4, num_heads <= 8 and dividing hidden_units,
batch_size <= 2048, one GPU.
"""
import numpy as np
import torch

from .. import _hip
from ..utils.py import ModelConfig, batch_randint_choice, pad_sequences
from .base import DenseAdam, DeviceRecommender, on_compute_stream

__all__ = ["SASRec", "SASRecConfig"]


class SASRecConfig(ModelConfig):
    def __init__(self, lr=1e-3, l2_emb=0.0, hidden_units=64, dropout_rate=0.5, max_len=50, num_blocks=2, num_heads=1,
                 batch_size=128, epochs=1000, early_stop=100, **kwargs):
        super().__init__()
        self.lr: float = lr
        self.l2_emb: float = l2_emb
        self.hidden_units: int = hidden_units
        self.dropout_rate: float = dropout_rate
        self.max_len: int = max_len
        self.num_blocks: int = num_blocks
        self.num_heads: int = num_heads
        self.batch_size: int = batch_size
        self.epochs: int = epochs
        self.early_stop: int = early_stop

    def _validate(self):
        assert isinstance(self.lr, float) and self.lr > 0
        assert isinstance(self.l2_emb, float) and self.l2_emb >= 0
        assert isinstance(self.hidden_units, int) and self.hidden_units > 0
        assert isinstance(self.dropout_rate, float) and 1 > self.dropout_rate >= 0
        assert isinstance(self.max_len, int) and self.max_len > 0
        assert isinstance(self.num_blocks, int) and self.num_blocks > 0
        assert isinstance(self.num_heads, int) and self.num_heads > 0
        assert isinstance(self.batch_size, int) and self.batch_size > 0
        assert isinstance(self.epochs, int) and self.epochs >= 0
        assert isinstance(self.early_stop, int)


# rows (of 64 floats) of a block's part of the shared parameters: include/skrec_hip.h, section SASRec
_ROWS = dict(ln1_gamma=0, ln1_beta=1, Wq=2, bq=66, Wk=67, bk=131, Wv=132, bv=196, ln2_gamma=197, ln2_beta=198, W1=199, b1=263,
             W2=264, b2=328)
BLOCK_NAMES = tuple(_ROWS)


def param_names(blocks):
    """every parameter's name, in the flat buffer's order"""
    return ["item_embeddings", "position_embeddings"] + [f"{k}_{b}" for b in range(blocks) for k in BLOCK_NAMES] + \
        ["ln_out_gamma", "ln_out_beta"]


class _Layout(object):
    """offsets (in floats) of the flat buffer [item rows, the padding row included | position rows | shared block]"""

    def __init__(self, ni, T, blocks):
        self.ni, self.T, self.blocks = ni, T, blocks
        self.E, self.P = 0, (ni + 1) * 64
        self.shared = self.P + T * 64
        self.ns = _hip.sasrec_shared_floats(blocks)
        self.total = self.shared + self.ns


def parameter_views(flat, lay, d):
    """the reference's parameters, under its names and in its shapes, as VIEWS into the flat buffer: a dense kernel [in, out]
    is the transposed view of its stored [out, in] rows"""
    ni, T = lay.ni, lay.T
    v = {"item_embeddings": flat[lay.E:lay.E + ni * 64].view(ni, 64)[:, :d],
         "position_embeddings": flat[lay.P:lay.shared].view(T, 64)[:, :d]}
    s = flat[lay.shared:lay.total].view(-1, 64)
    for b in range(lay.blocks):
        r0 = b * _hip.SKR_SASREC_BLOCK_ROWS
        for k, r in _ROWS.items():
            v[f"{k}_{b}"] = s[r0 + r:r0 + r + 64, :d][:d].t() if k[0] == "W" else s[r0 + r, :d]
    r0 = lay.blocks * _hip.SKR_SASREC_BLOCK_ROWS
    v["ln_out_gamma"], v["ln_out_beta"] = s[r0, :d], s[r0 + 1, :d]
    return v


def pack_parameters(tables, lay, d):
    """the flat fp32 buffer of ``lay`` from tensors in the reference's shapes (zero where padded, the padding row included)"""
    flat = torch.zeros(lay.total, dtype=torch.float32)
    for k, view in parameter_views(flat, lay, d).items():
        view.copy_(torch.as_tensor(tables[k], dtype=torch.float32))
    return flat


def _glorot(gen, shape):
    limit = float(np.sqrt(6.0 / (shape[0] + shape[1])))
    return (torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * limit


def init_tables(ni, T, d, blocks, seed):
    """TensorFlow's defaults (tf.get_variable and tf.layers without an initializer: glorot_uniform kernels and tables, zero
    biases; normalize: gamma 1, beta 0) from a generator seeded with ``seed``"""
    gen = torch.Generator().manual_seed(int(seed))
    t = {"item_embeddings": _glorot(gen, (ni, d)), "position_embeddings": _glorot(gen, (T, d))}
    for b in range(blocks):
        for k in BLOCK_NAMES:
            if k[0] == "W":
                t[f"{k}_{b}"] = _glorot(gen, (d, d))
            else:
                t[f"{k}_{b}"] = torch.ones(d) if k.endswith("gamma") else torch.zeros(d)
    t["ln_out_gamma"], t["ln_out_beta"] = torch.ones(d), torch.zeros(d)
    return t


def generate_train_data(user_pos_train, users, pad, max_len):
    """(seq, pos) int32 [len(users), max_len]: items[:-1] against items[1:], padded and truncated in front (SASRec.py:335-350)"""
    seq = pad_sequences([user_pos_train[u][:-1] for u in users], value=pad, max_len=max_len, padding="pre", truncating="pre")
    pos = pad_sequences([user_pos_train[u][1:] for u in users], value=pad, max_len=max_len, padding="pre", truncating="pre")
    return seq, pos


def sample_negative(user_pos_train, users, num_items, max_len):
    """neg int32 [len(users), max_len]: per user len(items) - 1 draws outside the user's items, in chunks of 1 024 users
    (SASRec.py:352-364)"""
    rows = []
    for s in range(0, len(users), 1024):
        bat = users[s:s + 1024]
        n_neg = [len(user_pos_train[u][1:]) for u in bat]
        exclusion = [user_pos_train[u] for u in bat]
        neg = batch_randint_choice(num_items, n_neg, replace=True, exclusion=exclusion, thread_num=4)
        rows.append(pad_sequences(neg, value=num_items, max_len=max_len, padding="pre", truncating="pre"))
    return np.concatenate(rows, 0) if rows else np.zeros((0, max_len), np.int32)


def eval_windows(user_pos_train, num_users, pad, max_len):
    """int32 [num_users, max_len]: every user's last max_len training items, left-padded; all padding without any
    (SASRec.py:327-333)"""
    seqs = [user_pos_train[u][-max_len:] if u in user_pos_train else [pad] for u in range(num_users)]
    return pad_sequences(seqs, value=pad, max_len=max_len, padding="pre", truncating="pre", dtype=np.int32)


class SASRec(DeviceRecommender):
    """limits: hidden_units <= 64 and one GPU (NotImplementedError beyond), max_len <= 64, num_blocks <= 4, num_heads <= 8
    and dividing hidden_units, batch_size <= 2048 (ValueError).  ``detached``: ``train`` = (seq, pos, user_pos_train, users) or
    None, ``windows`` int32 [num_users, max_len], ``seed``: the key of the initialisation and of the device draws"""
    config_class = SASRecConfig

    def _check_limits(self, world):
        c = self.config
        if c.hidden_units > _hip.SKR_SASREC_MAX_HIDDEN:
            raise NotImplementedError(f"SASRec: hidden_units <= {_hip.SKR_SASREC_MAX_HIDDEN} (got {c.hidden_units}): rows are 64 "
                                      f"floats and a sequence's activations live in LDS")
        if world > 1:
            raise NotImplementedError("SASRec runs on one GPU: there is no sharded engine for it")
        for name, hi in (("max_len", _hip.SKR_SASREC_MAX_LEN), ("num_blocks", _hip.SKR_SASREC_MAX_BLOCKS),
                         ("num_heads", _hip.SKR_SASREC_MAX_HEADS), ("batch_size", _hip.SKR_SASREC_MAX_BATCH)):
            if not 1 <= getattr(c, name) <= hi:
                raise ValueError(f"SASRec: 1 <= {name} <= {hi} (got {getattr(c, name)}): a limit of skr_sasrec_step")
        if c.hidden_units % c.num_heads:
            raise ValueError(f"SASRec: num_heads must divide hidden_units (got {c.num_heads}, {c.hidden_units}): a limit of "
                             f"skr_sasrec_step")

    def _build_args(self, run_config):
        T, pad = self.config.max_len, self.num_items
        self.user_pos_train = self.dataset.train_data.to_user_dict_by_time()
        self.all_users = list(self.user_pos_train.keys())
        seq, pos = generate_train_data(self.user_pos_train, self.all_users, pad, T)
        return dict(train=(seq, pos, self.user_pos_train, self.all_users),
                    windows=eval_windows(self.user_pos_train, self.num_users, pad, T), seed=getattr(run_config, "seed", 0) or 0)

    def _build(self, train=None, windows=None, seed=0):
        cfg = self.config
        d, T, nb, nh = cfg.hidden_units, cfg.max_len, cfg.num_blocks, cfg.num_heads
        ni, nu = self.num_items, self.num_users
        self.pad_idx = ni
        self.seed, self.update_count = int(seed), 0
        self.keep_in, self.keep_out, self._keep_cursor = None, None, 0
        self.record_batches = None
        self.timed_ms = None      # float32 numpy [SKR_SASREC_LAUNCHES]: every step goes through skr_sasrec_step_timed (tools)
        self.step_losses = None   # device [n_steps, 2]: (mean loss, l2 term) per step of the last epoch
        self._train = None
        if train is not None:
            seq, pos, upt, users = train
            self._train = (self._ids(seq), self._ids(pos), upt, list(users))
        win = np.full((nu, T), ni, np.int32)
        if windows is not None:
            win[:] = np.asarray(windows, dtype=np.int32).reshape(nu, T)
        self._windows = torch.from_numpy(win).to(self.device)
        self._lay = lay = _Layout(ni, T, nb)
        self._flat = pack_parameters(init_tables(ni, T, d, nb, seed), lay, d).to(self.device).contiguous()
        self.optimizer = DenseAdam(self._flat, lr=cfg.lr, betas=(0.9, 0.98), tf_epsilon=True)   # SASRec.py:459
        f, opt = self._flat, self.optimizer
        self._item_rows, self._pos_rows = f[lay.E:lay.P].view(ni + 1, 64), f[lay.P:lay.shared].view(T, 64)
        self._shared = f[lay.shared:lay.total]
        self._grads = (opt.grad_view(lay.E, (ni + 1, 64)), opt.grad_view(lay.P, (T, 64)), opt.grad_view(lay.shared, (lay.ns,)))
        for k, v in parameter_views(f, lay, d).items():
            setattr(self, k, v)
        L = _hip.lib()
        self._kbytes = _hip.sasrec_keep_bytes(d, T, nb, nh)
        nbytes = int(L.skr_sasrec_workspace(cfg.batch_size, T, nb, nh))
        self._work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._Q = torch.empty((nu, 64), dtype=torch.float32, device=self.device)
        self._q_current = False
        pt = [t.data_ptr() for t in (self._item_rows, self._pos_rows, self._shared)]
        pg = [t.data_ptr() for t in self._grads]
        pw, rate = self._work.data_ptr(), float(cfg.dropout_rate)

        def step(ps, pp, pn, n, ploss, st):
            pk = pko = None
            if rate > 0.0 and self.keep_in is not None:
                assert self._keep_cursor + n <= self.keep_in.shape[0], "keep_in holds fewer rows than the steps consume"
                pk = self.keep_in.data_ptr() + self._keep_cursor * self._kbytes
                self._keep_cursor += n
            if self.keep_out is not None:
                ko = torch.empty((n, self._kbytes), dtype=torch.uint8, device=self.device)
                self.keep_out.append(ko)
                pko = ko.data_ptr()
            self.update_count += 1
            args = (*pt, ps, pp, pn, n, ni, d, T, nb, nh, rate, pk, pko, self.seed, self.update_count, *pg, pw, nbytes, ploss,
                    _hip.SKR_LOSS_SLOTS, st)
            if self.timed_ms is None:
                return L.skr_sasrec_step(*args)
            return L.skr_sasrec_step_timed(*args, self.timed_ms.ctypes.data)
        self._step_launch = step

    def reference_parameters(self):
        """every parameter under the reference's name (``param_names``) in the reference's shape: views of the flat buffer"""
        return parameter_views(self._flat, self._lay, self.config.hidden_units)

    # ---- training --------------------------------------------------------------------------------
    def _make_iterator(self):
        return None           # the epoch's tables are made in train_epoch: the negatives change every epoch

    def train_step(self, d_seq, d_pos, d_neg, loss_out=None):
        """one batch: int32 device tensors [n, max_len]; ``loss_out``: float32 device [2 * SKR_LOSS_SLOTS] or None"""
        if loss_out is None:
            loss_out = torch.zeros(2 * _hip.SKR_LOSS_SLOTS, dtype=torch.float32, device=self.device)
        n = int(d_seq.shape[0])
        self._q_current = False
        if self.record_batches is not None:
            self.record_batches.append((d_seq.clone(), d_pos.clone(), d_neg.clone()))
        _hip.check(self._step_launch(d_seq.data_ptr(), d_pos.data_ptr(), d_neg.data_ptr(), n, loss_out.data_ptr(), _hip.stream()))
        l2 = self.config.l2_emb
        if l2 > 0.0:          # the dense regulariser of both tables (SASRec.py:374-385,453-455): l2 / 2 |w|^2, gradient l2 w
            gE, gP = self._grads[0], self._grads[1]
            gE.add_(self._item_rows, alpha=l2)
            gP.add_(self._pos_rows, alpha=l2)
            loss_out[1] = 0.5 * l2 * (self._item_rows.square().sum() + self._pos_rows.square().sum())
        self.optimizer.step()
        return loss_out

    @on_compute_stream
    def train_epoch(self, data_iter=None):
        """one epoch: fresh negatives, the permutation of ``BatchIterator(shuffle=True)``, one step per slice"""
        seq, pos, upt, users = self._train
        T, bs = self.config.max_len, self.config.batch_size
        neg = self._ids(sample_negative(upt, users, self.num_items, T))
        n_all = seq.shape[0]
        perm = torch.from_numpy(np.random.permutation(n_all)).to(self.device)
        seq_p, pos_p, neg_p = (t.index_select(0, perm).contiguous() for t in (seq, pos, neg))
        n_steps = (n_all + bs - 1) // bs
        spread = torch.zeros((n_steps, 2 * _hip.SKR_LOSS_SLOTS), dtype=torch.float32, device=self.device)
        for k in range(n_steps):
            a, b = k * bs, min((k + 1) * bs, n_all)
            self.train_step(seq_p[a:b], pos_p[a:b], neg_p[a:b], spread[k])
        self.step_losses = spread[:, :2]

    # ---- ranking ---------------------------------------------------------------------------------
    @on_compute_stream
    def predict_factors(self):
        """(Q [num_users, 64], item rows [num_items, 64], None): score = <Q[u], E[i]>, Q[u] = sqrt(d) out_u[max_len - 1].
        Q is computed by one ``skr_sasrec_queries`` call over all users and kept until the next training step"""
        if not self._q_current:
            cfg = self.config
            _hip.check(_hip.lib().skr_sasrec_queries(_hip.ptr(self._item_rows), _hip.ptr(self._pos_rows), _hip.ptr(self._shared), None,
                                                     self.num_users, _hip.ptr(self._windows), self.num_users, self.num_items,
                                                     cfg.hidden_units, cfg.max_len, cfg.num_blocks, cfg.num_heads, _hip.ptr(self._Q),
                                                     _hip.stream()))
            self._q_current = True
        return self._Q, self._item_rows[:self.num_items], None
