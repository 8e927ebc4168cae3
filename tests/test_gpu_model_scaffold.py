"""GPU suite of the models' shared scaffold (``DeviceRecommender``, skrec/recommender/base.py): a model built from a data set
and one built with ``detached`` from the same train CSR / last items / windows reach the same ``_build`` -- the same
parameters under the same seed, and after two training steps on the same recorded batch the same parameters, Adam
moments and scores, byte for byte."""
import importlib

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
SEED = 2021
CONFIGS = {"CDAE": dict(lr=1e-2, reg=1e-3, hidden_dim=40, dropout=0.5, num_neg=2, batch_size=8),
           "MultVAE": dict(lr=1e-2, reg=1e-3, p_dims=[40], keep_prob=0.5, anneal_steps=10, batch_size=8),
           "FPMC": dict(lr=1e-2, reg=1e-3, embed_size=64, batch_size=4),
           "TransRec": dict(lr=1e-2, reg=1e-3, embed_size=64, batch_size=4),
           "HGN": dict(lr=1e-2, reg=1e-3, embed_size=40, seq_L=3, seq_T=2, batch_size=4)}
SEQUENTIAL = ("FPMC", "TransRec", "HGN")


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


@pytest.fixture()
def seq_dir(tmp_path, golden):
    """tiny_dataset without user 63's test rows (that user has no training history), in the reference's TSV format"""
    root = tmp_path / "tiny_seq"
    root.mkdir()
    for split in ("train", "test"):
        with open(root / f"tiny_seq.{split}", "w") as f:
            for u, i, t in golden("tiny_seq_dataset")[split]:
                f.write(f"{int(u)}\t{int(i)}\t1.0\t{int(t)}\n")
    return str(root)


def _both(name, data_dir):
    """(the model from the data set, the detached one on what the first took from the data set)"""
    from skrec import RunConfig
    from skrec.recommender._graph import train_csr
    cls = getattr(importlib.import_module(f"skrec.recommender.{name}"), name)
    run_config = RunConfig(recommender=name, data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                           metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                           test_thread=2, seed=SEED)
    _seed()
    a = cls(run_config, dict(CONFIGS[name]))
    _seed()
    if name == "HGN":
        b = cls.detached(a.num_users, a.num_items - 1, dict(CONFIGS[name]), a._windows.cpu().numpy(), last_items=a._last_host)
    elif name in SEQUENTIAL:
        b = cls.detached(a.num_users, a.num_items, dict(CONFIGS[name]), a._last_host)
    else:
        b = cls.detached(a.num_users, a.num_items, dict(CONFIGS[name]), train_csr(a.dataset), seed=SEED)
    return a, b


def _state(m):
    """name -> the flat parameter buffers and both Adam moments of each, as bytes"""
    opts = {"w": m.opt_w, "b": m.opt_b} if type(m).__name__ == "MultVAE" else {"flat": m.optimizer}
    out = {}
    for k, o in opts.items():
        for part in ("flat", "m", "v"):
            out[f"{k}.{part}"] = getattr(o, part).cpu().numpy().tobytes()
    return out


class _Epoch(object):
    """what ``train_epoch`` of the sequential models reads of an iterator: the epoch's columns and the batches' bounds"""

    def __init__(self, cols, batch_size):
        n = cols[0].shape[0]
        self.cols, self.batch_size = cols, batch_size
        self.bounds = [(a, a + batch_size) for a in range(0, n, batch_size)]

    def epoch_columns(self):
        return self.cols, self.bounds


def _recorded(name, m, rng):
    """-> run(model): two training steps on one recorded batch of at most four distinct users, with the negatives / keep
    flags / eps recorded here.  Kernels that add rows with float atomics get one addend per row, which is reproducible:
    the items of a sequential batch are all distinct"""
    import torch
    from skrec.recommender import CDAE as C
    if name in ("CDAE", "MultVAE"):
        # MultVAE's encoder backward adds an item's row once per user that holds it, with float atomics: users whose train
        # rows share no item, the shortest rows first (three such users on the tiny data set)
        rowptr, items = m._rowptr_host, m._items.cpu().numpy()
        users, seen = [], set()
        for u in np.argsort(np.diff(rowptr), kind="stable"):
            row = set(items[rowptr[u]:rowptr[u + 1]].tolist())
            if row and len(users) < 4 and not row & seen:
                users.append(u)
                seen |= row
        assert len(users) >= 2
        users = np.array(users, np.int32)
        lens = (rowptr[users + 1] - rowptr[users]).astype(np.int64)
    if name == "CDAE":
        negs = [rng.integers(0, m.num_items, n * m.config.num_neg).astype(np.int32) for n in lens]
        pairs = int(C.batch_layout(rowptr, items, users, negs)["pitem"].shape[0])
        steps = [(users, np.concatenate(negs), (rng.random(pairs) < 0.5).astype(np.uint8)) for _ in range(2)]
        return lambda model: [model.train_step(*s) for s in steps]
    if name == "MultVAE":
        steps = [(users, (rng.random(int(lens.sum())) < 0.5).astype(np.uint8),
                  rng.standard_normal((len(users), m.d)).astype(np.float32)) for _ in range(2)]
        return lambda model: [model.train_step(*s) for s in steps]
    L, T = (m.config.seq_L, m.config.seq_T) if name == "HGN" else (1, 1)
    n_items = m.num_items - (1 if name == "HGN" else 0)                               # not the padding item
    users = rng.choice(m.num_users, 4, replace=False).astype(np.int32)
    items = rng.choice(n_items, 4 * (L + 2 * T), replace=False).astype(np.int32)
    prev, pos, neg = items[:4 * L].reshape(4, L), items[4 * L:4 * (L + T)].reshape(4, T), items[4 * (L + T):].reshape(4, T)
    if name != "HGN":
        prev, pos, neg = prev.reshape(4), pos.reshape(4), neg.reshape(4)
    cols = [np.concatenate([c, c]) for c in (users, prev, pos, neg)]                  # the batch, twice

    def run(model):
        model.train_epoch(_Epoch([torch.from_numpy(c).to(model.device).contiguous() for c in cols], 4))
    return run


@pytest.mark.parametrize("name", ["CDAE", "MultVAE", "FPMC", "TransRec", "HGN"])
def test_data_set_and_detached_reach_the_same_build(name, tiny_dir, seq_dir, monkeypatch, tmp_path):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SKR_ADAM_BLOCK", raising=False)
    a, b = _both(name, seq_dir if name in SEQUENTIAL else tiny_dir)
    assert type(a) is type(b) and (a.num_users, a.num_items) == (b.num_users, b.num_items)
    before = _state(a)
    assert before == _state(b)                                                        # the same draws into the same layout
    run = _recorded(name, a, np.random.default_rng(7))
    run(a)
    run(b)
    torch.cuda.synchronize()
    after = _state(a)
    assert after == _state(b)
    for k in before:                                                                  # the steps did move all of them
        assert after[k] != before[k], k
    if name in SEQUENTIAL:
        assert a.step_losses.cpu().numpy().tobytes() == b.step_losses.cpu().numpy().tobytes()
        users = np.flatnonzero(a._last_host >= 0)[[0, 5, -1]]
    else:
        users = np.array([0, 31, a.num_users - 1])
    pa, pb = a.predict(list(users)), b.predict(list(users))
    assert pa.shape == (3, a.num_items) and np.isfinite(pa).all()
    assert pa.tobytes() == pb.tobytes()
