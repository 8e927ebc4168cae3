"""GPU suite of Caser (csrc/caser.hip, skrec/recommender/Caser.py): the step against float64 autograd of the twin
(tests/caser_twin.py), determinism, the device draws, golden replay of the reference's fit(), the blocked Adam against the
dense launch bit for bit, the query rows against float64, the evaluator's two paths, and the API edges."""
import os

import numpy as np
import pytest

import caser_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
MARGIN = 1e-4


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


# ---------------------------------------------------------------------------------------------------------------------
# cases of the step: tables, a batch, keep flags, and the float64 result
# ---------------------------------------------------------------------------------------------------------------------
def _draw_windows(rng, rows, seq, nI, pad, left):
    """fresh items for the non-padding positions of ``rows``"""
    L = seq.shape[1]
    for r in rows:
        seq[r] = rng.integers(0, nI, L)
        seq[r, :left[r]] = pad


def step_case(n, L, Tn, nv, nh, e, rate, seed):
    """a batch whose every decision (arg-max position, ReLU sign) has a float64 margin of at least MARGIN: the window of an
    instance below it is drawn again until none is left, so no instance is left out of the comparison.  -> dict"""
    import torch
    rng = np.random.default_rng(seed)
    nU, nI = 23, 41
    pad = nI
    raw = T.random_params(rng, nU, nI, e, L, nv, nh)
    raw["item_embeddings"][pad] = 0.0
    raw["W2"][pad] = 0.0
    raw["b2"][pad] = 0.0
    u = rng.integers(0, nU, n).astype(np.int32)
    pos, neg = (rng.integers(0, nI, (n, Tn)).astype(np.int32) for _ in range(2))
    u[1::5] = u[0]                                                   # users and targets that repeat inside the batch
    pos[2::9, 0] = pos[1 % n, 0]
    neg[::7, Tn - 1] = pos[0, 0]
    left = np.where(np.arange(n) % 3 == 0, rng.integers(0, L, n), 0)  # left padding of varying length
    left[n - 1] = L - 1                                              # all padding but the last position
    seq = np.zeros((n, L), np.int32)
    _draw_windows(rng, range(n), seq, nI, pad, left)
    if n > 4 and L > 1:
        seq[4, L - 1] = seq[4, 0] if left[4] == 0 else seq[4, L - 1]     # an item that repeats inside a window
        seq[3] = seq[2]                                              # two instances with the same window
    F = nv * e + nh * L
    keep = (rng.random((n, F)) >= rate).astype(np.uint8)
    P = T.to_torch(raw)
    tk = torch.from_numpy(keep)
    rounds = 0
    while True:
        m = T.decision_margins(P, torch.from_numpy(u).long(), torch.from_numpy(seq).long(), pad, tk, rate).numpy()
        bad = np.nonzero(m < MARGIN)[0]
        if not len(bad):
            break
        rounds += 1
        assert rounds < 200, "the margin loop does not end"
        _draw_windows(rng, bad, seq, nI, pad, left)
    # an id outside its range in each id column: those instances are skipped
    valid = np.ones(n)
    bu, bseq, bpos, bneg = u.copy(), seq.copy(), pos.copy(), neg.copy()
    if n >= 17:
        bu[5], bseq[6, L - 1], bpos[7, 0], bneg[8, Tn - 1] = nU, -1, nI + 1, -3
        valid[5:9] = 0
        bu[9] = -1
        valid[9] = 0
    elif n == 3:
        bpos[1, Tn - 1] = nI + 1
        valid[1] = 0
    tu, ts, tp, tn_ = (torch.from_numpy(a).long() for a in (u, seq, pos, neg))
    lp, ln, loss = T.step_losses(P, tu, ts, tp, tn_, tk, rate, pad, torch.from_numpy(valid))
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return dict(n=n, L=L, T=Tn, nv=nv, nh=nh, e=e, rate=rate, nU=nU, nI=nI, pad=pad, raw=raw, ids=(bu, bseq, bpos, bneg),
                clean_ids=(u, seq, pos, neg), keep=keep, valid=valid, loss=(lp.item(), ln.item()), grads=grads, rounds=rounds)


_CASES = {}


def cached_case(*key):
    if key not in _CASES:
        _CASES[key] = step_case(*key, seed=hash(key) % (2 ** 31))
    return _CASES[key]


class Device(object):
    """the tables of a case on the device, and one call of the step"""

    def __init__(self, c):
        import torch
        from skrec import _hip
        self.c = c
        e, L, nv, nh = c["e"], c["L"], c["nv"], c["nh"]
        raw = c["raw"]
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()    # noqa: E731
        self.tabs = [d(T.pad_cols(raw["user_embeddings"], 64)), d(T.pad_cols(raw["item_embeddings"], 64)), d(T.w2_rows(raw["W2"], e)),
                     d(raw["b2"].reshape(-1)), d(T.shared_block(raw, e, L, nv, nh))]
        assert self.tabs[4].numel() == _hip.caser_shared_floats(L, nv, nh)
        self.nbytes = int(_hip.lib().skr_caser_workspace(max(c["n"], 64), L, nv, nh))
        self.work = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def step(self, ids=None, keep="case", keep_out=False, rate=None, seed=0, step=0, pad="case", timed=False):
        """-> (loss [2 * slots], the five gradients, keep_out or None), as numpy"""
        import torch
        from skrec import _hip
        c = self.c
        ids = c["ids"] if ids is None else ids
        n = len(ids[0])
        d_ids = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in ids]
        grads = [torch.zeros_like(t) for t in self.tabs]
        loss = torch.full((2 * _hip.SKR_LOSS_SLOTS,), 7.0, device="cuda")
        rate = c["rate"] if rate is None else rate
        dk = torch.from_numpy(c["keep"]).cuda() if isinstance(keep, str) else (None if keep is None else torch.from_numpy(keep).cuda())
        F = c["nv"] * c["e"] + c["nh"] * c["L"]
        ko = torch.full((n, F), 9, dtype=torch.uint8, device="cuda") if keep_out else None
        pad = c["pad"] if isinstance(pad, str) else pad
        args = [*[_hip.ptr(t) for t in self.tabs], *[_hip.ptr(t) for t in d_ids], n, c["nU"], c["nI"] + 1, pad, 64, c["e"], c["L"],
                c["T"], c["nv"], c["nh"], rate, _hip.ptr(dk), _hip.ptr(ko), seed, step, *[_hip.ptr(g) for g in grads],
                _hip.ptr(self.work), self.nbytes, _hip.ptr(loss), _hip.SKR_LOSS_SLOTS, _hip.stream()]
        if timed:
            ms = np.zeros(_hip.SKR_CASER_LAUNCHES, np.float32)
            _hip.check(_hip.lib().skr_caser_step_timed(*args, ms.ctypes.data))
            self.ms = ms
        else:
            _hip.check(_hip.lib().skr_caser_step(*args))
        torch.cuda.synchronize()
        return loss.cpu().numpy(), [g.cpu().numpy() for g in grads], None if ko is None else ko.cpu().numpy()


def _compare(c, loss, grads, padding_row=True):
    gU, gE, gW2, gb2, gS = grads
    e, L, nv, nh = c["e"], c["L"], c["nv"], c["nh"]
    want = c["grads"]
    print("loss", loss[:2], c["loss"], "margin rounds", c["rounds"])
    np.testing.assert_allclose(loss[:2], c["loss"], rtol=1e-5)
    assert not loss[2:].any()
    shared, rest = T.unpack_shared(gS, e, L, nv, nh)
    assert not rest.any()                                            # what is padding gets no gradient
    got = dict(shared, user_embeddings=gU[:, :e], item_embeddings=gE[:, :e], b2=gb2[:, None],
               W2=np.concatenate([gW2[:, :e], gW2[:, 64:64 + e]], 1))
    assert not gU[:, e:].any() and not gE[:, e:].any() and not gW2[:, e:64].any() and not gW2[:, 64 + e:].any()
    assert set(got) == set(want)
    for k in want:
        w = want[k]
        print(k, "max abs err", np.abs(got[k] - w).max(), "max |grad|", np.abs(w).max())
    for k in want:
        w = want[k]
        np.testing.assert_allclose(got[k], w, rtol=1e-4, atol=2e-5 * np.abs(w).max(), err_msg=k)
    pad = c["pad"]
    if padding_row:                                                  # the padding row gets none either
        assert not gE[pad].any() and not gW2[pad].any() and gb2[pad] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step against float64 autograd of the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("e", [16, 64])
@pytest.mark.parametrize("L,Tn,nv,nh", [(1, 1, 1, 1), (5, 3, 4, 16), (8, 2, 8, 32)])
@pytest.mark.parametrize("n", [1, 3, 17, 70, 260])
def test_caser_step_matches_float64_autograd(n, L, Tn, nv, nh, e, rate):
    """n: one instance; less than a 16-row tile; one tile plus one row (three conv workgroups of 8); more than one fc1
    workgroup's 64; more than one 256-instance trip of the filter-gradient workgroups.  Tolerances: those of
    test_hgn_step_matches_float64_autograd for the same quantities (loss rtol 1e-5; gradients rtol 1e-4 and
    atol 2e-5 max|grad|).  Measured for comparison: the twin evaluated in fp32 on torch-CPU lies within 3e-6 max|grad| of its
    float64 self on these cases (L = 8, nh = 32, n = 260: the largest), so the bound is not widened."""
    c = cached_case(n, L, Tn, nv, nh, e, rate)
    loss, grads, _ = Device(c).step()
    _compare(c, loss, grads)


def test_caser_step_more_than_1024_instances():
    """the loss workgroup's second trip, and rank lists longer than one workgroup of the ordered adds can see at once"""
    c = cached_case(1030, 5, 3, 4, 16, 64, 0.5)
    dev = Device(c)
    loss, grads, _ = dev.step(timed=True)
    assert (dev.ms >= 0).all() and dev.ms.sum() > 0
    _compare(c, loss, grads)


def test_caser_step_without_a_padding_row():
    """pad_idx = -1 (what the model passes: the reference's padding item is an ordinary row): the row is read and trained"""
    import torch
    c = dict(cached_case(17, 5, 3, 4, 16, 64, 0.5))
    rng = np.random.default_rng(3)
    raw = dict(c["raw"])
    raw["item_embeddings"] = raw["item_embeddings"].copy()
    raw["item_embeddings"][c["pad"]] = rng.standard_normal(64).astype(np.float32)
    c["raw"] = raw
    P = T.to_torch(raw)
    u, seq, pos, neg = (torch.from_numpy(a).long() for a in c["clean_ids"])
    m = T.decision_margins(P, u, seq, None, torch.from_numpy(c["keep"]), 0.5)
    lp, ln, loss = T.step_losses(P, u, seq, pos, neg, torch.from_numpy(c["keep"]), 0.5, None, torch.from_numpy(c["valid"]))
    loss.backward()
    ok = (m.numpy() >= MARGIN) | (c["valid"] == 0)
    assert ok.all(), "choose another seed for the padding row: a decision margin fell below the bound"
    c["grads"] = {k: v.grad.numpy() for k, v in P.items()}
    c["loss"] = (lp.item(), ln.item())
    lo, grads, _ = Device(c).step(pad=-1)
    assert np.abs(grads[1][c["pad"]]).max() > 0
    _compare(c, lo, grads, padding_row=False)


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism
# ---------------------------------------------------------------------------------------------------------------------
def _bits(loss, grads):
    return [loss.view(np.uint32)] + [g.view(np.uint32) for g in grads]


def test_caser_step_is_deterministic():
    c = cached_case(70, 5, 3, 4, 16, 64, 0.5)
    dev = Device(c)
    a = dev.step()
    b = dev.step()
    assert all(np.array_equal(x, y) for x, y in zip(_bits(*a[:2]), _bits(*b[:2])))
    assert all(np.count_nonzero(g) for g in a[1])
    # device draws under a fixed (seed, step); the flags they used, fed back, give the same bits
    d1 = dev.step(keep=None, keep_out=True, seed=11, step=3)
    d2 = dev.step(keep=None, keep_out=True, seed=11, step=3)
    assert np.array_equal(d1[2], d2[2]) and set(np.unique(d1[2])) <= {0, 1}
    assert all(np.array_equal(x, y) for x, y in zip(_bits(*d1[:2]), _bits(*d2[:2])))
    d3 = dev.step(keep=d1[2], keep_out=True)
    assert np.array_equal(d3[2], d1[2])
    assert all(np.array_equal(x, y) for x, y in zip(_bits(*d1[:2]), _bits(*d3[:2])))
    d4 = dev.step(keep=None, keep_out=True, seed=11, step=4)
    assert not np.array_equal(d4[2], d1[2])


# ---------------------------------------------------------------------------------------------------------------------
# 3. device draws
# ---------------------------------------------------------------------------------------------------------------------
def test_caser_device_draws():
    c = cached_case(70, 5, 3, 4, 16, 64, 0.5)
    dev = Device(c)
    ids = [a.copy() for a in c["clean_ids"]]
    ids[0] = np.arange(70, dtype=np.int32) % c["nU"]
    _, _, k = dev.step(ids=ids, keep=None, keep_out=True, seed=5, step=1)
    F = k.shape[1]
    nU = c["nU"]                                                     # 23 distinct users: the flags are keyed by the user
    frac, sd = k[:nU].mean(), np.sqrt(0.25 / (nU * F))
    print("kept fraction", frac, "sd", sd)
    assert abs(frac - 0.5) < 5 * sd
    assert np.array_equal(k[nU:2 * nU], k[:nU]) and np.array_equal(k[2 * nU:3 * nU], k[:nU])    # the same user, the same flags
    assert 0.3 < k.mean(1).min() and k.mean(1).max() < 0.7 and 0.05 < k[:nU].mean(0).min() and k[:nU].mean(0).max() < 0.95
    # the whole [70, F] block of distinct (user, column) keys: users 0..69 of a larger table
    c2 = dict(c, nU=70)
    raw = dict(c["raw"])
    raw["user_embeddings"] = np.resize(raw["user_embeddings"], (70, c["e"]))
    c2["raw"] = raw
    dev2 = Device(c2)
    ids[0] = np.arange(70, dtype=np.int32)
    _, _, k70 = dev2.step(ids=ids, keep=None, keep_out=True, seed=5, step=1)
    frac, sd = k70.mean(), np.sqrt(0.25 / k70.size)
    print("kept fraction over [70, F]", frac, "sd", sd)
    assert abs(frac - 0.5) < 5 * sd
    # a user's flags do not change when the rest of the batch does
    perm = np.random.default_rng(1).permutation(70)[:33]
    sub = [a[perm] for a in ids]
    sub[1] = sub[1][::-1].copy()                                     # other windows, too
    _, _, ksub = dev2.step(ids=sub, keep=None, keep_out=True, seed=5, step=1)
    assert np.array_equal(ksub, k70[perm])
    # rate 0 keeps all and draws nothing
    _, _, k0 = dev2.step(ids=ids, keep=None, keep_out=True, rate=0.0, seed=5, step=1)
    assert (k0 == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. golden replay of the reference's fit(); 5. the blocked Adam against the dense launch
# ---------------------------------------------------------------------------------------------------------------------
def _write_set(d, root):
    root.mkdir()
    for split in ("train", "test"):
        with open(root / f"{root.name}.{split}", "w") as f:
            for u, i, t in d[split]:
                f.write(f"{int(u)}\t{int(i)}\t1.0\t{int(t)}\n")
    return str(root)


@pytest.fixture()
def seq_dir(tmp_path, golden):
    return _write_set(golden("tiny_seq_dataset"), tmp_path / "tiny_seq")


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="Caser", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    from skrec.recommender.Caser import Caser
    from skrec.utils.py.random import reset_global_sampler
    cfg = dict(T.CONFIG)
    cfg.update(kw)
    reset_global_sampler(2020)
    _seed()
    return Caser(_run_config(data_dir), cfg)


def _fit_and_record(model):
    reports, losses = [], []
    ev, te = model.evaluate, model.train_epoch

    def evaluate(test_users=None):
        r = ev(test_users)
        reports.append(np.array(list(r.values()), np.float32))
        return r

    def train_epoch(it):
        te(it)
        losses.append(model.step_losses.cpu().numpy().copy())
    model.evaluate, model.train_epoch = evaluate, train_epoch
    best = model.fit()
    return np.stack(reports), np.concatenate(losses, 0), np.array(list(best.values()), np.float32)


def _golden_keep(g):
    import torch
    return torch.from_numpy(np.ascontiguousarray(T.unpack_bits(g["keep_bits"], g["keep_shape"]))).cuda()


# parameters whose trajectory would be rounding noise magnified by Adam (a gradient that is exactly zero in exact
# arithmetic): none was found
NOISE_DRIVEN = ()


def _replay(golden, seq_dir, adam_block):
    g = golden("golden_caser")
    m = _model(seq_dir)
    assert m.adam_block == (32 if adam_block is None else int(adam_block))
    assert m.num_items == 97 and m.pad_idx == 96
    names = T.param_names(5)
    p0 = m.reference_parameters()
    for k in names:
        assert np.array_equal(p0[k].cpu().numpy(), g[k + "0"]), k     # same init under the same seed
    assert list(m.evaluator.metrics_list) == list(g["names"])
    assert list(m.user_truncated_seq.keys()) == [int(u) for u in g["trunc_users"]]
    m.keep_in = _golden_keep(g)
    reports, losses, best = _fit_and_record(m)
    assert m._keep_cursor == m.keep_in.shape[0]                      # every recorded flag was consumed
    print("bce sums", losses.ravel(), "golden", g["bce_sums"].ravel())
    assert losses.shape == g["bce_sums"].shape
    np.testing.assert_allclose(losses, g["bce_sums"], rtol=1e-5)
    p1 = {k: v.cpu().numpy() for k, v in m.reference_parameters().items()}
    for k in names:
        print(k, "max abs diff", np.abs(p1[k] - g[k + "1"]).max(), "allowed", 2 * T.TWIN_DEVIATION[k])
    for k in names:
        if k not in NOISE_DRIVEN:
            np.testing.assert_allclose(p1[k], g[k + "1"], rtol=0, atol=2 * T.TWIN_DEVIATION[k], err_msg=k)
    pred = m.predict(list(g["pred_users"]))
    assert pred.shape == (4, 97)
    print("pred max abs diff", np.abs(pred - g["pred"]).max(), "reports max rel", np.abs(reports / g["reports"] - 1).max())
    np.testing.assert_allclose(pred, g["pred"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(reports, g["reports"], rtol=1e-5, atol=0, err_msg=str(g["names"]))
    np.testing.assert_allclose(best, g["best"], rtol=1e-5, atol=0)
    return m


@pytest.mark.parametrize("adam_block", ["8", "3", "1", None])
def test_replays_reference(golden, seq_dir, monkeypatch, tmp_path, adam_block):
    """8 and 3: blocks that do not divide the 9-step run; 1: one dense skr_adam_step_wd per batch; None: the default"""
    monkeypatch.chdir(tmp_path)
    if adam_block is None:
        monkeypatch.delenv("SKR_ADAM_BLOCK", raising=False)
    else:
        monkeypatch.setenv("SKR_ADAM_BLOCK", adam_block)
    _replay(golden, seq_dir, adam_block)


def test_blocked_adam_is_bit_identical_to_the_dense_launch(golden, seq_dir, monkeypatch, tmp_path):
    """the same 9 steps under SKR_ADAM_BLOCK = 1, 8 and 3: every parameter and both moments, bit for bit -- the check that a
    W2 row's two blocks and the shared block are named"""
    import torch
    monkeypatch.chdir(tmp_path)
    g = golden("golden_caser")
    runs = []
    for blk in ("1", "8", "3"):
        monkeypatch.setenv("SKR_ADAM_BLOCK", blk)
        m = _model(seq_dir)
        assert m.adam_block == int(blk) and m.optimizer.weight_decay == 1e-6
        m.keep_in = _golden_keep(g)
        it = m._make_iterator()
        for _ in range(3):
            m.train_epoch(it)
        torch.cuda.synchronize()
        o = m.optimizer
        assert o.t == 9 and float(o.grad.abs().max()) == 0.0         # every gradient was consumed
        runs.append((o.flat.clone(), o.m.clone(), o.v.clone(), m.step_losses.cpu().numpy()))
    for fb, mb, vb, lb in runs[1:]:
        fa, ma, va, la = runs[0]
        print("p/m/v differing elements", int((fa != fb).sum()), int((ma != mb).sum()), int((va != vb).sum()))
        assert torch.equal(fa, fb) and torch.equal(ma, mb) and torch.equal(va, vb)
        assert np.array_equal(la, lb)


# ---------------------------------------------------------------------------------------------------------------------
# 6. query rows against float64; the evaluator's device rows against predict()'s dense matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("L,e,nv,nh", [(5, 64, 4, 16), (1, 16, 1, 1), (8, 40, 8, 32)])
def test_caser_queries_match_float64(L, e, nv, nh, with_list):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(L + e)
    nU, nI = 301, 200
    pad = nI
    raw = T.random_params(rng, nU, nI, e, L, nv, nh)
    raw["item_embeddings"][pad] = 0.0
    users = rng.permutation(nU)[:77].astype(np.int32) if with_list else np.arange(nU, dtype=np.int32)
    n = len(users)
    win = rng.integers(0, nI, (n, L)).astype(np.int32)
    for r in range(0, n, 2):                               # short histories: left padding
        win[r, :rng.integers(0, L)] = pad
    win[5::10] = -1                                        # users without history
    if with_list:
        users[3] = nU + 2                                  # a user out of range: skipped
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()    # noqa: E731
    dP, dE, dS = d(T.pad_cols(raw["user_embeddings"], 64)), d(T.pad_cols(raw["item_embeddings"], 64)), d(T.shared_block(raw, e, L, nv, nh))
    Q = torch.full((nU + 1, 128), 7.0, device="cuda")
    du, dw = d(users), d(win)
    # a workspace of 128 users' worth: the 301 users go through it in three chunks
    nbytes = 128 * (4 * T.caser_fp(L, nv, nh) + 4) + 16
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _hip.check(_hip.lib().skr_caser_queries(_hip.ptr(dP), _hip.ptr(dE), _hip.ptr(dS), _hip.ptr(du) if with_list else None, n,
                                            _hip.ptr(dw), nU, nI + 1, pad, 64, e, L, nv, nh, _hip.ptr(work), nbytes, _hip.ptr(Q),
                                            _hip.stream()))
    got = Q.cpu().numpy()
    assert (got[nU] == 7.0).all()                          # nothing written beyond the user table
    inr = users < nU
    untouched = np.setdiff1d(np.arange(nU), users[inr])
    assert (got[untouched] == 7.0).all()
    ok = (win[:, 0] >= 0) & inr
    none = (win[:, 0] < 0) & inr
    assert np.isnan(got[users[none]]).all() and ok.sum() > 0 and none.sum() > 0
    P = T.to_torch(raw, requires_grad=False)
    want = T.query_rows(P, torch.from_numpy(users[ok]).long(), torch.from_numpy(win[ok]).long(), pad).numpy()
    have = np.concatenate([got[users[ok], :e], got[users[ok], 64:64 + e]], 1)
    print("max abs err", np.abs(have - want).max(), "max |x|", np.abs(want).max())
    np.testing.assert_allclose(have, want, rtol=1e-5, atol=2e-6 * max(1.0, np.abs(want).max()))
    assert not got[users[ok], e:64].any() and not got[users[ok], 64 + e:].any()


class _PredictOnly(object):
    """the reference's evaluator contract only: predict() -> ndarray (the generic path)"""

    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def test_device_score_rows_equal_the_dense_matrix(seq_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(seq_dir, epochs=1, embed_size=40, seq_L=4, nh=5)
    m.fit()
    ev = m.evaluator
    users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    rows_dev, sums_dev, n_dev = ev.per_user_rows(m, users)
    rows_gen, sums_gen, n_gen = ev.per_user_rows(_PredictOnly(m), users)
    assert n_dev == n_gen == len(users) == 62
    assert rows_dev.shape == rows_gen.shape
    assert np.array_equal(rows_dev, rows_gen)
    r = m.evaluate()
    assert r["NDCG@10"] == m.evaluate()["NDCG@10"]
    # the query rows are kept between evaluations and dropped by a training step
    assert m._q_current
    q0 = m.predict_factors()[0].clone()
    m.train_epoch(m._make_iterator())
    assert not m._q_current
    assert not np.array_equal(m.predict_factors()[0].cpu().numpy(), q0.cpu().numpy())
    # the views at a width below 64: the reference's shapes
    p = m.reference_parameters()
    assert tuple(p["fc1_weight"].shape) == (40, 4 * 40 + 5 * 4) and tuple(m.W2.shape) == (97, 80)
    assert tuple(m.conv_h_weight[3].shape) == (5, 1, 4, 40) and tuple(m.item_embeddings.shape) == (97, 40)


# ---------------------------------------------------------------------------------------------------------------------
# 7. a test user without training history: the reference's KeyError; limits; the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_user_without_history_raises_key_error(tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(tiny_dir, epochs=1)
    assert m.predict([0, 3]).shape == (2, m.num_items) and m.num_items == 97
    with pytest.raises(KeyError) as e:
        m.predict([63])
    assert e.value.args == (63,)
    with pytest.raises(KeyError) as e:
        m.evaluate()
    assert e.value.args == (63,)


def test_limits_are_named(seq_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="embed_size <= 64"):
        _model(seq_dir, embed_size=65)
    for kw, match in ((dict(seq_L=9), "seq_L <= 8"), (dict(seq_T=17), "seq_T <= 16"), (dict(nv=9), "nv <= 8"),
                      (dict(nh=33), "nh <= 32"), (dict(batch_size=4096), "batch_size <= 2048")):
        with pytest.raises(ValueError, match=match):
            _model(seq_dir, **kw)


def test_run_skrec_cli(seq_dir, tmp_path):
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "Caser", "--data_dir", seq_dir, "--seq_L", "4", "--seq_T", "2",
                        "--nh", "8", "--epochs", "2", "--batch_size", "256", "--top_k", "[5,10]", "--metric", "['Recall','NDCG']",
                        "--seed", "7"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 1:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout
    logs = list((tmp_path / "log").rglob("*.log"))
    assert len(logs) == 1 and "NDCG@10" in logs[0].read_text()
