"""GPU suite of HGN (csrc/hgn.hip, the weight-decay Adam of csrc/adam.hip, skrec/recommender/HGN.py): golden replay of
the reference's fit(), the step kernel against float64 autograd of a plain-torch restatement, the ordered gate
gradients, skr_adam_step_wd against torch and the blocked form against the dense one, the query rows against float64
numpy, the evaluator's fused path against its generic one, the reference's KeyError, and the command line."""
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
PARAMS = ("user_embeddings", "item_embeddings", "feature_gate_item_weight", "feature_gate_item_bias",
          "feature_gate_user_weight", "feature_gate_user_bias", "instance_gate_item", "instance_gate_user", "W2", "b2")


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _write_set(d, root):
    root.mkdir()
    for split in ("train", "test"):
        with open(root / f"{root.name}.{split}", "w") as f:
            for u, i, t in d[split]:
                f.write(f"{int(u)}\t{int(i)}\t1.0\t{int(t)}\n")
    return str(root)


@pytest.fixture()
def seq_dir(tmp_path, golden):
    """tiny_dataset without user 63's test rows (that user has no training history), in the reference's TSV format"""
    return _write_set(golden("tiny_seq_dataset"), tmp_path / "tiny_seq")


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="HGN", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    from skrec.recommender.HGN import HGN
    from skrec.utils.py.random import reset_global_sampler
    cfg = dict(lr=1e-3, reg=1e-3, seq_L=5, seq_T=3, embed_size=64, batch_size=256, epochs=3)
    cfg.update(kw)
    reset_global_sampler(2020)
    _seed()
    return HGN(_run_config(data_dir), cfg)


def _tables(m):
    return {k: getattr(m, k) for k in PARAMS}


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


# ---------------------------------------------------------------------------------------------------------------------
# 1. golden replay of the reference's fit()
# ---------------------------------------------------------------------------------------------------------------------
def _replay(golden, seq_dir, adam_block):
    g = golden("golden_hgn")
    m = _model(seq_dir)
    assert m.adam_block == (32 if adam_block is None else int(adam_block))
    assert m.num_items == 97 and m.pad_idx == 96
    for k, t in _tables(m).items():
        assert np.array_equal(t.cpu().numpy(), g[k + "0"]), k          # same init under the same seed
    assert list(m.evaluator.metrics_list) == list(g["names"])
    assert list(m.user_truncated_seq.keys()) == [int(u) for u in g["trunc_users"]]
    reports, losses, best = _fit_and_record(m)
    print("bpr_sum", losses[:, 0], "golden", g["bpr_sum"])
    print("reports max rel", np.abs(reports / g["reports"] - 1).max())
    assert losses.shape[0] == len(g["bpr_sum"])
    np.testing.assert_allclose(losses[:, 0], g["bpr_sum"], rtol=1e-5)
    assert not losses[:, 1].any()                                      # no l2 term: the regulariser is the weight decay
    for k, t in _tables(m).items():
        print(k, "max abs diff", np.abs(t.cpu().numpy() - g[k + "1"]).max())
    for k, t in _tables(m).items():
        np.testing.assert_allclose(t.cpu().numpy(), g[k + "1"], rtol=0, atol=2e-6, err_msg=k)
    pred = m.predict(list(g["pred_users"]))
    assert pred.shape == (4, 97) and not pred[:, 96].any()             # the padding item's column: b2[pad] = 0
    np.testing.assert_allclose(pred, g["pred"], rtol=1e-4, atol=1e-6)
    return reports, best, g


@pytest.mark.parametrize("adam_block", ["8", "3", "1"])
def test_replays_reference(golden, seq_dir, monkeypatch, tmp_path, adam_block):
    """8 and 3: blocks that do not divide the 9-step run; 1: one dense skr_adam_step_wd per batch"""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SKR_ADAM_BLOCK", adam_block)
    reports, best, g = _replay(golden, seq_dir, adam_block)
    np.testing.assert_allclose(reports, g["reports"], rtol=1e-5, atol=0, err_msg=str(g["names"]))
    np.testing.assert_allclose(best, g["best"], rtol=1e-5, atol=0)


def test_replays_reference_default_block(golden, seq_dir, monkeypatch, tmp_path, fused_mode):
    """the shipped default (blocks of 32 batches) under every arithmetic of the fused evaluator"""
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SKR_ADAM_BLOCK", raising=False)
    reports, best, g = _replay(golden, seq_dir, None)
    np.testing.assert_allclose(reports, g["reports"], rtol=1e-5, atol=0, err_msg=str(g["names"]))
    np.testing.assert_allclose(best, g["best"], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the step kernel against float64 autograd of a plain restatement of the model
# ---------------------------------------------------------------------------------------------------------------------
def _restated_query(P, E, Wi, bi, Wu, bu, wi, Wiu, u, seq, pad, numerator_only=False):
    """q = p + union + sum_l e_l for float64 torch tensors; the window's padding positions read as zero rows
    (``numerator_only``: the instance gates of the denominator are constants for autograd)"""
    import torch
    p = P[u]
    e = E[seq] * (seq != pad).unsqueeze(-1)
    gate = torch.sigmoid(e @ Wi.T + bi + (p @ Wu.T + bu).unsqueeze(1))
    g = e * gate
    a = torch.sigmoid((g @ wi).squeeze(-1) + p @ Wiu)
    union = (a.unsqueeze(-1) * g).sum(1) / (a.detach() if numerator_only else a).sum(1, keepdim=True)
    return p + union + e.sum(1)


def _pad2(a, rows, cols):
    out = np.zeros((rows, cols), np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def _gate_block(Wi, bi, Wu, bu, wi, Wiu):
    """skr_hgn_step's layout of the shared parameters, from arrays of width e"""
    L = Wiu.shape[1]
    return np.concatenate([_pad2(Wi, 64, 64).ravel(), _pad2(Wu, 64, 64).ravel(), _pad2(bi[None], 1, 64).ravel(),
                           _pad2(bu[None], 1, 64).ravel(), _pad2(wi.T, 1, 64).ravel(), _pad2(Wiu.T, L, 64).ravel()])


def _hgn_case(rng, nU, nI, n, L, T, width):
    """tables of ``width`` columns and a batch with repeated users and items, windows with padding (one of them all
    padding but the last position) and a positive that also sits in its window"""
    pad = nI
    s = 0.3
    P = (rng.standard_normal((nU, width)) * s).astype(np.float32)
    E = (rng.standard_normal((nI + 1, width)) * s).astype(np.float32)
    W2 = (rng.standard_normal((nI + 1, width)) * s).astype(np.float32)
    b2 = (rng.standard_normal(nI + 1) * s).astype(np.float32)
    E[pad], W2[pad], b2[pad] = 0.0, 0.0, 0.0
    Wi, Wu = ((rng.standard_normal((width, width)) * s).astype(np.float32) for _ in range(2))
    bi, bu = ((rng.standard_normal(width) * s).astype(np.float32) for _ in range(2))
    wi = (rng.standard_normal((width, 1)) * s).astype(np.float32)
    Wiu = (rng.standard_normal((width, L)) * s).astype(np.float32)
    u = rng.integers(0, nU, n).astype(np.int32)
    seq = rng.integers(0, nI, (n, L)).astype(np.int32)
    pos, neg = (rng.integers(0, nI, (n, T)).astype(np.int32) for _ in range(2))
    u[1::5] = u[0]
    pos[2::9, 0] = pos[1 % n, 0]
    neg[::7, T - 1] = seq[::7, L - 1]
    pos[::4, 0] = seq[::4, L - 1]                                    # a positive equal to a window item
    for r in range(0, n, 3):                                        # left padding of varying length
        seq[r, :rng.integers(0, L)] = pad
    seq[n - 1, :L - 1] = pad                                        # all but one
    return pad, (P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu), (u, seq, pos, neg)


@pytest.mark.parametrize("n", [700, 3])
@pytest.mark.parametrize("width", [16, 64])
@pytest.mark.parametrize("L,T", [(1, 1), (5, 3), (8, 2)])
def test_hgn_step_matches_float64_autograd(L, T, width, n):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(1000 * L + 10 * T + width + n)
    nU, nI = 50, 80
    pad, par, ids = _hgn_case(rng, nU, nI, n, L, T, width)
    P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu = par
    dP, dE, dW2 = (torch.from_numpy(_pad2(t, t.shape[0], 64)).cuda() for t in (P, E, W2))
    db2 = torch.from_numpy(b2).cuda()
    dG = torch.from_numpy(_gate_block(Wi, bi, Wu, bu, wi, Wiu)).cuda()
    ng = _hip.hgn_gate_floats(L)
    assert dG.numel() == ng
    grads = [torch.zeros_like(t) for t in (dP, dE, dW2, db2, dG)]
    work = torch.empty(_hip.SKR_HGN_MAX_BLOCKS * ng, device="cuda")
    d_ids = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ids]
    loss = torch.zeros(2, device="cuda")
    _hip.check(_hip.lib().skr_hgn_step(*[_hip.ptr(t) for t in (dP, dE, dW2, db2, dG)], *[_hip.ptr(t) for t in d_ids], n, nU,
                                       nI + 1, pad, 64, L, T, *[_hip.ptr(t) for t in grads], _hip.ptr(work), _hip.ptr(loss), 1,
                                       _hip.stream()))
    torch.cuda.synchronize()
    t64 = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in par]
    tP, tE, tW2, tb2, tWi, tbi, tWu, tbu, twi, tWiu = t64
    U_, S_, P_, N_ = (torch.from_numpy(a).long() for a in ids)
    q = _restated_query(tP, tE, tWi, tbi, tWu, tbu, twi, tWiu, U_, S_, pad)
    yp = (tW2[P_] * q.unsqueeze(1)).sum(-1) + tb2[P_]
    yn = (tW2[N_] * q.unsqueeze(1)).sum(-1) + tb2[N_]
    bpr = -torch.nn.functional.logsigmoid(yp - yn).sum()
    bpr.backward()
    # With a window of ONE position the instance gate cancels out of the union (a g / a): the gradients of the two
    # instance-gate parameters are identically zero, and what either program returns is the rounding residue of two terms
    # that cancel (1e-17 in float64, 1e-8 in fp32), so max|grad| is no scale for them.  Their scale is the size of the
    # terms that cancel: the gradient through the numerator alone.
    cancel = {}
    if L == 1:
        assert float(twi.grad.abs().max()) < 1e-12 and float(tWiu.grad.abs().max()) < 1e-12
        qn = _restated_query(tP, tE, tWi, tbi, tWu, tbu, twi, tWiu, U_, S_, pad, numerator_only=True)
        ln = -torch.nn.functional.logsigmoid(((tW2[P_] - tW2[N_]) * qn.unsqueeze(1)).sum(-1) + tb2[P_] - tb2[N_]).sum()
        gn = torch.autograd.grad(ln, [twi, tWiu])
        cancel = {"wi": float(gn[0].abs().max()), "Wiu": float(gn[1].abs().max())}
        assert min(cancel.values()) > 1e-6
    got = loss.cpu().numpy()
    print("loss", got[0], bpr.item())
    np.testing.assert_allclose(got[0], bpr.item(), rtol=1e-5)
    assert got[1] == 0.0
    gP, gE, gW2, gb2, gG = (t.cpu().numpy() for t in grads)
    gm = gG[:8192].reshape(2, 64, 64)
    gv = gG[8192:8384].reshape(3, 64)
    checks = [("P", gP, tP.grad), ("E", gE, tE.grad), ("W2", gW2, tW2.grad), ("b2", gb2[:, None], tb2.grad[:, None]),
              ("Wi", gm[0], tWi.grad), ("Wu", gm[1], tWu.grad), ("bi", gv[0][None], tbi.grad[None]),
              ("bu", gv[1][None], tbu.grad[None]), ("wi", gv[2][None], twi.grad.T), ("Wiu", gG[8384:].reshape(L, 64), tWiu.grad.T)]
    for name, g, want in checks:
        w = want.numpy()
        r, c = w.shape
        print(name, "max abs err", np.abs(g[:r, :c] - w).max(), "max |grad|", np.abs(w).max())
    for name, g, want in checks:
        w = want.numpy()
        r, c = w.shape
        np.testing.assert_allclose(g[:r, :c], w, rtol=1e-4, atol=2e-5 * max(np.abs(w).max(), cancel.get(name, 0.0)),
                                   err_msg=name)
        assert not g[:, c:].any() and not g[r:].any(), name         # padded columns (and rows) get no gradient
    assert not gE[pad].any() and not gW2[pad].any() and gb2[pad] == 0.0        # nor do the padding rows


# ---------------------------------------------------------------------------------------------------------------------
# 3. the shared parameters' gradients do not depend on timing
# ---------------------------------------------------------------------------------------------------------------------
def test_hgn_gate_gradients_are_deterministic():
    import torch
    from skrec import _hip
    rng = np.random.default_rng(7)
    nU, nI, n, L, T = 3000, 2000, 6000, 5, 3       # 1500 wavefront-batches: more than SKR_HGN_MAX_BLOCKS workgroups
    assert (n + 3) // 4 > _hip.SKR_HGN_MAX_BLOCKS
    pad, par, ids = _hgn_case(rng, nU, nI, n, L, T, 64)
    P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu = par
    tabs = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (P, E, W2, b2, _gate_block(Wi, bi, Wu, bu, wi, Wiu))]
    d_ids = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ids]
    ng = _hip.hgn_gate_floats(L)
    work = torch.empty(_hip.SKR_HGN_MAX_BLOCKS * ng, device="cuda")
    outs = []
    for _ in range(2):
        grads = [torch.zeros_like(t) for t in tabs]
        loss = torch.zeros(2 * _hip.SKR_LOSS_SLOTS, device="cuda")
        _hip.check(_hip.lib().skr_hgn_step(*[_hip.ptr(t) for t in tabs], *[_hip.ptr(t) for t in d_ids], n, nU, nI + 1, pad, 64,
                                           L, T, *[_hip.ptr(t) for t in grads], _hip.ptr(work), _hip.ptr(loss),
                                           _hip.SKR_LOSS_SLOTS, _hip.stream()))
        outs.append(grads[4].cpu().numpy())
    assert np.count_nonzero(outs[0]) > 0.99 * outs[0].size
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 4. weight-decay Adam: the dense launch against torch, the blocked form against the dense one bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_adam_wd_matches_torch_cpu():
    import torch
    from skrec import _hip
    rng = np.random.default_rng(11)
    n, lr, wd = 4096 + 3, 1e-2, 1e-2
    p0 = rng.standard_normal(n).astype(np.float32)
    p0[::13] = 0.0                                          # exact-zero parameters
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([ref], lr=lr, weight_decay=wd)
    p = torch.from_numpy(p0.copy()).cuda()
    g, m, v = (torch.zeros_like(p) for _ in range(3))
    for t in range(1, 6):
        grad = rng.standard_normal(n).astype(np.float32)
        grad[rng.random(n) < 0.4] = 0.0                     # zero-gradient elements
        ref.grad = torch.from_numpy(grad.copy())
        opt.step()
        g.copy_(torch.from_numpy(grad))
        _hip.check(_hip.lib().skr_adam_step_wd(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), n, lr, 0.9, 0.999, 1e-8, wd,
                                               t, 1, None, _hip.stream()))
        assert float(g.abs().max()) == 0.0
        diff = np.abs(p.cpu().numpy() - ref.detach().numpy()).max()
        print("step", t, "max abs diff", diff)
        np.testing.assert_allclose(p.cpu().numpy(), ref.detach().numpy(), rtol=1e-6, atol=1e-7)
    st = opt.state[ref]
    np.testing.assert_allclose(m.cpu().numpy(), st["exp_avg"].numpy(), rtol=1e-6, atol=1e-7)
    # the library receives beta2 as a float, like skr_adam_step: its 1 - float(0.999) = 0.00099998713 stands against torch's
    # float(1 - 0.999) = 0.001, 1.29e-5 relative, and v is linear in that factor (sqrt(v) moves by half of it, the
    # parameters by 6.4e-6 of a step of lr: inside their tolerance above)
    np.testing.assert_allclose(v.cpu().numpy(), st["exp_avg_sq"].numpy(), rtol=1.29e-5 + 1e-6, atol=1e-7)


class _DistinctRowsEpoch(object):
    """an epoch of (user, window, positives, negatives) batches whose rows are distinct within a batch (every float
    atomic of a step then happens once: the gradients are deterministic and the comparison isolates the optimiser);
    some windows start with the padding item, the last batch is short"""

    def __init__(self, nU, nI, pad, L, T, bsz, n_steps, seed):
        import torch
        rng = np.random.default_rng(seed)
        assert bsz * (L + 2 * T) <= nI and bsz <= nU
        cols = [[], [], [], []]
        for s in range(n_steps):
            m = bsz if s < n_steps - 1 else max(1, bsz // 3)
            it = rng.permutation(nI)[:m * (L + 2 * T)].reshape(m, L + 2 * T)
            seq = it[:, :L].copy()
            if L > 1:
                seq[::3, 0] = pad
            for c, a in zip(cols, (rng.permutation(nU)[:m], seq, it[:, L:L + T], it[:, L + T:])):
                c.append(a)
        self.cols = [torch.from_numpy(np.ascontiguousarray(np.concatenate(c).astype(np.int32))).cuda() for c in cols]
        n = self.cols[0].shape[0]
        self.batch_size = bsz
        self.bounds = [(a, min(a + bsz, n)) for a in range(0, n, bsz)]

    def epoch_columns(self):
        return self.cols, self.bounds


@pytest.mark.parametrize("k", ["8", "3"])
def test_blocked_adam_wd_is_bit_identical(seq_dir, monkeypatch, tmp_path, k):
    import torch
    monkeypatch.chdir(tmp_path)
    runs = []
    for blk in ("1", k):
        monkeypatch.setenv("SKR_ADAM_BLOCK", blk)
        m = _model(seq_dir, batch_size=8)
        assert m.adam_block == int(blk) and m.optimizer.weight_decay == 1e-3
        ep = _DistinctRowsEpoch(m.num_users, m.num_items - 1, m.pad_idx, 5, 3, 8, 11, seed=5)
        for _ in range(2):
            m.train_epoch(ep)
        torch.cuda.synchronize()
        o = m.optimizer
        runs.append((o.flat.clone(), o.m.clone(), o.v.clone(), o.t, m.step_losses.cpu().numpy()))
        assert float(o.grad.abs().max()) == 0.0          # every gradient was consumed
        assert not m.item_embeddings[m.pad_idx].any() and not m.W2[m.pad_idx].any()
    (fa, ma, va, ta, la), (fb, mb, vb, tb, lb) = runs
    assert ta == tb == 22
    print("p/m/v differing elements", int((fa != fb).sum()), int((ma != mb).sum()), int((va != vb).sum()))
    assert torch.equal(fa, fb) and torch.equal(ma, mb) and torch.equal(va, vb)
    np.testing.assert_allclose(la, lb, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 5. query rows against float64 numpy; the evaluator's fused path against its generic path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("L,width", [(5, 64), (1, 16), (32, 40)])
def test_hgn_queries_match_float64(L, width, with_list):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(L + width)
    nU, nI = 301, 200
    pad, par, _ = _hgn_case(rng, nU, nI, 8, L, 1, width)
    P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu = par
    users = rng.permutation(nU)[:77].astype(np.int32) if with_list else np.arange(nU, dtype=np.int32)
    n = len(users)
    win = rng.integers(0, nI, (n, L)).astype(np.int32)
    for r in range(0, n, 2):                               # short histories: left padding
        win[r, :rng.integers(0, L)] = pad
    win[5::10] = -1                                        # users without history
    dP, dE = (torch.from_numpy(_pad2(t, t.shape[0], 64)).cuda() for t in (P, E))
    dG = torch.from_numpy(_gate_block(Wi, bi, Wu, bu, wi, Wiu)).cuda()
    Q = torch.full((nU + 1, 64), 7.0, device="cuda")
    du, dw = torch.from_numpy(users).cuda(), torch.from_numpy(win).cuda()
    _hip.check(_hip.lib().skr_hgn_queries(_hip.ptr(dP), _hip.ptr(dE), _hip.ptr(dG), _hip.ptr(du) if with_list else None, n,
                                          _hip.ptr(dw), nU, nI + 1, pad, 64, L, _hip.ptr(Q), _hip.stream()))
    got = Q.cpu().numpy()
    assert (got[nU] == 7.0).all()                          # nothing written beyond the user table
    untouched = np.setdiff1d(np.arange(nU), users)
    assert (got[untouched] == 7.0).all()
    ok = win[:, 0] >= 0
    assert np.isnan(got[users[~ok]]).all() and ok.sum() > 0 and (~ok).sum() > 0
    t64 = [torch.tensor(a, dtype=torch.float64) for a in (P, E, Wi, bi, Wu, bu, wi, Wiu)]
    want = _restated_query(*t64, torch.from_numpy(users[ok]).long(), torch.from_numpy(win[ok]).long(), pad).numpy()
    print("max abs err", np.abs(got[users[ok], :width] - want).max())
    np.testing.assert_allclose(got[users[ok], :width], want, rtol=1e-5, atol=2e-6)
    assert not got[users[ok], width:].any()


class _PredictOnly(object):
    """the reference's evaluator contract only: predict() -> ndarray (the generic path)"""

    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def test_fused_path_equals_generic_path(seq_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SKR_FUSED_MODE", "fp32")
    m = _model(seq_dir, epochs=1)
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


# ---------------------------------------------------------------------------------------------------------------------
# 6. a test user without training history: the reference's KeyError; limits; the command line
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
    with pytest.raises(ValueError, match="seq_L <= 32"):
        _model(seq_dir, seq_L=33)
    with pytest.raises(ValueError, match="seq_T <= 16"):
        _model(seq_dir, seq_T=17)


def test_run_skrec_cli(seq_dir, tmp_path):
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "HGN", "--data_dir", seq_dir, "--seq_L", "4", "--seq_T", "2",
                        "--epochs", "2", "--batch_size", "256", "--top_k", "[5,10]", "--metric", "['Recall','NDCG']",
                        "--seed", "7"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 1:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout
    logs = list((tmp_path / "log").rglob("*.log"))
    assert len(logs) == 1 and "NDCG@10" in logs[0].read_text()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
NU, NI = 50, 80
GRADS = ("P", "E", "W2", "b2", "Wi", "Wu", "bi", "bu", "wi", "Wiu")


def _hgn_device(par, ids, L, T, pad, n=None, slots=1, loss=None):
    """one skr_hgn_step on zeroed gradients -> ([gP, gE, gW2, gb2, gG] on the host, the loss words)"""
    import torch
    from skrec import _hip
    P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu = par
    tabs = [torch.from_numpy(_pad2(t, t.shape[0], 64)).cuda() for t in (P, E, W2)]
    tabs += [torch.from_numpy(b2).cuda(), torch.from_numpy(_gate_block(Wi, bi, Wu, bu, wi, Wiu)).cuda()]
    ng = _hip.hgn_gate_floats(L)
    assert tabs[4].numel() == ng
    grads = [torch.zeros_like(t) for t in tabs]
    work = torch.full((_hip.SKR_HGN_MAX_BLOCKS * ng,), float("nan"), device="cuda")      # no initial contents
    d_ids = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in ids]
    loss = torch.zeros(2 * slots, device="cuda") if loss is None else loss
    n = len(ids[0]) if n is None else n
    _hip.check(_hip.lib().skr_hgn_step(*[_hip.ptr(t) for t in tabs], *[_hip.ptr(t) for t in d_ids], n, P.shape[0], E.shape[0], pad,
                                       64, L, T, *[_hip.ptr(t) for t in grads], _hip.ptr(work), _hip.ptr(loss), slots,
                                       _hip.stream()))
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], loss.cpu().numpy()


def _hgn_twin(par, ids, pad, ok):
    """float64 autograd of the restatement on the instances ``ok`` (the loss is a sum: no divisor) -> (loss, {name: gradient});
    the padding row of W2 and b2 gets no gradient, whatever names it"""
    import torch
    t64 = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in par]
    tP, tE, tW2, tb2, tWi, tbi, tWu, tbu, twi, tWiu = t64
    U_, S_, P_, N_ = (torch.from_numpy(np.asarray(a)[ok]).long() for a in ids)
    q = _restated_query(tP, tE, tWi, tbi, tWu, tbu, twi, tWiu, U_, S_, pad)
    yp = (tW2[P_] * q.unsqueeze(1)).sum(-1) + tb2[P_]
    yn = (tW2[N_] * q.unsqueeze(1)).sum(-1) + tb2[N_]
    bpr = -torch.nn.functional.logsigmoid(yp - yn).sum()
    bpr.backward()
    g = {k: (np.zeros(t.shape) if t.grad is None else t.grad.numpy().copy())
         for k, t in zip(("P", "E", "W2", "b2", "Wi", "bi", "Wu", "bu", "wi", "Wiu"), t64)}
    if pad >= 0:
        g["W2"][pad], g["b2"][pad] = 0.0, 0.0
    return bpr.item(), g


def _hgn_edge_compare(what, par, ids, L, T, pad, ok=None, gates_only=False):
    """the device step against the twin on the instances ``ok`` (all when None) with the suite's bounds; then the rows that
    no instance of ``ok`` names, the padded columns and the padding rows are exactly zero.  Prints one ``edge-error`` line
    per tensor (collected into profiles/scaffold_edges_errors.txt)"""
    n = len(ids[0])
    ok = np.ones(n, bool) if ok is None else ok
    want_loss, G = _hgn_twin(par, ids, pad, ok)
    assert np.isfinite(want_loss) and all(np.isfinite(v).all() for v in G.values())
    (gP, gE, gW2, gb2, gG), loss = _hgn_device(par, ids, L, T, pad)
    print(what, "loss", loss[0], want_loss)
    np.testing.assert_allclose(loss[0], want_loss, rtol=1e-5, err_msg=what)
    assert loss[1] == 0.0
    gm, gv = gG[:8192].reshape(2, 64, 64), gG[8192:8384].reshape(3, 64)
    checks = [("P", gP, G["P"]), ("E", gE, G["E"]), ("W2", gW2, G["W2"]), ("b2", gb2[:, None], G["b2"][:, None]),
              ("Wi", gm[0], G["Wi"]), ("Wu", gm[1], G["Wu"]), ("bi", gv[0][None], G["bi"][None]), ("bu", gv[1][None], G["bu"][None]),
              ("wi", gv[2][None], G["wi"].T), ("Wiu", gG[8384:].reshape(L, 64), G["Wiu"].T)]
    if gates_only:
        checks = checks[4:]
    for name, g, w in checks:                       # every tensor is measured before the assertion
        r, c = w.shape
        print(f"edge-error HGN | {what} | {name} | {np.abs(g[:r, :c] - w).max():.3e} | {np.abs(w).max():.3e}")
    for name, g, w in checks:
        r, c = w.shape
        assert np.isfinite(g).all(), (what, name)
        np.testing.assert_allclose(g[:r, :c], w, rtol=1e-4, atol=2e-5 * np.abs(w).max(), err_msg=f"{what}: {name}")
        assert not g[:, c:].any() and not g[r:].any(), (what, name)
    u, seq, pos, neg = (np.asarray(a)[ok] for a in ids)
    named_u, named_e, named_w = (np.zeros(k, bool) for k in (par[0].shape[0], par[1].shape[0], par[1].shape[0]))
    named_u[u] = True
    named_e[seq[seq != pad]] = True
    named_w[np.concatenate([pos.ravel(), neg.ravel()])] = True
    if pad >= 0:
        named_w[pad] = False
    assert not gP[~named_u].any() and not gE[~named_e].any() and not gW2[~named_w].any() and not gb2[~named_w].any(), what
    return named_u, named_e, named_w


@pytest.mark.parametrize("width", [64, 24])
@pytest.mark.parametrize("L,T", [(16, 4), (17, 5), (32, 16), (3, 8)])
def test_window_and_target_counts_at_their_edges(L, T, width):
    """a window that exactly fills the LDS stage of 16 positions, one position past it (window_row's read from global memory),
    both maxima at once; targets on and past load_pairs' group of four.  Past the stage the windows hold items and padding"""
    rng = np.random.default_rng(100 * L + T + width)
    pad, par, ids = _hgn_case(rng, NU, NI, 37, L, T, width)
    seq = ids[1]
    if L > 16:
        seq[5, 16:] = rng.integers(0, NI, L - 16)
        seq[5, 16 + (L - 16) // 2] = pad                      # padding past the stage, between items
        seq[8, L - 1] = pad                                   # ... and in the last position
        assert (seq[:, 16:] != pad).sum() > 20 and (seq[:, 16:] == pad).sum() >= 2
        assert (seq[:, 16:] != pad).any(1).sum() > 30 and (seq[:, L - 1] != pad).sum() > 30
    _hgn_edge_compare(f"L = {L}, T = {T}, width = {width}", par, ids, L, T, pad)


@pytest.mark.parametrize("n", [1, 2, 4, 5, 4 * 256 - 1, 4 * 256, 4 * 256 + 1, 4 * 256 + 70])
def test_instance_counts_around_the_grid(n):
    """fewer instances than a workgroup has wavefronts, one workgroup exactly, one instance more; SKR_HGN_MAX_BLOCKS
    workgroups less one instance, exactly, and the grid-stride loop's second trip for one and for 70 instances"""
    from skrec import _hip
    assert _hip.SKR_HGN_MAX_BLOCKS == 256
    pad, par, ids = _hgn_case(np.random.default_rng(200 + n), NU, NI, n, 5, 3, 64)
    _hgn_edge_compare(f"n = {n}", par, ids, 5, 3, pad)


@pytest.mark.parametrize("n", [61, 64, 65, 253, 257])
def test_partial_counts_around_the_reduction(n):
    """16, 16, 17, 64 and 65 workgroup partials: on either side of hgn_reduce_kernel's R_WAVES wavefronts and of its
    four-way unrolled trip; the gate block's gradients against the twin"""
    pad, par, ids = _hgn_case(np.random.default_rng(300 + n), NU, NI, n, 5, 3, 64)
    _hgn_edge_compare(f"{(n + 3) // 4} partials", par, ids, 5, 3, pad, gates_only=True)


def _without(ids, users, items, rng):
    """the batch with every occurrence of ``users`` / ``items`` replaced by other ids"""
    u, seq, pos, neg = ids
    u[np.isin(u, users)] = 0
    for a in (seq, pos, neg):
        hit = np.isin(a, items)
        a[hit] = rng.integers(0, 60, hit.sum())


def test_ids_out_of_range_skip_their_instance():
    """one bad id per instance: d_u (instance 0 and n - 1), the first and the last position of a window, the first and the
    last positive, the first and the last negative; below 0 and equal to n_users / n_rows.  The result is that of the batch
    without those eight instances; instance 3 alone names user 49 and the items 77, 78, 79: their rows stay exactly zero"""
    rng = np.random.default_rng(400)
    n, L, T = 37, 5, 3
    pad, par, ids = _hgn_case(rng, NU, NI, n, L, T, 64)
    _without(ids, [49], [77, 78, 79], rng)
    u, seq, pos, neg = ids
    u[3], seq[3, 1], pos[3, 1], neg[3, 1] = 49, 79, 78, 77
    n_rows = NI + 1
    u[0], u[n - 1] = -1, NU
    seq[3, 0], seq[7, L - 1] = -2, n_rows
    pos[10, 0], pos[13, T - 1] = -1, n_rows
    neg[20, 0], neg[25, T - 1] = n_rows, -5
    ok = np.ones(n, bool)
    ok[[0, n - 1, 3, 7, 10, 13, 20, 25]] = False
    for a, lim in zip(ids, (NU, n_rows, n_rows, n_rows)):
        assert ((a[ok] >= 0) & (a[ok] < lim)).all()
    named_u, named_e, named_w = _hgn_edge_compare("ids out of range", par, ids, L, T, pad, ok=ok)
    assert not named_u[49] and not named_e[79] and not named_w[78] and not named_w[77]


def test_without_a_padding_row_a_minus_one_is_an_id_out_of_range():
    """pad_idx = -1: a -1 in a window skips the instance, it is not read as padding"""
    rng = np.random.default_rng(401)
    n, L, T = 21, 5, 3
    pad, par, ids = _hgn_case(rng, NU, NI, n, L, T, 64)
    seq = ids[1]
    seq[seq == pad] = rng.integers(0, NI, (seq == pad).sum())
    seq[4, 2] = -1
    ok = np.arange(n) != 4
    _hgn_edge_compare("pad_idx = -1", par, ids, L, T, -1, ok=ok)


def test_padding_in_windows_and_targets():
    """a window of nothing but padding (den > 0, e = 0: q = p); a positive and a negative equal to pad_idx: scored against
    the padding row's zeros, and that row gets no gradient"""
    rng = np.random.default_rng(500)
    n, L, T = 21, 5, 3
    pad, par, ids = _hgn_case(rng, NU, NI, n, L, T, 64)
    u, seq, pos, neg = ids
    seq[2, :] = pad
    pos[4, 0], neg[6, T - 1] = pad, pad
    assert (seq[2] == pad).all() and (pos == pad).sum() == 1 and (neg == pad).sum() == 1
    _hgn_edge_compare("padding everywhere", par, ids, L, T, pad)


def test_loss_slots():
    """loss_slots = SKR_LOSS_SLOTS: word 0 of the slots sums to the single-slot loss, word 1 of every slot is untouched"""
    import torch
    from skrec import _hip
    S = _hip.SKR_LOSS_SLOTS
    pad, par, ids = _hgn_case(np.random.default_rng(600), NU, NI, 300, 5, 3, 64)
    _, one = _hgn_device(par, ids, 5, 3, pad)
    loss = torch.zeros((S, 2), device="cuda")
    loss[:, 1] = 7.0
    _, spread = _hgn_device(par, ids, 5, 3, pad, slots=S, loss=loss.view(-1))
    spread = spread.reshape(S, 2)
    assert (spread[:, 1] == 7.0).all() and (spread[:, 0] != 0).all()
    np.testing.assert_allclose(spread[:, 0].astype(np.float64).sum(), one[0], rtol=1e-6)


def test_an_empty_batch_touches_nothing():
    import torch
    from skrec import _hip
    pad, par, ids = _hgn_case(np.random.default_rng(700), NU, NI, 5, 5, 3, 64)
    P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu = par
    tabs = [torch.from_numpy(a).cuda() for a in (P, E, W2, b2, _gate_block(Wi, bi, Wu, bu, wi, Wiu))]
    grads = [torch.full_like(t, 3.0) for t in tabs]
    work = torch.full((_hip.SKR_HGN_MAX_BLOCKS * _hip.hgn_gate_floats(5),), 5.0, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    d_ids = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ids]
    _hip.check(_hip.lib().skr_hgn_step(*[_hip.ptr(t) for t in tabs], *[_hip.ptr(t) for t in d_ids], 0, NU, NI + 1, pad, 64, 5, 3,
                                       *[_hip.ptr(t) for t in grads], _hip.ptr(work), _hip.ptr(loss), 1, _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and all((g == 3.0).all() for g in grads) and (work == 5.0).all()


def test_queries_skip_users_out_of_range():
    """d_users with an id below 0, one at n_users and a valid id twice (with the same window): rows nobody names, the skipped
    ids' would-be rows among them, keep the sentinel bit for bit; n = 0 is allowed"""
    import torch
    from skrec import _hip
    rng = np.random.default_rng(800)
    L = 5
    pad, par, _ = _hgn_case(rng, NU, NI, 8, L, 1, 64)
    P, E, W2, b2, Wi, bi, Wu, bu, wi, Wiu = par
    users = np.array([5, -1, 12, NU, 5, 0, NU - 1], np.int32)
    win = rng.integers(0, NI, (len(users), L)).astype(np.int32)
    win[4] = win[0]
    win[2, :2] = pad
    dP, dE = (torch.from_numpy(t).cuda() for t in (P, E))
    dG = torch.from_numpy(_gate_block(Wi, bi, Wu, bu, wi, Wiu)).cuda()
    Q = torch.full((NU + 1, 64), 7.0, device="cuda")
    du, dw = torch.from_numpy(users).cuda(), torch.from_numpy(win).cuda()
    args = (_hip.ptr(dP), _hip.ptr(dE), _hip.ptr(dG), _hip.ptr(du))
    _hip.check(_hip.lib().skr_hgn_queries(*args, 0, _hip.ptr(dw), NU, NI + 1, pad, 64, L, _hip.ptr(Q), _hip.stream()))
    torch.cuda.synchronize()
    assert (Q == 7.0).all()
    _hip.check(_hip.lib().skr_hgn_queries(*args, len(users), _hip.ptr(dw), NU, NI + 1, pad, 64, L, _hip.ptr(Q), _hip.stream()))
    got = Q.cpu().numpy()
    rows = np.array([0, 2, 5, 6])                         # the list's entries with a valid id, the repeated one once
    valid = users[rows]
    assert (got[np.setdiff1d(np.arange(NU + 1), valid)] == 7.0).all()
    t64 = [torch.tensor(a, dtype=torch.float64) for a in (P, E, Wi, bi, Wu, bu, wi, Wiu)]
    want = _restated_query(*t64, torch.from_numpy(valid).long(), torch.from_numpy(win[rows]).long(), pad).numpy()
    np.testing.assert_allclose(got[valid], want, rtol=1e-5, atol=2e-6)
