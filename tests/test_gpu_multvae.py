"""GPU suite of MultVAE (csrc/multvae.hip, skrec/recommender/MultVAE.py): the fused step against float64 autograd of a
restatement (tests/multvae_twin.py), the decoder gradients' determinism, the query rows, the golden replay of the
reference's fit() from its recorded draws, the evaluator's fused path against its generic one, and the device draws."""
import numpy as np
import pytest

import multvae_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
CONFIG = dict(lr=1e-2, reg=1e-3, p_dims=[64], keep_prob=0.5, anneal_steps=6, anneal_cap=0.2, batch_size=24, epochs=3)


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="MultVAE", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    from skrec.recommender.MultVAE import MultVAE
    cfg = dict(CONFIG)
    cfg.update(kw)
    _seed()
    return MultVAE(_run_config(data_dir), cfg)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step kernel against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def _case(rng, B, I, d, keep_prob, wide):
    """parameters of width d, a CSR of B + 3 users (the batch is a permutation of B of them) and explicit draws.
    Batch position 0: a user with one item; 1: a user whose every item is dropped; 2: a user with the first and the
    last item of the catalogue; 3 (if B > 3): a long row.  ``wide``: Wp scaled so that the logits span +-80."""
    nU = B + 3
    lens = rng.integers(2, min(40, I // 2), nU)
    lens[0], lens[2] = 1, max(2, lens[2])
    if B > 3:
        lens[3] = min(I - 2, 700)
    cand = np.setdiff1d(np.arange(I), [5, I // 2])       # two items no row holds: their gradient rows stay zero
    rows = [np.sort(rng.choice(cand, n, replace=False)).astype(np.int32) for n in lens]
    rows[2][0], rows[2][-1] = 0, I - 1
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate(rows)
    users = np.concatenate([np.arange(4), 4 + rng.permutation(nU - 4)])[:B].astype(np.int32)
    Wq = (rng.standard_normal((2 * d, I)) * 0.2).astype(np.float32)
    bq = (rng.standard_normal(2 * d) * 0.2).astype(np.float32)
    Wp = (rng.standard_normal((I, d)) * 0.3).astype(np.float32)
    bp = (rng.standard_normal(I) * 0.3).astype(np.float32)
    keep = [(rng.random(lens[u]) < keep_prob).astype(np.uint8) if keep_prob < 1 else np.ones(lens[u], np.uint8) for u in users]
    if keep_prob < 1:
        keep[1][:] = 0                                   # every item dropped: e = bq
        keep[0][:] = 1
    eps = rng.standard_normal((B, d)).astype(np.float32)
    x = T.dense_rows(rowptr, items, users, I)
    mask = T.keep_mask(x, np.concatenate(keep))
    if wide:
        import torch
        with torch.no_grad():
            t = [torch.tensor(a, dtype=torch.float64) for a in (Wq, bq)]
            h = torch.tensor(x / np.linalg.norm(x, axis=1, keepdims=True) * mask / keep_prob)
            e = h @ t[0].T + t[1]
            z = e[:, :d] + torch.tensor(eps, dtype=torch.float64) * (0.5 * e[:, d:]).exp()
            Wp = (Wp * (80.0 / float((z @ torch.tensor(Wp, dtype=torch.float64).T).abs().max()))).astype(np.float32)
    return dict(nU=nU, I=I, d=d, B=B, rowptr=rowptr, items=items, users=users, Wq=Wq, bq=bq, Wp=Wp, bp=bp,
                keep=np.concatenate(keep), eps=eps, x=x, mask=mask, keep_prob=keep_prob)


def _device_tables(c):
    """the kernel's layout of a case's parameters: WqT [I, 128], bq [128], Wp [I, 64], bp [I]"""
    import torch
    d, I = c["d"], c["I"]
    wqt = np.zeros((I, 128), np.float32)
    wqt[:, :d], wqt[:, 64:64 + d] = c["Wq"][:d].T, c["Wq"][d:].T
    bq = np.zeros(128, np.float32)
    bq[:d], bq[64:64 + d] = c["bq"][:d], c["bq"][d:]
    wp = np.zeros((I, 64), np.float32)
    wp[:, :d] = c["Wp"]
    return [torch.from_numpy(a).cuda() for a in (wqt, bq, wp, c["bp"])]


def _step(c, tabs, anneal, draws=True, seed=0, step=0):
    """one skr_multvae_step on zeroed gradients -> (grads on the host, loss)"""
    import torch
    from skrec import _hip
    L = _hip.lib()
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("rowptr", "items", "users")]
    eps = np.zeros((c["B"], 64), np.float32)
    eps[:, :c["d"]] = c["eps"]
    dk, de = (torch.from_numpy(c["keep"]).cuda(), torch.from_numpy(eps).cuda()) if draws else (None, None)
    grads = [torch.zeros_like(t) for t in tabs]
    nb = int(L.skr_multvae_workspace(c["B"], c["I"]))
    assert nb > 0
    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    _hip.check(L.skr_multvae_step(*[_hip.ptr(t) for t in tabs], *[_hip.ptr(t) for t in dev], c["B"], c["nU"], c["I"], c["d"],
                                  c["keep_prob"], anneal, _hip.ptr(dk), _hip.ptr(de), seed, step,
                                  *[_hip.ptr(t) for t in grads], _hip.ptr(work), nb, _hip.ptr(loss), _hip.stream()))
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], loss.cpu().numpy()


@pytest.mark.parametrize("variant", ["dropout", "keep1", "wide"])
@pytest.mark.parametrize("B,I,d", [(3, 70, 16), (37, 1000, 64), (256, 4099, 64), (1024, 2053, 40)])
def test_step_matches_float64_autograd(B, I, d, variant):
    """shapes: item counts off every tile boundary, a ragged user chunk, padded columns; every case holds a user with one
    item, one whose every item is dropped (dropout variants), a positive in the first and the last item; ``keep1``:
    keep_prob = 1; ``wide``: logits spanning +-80 (the online max)"""
    import torch
    rng = np.random.default_rng(B + I + d + len(variant))
    keep_prob, anneal = (1.0 if variant == "keep1" else 0.5), 0.15
    c = _case(rng, B, I, d, keep_prob, variant == "wide")
    tabs = _device_tables(c)
    (gWqT, gbq, gWp, gbp), loss = _step(c, tabs, anneal)
    t64 = [torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in T.PARAMS]
    neg_ll, kl = T.losses_f64(*t64, c["x"], c["mask"], c["eps"], keep_prob)
    (neg_ll + anneal * kl).backward()
    print("neg_ll", loss[0], neg_ll.item(), "kl", loss[1], kl.item())
    np.testing.assert_allclose(loss[0], neg_ll.item(), rtol=1e-5)
    np.testing.assert_allclose(loss[1], kl.item(), rtol=1e-5)
    wq = t64[0].grad.numpy()
    checks = [("Wq_mu", gWqT[:, :d], wq[:d].T), ("Wq_logvar", gWqT[:, 64:64 + d], wq[d:].T),
              ("bq_mu", gbq[None, :d], t64[1].grad.numpy()[None, :d]), ("bq_logvar", gbq[None, 64:64 + d], t64[1].grad.numpy()[None, d:]),
              ("Wp", gWp[:, :d], t64[2].grad.numpy()), ("bp", gbp[None], t64[3].grad.numpy()[None])]
    # the two halves of Wq (bq) are one parameter each: the scale of a gradient is its parameter's largest element
    scale = {"Wq": np.abs(wq).max(), "bq": np.abs(t64[1].grad.numpy()).max()}
    for name, got, want in checks:
        print(name, "max abs err", np.abs(got - want).max(), "max |grad|", np.abs(want).max())
    for name, got, want in checks:
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * scale.get(name[:2], np.abs(want).max()), err_msg=name)
    # padded columns, and the rows of items no kept non-zero of the batch names, are exactly zero
    assert not gWqT[:, d:64].any() and not gWqT[:, 64 + d:].any() and not gWp[:, d:].any()
    assert not gbq[d:64].any() and not gbq[64 + d:].any()
    untouched = ~(c["mask"] != 0).any(0)
    assert untouched.sum() > 0 and not gWqT[untouched].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. nothing on the decoder side depends on timing
# ---------------------------------------------------------------------------------------------------------------------
def test_decoder_gradients_are_deterministic():
    rng = np.random.default_rng(5)
    B, I, d = 150, 64 * 512 + 64 * 90 + 7, 64          # 603 tiles for 512 workgroups; three user chunks, the last ragged
    from skrec import _hip
    assert (I + 63) // 64 > 512 and B > 2 * 64 and _hip.SKR_MULTVAE_MAX_BATCH == 1024
    c = _case(rng, B, I, d, 0.5, False)
    tabs = _device_tables(c)
    outs = [_step(c, tabs, 0.2) for _ in range(2)]
    (g0, l0), (g1, l1) = outs
    assert np.count_nonzero(g0[2]) > 0.99 * g0[2].size and np.count_nonzero(g0[3]) == I
    for k in (2, 3):                                   # dWp, dbp
        assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32))
    assert np.array_equal(g0[1].view(np.uint32), g1[1].view(np.uint32))      # dbq: an ordered sum of de, itself ordered
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))           # neg_ll, kl


# ---------------------------------------------------------------------------------------------------------------------
# 3. query rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("d", [64, 24])
def test_queries_match_float64(d, with_list):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(d)
    nU, I = 301, 3000
    lens = rng.integers(1, 60, nU)
    lens[7], lens[11] = 0, 2000                           # an empty row, a long row
    rows = [np.sort(rng.choice(I, n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate(rows)
    c = dict(d=d, I=I, Wq=(rng.standard_normal((2 * d, I)) * 0.2).astype(np.float32),
             bq=(rng.standard_normal(2 * d) * 0.2).astype(np.float32), Wp=np.zeros((I, d), np.float32), bp=np.zeros(I, np.float32))
    wqt, bq, _, _ = _device_tables(c)
    users = np.concatenate([[7, 11], 12 + rng.permutation(nU - 12)[:75]]).astype(np.int32) if with_list \
        else np.arange(nU, dtype=np.int32)
    Q = torch.full((nU + 1, 64), 7.0, device="cuda")
    drp, dit, du = (torch.from_numpy(a).cuda() for a in (rowptr, items, users))
    _hip.check(_hip.lib().skr_multvae_queries(_hip.ptr(wqt), _hip.ptr(bq), _hip.ptr(drp), _hip.ptr(dit),
                                              _hip.ptr(du) if with_list else None, len(users), nU, I, _hip.ptr(Q), _hip.stream()))
    got = Q.cpu().numpy()
    assert (got[nU] == 7.0).all() and (got[np.setdiff1d(np.arange(nU), users)] == 7.0).all()
    x = T.dense_rows(rowptr, items, users, I)
    h = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    want = h @ c["Wq"][:d].astype(np.float64).T + c["bq"][:d].astype(np.float64)
    print("max abs err", np.abs(got[users, :d] - want).max())
    np.testing.assert_allclose(got[users, :d], want, rtol=1e-5, atol=2e-6)
    assert np.array_equal(got[7, :d], c["bq"][:d])        # the empty row: bq itself
    assert not got[users, d:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. golden replay of the reference's fit() from its recorded draws
# ---------------------------------------------------------------------------------------------------------------------
class _Recorded(object):
    """the reference's evaluator contract on recorded scores: predict() -> ndarray (the generic path)"""

    def __init__(self, users, scores):
        self.row = {int(u): r for r, u in enumerate(users)}
        self.scores = scores

    def predict(self, users):
        return self.scores[[self.row[int(u)] for u in users]]


def _gap_ok(ev, users, scores, gap=5e-6):
    """users whose 22 best unmasked reference scores are pairwise more than ``gap`` apart"""
    ok = np.zeros(len(users), bool)
    for r, u in enumerate(users):
        row = scores[r].astype(np.float64).copy()
        row[np.asarray(ev.user_pos_train.get(int(u), []), dtype=np.int64)] = -np.inf
        top = np.sort(row)[::-1][:22]
        ok[r] = np.min(top[:-1] - top[1:]) > gap
    return ok


def test_replays_reference(golden, tiny_dir, monkeypatch, tmp_path, fused_mode):
    monkeypatch.chdir(tmp_path)
    g = golden("golden_multvae")
    m = _model(tiny_dir)
    assert (m.num_users, m.num_items, m.d) == (64, 96, 64)
    for k, t in zip(T.PARAMS, m.parameters()):
        assert np.array_equal(t.cpu().numpy(), g[k + "0"]), k          # same init under the same seed
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    losses, n_eval = [], 0
    for s, (users, keep, eps) in enumerate(T.fixture_steps(g)):
        losses.append(m.train_step(users, keep, eps).cpu().numpy())
        if (s + 1) % 3:
            continue
        report = np.array(list(m.evaluate().values()), np.float32)
        pred = m.predict(test_users)
        ref = g["pred"][n_eval]
        print("evaluation", n_eval, "max score diff", np.abs(pred - ref).max(), "allowed", 6 * dev_s[n_eval])
        assert np.abs(pred - ref).max() <= 6 * dev_s[n_eval]
        rows, _, n = ev.per_user_rows(m, test_users)
        rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, ref), test_users)
        ok = _gap_ok(ev, test_users, ref)
        print("users left out", int((~ok).sum()))
        assert n == 63 and (~ok).sum() <= 3
        assert np.array_equal(rows[ok], rows_ref[ok])
        if ok.all():
            np.testing.assert_allclose(report, g["reports"][n_eval], rtol=1e-5, atol=0, err_msg=str(g["names"]))
        n_eval += 1
    assert n_eval == 3
    losses = np.stack(losses)
    print("neg_ll", losses[:, 0], "golden", g["neg_ll"], "\nkl", losses[:, 1], "golden", g["kl"])
    np.testing.assert_allclose(losses[:, 0], g["neg_ll"], rtol=1e-5)
    np.testing.assert_allclose(losses[:, 1], g["kl"], rtol=1e-5)
    for k, t, lim in zip(T.PARAMS, m.parameters(), dev_p):
        print(k, "max abs diff", np.abs(t.cpu().numpy() - g[k + "1"]).max(), "allowed", 6 * lim)
    for k, t, lim in zip(T.PARAMS, m.parameters(), dev_p):
        assert np.abs(t.cpu().numpy() - g[k + "1"]).max() <= 6 * lim, k
    # padded entries of bp stay zero
    assert not m._biases[128 + 96:].any()


def test_rows_equal_the_oracle_loop(golden, tiny_dir, monkeypatch, tmp_path):
    """the per-user rows of the recorded reference scores through this evaluator are the rows of the oracle's
    restatement of the reference's evaluator loop (what test_replays_reference compares against)"""
    monkeypatch.chdir(tmp_path)
    from oracle import oracle as O
    g = golden("golden_multvae")
    m = _model(tiny_dir)
    ev = m.evaluator
    test_users = g["test_users"]
    for ref in g["pred"]:
        rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, ref), test_users)
        _, _, rows_orc = O.ranking_evaluate(_Recorded(test_users, ref).predict, ev.user_pos_train, ev.user_pos_test,
                                            top_k=(5, 10, 20), batch_size=16)
        assert np.array_equal(rows_ref, rows_orc)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the evaluator's fused path against its generic path
# ---------------------------------------------------------------------------------------------------------------------
class _PredictOnly(object):
    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def test_fused_path_equals_generic_path(tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SKR_FUSED_MODE", "fp32")
    m = _model(tiny_dir, epochs=1)
    m.fit()
    ev = m.evaluator
    users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert 63 in users and m._rowptr_host[64] == m._rowptr_host[63]          # the cold user is ranked like anyone else
    rows_dev, _, n_dev = ev.per_user_rows(m, users)
    rows_gen, _, n_gen = ev.per_user_rows(_PredictOnly(m), users)
    assert n_dev == n_gen == len(users) == 63
    assert np.array_equal(rows_dev, rows_gen)
    Q, _, _ = m.predict_factors()
    assert np.array_equal(Q[63].cpu().numpy(), m._bq[:64].cpu().numpy())
    # the query rows are kept between evaluations and dropped by a training step
    assert m._q_current
    q0 = Q.clone()
    m.train_step(np.arange(24, dtype=np.int32))
    assert not m._q_current
    assert not np.array_equal(m.predict_factors()[0].cpu().numpy(), q0.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 6. device draws
# ---------------------------------------------------------------------------------------------------------------------
def _draws(rowptr, items, users, nU, d, keep_prob, seed, step):
    import torch
    from skrec import _hip
    n = len(users)
    nnz = int((rowptr[users + 1] - rowptr[users]).sum())
    drp, dit, du = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rowptr, items, users))
    off = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    keep = torch.full((nnz + 1,), 9, dtype=torch.uint8, device="cuda")
    eps = torch.empty((n, 64), device="cuda")
    _hip.check(_hip.lib().skr_multvae_draws(_hip.ptr(drp), _hip.ptr(dit), _hip.ptr(du), n, nU, d, keep_prob, seed, step,
                                            _hip.ptr(off), _hip.ptr(keep), _hip.ptr(eps), _hip.stream()))
    k = keep.cpu().numpy()
    assert k[nnz] == 9 and int(off[n]) == nnz
    return off.cpu().numpy(), k[:nnz], eps.cpu().numpy()


def test_device_draws(tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(3)
    nU, I, d, p = 1024, 5000, 64, 0.5
    lens = rng.integers(60, 140, nU)
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate([np.sort(rng.choice(I, n, replace=False)).astype(np.int32) for n in lens])
    users = np.arange(nU, dtype=np.int32)
    off, keep, eps = _draws(rowptr, items, users, nU, d, p, 11, 4)
    n = len(keep)
    assert 9e4 < n < 1.2e5 and set(np.unique(keep)) == {0, 1}
    assert abs(keep.mean() - p) <= 4 * np.sqrt(p * (1 - p) / n)
    N = eps.size
    assert abs(eps.mean()) <= 4 / np.sqrt(N) and abs(eps.var() - 1) <= 4 * np.sqrt(2 / N)
    off2, keep2, eps2 = _draws(rowptr, items, users, nU, d, p, 11, 4)
    assert np.array_equal(keep, keep2) and np.array_equal(eps, eps2)                 # the same (seed, step)
    _, keep3, eps3 = _draws(rowptr, items, users, nU, d, p, 11, 5)
    assert not np.array_equal(keep, keep3) and not np.array_equal(eps, eps3)
    sub = rng.permutation(nU)[:100].astype(np.int32)                                 # another batch: the users' draws are the same
    offs, keeps, epss = _draws(rowptr, items, sub, nU, d, p, 11, 4)
    for r, u in enumerate(sub):
        assert np.array_equal(keeps[offs[r]:offs[r + 1]], keep[off[u]:off[u + 1]])
        assert np.array_equal(epss[r], eps[u])
    _, _, eps40 = _draws(rowptr, items, sub, nU, 40, p, 11, 4)
    assert np.array_equal(eps40[:, :40], epss[:, :40]) and not eps40[:, 40:].any()
    # the step with no draws handed in makes exactly these
    c = _case(np.random.default_rng(8), 37, 1000, 24, 0.5, False)
    tabs = _device_tables(c)
    _, c["keep"], e = _draws(c["rowptr"], c["items"], c["users"], c["nU"], 24, 0.5, 5, 9)
    c["eps"] = e[:, :24]
    (ga, la), (gb, lb) = _step(c, tabs, 0.1), _step(c, tabs, 0.1, draws=False, seed=5, step=9)
    assert np.array_equal(la, lb) and np.array_equal(ga[2], gb[2]) and np.array_equal(ga[3], gb[3])
    np.testing.assert_allclose(ga[0], gb[0], rtol=1e-5, atol=1e-7)
    # fit() on device draws
    m = _model(tiny_dir, epochs=2, batch_size=8)
    first = []
    ts = m.train_step

    def train_step(users, keep=None, eps=None):
        r = ts(users, keep, eps)
        first.append(r)
        return r
    m.train_step = train_step
    best = m.fit()
    nll = np.stack([t.cpu().numpy() for t in first])[:, 0]
    sizes = np.array([8] * 7 + [7] * 1, np.float64)                  # the 63 users with history
    per_epoch = (nll.reshape(2, 8) * sizes).sum(1) / 63             # mean over the same users in both epochs
    print("neg_ll per user and epoch", per_epoch)
    assert len(nll) == 16 and np.isfinite(nll).all() and per_epoch[1] < per_epoch[0]
    assert np.isfinite(np.array(list(best.values()))).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_run_skrec_cli(tiny_dir, tmp_path):
    import os
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "MultVAE", "--data_dir", tiny_dir, "--p_dims", "[32]",
                        "--epochs", "2", "--batch_size", "16", "--top_k", "[5,10]", "--metric", "['Recall','NDCG']",
                        "--seed", "7"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 1:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# 8. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
ANNEAL = 0.15


def _rows(rng, nU, I, lo=1, hi=30):
    """nU ascending train rows of lo .. hi - 1 items (at most I)"""
    return [np.sort(rng.choice(I, min(int(n), I), replace=False)).astype(np.int32) for n in rng.integers(lo, hi, nU)]


def _edge_case(rng, rows, users, I, d, keep_prob):
    """a case of _step's form on the CSR ``rows`` for the batch ``users`` as it stands: ids out of range and users that come
    twice included.  A user out of range is an all-zero row of x, as an empty train row is; the keep flags follow the
    non-zeros of the valid rows in batch order.  In every row of two or more items at least one is kept"""
    nU, B = len(rows), len(users)
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate(rows + [np.zeros(1, np.int32)])[:rowptr[-1] + 1].astype(np.int32)    # never an empty array
    x = np.zeros((B, I), np.float64)
    keep = []
    for r, u in enumerate(users):
        if 0 <= u < nU:
            x[r, rows[u]] = 1.0
            k = (rng.random(len(rows[u])) < keep_prob).astype(np.uint8) if keep_prob < 1 else np.ones(len(rows[u]), np.uint8)
            if len(k) > 1:
                k[rng.integers(len(k))] = 1
            keep.append(k)
    keep = np.concatenate(keep + [np.zeros(0, np.uint8)])
    c = dict(nU=nU, I=I, d=d, B=B, rowptr=rowptr, items=items, users=np.asarray(users, np.int32), keep_prob=keep_prob,
             Wq=(rng.standard_normal((2 * d, I)) * 0.2).astype(np.float32), bq=(rng.standard_normal(2 * d) * 0.2).astype(np.float32),
             Wp=(rng.standard_normal((I, d)) * 0.3).astype(np.float32), bp=(rng.standard_normal(I) * 0.3).astype(np.float32),
             keep=keep, eps=rng.standard_normal((B, d)).astype(np.float32), x=x)
    c["mask"] = T.keep_mask(x, keep)
    return c


def _edge_compare(c, what, got, anneal=ANNEAL, cancel=None):
    """the device's (gradients, loss) against float64 autograd of the twin (n the divisor of both means, zero rows of x
    included) with the suite's bounds and its per-parameter scale for the two halves of Wq and bq; the rows of WqT that no
    kept non-zero names are exactly zero.  ``cancel`` ({"neg_ll", "Wp", "bp": size}): a case in which those three are
    identically zero takes their scale from the terms that cancel (see _decoder_terms), as the HGN suite does at L = 1.
    Prints one ``edge-error`` line per tensor"""
    import torch
    (gWqT, gbq, gWp, gbp), loss = got
    d = c["d"]
    t64 = [torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in T.PARAMS]
    neg_ll, kl = T.losses_f64(*t64, c["x"], c["mask"], c["eps"], c["keep_prob"])
    (neg_ll + anneal * kl).backward()
    want = [t.grad.numpy() for t in t64]
    assert np.isfinite(neg_ll.item()) and np.isfinite(kl.item()) and all(np.isfinite(w).all() for w in want)
    print(what, "neg_ll", loss[0], neg_ll.item(), "kl", loss[1], kl.item())
    assert np.isfinite(loss).all() and all(np.isfinite(g).all() for g in got[0]), what
    cancel = cancel or {}
    np.testing.assert_allclose(loss[0], neg_ll.item(), rtol=1e-5, atol=1e-5 * cancel.get("neg_ll", 0.0), err_msg=what)
    np.testing.assert_allclose(loss[1], kl.item(), rtol=1e-5, err_msg=what)
    wq, wbq = want[0], want[1]
    checks = [("Wq_mu", gWqT[:, :d], wq[:d].T), ("Wq_logvar", gWqT[:, 64:64 + d], wq[d:].T), ("bq_mu", gbq[None, :d], wbq[None, :d]),
              ("bq_logvar", gbq[None, 64:64 + d], wbq[None, d:]), ("Wp", gWp[:, :d], want[2]), ("bp", gbp[None], want[3][None])]
    scale = {"Wq": np.abs(wq).max(), "bq": np.abs(wbq).max()}
    scale.update({k: max(np.abs(want[i]).max(), cancel[k]) for i, k in ((2, "Wp"), (3, "bp")) if k in cancel})
    for name, g, w in checks:                       # every tensor is measured before the assertion
        print(f"edge-error MultVAE | {what} | {name} | {np.abs(g - w).max():.3e} | {scale.get(name[:2], np.abs(w).max()):.3e}")
    for name, g, w in checks:
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=2e-5 * scale.get(name[:2], np.abs(w).max()), err_msg=f"{what}: {name}")
    assert not gWqT[:, d:64].any() and not gWqT[:, 64 + d:].any() and not gWp[:, d:].any()
    assert not gbq[d:64].any() and not gbq[64 + d:].any()
    untouched = ~(c["mask"] != 0).any(0)
    assert not gWqT[untouched].any(), what
    return untouched


@pytest.mark.parametrize("keep_prob", [0.5, 1.0])
@pytest.mark.parametrize("d", [64, 24])
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 63, 64, 65])
def test_batch_sizes_around_the_tiles(B, d, keep_prob):
    """users below, at and above the 16 rows of an MFMA tile and the 64 of a user chunk (load_a, sZ, sG); I = 200: three
    full tiles and one of eight items"""
    rng = np.random.default_rng(1000 + 10 * B + d + int(keep_prob))
    rows = _rows(rng, B + 3, 200)
    rows[0] = np.array([0, 199], np.int32)
    c = _edge_case(rng, rows, rng.permutation(B + 3)[:B], 200, d, keep_prob)
    untouched = _edge_compare(c, f"B = {B}, d = {d}, keep_prob = {keep_prob}", _step(c, _device_tables(c), ANNEAL))
    assert B > 15 or untouched.any()


def _decoder_terms(c):
    """The sizes of the decoder side's terms in the float64 twin: neg_ll = mean_u (n_u lse_u - sum_{i in x_u} logit_ui),
    d bp[i] = sum_u (n_u softmax_ui - x_ui) / B and d Wp[i] = sum_u (n_u softmax_ui - x_ui) z_u / B are differences of two
    terms that the step computes apart (lse over the tiles, the positives' logits in the encoder launch; n_u softmax in
    pass 2, then - x).  With ONE item softmax is 1, every row is that item, and all three are identically zero in exact
    arithmetic: what any fp32 evaluation returns is the rounding residue of the subtraction, so max|twin| = 0 is no scale.
    Their scale is the size of the term that is subtracted: mean_u |sum logits|, max_i sum_u x_ui / B, max sum_u x_ui |z_u| / B"""
    import torch
    d, B = c["d"], c["B"]
    with torch.no_grad():
        Wq, bq, Wp, bp = (torch.tensor(c[k], dtype=torch.float64) for k in T.PARAMS)
        x, mask, eps = (torch.as_tensor(a, dtype=torch.float64) for a in (c["x"], c["mask"], c["eps"]))
        e = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) * mask / c["keep_prob"] @ Wq.T + bq
        z = e[:, :d] + eps * (0.5 * e[:, d:]).exp()
        pos = ((z @ Wp.T + bp) * x).sum(1)
        return {"neg_ll": float(pos.abs().mean()), "bp": float(x.sum(0).max() / B), "Wp": float((x.T @ z.abs()).max() / B)}


@pytest.mark.parametrize("I", [1, 63, 64, 65, 128, 64 * 512, 64 * 512 + 1, 64 * (512 + 90) + 7])
def test_catalogue_sizes_around_the_tiles(I):
    """one item; less than a tile; the last tile exactly full (64, 128); one item into the next; and beyond 64 x
    SKR_MULTVAE_MAX_WG items, where tile_range hands a workgroup several tiles: every workgroup exactly one, the first
    workgroup two, a ragged split of 603 tiles.  B = 5; a row holds the first and the last item, another is long.
    At I = 1 neg_ll, d Wp and d bp are identically zero (the twin returns exact zeros; measured on the device: neg_ll =
    3.2e-07): their bounds take _decoder_terms' scales, 1e-5 and 2e-5 of the terms that cancel"""
    rng = np.random.default_rng(2000 + I)                  # (SKR_MULTVAE_MAX_WG of include/skrec_hip.h is 512)
    rows = _rows(rng, 7, I, 1, 40)
    rows[1] = np.unique(np.array([0, I - 1], np.int32))
    if I > 128:
        rows[2] = np.sort(rng.choice(I, 700, replace=False)).astype(np.int32)
        # pass 2's cursor has to move on only where a workgroup owns a second tile (tile_range: workgroup b of wg owns the
        # tiles [b tiles / wg, (b + 1) tiles / wg)): a row holding every item of both tiles of such a workgroup, so that the
        # second tile's entries lie 64 entries past the cursor the workgroup started from
        tiles, wg = (I + 63) // 64, 512
        if tiles > wg:
            b = next(b for b in range(wg) if (b + 1) * tiles // wg - b * tiles // wg == 2)
            t = b * tiles // wg
            rows[3] = np.arange(64 * t, min(64 * (t + 2), I), dtype=np.int32)
            assert len(rows[3]) > 64
    c = _edge_case(rng, rows, [1, 2, 0, 5, 3], I, 64 if I % 2 else 40, 0.5)
    cancel = None
    if I == 1:
        assert c["x"].all()
        cancel = _decoder_terms(c)
        print("the terms that cancel at I = 1:", cancel)
        assert min(cancel.values()) > 1e-2
    _edge_compare(c, f"I = {I}", _step(c, _device_tables(c), ANNEAL), cancel=cancel)


def test_rows_that_fill_a_tile():
    """pass 2 reads one CSR entry per lane and tile and moves the cursor on by a ballot count: a row that is exactly the 64
    items of tile 1, a row that is the whole catalogue (every lane of every tile, the last tile ragged), a row of the two
    items on either side of a tile boundary"""
    I = 200
    rng = np.random.default_rng(3000)
    rows = _rows(rng, 6, I)
    rows[0], rows[1], rows[2] = np.arange(64, 128, dtype=np.int32), np.arange(I, dtype=np.int32), np.array([63, 64], np.int32)
    users = [3, 0, 1, 2, 4]
    c = _edge_case(rng, rows, users, I, 64, 0.5)
    assert [int(c["x"][r].sum()) for r in (1, 2, 3)] == [64, I, 2]
    assert c["x"][1, 64:128].all() and c["x"][3, 63] == c["x"][3, 64] == 1
    _edge_compare(c, "rows that fill a tile", _step(c, _device_tables(c), ANNEAL))


def _draws_of(c, seed, step):
    """skr_multvae_draws for the batch of ``c``, users out of range included -> (keep, eps [B, 64])"""
    import torch
    from skrec import _hip
    n, nnz = c["B"], int(c["x"].sum())
    drp, dit, du = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("rowptr", "items", "users"))
    off = torch.full((n + 2,), -5, dtype=torch.int32, device="cuda")
    keep = torch.full((nnz + 1,), 9, dtype=torch.uint8, device="cuda")
    eps = torch.empty((n, 64), device="cuda")
    _hip.check(_hip.lib().skr_multvae_draws(_hip.ptr(drp), _hip.ptr(dit), _hip.ptr(du), n, c["nU"], c["d"], c["keep_prob"], seed,
                                            step, _hip.ptr(off), _hip.ptr(keep), _hip.ptr(eps), _hip.stream()))
    k, o = keep.cpu().numpy(), off.cpu().numpy()
    assert k[nnz] == 9 and o[n] == nnz and o[n + 1] == -5 and np.array_equal(np.diff(o[:n + 1]), c["x"].sum(1).astype(np.int64))
    return k[:nnz], eps.cpu().numpy()


def _with_zero_rows(seed):
    """B = 6 on 9 users: batch positions 1, 2 and 4 are a user with an empty train row, an id below 0 and the id n_users;
    no row holds item 5"""
    rng = np.random.default_rng(seed)
    I = 200
    rows = [np.setdiff1d(r, [5]).astype(np.int32) for r in _rows(rng, 9, I, 2, 30)]
    rows[4] = np.zeros(0, np.int32)
    users = [2, 4, -1, 7, 9, 0]
    c = _edge_case(rng, rows, users, I, 40, 0.5)
    assert [int(s) for s in c["x"].sum(1)][1:5:1] == [0, 0, len(rows[7]), 0] and not c["x"][:, 5].any()
    return c


def test_empty_rows_and_users_out_of_range_are_rows_of_the_batch():
    """n stays the divisor of both means; such a row adds nothing to neg_ll, the KL of bq to kl, and that term's gradient
    to gbq alone (h = 0: nothing for Wq, and (n_u softmax - x) = 0: nothing for the decoder)"""
    import torch
    c = _with_zero_rows(4000)
    tabs = _device_tables(c)
    got = _step(c, tabs, ANNEAL)
    untouched = _edge_compare(c, "empty rows, recorded draws", got)
    assert untouched[5]
    # the same batch without the three rows, the means over 6 still: the device's own result, scaled
    live = c["x"].any(1)
    assert live.sum() == 3
    c3 = dict(c, B=3, users=c["users"][live], x=c["x"][live], mask=c["mask"][live], eps=c["eps"][live])
    g3, l3 = _step(c3, tabs, ANNEAL)
    t64 = [torch.tensor(c[k], dtype=torch.float64) for k in T.PARAMS]
    zero = np.zeros((3, c["I"]))
    kl0 = T.losses_f64(*t64, zero, zero, np.zeros((3, c["d"])), 0.5)[1].item()           # the KL of bq, per row
    np.testing.assert_allclose(got[1][0], l3[0] * 3 / 6, rtol=1e-5)
    np.testing.assert_allclose(got[1][1], (l3[1] * 3 + kl0 * 3) / 6, rtol=1e-5)
    for k in (0, 2, 3):                                     # Wq, Wp, bp: nothing from the three rows
        np.testing.assert_allclose(got[0][k], g3[k] * np.float32(0.5), rtol=1e-4, atol=2e-5 * np.abs(got[0][k]).max())


def test_empty_rows_and_users_out_of_range_under_device_draws():
    """d_keep = d_eps = NULL: two calls give the same bits on the decoder side, and the step equals the explicit-draw step
    fed with skr_multvae_draws' output, which equals the twin"""
    c = _with_zero_rows(4001)
    tabs = _device_tables(c)
    (ga, la), (gb, lb) = (_step(c, tabs, ANNEAL, draws=False, seed=5, step=9) for _ in range(2))
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    for k in (1, 2, 3):
        assert np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32))
    c["keep"], e = _draws_of(c, 5, 9)
    c["eps"], c["mask"] = e[:, :c["d"]], T.keep_mask(c["x"], c["keep"])
    assert not e[:, c["d"]:].any() and np.isfinite(e).all()
    ge, le = _step(c, tabs, ANNEAL)
    assert np.array_equal(la, le) and np.array_equal(ga[2], ge[2]) and np.array_equal(ga[3], ge[3])
    np.testing.assert_allclose(ga[0], ge[0], rtol=1e-5, atol=1e-7)
    _edge_compare(c, "empty rows, device draws", (ga, la))


def test_the_same_user_twice_is_two_rows():
    rng = np.random.default_rng(5000)
    rows = _rows(rng, 8, 200, 2, 30)
    c = _edge_case(rng, rows, [3, 6, 3, 1, 3], 200, 64, 0.5)
    assert np.array_equal(c["x"][0], c["x"][2]) and not np.array_equal(c["mask"][0], c["mask"][2])
    _edge_compare(c, "one user three times", _step(c, _device_tables(c), ANNEAL))


def test_one_column_and_no_annealing():
    """dim = 1; anneal = 0: kl is still written, the gradient is that of neg_ll alone"""
    rng = np.random.default_rng(6000)
    rows = _rows(rng, 8, 200, 2, 30)
    c = _edge_case(rng, rows, [3, 6, 0, 1, 5], 200, 1, 0.5)
    _edge_compare(c, "dim = 1", _step(c, _device_tables(c), ANNEAL))
    c = _edge_case(rng, rows, [3, 6, 0, 1, 5], 200, 40, 0.5)
    got = _step(c, _device_tables(c), 0.0)
    assert got[1][1] > 0
    _edge_compare(c, "anneal = 0", got, anneal=0.0)


def test_full_batch_and_the_batch_over_the_limit():
    """B = SKR_MULTVAE_MAX_BATCH on 129 items (two full tiles and one item) with rows of 1 to 3 items: 16 user chunks per
    workgroup; twice: the same bits on the decoder side.  Then 1025 users: refused by name, the workspace size is 0"""
    import torch
    from skrec import _hip
    B = _hip.SKR_MULTVAE_MAX_BATCH
    assert B == 1024
    rng = np.random.default_rng(7000)
    rows = _rows(rng, B + 6, 129, 1, 4)
    c = _edge_case(rng, rows, rng.permutation(B + 6)[:B], 129, 64, 0.5)
    tabs = _device_tables(c)
    got = _step(c, tabs, ANNEAL)
    _edge_compare(c, "B = 1024", got)
    again = _step(c, tabs, ANNEAL)
    for k in (1, 2, 3):
        assert np.array_equal(got[0][k].view(np.uint32), again[0][k].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), again[1].view(np.uint32))
    L = _hip.lib()
    assert L.skr_multvae_workspace(B + 1, 129) == 0
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["rowptr"], c["items"], np.zeros(B + 1, np.int32))]
    grads = [torch.zeros_like(t) for t in tabs]
    work, loss = torch.zeros(1024, device="cuda"), torch.full((2,), 7.0, device="cuda")
    rc = L.skr_multvae_step(*[_hip.ptr(t) for t in tabs], *[_hip.ptr(t) for t in dev], B + 1, c["nU"], 129, 64, 0.5, ANNEAL, None,
                            None, 0, 0, *[_hip.ptr(t) for t in grads], _hip.ptr(work), 4096, _hip.ptr(loss), _hip.stream())
    with pytest.raises(ValueError, match="at most 1024"):
        _hip.check(rc)
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and not any(g.any() for g in grads)


def test_an_empty_batch_writes_a_zero_loss_and_nothing_else():
    import torch
    from skrec import _hip
    from skrec.recommender.MultVAE import MultVAE
    rng = np.random.default_rng(8000)
    rows = _rows(rng, 8, 200, 2, 30)
    c = _edge_case(rng, rows, [3], 200, 64, 0.5)
    tabs = _device_tables(c)
    dev = [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("rowptr", "items", "users")]
    grads = [torch.full_like(t, 3.0) for t in tabs]
    work = torch.full((4096,), 255, dtype=torch.uint8, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    _hip.check(_hip.lib().skr_multvae_step(*[_hip.ptr(t) for t in tabs], *[_hip.ptr(t) for t in dev], 0, c["nU"], 200, 64, 0.5,
                                           ANNEAL, None, None, 0, 0, *[_hip.ptr(t) for t in grads], _hip.ptr(work), work.numel(),
                                           _hip.ptr(loss), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 0.0).all() and all((g == 3.0).all() for g in grads) and (work == 255).all()
    # through the class: zeros, and a fresh model keeps its bits (the weights' decay included: an empty batch is no step)
    m = MultVAE.detached(8, 200, dict(CONFIG, p_dims=[48]), (c["rowptr"], c["items"]), seed=9)
    w, b = m._weights.clone(), m._biases.clone()
    out = m.train_step(np.zeros(0, np.int32))
    assert out.shape == (2,) and not out.any() and torch.equal(w, m._weights) and torch.equal(b, m._biases)
    assert m.update_count == 0 and not m.step_losses


def test_queries_skip_users_out_of_range():
    """d_users with an id below 0, one at n_users and a valid id twice: rows nobody names, the skipped ids' would-be rows
    among them, keep the sentinel bit for bit; n = 0 is allowed"""
    import torch
    from skrec import _hip
    rng = np.random.default_rng(9000)
    nU, I, d = 30, 200, 24
    rows = _rows(rng, nU, I)
    c = _edge_case(rng, rows, [0], I, d, 1.0)
    wqt, bq, _, _ = _device_tables(c)
    users = np.array([5, -1, 12, nU, 5, 0, nU - 1], np.int32)
    Q = torch.full((nU + 1, 64), 7.0, device="cuda")
    drp, dit, du = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["rowptr"], c["items"], users))
    args = (_hip.ptr(wqt), _hip.ptr(bq), _hip.ptr(drp), _hip.ptr(dit), _hip.ptr(du))
    _hip.check(_hip.lib().skr_multvae_queries(*args, 0, nU, I, _hip.ptr(Q), _hip.stream()))
    torch.cuda.synchronize()
    assert (Q == 7.0).all()
    _hip.check(_hip.lib().skr_multvae_queries(*args, len(users), nU, I, _hip.ptr(Q), _hip.stream()))
    got = Q.cpu().numpy()
    valid = np.array([5, 12, 0, nU - 1])
    assert (got[np.setdiff1d(np.arange(nU + 1), valid)] == 7.0).all()
    x = T.dense_rows(c["rowptr"], c["items"], valid, I)
    want = x / np.linalg.norm(x, axis=1, keepdims=True) @ c["Wq"][:d].astype(np.float64).T + c["bq"][:d].astype(np.float64)
    np.testing.assert_allclose(got[valid, :d], want, rtol=1e-5, atol=2e-6)
    assert not got[valid, d:].any()
