"""GPU suite of BM3 (csrc/bm3.hip, skrec/recommender/BM3.py): the gather-and-project product against float64, the whole step
against float64 autograd of a restatement (tests/bm3_twin.py), the clearing of the feature-gradient rows, the step's
determinism, the device draws, Adam against torch, the golden replay of the reference's fit() from its recorded batches and
masks, fit() with device draws, the CLI, the limits."""
import os

import numpy as np
import pytest

import bm3_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
CONFIG = dict(lr=1e-2, reg=0.1, embed_dim=64, n_layers=2, dropout=0.3, cl_weight=2.0, batch_size=256, epochs=3)


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="BM3", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    from skrec.recommender.BM3 import BM3
    cfg = dict(CONFIG)
    cfg.update(kw)
    _seed()
    return BM3(_run_config(data_dir), cfg)


def _write_features(tiny_dir, g, text=True):
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), features=g["image_embedding_weight_0"])
    if text:
        np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), features=g["text_embedding_weight_0"])


def _check_grad(name, got, want):
    """SelfCF's rule (tests/test_gpu_selfcf.py) for a gradient against float64 autograd"""
    print(name, "max abs err", np.abs(got - want).max(), "max |grad|", np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * np.abs(want).max(), err_msg=name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gather-and-project product
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("F", [1, 37, 64, 100, 4096])
def test_project_matches_float64(F, d):
    import torch
    from gpu_utils import dev, to_dev
    from skrec import _hip
    rng = np.random.default_rng(1000 * d + F)
    I, ld = 40, (F + 3) // 4 * 4
    X = np.zeros((I, ld), np.float32)
    X[:, :F] = rng.standard_normal((I, F))
    W = np.zeros((64, ld), np.float32)
    W[:d, :F] = rng.standard_normal((d, F)) / np.sqrt(F)
    b = np.zeros(64, np.float32)
    b[:d] = rng.standard_normal(d) * 0.1
    dX, dtrs = to_dev(X), to_dev(np.concatenate([W.reshape(-1), b]))
    for n in (1, 17, 300):
        ids = rng.integers(0, I, n).astype(np.int32)
        if n > 1:
            ids[1] = ids[0]                                  # a repeated id for certain
        Y = torch.full((n + 1, 64), 7.0, device=dev())
        _hip.check(_hip.lib().skr_bm3_project(_hip.ptr(dX), I, F, ld, _hip.ptr(dtrs), _hip.ptr(to_dev(ids)), n, _hip.ptr(Y), _hip.stream()))
        torch.cuda.synchronize()
        got = Y.cpu().numpy()
        assert (got[n] == 7.0).all()                         # nothing beyond the n rows is written
        got = got[:n]
        X64, W64 = X[ids].astype(np.float64), W.astype(np.float64)
        want = X64 @ W64.T + b
        mass = np.abs(X64) @ np.abs(W64).T + np.abs(b)
        cpu = (torch.from_numpy(X[ids]) @ torch.from_numpy(W).T + torch.from_numpy(b)).numpy()
        r = float((np.abs(cpu - want) / np.maximum(mass, 1e-30)).max())
        err = float((np.abs(got - want) / np.maximum(mass, 1e-30)).max())
        print("n", n, "torch-CPU fp32 error / mass", r, "ours", err)
        assert np.all(np.abs(got - want) <= max(2e-6, 4 * r) * mass + 1e-6)
        assert not got[:, d:].any()                          # padding columns stay zero


# ---------------------------------------------------------------------------------------------------------------------
# 2. the whole step against the twin
# ---------------------------------------------------------------------------------------------------------------------
def _graph(U, I, rng, max_len=10):
    """a bipartite CSR whose last user and last item have no entry"""
    lens = rng.integers(1, max_len, U)
    lens[U - 1] = 0
    rows = [np.sort(rng.choice(I - 1, n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    return rowptr, np.concatenate(rows), rows


def _step_case(n, L, d, Fv, Ft, seed, U=48, I=40):
    """U = 48, I = 40, the last user and the last item isolated; a batch with a repeated user and a repeated item and the
    isolated user and item (n >= 3); per target table one node whose 64 flags are all zero; a node that occurs twice has one
    row of flags"""
    rng = np.random.default_rng(seed)
    rowptr, items, rows = _graph(U, I, rng)
    users = rng.integers(0, U - 1, n).astype(np.int32)
    its = np.array([rows[u][rng.integers(0, len(rows[u]))] for u in users], np.int32)
    if n >= 3:
        users[1], its[1] = U - 1, I - 1                      # the isolated user and the isolated item
        users[2], its[2] = users[0], its[0]                  # a repeated user and a repeated item for certain
    full = {k: (rng.random((rows_, 64)) >= 0.3).astype(np.uint8) for k, rows_ in (("u", U), ("i", I), ("t", I), ("v", I))}
    full["u"][users[0]] = 0                                  # zero targets: both norms' clamp, a zero gradient
    full["i"][its[0]] = 0
    full["t"][its[n - 1]] = 0
    full["v"][its[n // 2]] = 0
    keeps = {"u": full["u"][users], "i": full["i"][its], "t": full["t"][its], "v": full["v"][its]}
    P = {"user_embedding.weight": (rng.standard_normal((U, d)) * 0.3).astype(np.float32),
         "item_id_embedding.weight": (rng.standard_normal((I, d)) * 0.3).astype(np.float32),
         "predictor.weight": (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32),
         "predictor.bias": (rng.standard_normal(d) * 0.1).astype(np.float32)}
    for prefix, F in (("image", Fv), ("text", Ft)):
        if F:
            P[prefix + "_embedding.weight"] = rng.standard_normal((I, F)).astype(np.float32)
            P[prefix + "_trs.weight"] = (rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32)
            P[prefix + "_trs.bias"] = (rng.standard_normal(d) * 0.1).astype(np.float32)
    return dict(U=U, I=I, n=n, L=L, d=d, Fv=Fv, Ft=Ft, rowptr=rowptr, items=items, users=users, its=its, keeps=keeps, P=P)


def _target_keep(c):
    k = c["keeps"]
    return (k["u"], k["i"], k["t"] if c["Ft"] else None, k["v"] if c["Fv"] else None)


def _detached(c, reg=0.1, dropout=0.3, cl_weight=2.0):
    from skrec.recommender.BM3 import BM3
    cfg = dict(lr=1e-2, reg=reg, embed_dim=c["d"], n_layers=c["L"], dropout=dropout, cl_weight=cl_weight, batch_size=max(c["n"], 1))
    P = c["P"]
    m = BM3.detached(c["U"], c["I"], cfg, (c["rowptr"], c["items"]), img=P.get("image_embedding.weight"),
                     txt=P.get("text_embedding.weight"), seed=SEED)
    m.load_parameters(P)
    return m


BASE = (64, 2, 64, 100, 37)
STEP_CASES = ([BASE, (1, 0, 20, 1, 0), (300, 3, 20, 100, 37), (3, 1, 64, 4096, 1)]
              + [(n,) + BASE[1:] for n in (1, 3, 300)]
              + [BASE[:1] + (L,) + BASE[2:] for L in (0, 1, 3)]
              + [BASE[:2] + (20,) + BASE[3:]]
              + [BASE[:3] + f for f in ((0, 37), (64, 0), (0, 0), (4096, 1))])


def _check_step(c, reg):
    import torch
    dropout, cl = 0.3, 2.0
    n, L, d, U, I = c["n"], c["L"], c["d"], c["U"], c["I"]
    assert c["rowptr"][U] == c["rowptr"][U - 1] and not (c["items"] == I - 1).any()
    if n >= 3:
        assert len(np.unique(c["users"])) < n and len(np.unique(c["its"])) < n and (c["users"] == U - 1).any() and (c["its"] == I - 1).any()
    m = _detached(c, reg, dropout, cl)
    val = m.adj.val.cpu().numpy()[:len(c["items"])]
    np.testing.assert_allclose(val, T.normalised_values(c["rowptr"], c["items"], I), rtol=2e-7)
    P = {k: T.t64(v, True) for k, v in c["P"].items()}
    R = T.t64(T.dense_block(c["rowptr"], c["items"], I, val))
    keeps = {k: v[:, :d] for k, v in c["keeps"].items()}
    (graph, modal, regl), Mu, Mi = T.losses_f64(P, R, c["users"], c["its"], keeps, L, dropout, reg, cl)
    (graph + modal + regl).backward()
    loss = m.gradient_step(c["users"], c["its"], target_keep=_target_keep(c)).cpu().numpy()
    want = np.array([graph.item(), modal.item(), regl.item()])
    print("loss", loss, "twin", want)
    np.testing.assert_allclose(loss[:3], want, rtol=1e-5)
    np.testing.assert_allclose(loss[3], want.sum(), rtol=1e-5)
    Mg = m.M.cpu().numpy()
    np.testing.assert_allclose(Mg[:U, :d], Mu.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(Mg[U:, :d], Mi.detach().numpy(), rtol=1e-5, atol=1e-6)
    G = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    assert set(G) == set(P) == set(T.param_names(bool(c["Fv"]), bool(c["Ft"])))
    for name in P:
        grad = P[name].grad
        _check_grad(name, G[name], np.zeros(P[name].shape) if grad is None else grad.numpy())
    # all padding stays zero: whatever of the gradient buffer no named tensor covers, and the tables' columns beyond d
    rest = m._grad.clone()
    for v in m._views(rest).values():
        v.zero_()
    assert not bool(rest.any()) and not Mg[:, d:].any()
    torch.cuda.synchronize()
    return m, G


@pytest.mark.parametrize("n,L,d,Fv,Ft", STEP_CASES)
def test_step_matches_float64_autograd(n, L, d, Fv, Ft):
    c = _step_case(n, L, d, Fv, Ft, 100 * n + 10 * L + d + Fv + Ft)
    _, G = _check_step(c, 0.1)
    # the feature tables' gradient is dense in shape and zero outside the batch's items
    for prefix in ("image", "text"):
        g = G.get(prefix + "_embedding.weight")
        if g is not None:
            outside = np.setdiff1d(np.arange(c["I"]), c["its"])
            assert not g[outside].any()
            assert n == 1 or g[np.unique(c["its"])].any()         # (n = 1: every target of the one row is zero)


def test_step_without_the_regulariser():
    _check_step(_step_case(*BASE, seed=7), 0.0)


def test_step_with_a_zero_norm():
    """an all-zero user table without propagation: |M_u| = 0, its regulariser gradient is exactly zero"""
    c = _step_case(64, 0, 64, 100, 37, seed=8)
    c["P"]["user_embedding.weight"][:] = 0.0
    m, G = _check_step(c, 0.1)
    outside = np.setdiff1d(np.arange(c["U"]), c["users"])
    assert not G["user_embedding.weight"][outside].any() and np.isfinite(m._grad.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the feature-gradient rows of the previous step are cleared, 4. the step is bit-reproducible
# ---------------------------------------------------------------------------------------------------------------------
def test_feature_gradient_rows_of_the_previous_step_are_cleared():
    c = _step_case(64, 1, 64, 100, 37, seed=9)
    m = _detached(c)
    first = c["its"] < 20
    u1, i1, u2, i2 = c["users"][first], c["its"][first], c["users"][~first], c["its"][~first]
    assert len(i1) > 3 and len(i2) > 3 and not set(i1) & set(i2)
    m.gradient_step(u1, i1)
    G = m.gradients()
    for name in ("image_embedding.weight", "text_embedding.weight"):
        rows = np.flatnonzero(G[name].cpu().numpy().any(axis=1))
        assert np.array_equal(rows, np.unique(i1)), name
    m.gradient_step(u2, i2)
    G = m.gradients()
    for name in ("image_embedding.weight", "text_embedding.weight"):
        rows = np.flatnonzero(G[name].cpu().numpy().any(axis=1))
        assert np.array_equal(rows, np.unique(i2)), name


def test_step_is_deterministic():
    c = _step_case(300, 3, 64, 100, 37, seed=5)
    m = _detached(c)
    outs = []
    for _ in range(2):
        loss = m.gradient_step(c["users"], c["its"], target_keep=_target_keep(c)).cpu().numpy()
        outs.append((m._grad.cpu().numpy().copy(), loss))
    (g0, l0), (g1, l1) = outs
    rows = g0[:(c["U"] + c["I"]) * 64]
    assert np.count_nonzero(rows) > 0.8 * rows.size
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the device draws
# ---------------------------------------------------------------------------------------------------------------------
def test_device_draws():
    from skrec import _hip
    c = _step_case(64, 1, 64, 100, 37, seed=11)
    m = _detached(c)
    ids = np.arange(2048, dtype=np.int32)
    ids[7] = ids[3]                                          # a repeated node
    a = m.target_draws(ids, _hip.SKR_BM3_DRAW_ITEM, step=5).cpu().numpy()
    assert a.shape == (2048, 64) and set(np.unique(a)) == {0, 1}
    print("kept share", a.mean())
    assert abs(a.mean() - 0.7) <= 0.01
    assert np.array_equal(a[7], a[3]) and not np.array_equal(a[4], a[3])
    assert np.array_equal(a, m.target_draws(ids, _hip.SKR_BM3_DRAW_ITEM, step=5).cpu().numpy())
    assert not np.array_equal(a, m.target_draws(ids, _hip.SKR_BM3_DRAW_ITEM, step=6).cpu().numpy())
    assert not np.array_equal(a, m.target_draws(ids, _hip.SKR_BM3_DRAW_TEXT, step=5).cpu().numpy())
    m2 = _detached(c)
    m2._seed = SEED + 1
    assert not np.array_equal(a, m2.target_draws(ids, _hip.SKR_BM3_DRAW_ITEM, step=5).cpu().numpy())
    # the step draws the same flags: a step with device draws equals the step that is handed them
    u, i = c["users"], c["its"]
    keep = tuple(m.target_draws(x, t).clone() for x, t in ((u, _hip.SKR_BM3_DRAW_USER), (i, _hip.SKR_BM3_DRAW_ITEM),
                                                            (i, _hip.SKR_BM3_DRAW_TEXT), (i, _hip.SKR_BM3_DRAW_IMAGE)))
    step = m._step
    l0 = m.gradient_step(u, i).cpu().numpy()
    g0 = m._grad.cpu().numpy().copy()
    m._step = step
    l1 = m.gradient_step(u, i, target_keep=keep).cpu().numpy()
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    assert np.array_equal(g0.view(np.uint32), m._grad.cpu().numpy().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 6. Adam over the flat buffer against torch.optim.Adam per tensor
# ---------------------------------------------------------------------------------------------------------------------
def test_adam_matches_torch_per_tensor():
    """two steps with disjoint item sets: a feature row of the first batch gets a zero gradient in the second step and still
    moves by its leftover momentum.  The bound is test_gpu_hgn.py's for the dense launch"""
    import torch
    c = _step_case(64, 1, 64, 100, 37, seed=13)
    m = _detached(c)
    first = c["its"] < 20
    batches = [(c["users"][first], c["its"][first]), (c["users"][~first], c["its"][~first])]
    ref = {k: torch.nn.Parameter(v.cpu().clone()) for k, v in m.parameters().items()}
    opt = torch.optim.Adam(list(ref.values()), lr=1e-2)
    row = int(batches[0][1][0])
    assert row not in set(batches[1][1])
    for s, (u, i) in enumerate(batches):
        before = m.parameters()["image_embedding.weight"][row].cpu().numpy()
        m.gradient_step(u, i)
        G = m.gradients()
        if s == 1:
            assert not G["image_embedding.weight"][row].any()
        for k, p in ref.items():
            p.grad = G[k].cpu().clone()
        m.optimizer.step()
        opt.step()
        got = m.parameters()
        for k, p in ref.items():
            diff = np.abs(got[k].cpu().numpy() - p.detach().numpy()).max()
            print("step", s, k, "max abs diff", diff)
            np.testing.assert_allclose(got[k].cpu().numpy(), p.detach().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
        after = got["image_embedding.weight"][row].cpu().numpy()
        assert not np.array_equal(before, after)             # the row moves in both steps
    assert float(m._grad.abs().max()) == 0.0                  # the launch zeroes the gradient it has read


# ---------------------------------------------------------------------------------------------------------------------
# 7. golden replay of the reference's fit() from its recorded batches and masks
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
    g = golden("golden_bm3")
    _write_features(tiny_dir, g)
    m = _model(tiny_dir)
    assert (m.num_users, m.num_items) == (64, 96) and m.feat_dim == {"img": 100, "txt": 37}
    P0 = m.parameters()
    want0 = T.fixture_params(g, 0)
    assert set(P0) == set(want0)
    for name, want in want0.items():
        assert np.array_equal(P0[name].cpu().numpy(), want), name        # same init, same seed
    np.testing.assert_allclose(m.adj.val.cpu().numpy(), g["adj_val"], rtol=2e-7)
    np.testing.assert_allclose(m.adj_t.val.cpu().numpy(), g["adj_t_val"], rtol=2e-7)
    assert np.array_equal(m.adj.col.cpu().numpy(), g["adj_cols"]) and np.array_equal(m.adj_t.col.cpu().numpy(), g["adj_t_cols"])
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    steps = T.fixture_steps(g)
    assert len(steps) == 9
    losses, n_eval = [], 0
    for s, st in enumerate(steps):
        losses.append(m.train_step(st["users"], st["items"], target_keep=(st["ku"], st["ki"], st["kt"], st["kv"])).cpu().numpy())
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
    print("loss", losses[:, 3], "golden", g["loss"])
    np.testing.assert_allclose(losses[:, 3], g["loss"], rtol=1e-5)
    P1 = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    final = T.fixture_params(g, 1)
    for k, name in enumerate(T.param_names(True, True)):
        print(name, "max abs diff", np.abs(P1[name] - final[name]).max(), "allowed", 6 * dev_p[k])
        assert np.abs(P1[name] - final[name]).max() <= 6 * dev_p[k]


# ---------------------------------------------------------------------------------------------------------------------
# 8. fit() with device draws, the command line, the limits
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_with_device_draws_learns(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    _write_features(tiny_dir, golden("golden_bm3"))
    m = _model(tiny_dir)
    reports = []
    orig = m.evaluate

    def evaluate(tu=None):
        r = orig(tu)
        reports.append(dict(r.items()))
        return r
    m.evaluate = evaluate
    best = m.fit()
    assert np.isfinite(np.array(list(best.values()))).all() and len(reports) == 3 and len(m.step_losses) == 3
    import torch
    assert torch.isfinite(torch.stack(m.step_losses)).all()
    print("NDCG@10", [r["NDCG@10"] for r in reports])
    assert reports[-1]["NDCG@10"] > reports[0]["NDCG@10"]


@pytest.mark.parametrize("text", [True, False])
def test_run_skrec_cli(golden, tiny_dir, tmp_path, text):
    """both modalities, and a copy of the tiny set without its text file"""
    import subprocess
    import sys
    from conftest import REPO
    _write_features(tiny_dir, golden("golden_bm3"), text=text)
    assert os.path.exists(os.path.join(tiny_dir, "tiny.txt.npz")) == text
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "BM3", "--data_dir", tiny_dir, "--embed_dim", "32", "--epochs", "1",
                        "--batch_size", "128", "--top_k", "[5,10]", "--metric", "['Recall','NDCG']", "--seed", "7"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 0:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout
    assert "image features: (96, 100)" in r.stdout and ("txt features: (96, 37)" in r.stdout) == text


@pytest.mark.parametrize("kw,msg", [(dict(embed_dim=65), "embed_dim <= 64"), (dict(n_layers=5), "n_layers <= 4"),
                                    (dict(batch_size=2049), "batch_size <= 2048")])
def test_each_limit_raises(golden, tiny_dir, monkeypatch, tmp_path, kw, msg):
    monkeypatch.chdir(tmp_path)
    _write_features(tiny_dir, golden("golden_bm3"))
    with pytest.raises(NotImplementedError, match=msg):
        _model(tiny_dir, **kw)
    m = _model(tiny_dir)
    with pytest.raises(NotImplementedError, match="at most 2048"):
        m.gradient_step(np.zeros(2049, np.int32), np.zeros(2049, np.int32))
    from skrec.recommender.BM3 import BM3Config, check_limits
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(BM3Config(**CONFIG), world=2)


def test_a_too_wide_feature_table_raises(tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), features=np.zeros((96, 4097), np.float32))
    with pytest.raises(NotImplementedError, match="feature width <= 4096"):
        _model(tiny_dir)


# ---------------------------------------------------------------------------------------------------------------------
# 10. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
RTOL, ATOL = 1e-4, 2e-5        # _check_grad's


def _twin_run(c, m, rows, dtype, reg, n_div=None):
    """the twin in ``dtype`` on the batch rows ``rows`` of ``c``, on the model's own adjacency values
    -> ((graph, modal, reg part), {name: float64 gradient}, targets' norms (user table, item table))"""
    import torch
    d, I = c["d"], c["I"]
    val = m.adj.val.cpu().numpy()[:len(c["items"])]
    P = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in c["P"].items()}
    R = torch.tensor(T.dense_block(c["rowptr"], c["items"], I, val), dtype=dtype)
    keeps = {k: v[rows][:, :d] for k, v in c["keeps"].items()}
    comps, Mu, Mi = T.losses_f64(P, R, c["users"][rows], c["its"][rows], keeps, c["L"], 0.3, reg, 2.0, n_div=n_div)
    sum(comps).backward()
    with torch.no_grad():
        tn = ((Mu[c["users"][rows]] * torch.tensor(keeps["u"], dtype=dtype)).norm(dim=1).numpy() / 0.7,
              (Mi[c["its"][rows]] * torch.tensor(keeps["i"], dtype=dtype)).norm(dim=1).numpy() / 0.7)
    G = {k: np.zeros(v.shape) if v.grad is None else v.grad.numpy().astype(np.float64) for k, v in P.items()}
    return [x.item() for x in comps], G, tn


def _edge_compare(c, what, reg=0.1, ok=None, floor=None, widen=False, m=None):
    """The device step on the batch of ``c`` against the float64 twin on the rows ``ok`` (all when None) with n as the divisor.
    ``floor`` ({name: gradient}): each tensor's scale is max|want| or that tensor at a batch without the exact cancellation,
    whichever is more.  ``widen``: allow max(ATOL * scale, 4 x the error of the same twin in float32 on the CPU), both printed"""
    import torch
    n = c["n"]
    ok = np.ones(n, bool) if ok is None else ok
    m = _detached(c, reg) if m is None else m
    comps, G, _ = _twin_run(c, m, ok, torch.float64, reg, n_div=n)
    comps32, G32, _ = _twin_run(c, m, ok, torch.float32, reg, n_div=n) if widen else (comps, None, None)
    loss = m.gradient_step(c["users"], c["its"], target_keep=_target_keep(c)).cpu().numpy()
    want, want32 = (np.array(x + [sum(x)], np.float64) for x in (comps, comps32))
    print(what, "loss", loss, "twin", want, "abs err", np.abs(loss - want), "fp32-CPU err", np.abs(want32 - want))
    assert np.isfinite(loss).all()
    assert np.all(np.abs(loss - want) <= np.maximum(1e-5 * np.abs(want), 4 * np.abs(want32 - want)))
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    assert set(got) == set(G)
    for k in G:                       # every tensor is measured before the assertion
        scale = float(np.abs(G[k]).max())
        if floor is not None:
            scale = max(scale, float(np.abs(floor[k]).max()))
        err = np.abs(got[k].astype(np.float64) - G[k])
        atol = ATOL * scale
        if widen:
            err32 = float(np.abs(G32[k] - G[k]).max())
            atol = max(atol, 4 * err32)
            print(f"{what}: {k}: max abs err {err.max():.3e}, scale {scale:.3e}, fp32-CPU err {err32:.3e}")
        else:
            print(f"{what}: {k}: max abs err {err.max():.3e}, scale {scale:.3e}")
        assert np.isfinite(got[k]).all(), k
        assert np.all(err <= atol + RTOL * np.abs(G[k])), (what, k, float(err.max()), scale)
    return loss, got, m


@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("n", [15, 16, 17, 63, 65])
def test_batch_sizes_around_the_tiles(n, d):
    """below, at and above a wavefront's 16 rows and a workgroup's 64 (n = 64 is in STEP_CASES)"""
    c = _step_case(n, 2, d, 100, 37, 1000 + n + d)
    assert len(np.unique(c["users"])) < n and len(np.unique(c["its"])) < n and (c["users"] == 47).any() and (c["its"] == 39).any()
    _edge_compare(c, f"n = {n}, d = {d}")


def test_full_batch_at_four_layers():
    """n = 2048 at L = SKR_BM3_MAX_LAYERS = 4 on a 2100 x 2100 graph, both modalities: 32 batch workgroups, 128 MFMA trips of the
    projections' weight gradient; then the same call again: the same bits"""
    import time
    import torch
    from skrec import _hip
    t0 = time.time()
    assert _hip.SKR_BM3_MAX_LAYERS == 4 and _hip.SKR_BM3_MAX_BATCH == 2048
    c = _step_case(2048, 4, 64, 100, 37, 2100, U=2100, I=2100)
    loss, _, m = _edge_compare(c, "n = 2048", widen=True)
    g1, M1 = m._grad.clone(), m.M.clone()
    m._work.fill_(255)
    loss2 = m.gradient_step(c["users"], c["its"], target_keep=_target_keep(c)).cpu().numpy()
    assert np.array_equal(loss.view(np.uint32), loss2.view(np.uint32)) and torch.equal(g1, m._grad) and torch.equal(M1, m.M)
    print("full batch: wall time", time.time() - t0)


@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("which", ["user", "item"])
def test_one_id_in_every_row(which, n):
    """the longest segment: all n ranks of one list name one id, so one wavefront of seg_add (and, for the item, of the
    feature rows' seg_rows) walks them all and the rank kernel counts n equal keys; the node's flags are one row repeated.
    The scales are floored by the same batch with its random ids"""
    import torch
    c = _step_case(n, 2, 64, 100, 37, 3000 + n)
    m = _detached(c, 0.1)
    floor = _twin_run(c, m, np.ones(n, bool), torch.float64, 0.1, n_div=n)[1]
    if which == "user":
        c["users"][:] = c["users"][n - 1]
        c["keeps"]["u"][:] = c["keeps"]["u"][n - 1]
    else:
        c["its"][:] = c["its"][3]
        for k in "itv":
            c["keeps"][k][:] = c["keeps"][k][3]
    _edge_compare(c, f"one {which}, n = {n}", floor=floor, m=m)


def test_ids_out_of_range_contribute_nothing():
    """the result is that of the batch without those rows with n = 70 as the divisor of every cosine mean; the regulariser is
    that of the whole tables, as ever"""
    U, I, n = 48, 40, 70
    c = _step_case(n, 2, 64, 100, 37, 4000)
    users, its = c["users"], c["its"]
    users[3], its[17], users[40], its[40], users[69] = U, -1, -7, I, 2 ** 31 - 1
    ok = (users >= 0) & (users < U) & (its >= 0) & (its < I)
    assert ok.sum() == 66
    _edge_compare(c, "ids out of range", ok=ok)
    # the device's own result on the filtered batch: without the regulariser every gradient, and every sum of cosines
    # (2 - graph, 4 cl_weight - modal), scales by 66 / 70; the losses are compared as they are, at their own rtol
    m = _detached(c, 0.0)
    loss = m.gradient_step(users, its, target_keep=_target_keep(c)).cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    loss2 = m.gradient_step(users[ok], its[ok], target_keep=tuple(k[ok] for k in _target_keep(c))).cpu().numpy()
    got2 = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    assert loss[2] == 0 and loss2[2] == 0
    np.testing.assert_allclose(loss[:2], np.array([2.0, 8.0]) * (4 / 70) + loss2[:2] * (66 / 70), rtol=1e-5)
    for k in got:
        np.testing.assert_allclose(got[k], got2[k] * np.float32(66 / 70), rtol=RTOL, atol=ATOL * np.abs(got[k]).max(), err_msg=k)


def test_an_empty_batch_writes_nothing():
    import ctypes
    import torch
    from skrec import _hip
    c = _step_case(17, 2, 64, 100, 37, 5000)
    m = _detached(c)
    loss = torch.full((4,), 7.0, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    m._prev_items = ids               # rows that a step would clear first
    a = m._step_args(ids, ids, None, loss)
    assert a.n_clear == 4
    a.n = 0
    m._grad.fill_(3.0)
    m._work.fill_(5)
    tabs = [m.M, m._G, m._ping[0], m._ping[1]]
    for t in tabs:
        t.fill_(2.0)
    before = [t.clone() for t in tabs] + [m._work.clone(), m._flat.clone()]
    _hip.check(_hip.lib().skr_bm3_step(ctypes.byref(a), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (m._grad == 3.0).all()
    assert all(torch.equal(x, y) for x, y in zip(before, tabs + [m._work, m._flat]))
    # through the class: a zero loss, a zero gradient whatever the last step left there, nothing left to clear
    m._prev_items = None
    m._grad.zero_()
    m.gradient_step(c["users"], c["its"])
    assert m._grad.any() and m._prev_items is not None
    z, step = np.zeros(0, np.int32), m._step
    loss = m.gradient_step(z, z)
    assert loss.shape == (4,) and not loss.any() and not m._grad.any() and m._prev_items is None and m._step == step
    # train_step: the zero gradient through Adam, as MGCN, LATTICE and SLMRec do it; with no moments yet nothing moves
    m.gradient_step(c["users"], c["its"])
    flat = m._flat.clone()
    assert not m.train_step(z, z).any()
    assert torch.equal(flat, m._flat)


def test_a_predictor_output_of_exact_zeros():
    """W = 0 and b = 0: every P row is zero, |P| takes the 1e-8 clamp, every cosine is 0 (graph = 2, modal = 4 cl_weight) and the
    predictor's gradient is of the order 1e8 / n, finite"""
    c = _step_case(70, 2, 64, 100, 37, 6000)
    c["P"]["predictor.weight"][:] = 0
    c["P"]["predictor.bias"][:] = 0
    loss, got, _ = _edge_compare(c, "P = 0", widen=True)
    assert loss[0] == 2 and loss[1] == 8 and np.abs(got["predictor.bias"]).max() > 1e4


def test_target_rows_with_a_norm_under_the_clamp():
    """the isolated user's and the isolated item's embedding rows scaled by 1e-9: their target rows (row 1 of the batch) have
    0 < |t| < 1e-8, the max(|t|, 1e-8) branch of the cosine; the reference is the twin's own clamp"""
    import torch
    c = _step_case(70, 2, 64, 100, 37, 6001)
    U, I = c["U"], c["I"]
    assert c["users"][1] == U - 1 and c["its"][1] == I - 1 and (c["users"] == U - 1).sum() == 1 and (c["its"] == I - 1).sum() == 1
    c["keeps"]["u"][1], c["keeps"]["i"][1] = 1, 1
    c["P"]["user_embedding.weight"][U - 1] *= np.float32(1e-9)
    c["P"]["item_id_embedding.weight"][I - 1] *= np.float32(1e-9)
    m = _detached(c, 0.1)
    tn = _twin_run(c, m, np.ones(70, bool), torch.float64, 0.1)[2]
    print("target norms of row 1:", tn[0][1], tn[1][1])
    assert 0 < tn[0][1] < 1e-8 and 0 < tn[1][1] < 1e-8
    _edge_compare(c, "small targets", widen=True, m=m)
