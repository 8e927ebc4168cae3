"""CPU suite of CDAE (skrec/recommender/CDAE.py, csrc/cdae.hip's argument checks, tests/golden/golden_cdae.npz): the config,
the limits and the reference's refusals, the C ABI's checks without a GPU, the initialisation and the host batch layout
against the fixture, and the fixture itself against the float64 replay the GPU tests lean on (tests/cdae_twin.py)."""
import numpy as np
import pytest

import cdae_twin as T

SEED = 2021
CONFIG = dict(lr=1e-2, reg=1e-3, hidden_dim=64, dropout=0.5, num_neg=2, hidden_act="sigmoid", batch_size=24, epochs=3)


def test_config_defaults_and_validation():
    from skrec.recommender.CDAE import CDAEConfig
    c = CDAEConfig()
    assert dict(c.items()) == dict(lr=1e-3, reg=1e-3, hidden_dim=64, dropout=0.5, num_neg=5, hidden_act="sigmoid",
                                   loss_func="sigmoid_cross_entropy", batch_size=256, epochs=1000, early_stop=200)
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(reg=-1.0), dict(hidden_dim=0), dict(hidden_dim=64.0), dict(dropout=1.0),
                dict(dropout=1), dict(num_neg=-1), dict(num_neg=1.5), dict(hidden_act="relu"), dict(loss_func="hinge"),
                dict(batch_size=0), dict(epochs=-1), dict(early_stop=1.0)):
        with pytest.raises(AssertionError):
            CDAEConfig(**bad)
    CDAEConfig(loss_func="square", num_neg=0, dropout=-0.5)          # all three pass validation, as in the reference


def test_limits_and_the_reference_refusals():
    from skrec.recommender.CDAE import CDAE, CDAEConfig, check_limits
    assert check_limits(CDAEConfig(hidden_dim=40, batch_size=1024, hidden_act="identity", dropout=0.0)) == 40
    with pytest.raises(ValueError, match="loss function 'square' is invalid"):
        check_limits(CDAEConfig(loss_func="square"))
    with pytest.raises(ValueError, match=r"'keep_prob' must be a float in the range \(0, 1\]"):
        check_limits(CDAEConfig(dropout=-0.5))
    with pytest.raises(NotImplementedError, match="hidden_dim <= 64"):
        check_limits(CDAEConfig(hidden_dim=65))
    with pytest.raises(ValueError, match="batch_size <= 1024"):
        check_limits(CDAEConfig(batch_size=1025))
    # the constructor raises before it touches the data set or the GPU
    with pytest.raises(ValueError, match="square"):
        CDAE(None, dict(loss_func="square"))
    with pytest.raises(ValueError, match="keep_prob"):
        CDAE(None, dict(dropout=-0.25))
    with pytest.raises(NotImplementedError, match="hidden_dim <= 64"):
        CDAE(None, dict(hidden_dim=128))


def test_registry_finds_the_model():
    import os
    import skrec.recommender as R
    assert os.path.exists(os.path.join(os.path.dirname(R.__file__), "CDAE.py"))
    from skrec.recommender.CDAE import CDAE
    assert CDAE.config_class.__name__ == "CDAEConfig"


def test_abi_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    ok = dict(n=8, n_pairs=100, n_distinct=50, n_users=10, n_items=100, dim=64, act=1, keep_prob=0.5, work_bytes=1 << 30)

    def step(first=p, **kw):
        a = dict(ok, **kw)
        return L.skr_cdae_step(first, *([p] * 13), a["n"], a["n_pairs"], a["n_distinct"], a["n_users"], a["n_items"], a["dim"],
                               a["act"], a["keep_prob"], 1e-3, p, p, p, p, p, p, a["work_bytes"], p, None)
    assert step(first=None) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=1025) == -1 and b"at most 1024" in L.skr_last_error()
    assert step(n=-1) == -1
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(dim=0) == -1
    assert step(act=2) == -1 and b"act" in L.skr_last_error()
    assert step(keep_prob=0.0) == -1 and b"keep_prob" in L.skr_last_error()
    assert step(keep_prob=1.5) == -1
    assert step(n_distinct=101) == -1
    assert step(n_pairs=-1) == -1
    assert step(work_bytes=64) == -1 and b"skr_cdae_workspace" in L.skr_last_error()
    assert step(n_items=0) == -1
    # (an empty batch WRITES its zero loss pair, so it needs real device memory: tests/test_gpu_cdae.py,
    # test_an_empty_batch_writes_a_zero_loss_and_nothing_else; its arguments are checked like any batch's)
    assert step(n=0, dim=65) == -1 and step(n=0, act=2) == -1
    assert L.skr_cdae_queries(None, p, p, p, p, None, 4, 10, 100, 64, 1, p, None) == -1
    assert L.skr_cdae_queries(p, p, p, p, p, None, 11, 10, 100, 64, 1, p, None) == -1 and b"user list" in L.skr_last_error()
    assert L.skr_cdae_queries(p, p, p, p, p, None, 4, 10, 100, 64, 3, p, None) == -1
    assert L.skr_cdae_draws(p, p, p, None, 4, 4, 0.5, 1, 0, None, None) == -1
    assert L.skr_cdae_draws(p, p, p, None, 4, 4, 0.0, 1, 0, p, None) == -1
    # the workspace: two 64-float rows and two scalars per user, two scalars per pair
    assert L.skr_cdae_workspace(0, 100) == 0 and L.skr_cdae_workspace(1025, 100) == 0 and L.skr_cdae_workspace(8, -1) == 0
    for n, P in ((8, 100), (1024, 300000), (37, 4099)):
        r4 = lambda x: (x + 3) // 4 * 4      # noqa: E731
        assert L.skr_cdae_workspace(n, P) == 4 * (128 * n + 2 * r4(n) + 2 * r4(P))


def test_initialisation_equals_the_reference(golden):
    import torch
    from skrec.recommender.CDAE import _init_tables
    g = golden("golden_cdae")
    torch.manual_seed(SEED)
    got = _init_tables(64, 96, 64)
    for k, t in zip(T.PARAMS, got):
        assert t.shape == g[k + "0"].shape, k
        assert np.array_equal(t.numpy(), g[k + "0"]), k


def test_host_layout_reproduces_the_reference_batches(golden):
    from skrec.recommender.CDAE import batch_layout
    g = golden("golden_cdae")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    pb = np.concatenate([[0], np.cumsum(g["pair_sizes"])])
    steps = T.fixture_steps(g)
    assert [len(s[0]) for s in steps] == [24, 24, 15] * 3
    for s, (users, negs, keep, flat) in enumerate(steps):
        assert (rowptr[users + 1] > rowptr[users]).all()
        assert [len(n) for n in negs] == list(2 * (rowptr[users + 1] - rowptr[users])) and len(flat) == sum(map(len, negs))
        lay = batch_layout(rowptr, items, users, negs)
        sl = slice(pb[s], pb[s + 1])
        assert np.array_equal(lay["bat_items"], g["bat_items"][sl])
        assert np.array_equal(lay["bat_labels"], g["bat_labels"][sl].astype(np.float32))
        assert np.array_equal(lay["bat_idx"], g["bat_idx"][sl])
        P = pb[s + 1] - pb[s]
        assert len(keep) == P == len(lay["pitem"]) == lay["uptr"][-1]
        # the pair list: the same (user, item, label) triples, per user ascending
        ref = sorted(zip(g["bat_idx"][sl].tolist(), g["bat_items"][sl].tolist(), g["bat_labels"][sl].tolist()))
        assert list(zip(lay["puser"].tolist(), lay["pitem"].tolist(), lay["plabel"].tolist())) == ref
        for b in range(len(users)):
            row = lay["pitem"][lay["uptr"][b]:lay["uptr"][b + 1]]
            assert (np.diff(row) > 0).all() and (lay["puser"][lay["uptr"][b]:lay["uptr"][b + 1]] == b).all()
        # the item-major view lists every pair exactly once, under its item, users ascending
        assert np.array_equal(np.sort(lay["ipair"]), np.arange(P))
        assert (np.diff(lay["ditems"]) > 0).all() and lay["iptr"][0] == 0 and lay["iptr"][-1] == P
        for j, it in enumerate(lay["ditems"]):
            ps = lay["ipair"][lay["iptr"][j]:lay["iptr"][j + 1]]
            assert len(ps) > 0 and (lay["pitem"][ps] == it).all() and (np.diff(ps) > 0).all()


def test_fixture_matches_a_float64_replay(golden):
    g = golden("golden_cdae")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    steps = T.fixture_steps(g)
    test_users = g["test_users"]
    assert len(test_users) == 63 and 63 in test_users and rowptr[64] == rowptr[63]     # the cold test user
    init = {k: g[k + "0"] for k in T.PARAMS}
    par, losses, scores = T.replay_f64(rowptr, items, init, [s[:3] for s in steps], CONFIG, 3, test_users)
    np.testing.assert_allclose(losses[:, 0], g["bce"], rtol=1e-6)
    np.testing.assert_allclose(losses[:, 1], g["l2"], rtol=1e-6)
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    for k, lim in zip(T.PARAMS, dev_p):
        assert np.abs(par[k] - g[k + "1"]).max() <= lim * (1 + 1e-9), k
    assert len(scores) == 3 and g["pred"].shape == (3, 63, 96)
    for s, p, lim in zip(scores, g["pred"], dev_s):
        assert np.abs(s - p).max() <= lim * (1 + 1e-9)
    # what the GPU tests rely on: the recorded deviations are the reference's fp32 noise, not a recording error
    assert dev_s.max() < 2e-6 and dev_p.max() < 1e-5
    assert g["close_users"].max() <= 3
