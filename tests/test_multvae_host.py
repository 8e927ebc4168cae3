"""CPU suite of MultVAE (skrec/recommender/MultVAE.py, csrc/multvae.hip's argument checks, tests/golden/golden_multvae.npz):
the config and the limits, the C ABI's checks without a GPU, the initialisation against the fixture, and the fixture
itself against a float64 replay written here (tests/multvae_twin.py)."""
import numpy as np
import pytest

import multvae_twin as T

SEED = 2021
CONFIG = dict(lr=1e-2, reg=1e-3, p_dims=[64], keep_prob=0.5, anneal_steps=6, anneal_cap=0.2, batch_size=24, epochs=3)


def test_config_defaults_and_validation():
    from skrec.recommender.MultVAE import MultVAEConfig
    c = MultVAEConfig()
    assert dict(c.items()) == dict(lr=1e-3, reg=0.0, p_dims=[64], q_dims=None, keep_prob=0.5, anneal_steps=200000,
                                   anneal_cap=0.2, batch_size=256, epochs=1000, early_stop=200)
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(reg=-1.0), dict(p_dims=64), dict(q_dims=64), dict(keep_prob=1),
                dict(anneal_steps=-1), dict(anneal_steps=1.5), dict(anneal_cap=-0.1), dict(batch_size=0), dict(epochs=-1),
                dict(early_stop=1.0)):
        with pytest.raises(AssertionError):
            MultVAEConfig(**bad)


def test_limits_are_named():
    from skrec.recommender.MultVAE import MultVAE, MultVAEConfig, check_limits
    assert check_limits(MultVAEConfig(p_dims=[40], q_dims=[40], batch_size=1024)) == 40
    with pytest.raises(NotImplementedError, match=r"p_dims == \[d\]"):
        check_limits(MultVAEConfig(p_dims=[64, 32]))
    with pytest.raises(NotImplementedError, match="d <= 64"):
        check_limits(MultVAEConfig(p_dims=[65]))
    with pytest.raises(NotImplementedError, match="q_dims in"):
        check_limits(MultVAEConfig(p_dims=[64], q_dims=[128, 64]))
    with pytest.raises(ValueError, match="batch_size <= 1024"):
        check_limits(MultVAEConfig(batch_size=1025))
    # the constructor raises before it touches the data set or the GPU
    with pytest.raises(NotImplementedError, match="d <= 64"):
        MultVAE(None, dict(p_dims=[65]))
    with pytest.raises(ValueError, match="batch_size <= 1024"):
        MultVAE(None, dict(batch_size=2048))


def test_abi_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    ok = dict(n=8, n_users=10, n_items=100, dim=64, keep_prob=0.5, keep=None, eps=None, work_bytes=1 << 30)

    def step(**kw):
        a = dict(ok, **kw)
        return L.skr_multvae_step(p, p, p, p, p, p, p, a["n"], a["n_users"], a["n_items"], a["dim"], a["keep_prob"], 0.1,
                                  a["keep"], a["eps"], 1, 0, p, p, p, p, p, a["work_bytes"], p, None)
    assert L.skr_multvae_step(None, p, p, p, p, p, p, 8, 10, 100, 64, 0.5, 0.1, None, None, 1, 0, p, p, p, p, p, 1 << 30, p,
                              None) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=1025) == -1 and b"at most 1024" in L.skr_last_error()
    assert step(n=-1) == -1
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(dim=0) == -1
    assert step(keep_prob=0.0) == -1 and b"keep_prob" in L.skr_last_error()
    assert step(keep_prob=1.5) == -1
    assert step(keep=p) == -1 and b"together" in L.skr_last_error()
    assert step(work_bytes=64) == -1 and b"skr_multvae_workspace" in L.skr_last_error()
    assert step(n_items=0) == -1
    # (an empty batch WRITES its zero loss pair, so it needs real device memory: tests/test_gpu_multvae.py,
    # test_an_empty_batch_writes_a_zero_loss_and_nothing_else; its arguments are checked like any batch's)
    assert step(n=0, dim=65) == -1 and step(n=0, keep=p) == -1
    assert L.skr_multvae_queries(None, p, p, p, None, 4, 10, 100, p, None) == -1
    assert L.skr_multvae_queries(p, p, p, p, None, 11, 10, 100, p, None) == -1 and b"user list" in L.skr_last_error()
    assert L.skr_multvae_draws(p, p, p, 4, 10, 64, 0.5, 1, 0, None, p, p, None) == -1
    assert L.skr_multvae_draws(p, p, p, 4, 10, 64, 0.0, 1, 0, p, p, p, None) == -1
    # the workspace: per user 384 floats of rows and 4 scalars, 66 floats per user and workgroup, the offsets
    assert L.skr_multvae_workspace(0, 100) == 0 and L.skr_multvae_workspace(1025, 100) == 0
    assert L.skr_multvae_workspace(8, 0) == 0
    for n, ni in ((8, 100), (1024, 100000), (37, 64 * 512 + 1)):
        n4, wg = (n + 3) // 4 * 4, min((ni + 63) // 64, 512)
        assert L.skr_multvae_workspace(n, ni) == 4 * (n4 * (384 + 4 + 66 * wg) + (n + 1 + 3) // 4 * 4)
    # it grows with the batch and the workgroups, not with B * I
    assert L.skr_multvae_workspace(1024, 100000) == L.skr_multvae_workspace(1024, 10000000)


def test_initialisation_equals_the_reference(golden):
    import torch
    from skrec.recommender.MultVAE import _init_tables
    g = golden("golden_multvae")
    torch.manual_seed(SEED)
    got = _init_tables(96, 64)
    for k, t in zip(T.PARAMS, got):
        assert t.shape == g[k + "0"].shape, k
        assert np.array_equal(t.numpy(), g[k + "0"]), k


def test_fixture_matches_a_float64_replay(golden):
    g = golden("golden_multvae")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    steps = T.fixture_steps(g)
    assert [len(s[0]) for s in steps] == [24, 24, 15] * 3
    for users, keep, eps in steps:
        assert len(keep) == int((rowptr[users + 1] - rowptr[users]).sum()) and eps.shape == (len(users), 64)
        assert (rowptr[users + 1] > rowptr[users]).all()                 # users with history only
    test_users = g["test_users"]
    assert len(test_users) == 63 and 63 in test_users and rowptr[64] == rowptr[63]     # the cold test user
    init = {k: g[k + "0"] for k in T.PARAMS}
    par, losses, scores = T.replay_f64(rowptr, items, ni, init, steps, CONFIG, 3, test_users)
    np.testing.assert_allclose(losses[:, 0], g["neg_ll"], rtol=1e-6)
    # kl is between 0.017 and 1.5 here and is the fp32 sum over 64 columns of terms that cancel (-logvar + exp(logvar)
    # - 1 with exp(logvar) near 1): the fixture's fp32 value carries an absolute error, so the 1e-6 is absolute for it
    np.testing.assert_allclose(losses[:, 1], g["kl"], rtol=0, atol=1e-6)
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    for k, lim in zip(T.PARAMS, dev_p):
        assert np.abs(par[k] - g[k + "1"]).max() <= 10 * lim, k
    assert len(scores) == 3 and g["pred"].shape == (3, 63, 96)
    assert np.abs(scores[-1] - g["pred"][-1]).max() <= 10 * dev_s[-1]
    for s, p, lim in zip(scores, g["pred"], dev_s):
        assert np.abs(s - p).max() <= 10 * lim
    # what the GPU tests rely on: the recorded deviations are the reference's fp32 noise, not a recording error
    assert dev_s[-1] < 1e-6 and dev_p.max() < 1e-5
    assert list(g["close_users"]) == [2, 0, 0]
