"""CPU suite of LightGCL (skrec/recommender/LightGCL.py, csrc/lightgcl.hip's argument checks, tests/golden/golden_lightgcl.npz):
the config and the limits, the registry, the C ABI's checks without a GPU, the initialisation against the fixture, and the
fixture itself against a float64 replay written here (tests/lightgcl_twin.py, the per-layer form)."""
import ctypes

import numpy as np
import pytest

import lightgcl_twin as T

SEED = 2021
CONFIG = dict(lr=1e-2, lambda1=0.2, d=64, gnn_layer=2, batch_size=256, svd_q=5, dropout=0.0, temp=0.2, lambda2=1e-4, epochs=3)


def test_config_defaults_and_validation():
    from skrec.recommender.LightGCL import LightGCLConfig
    c = LightGCLConfig()
    assert dict(c.items()) == dict(lr=1e-3, lambda1=0.2, d=64, gnn_layer=2, batch_size=2048, svd_q=5, dropout=0.0, temp=0.2,
                                   lambda2=1e-7, epochs=500, early_stop=100)
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(lambda1=-0.1), dict(lambda1=1), dict(d=0), dict(d=64.0), dict(gnn_layer=0),
                dict(batch_size=0), dict(svd_q=0), dict(dropout=-0.1), dict(dropout=0), dict(temp=0.0), dict(lambda2=-1.0),
                dict(epochs=-1), dict(early_stop=1.0)):
        with pytest.raises(AssertionError):
            LightGCLConfig(**bad)


def test_limits_are_named():
    from skrec.recommender.LightGCL import LightGCL, LightGCLConfig, check_limits
    check_limits(LightGCLConfig(d=40, svd_q=16, batch_size=2048, lambda1=0.0))
    with pytest.raises(NotImplementedError, match="dropout == 0"):
        check_limits(LightGCLConfig(dropout=0.1))
    with pytest.raises(NotImplementedError, match="d <= 64"):
        check_limits(LightGCLConfig(d=65))
    with pytest.raises(NotImplementedError, match="svd_q <= 16"):
        check_limits(LightGCLConfig(svd_q=17))
    with pytest.raises(NotImplementedError, match="batch_size <= 2048"):
        check_limits(LightGCLConfig(batch_size=2049))
    # the constructor raises before it touches the data set or the GPU
    with pytest.raises(NotImplementedError, match="d <= 64"):
        LightGCL(None, dict(d=128))
    with pytest.raises(NotImplementedError, match="dropout == 0"):
        LightGCL(None, dict(dropout=0.25))


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.LightGCL import LightGCL, LightGCLConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("LightGCL")
    assert reg.get_model("LightGCL") == (LightGCL, LightGCLConfig)


def test_abi_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used

    def cl(**kw):
        a = dict(dict(Q=p, n=8, n_rows=100, inv_temp=5.0, work_bytes=1 << 30), **kw)
        return L.skr_lightgcl_cl(a["Q"], a["n"], p, a["n_rows"], a["inv_temp"], 0.1, p, p, p, p, a["work_bytes"], None)
    assert cl(Q=None) == -1 and b"NULL" in L.skr_last_error()
    assert cl(n=4097) == -1 and b"at most 4096" in L.skr_last_error()
    assert cl(n=-1) == -1 and cl(n_rows=0) == -1
    assert cl(inv_temp=0.0) == -1 and b"inv_temp" in L.skr_last_error()
    assert cl(work_bytes=64) == -1 and b"skr_lightgcl_cl_workspace" in L.skr_last_error()
    assert cl(n=0) == 0                       # no query: nothing to launch
    # the workspace: per query one lse, and 66 floats per workgroup; it grows with the workgroups, not with n * n_rows
    assert L.skr_lightgcl_cl_workspace(0, 100) == 0 and L.skr_lightgcl_cl_workspace(4097, 100) == 0
    assert L.skr_lightgcl_cl_workspace(8, 0) == 0
    for n, nr in ((8, 100), (4096, 100000), (37, 64 * 512 + 1)):
        n4, wg = (n + 3) // 4 * 4, min((nr + 63) // 64, 512)
        assert L.skr_lightgcl_cl_workspace(n, nr) == 4 * n4 * (1 + 66 * wg)
    assert L.skr_lightgcl_cl_workspace(2048, 1000000) == L.skr_lightgcl_cl_workspace(2048, 100000000)
    assert L.skr_lightgcl_workspace(2049, 10, 10) == 0 and L.skr_lightgcl_workspace(0, 10, 10) == 0
    assert L.skr_lightgcl_workspace(16, 70, 45) > L.skr_lightgcl_cl_workspace(32, 45)

    def step(**kw):
        a = _hip.LightGCLStepArgs()
        a.plan_a = a.plan_at = a.E0 = a.fac_us = a.fac_vs = a.fac_ut = a.fac_vt = a.uids = a.pos = a.neg = p
        a.sum = a.below = a.gsum = a.addend = a.grad = a.loss = a.work = p
        a.ping[0] = a.ping[1] = p
        a.n_users, a.n_items, a.dim, a.n_layers, a.q, a.n = 70, 45, 64, 2, 5, 16
        a.inv_temp, a.lambda1, a.lambda2, a.work_bytes = 5.0, 0.2, 1e-4, 1 << 30
        for k, v in kw.items():
            if k == "ping0":
                a.ping[0] = v
            else:
                setattr(a, k, v)
        return L.skr_lightgcl_step(ctypes.byref(a), None)
    assert L.skr_lightgcl_step(None, None) == -1
    assert step(E0=None) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=2049) == -1 and b"at most 2048" in L.skr_last_error()
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(n_layers=0) == -1 and b"n_layers" in L.skr_last_error()
    assert step(ping0=None) == -1 and b"ping" in L.skr_last_error()
    assert step(q=17) == -1 and b"lambda1 > 0" in L.skr_last_error()
    assert step(addend=None) == -1
    assert step(inv_temp=0.0) == -1
    assert step(work_bytes=64) == -1 and b"skr_lightgcl_workspace" in L.skr_last_error()
    assert step(work=8) == -1 and b"aligned" in L.skr_last_error()
    assert step(n=0) == 0                     # an empty batch: nothing to launch
    assert L.skr_lightgcl_step_timed(None, None, None) == -1


def test_initialisation_equals_the_reference(golden):
    """one torch.randn(min(U, I), q) before the two xavier draws (torch.svd_lowrank's test matrix, LightGCL.py:202)"""
    import torch
    from skrec.recommender.LightGCL import init_tables
    g = golden("golden_lightgcl")
    torch.manual_seed(SEED)
    R, eu, ei = init_tables(64, 96, 64, 5)
    assert R.shape == (64, 5)
    assert np.array_equal(eu.numpy(), g["E_u_00"]) and np.array_equal(ei.numpy(), g["E_i_00"])
    torch.manual_seed(SEED)                    # without the draw the tables differ
    assert not np.array_equal(torch.nn.init.xavier_uniform_(torch.empty(64, 64)).numpy(), g["E_u_00"])


def test_fixture_matches_a_float64_replay(golden):
    g = golden("golden_lightgcl")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    steps = T.fixture_steps(g)
    assert [len(s[0]) for s in steps] == [256, 256, 251] * 3
    # the recorded adjacency is the train CSR with 1 / sqrt(rowdeg * coldeg)
    rows = np.repeat(np.arange(64), np.diff(rowptr))
    assert np.array_equal(g["adj_rows"], rows) and np.array_equal(g["adj_cols"], items)
    A = T.dense_adjacency(rowptr, items, ni)
    np.testing.assert_allclose(g["adj_val"], A[rows, items], rtol=2e-7)
    assert rowptr[64] == rowptr[63] and not (items == 95).any()          # a zero-degree user and a zero-degree item
    # the recorded factors are a rank-5 SVD: orthonormal ut, vt (the reference's own: <= 1.2e-6)
    for f in (g["ut"], g["vt"]):
        assert np.abs(f.astype(np.float64) @ f.astype(np.float64).T - np.eye(5)).max() <= 1e-5
    test_users = g["test_users"]
    assert len(test_users) == 63 and 63 in test_users
    A32 = T.dense_adjacency(rowptr, items, ni, g["adj_val"])
    eu, ei, losses, scores = T.replay_f64(A32, T.fixture_factors(g), (g["E_u_00"], g["E_i_00"]), steps, CONFIG, 3, test_users)
    dev_p, dev_s, dev_l = g["f64_dev_params"], g["f64_dev_scores"], float(g["f64_dev_loss"])
    print("loss dev", np.abs(losses / g["loss"].astype(np.float64) - 1).max(), "allowed", 2 * dev_l)
    print("param dev", np.abs(eu - g["E_u_01"]).max(), np.abs(ei - g["E_i_01"]).max(), "allowed", 2 * dev_p)
    np.testing.assert_allclose(losses, g["loss"], rtol=2 * dev_l)
    assert np.abs(eu - g["E_u_01"]).max() <= 2 * dev_p[0]
    assert np.abs(ei - g["E_i_01"]).max() <= 2 * dev_p[1]
    assert len(scores) == 3 and g["pred"].shape == (3, 63, 96)
    for s, p, lim in zip(scores, g["pred"], dev_s):          # the stale sums: the scores of the last training forward
        assert np.abs(s - p).max() <= 2 * lim
    # the fixture's own conditions, and what the GPU tests rely on
    assert (g["close_users"] <= 3).all() and float(g["clamp_distance"]) >= 1e-4
    assert dev_s.max() < 1e-6 and dev_p.max() < 1e-6 and dev_l < 1e-6
