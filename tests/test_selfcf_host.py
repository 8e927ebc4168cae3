"""CPU suite of SelfCF (skrec/recommender/SelfCF.py, csrc/selfcf.hip's and skr_spmm_plan_run_dropped's argument checks,
tests/golden/golden_selfcf.npz): the config and the limits, the registry, the library's exports and checks without a GPU, the
initialisation against the fixture, the fixture against the float64 twin (tests/selfcf_twin.py), the keep permutation's numpy
mirror against a dense masked matrix, the folded score identity."""
import ctypes

import numpy as np
import pytest

import selfcf_twin as T

SEED = 2021
CONFIG = dict(lr=1e-2, reg=1e-3, embed_dim=64, n_layers=2, dropout=0.5, batch_size=256, epochs=3)


def test_config_defaults_and_validation():
    from skrec.recommender.SelfCF import SelfCFConfig
    c = SelfCFConfig()
    assert dict(c.items()) == dict(lr=1e-3, reg=0.0, embed_dim=64, n_layers=2, dropout=0.5, batch_size=2048, epochs=1000, early_stop=200,
                                   draws="device")
    assert SelfCFConfig.param_space() == {"n_layers": [2], "reg": [0.0], "dropout": [0.5]}
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(reg=-0.1), dict(reg=1), dict(embed_dim=0), dict(embed_dim=64.0), dict(n_layers=-1),
                dict(n_layers=2.0), dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=0), dict(batch_size=0), dict(epochs=-1),
                dict(early_stop=1.0), dict(draws="reference")):
        with pytest.raises(AssertionError):
            SelfCFConfig(**bad)


def test_limits_are_named():
    from skrec.recommender.SelfCF import SelfCF, SelfCFConfig, check_limits
    check_limits(SelfCFConfig(embed_dim=20, n_layers=4, batch_size=2048))
    check_limits(SelfCFConfig(n_layers=0))
    with pytest.raises(NotImplementedError, match="embed_dim <= 64"):
        check_limits(SelfCFConfig(embed_dim=65))
    with pytest.raises(NotImplementedError, match="n_layers <= 4"):
        check_limits(SelfCFConfig(n_layers=5))
    with pytest.raises(NotImplementedError, match="batch_size <= 2048"):
        check_limits(SelfCFConfig(batch_size=2049))
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(SelfCFConfig(), world=2)
    # the constructor raises before it touches the data set or the GPU
    with pytest.raises(NotImplementedError, match="embed_dim <= 64"):
        SelfCF(None, dict(embed_dim=128))
    with pytest.raises(NotImplementedError, match="n_layers <= 4"):
        SelfCF(None, dict(n_layers=7))


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.SelfCF import SelfCF, SelfCFConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("SelfCF")
    assert reg.get_model("SelfCF") == (SelfCF, SelfCFConfig)


def test_library_exports_and_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 13
    for name in ("skr_spmm_plan_run_dropped", "skr_selfcf_keeps", "skr_selfcf_workspace", "skr_selfcf_step", "skr_selfcf_step_timed",
                 "skr_selfcf_queries"):
        assert hasattr(L, name) and name in _hip.SIGNATURES
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    assert L.skr_spmm_plan_run_dropped(None, p, 64, p, p, 1.0, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_selfcf_workspace(0, 2) == 0 and L.skr_selfcf_workspace(2049, 2) == 0 and L.skr_selfcf_workspace(8, 5) == 0
    for n in (1, 3, 300, 2048):
        n4 = (n + 3) // 4 * 4
        assert L.skr_selfcf_workspace(n, 2) == 4 * (2 * n4 * 64 + 4 * n4 + (n + 63) // 64 * (64 * 64 + 64) + 2 * n4)
    assert L.skr_selfcf_keeps(None, 10, None, None, 0.5, 1, 1, p, p, p, p, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_selfcf_keeps(p, 10, p, None, 0.5, 1, 1, p, p, p, p, None) == -1 and b"together" in L.skr_last_error()
    assert L.skr_selfcf_keeps(p, 10, None, None, 1.0, 1, 1, p, p, p, p, None) == -1 and b"rate" in L.skr_last_error()
    assert L.skr_selfcf_keeps(p, 0, None, None, 0.5, 1, 1, p, p, p, p, None) == 0
    assert L.skr_selfcf_queries(None, p, 4, 4, p, p, p, None) == -1 and b"NULL" in L.skr_last_error()

    def step(**kw):
        a = _hip.SelfCFStepArgs()
        a.plan_a = a.plan_at = a.params = a.users = a.items = a.keep_fu = a.keep_fi = a.keep_bu = a.keep_bi = p
        a.M = a.G = a.grad = a.loss = a.work = p
        a.ping[0] = a.ping[1] = p
        a.n_users, a.n_items, a.dim, a.n_layers, a.n = 70, 45, 64, 2, 16
        a.edge_scale, a.dropout, a.reg, a.work_bytes = 2.0, 0.5, 1e-3, 1 << 30
        for k, v in kw.items():
            if k == "ping0":
                a.ping[0] = v
            else:
                setattr(a, k, v)
        return L.skr_selfcf_step(ctypes.byref(a), None)
    assert L.skr_selfcf_step(None, None) == -1
    assert step(params=None) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=2049) == -1 and b"at most 2048" in L.skr_last_error()
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(n_layers=5) == -1 and b"n_layers" in L.skr_last_error()
    assert step(plan_a=None) == -1 and b"plans" in L.skr_last_error()
    assert step(keep_bu=None) == -1 and b"keep" in L.skr_last_error()
    assert step(ping0=None) == -1 and b"ping" in L.skr_last_error()
    assert step(dropout=1.0) == -1 and b"dropout" in L.skr_last_error()
    assert step(work_bytes=64) == -1 and b"skr_selfcf_workspace" in L.skr_last_error()
    assert step(work=8) == -1 and b"aligned" in L.skr_last_error()
    assert step(n=0) == 0                     # an empty batch: nothing to launch
    assert L.skr_selfcf_step_timed(None, None, None) == -1


def test_initialisation_equals_the_reference(golden):
    """xavier user_emb, xavier item_emb, then nn.Linear(d, d) (SelfCF.py:86-93, :201-202)"""
    import torch
    from skrec.recommender.SelfCF import init_parameters
    g = golden("golden_selfcf")
    torch.manual_seed(SEED)
    eu, ei, W, b = init_parameters(64, 96, 64)
    for got, name in ((eu, "user_emb"), (ei, "item_emb"), (W, "predictor.weight"), (b, "predictor.bias")):
        assert np.array_equal(got.numpy(), T.fixture_params(g, 0)[name]), name


def test_fixture_matches_the_twin(golden):
    g = golden("golden_selfcf")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    steps = T.fixture_steps(g)
    assert [len(s["users"]) for s in steps] == [256, 256, 251] * 3
    # the recorded adjacency is the train CSR, in R order and in R^T order, with the twin's normalisation
    order, perm = T.transpose_order(rowptr, items)
    rows = T.csr_rows(rowptr)
    assert np.array_equal(g["adj_rows"], rows) and np.array_equal(g["adj_cols"], items) and len(items) == 763
    assert np.array_equal(g["adj_t_rows"], items[order]) and np.array_equal(g["adj_t_cols"], rows[order])
    assert np.array_equal(g["adj_t_val"], g["adj_val"][order])
    np.testing.assert_allclose(g["adj_val"], T.normalised_values(rowptr, items, ni), rtol=2e-7)
    assert rowptr[64] == rowptr[63] and not (items == 95).any()          # a zero-degree user and a zero-degree item
    # the masks: every rate in [0, 1), the kept share follows the rate, the two halves differ
    for s in steps:
        assert 0.0 <= s["rate"] < 1.0 and s["k1"].shape == s["k2"].shape == (763,)
        share = (s["k1"].sum() + s["k2"].sum()) / 1526.0
        assert abs(share - (1.0 - s["rate"])) < 0.06, (share, s["rate"])
        assert not np.array_equal(s["k1"][perm.argsort()], s["k2"])      # the masked matrix is not symmetric
        assert s["ku"].shape == s["ki"].shape == (len(s["users"]), 64) and 0.4 < s["ku"].mean() < 0.6 and 0.4 < s["ki"].mean() < 0.6
    test_users = g["test_users"]
    assert len(test_users) == 63 and 63 in test_users
    P, losses, scores = T.replay_f64((rowptr, items, ni), g["adj_val"], T.fixture_params(g, 0), steps, CONFIG, 3, test_users)
    dev_p, dev_s, dev_l = g["f64_dev_params"], g["f64_dev_scores"], float(g["f64_dev_loss"])
    print("loss dev", np.abs(losses / g["loss"].astype(np.float64) - 1).max(), "allowed", 10 * dev_l)
    np.testing.assert_allclose(losses, g["loss"], rtol=10 * dev_l)
    final = T.fixture_params(g, 1)
    for k, name in enumerate(T.PARAMS):
        print(name, "dev", np.abs(P[name] - final[name]).max(), "allowed", 10 * dev_p[k])
        assert np.abs(P[name] - final[name]).max() <= 10 * dev_p[k]
    assert len(scores) == 3 and g["pred"].shape == (3, 63, 96)
    for s, p, lim in zip(scores, g["pred"], dev_s):
        assert np.abs(s - p).max() <= 10 * lim
    # the fixture's own conditions, and what the GPU tests rely on
    assert (g["close_users"] <= 3).all()
    assert dev_s.max() < 1e-6 and dev_p.max() < 1e-5 and dev_l < 1e-6
    ndcg = [dict(zip(g["names"], r))["NDCG@10"] for r in g["reports"]]
    assert ndcg[0] < ndcg[1] < ndcg[2]


def test_keep_mirror_reproduces_the_masked_matrix_and_its_transpose():
    """the four arrays of skr_selfcf_keeps, applied to the CSR of R and of R^T, must give A-hat' (forward) and A-hat'^T
    (backward) exactly, for a mask whose two halves differ"""
    rng = np.random.default_rng(5)
    U, I = 48, 40
    lens = rng.integers(0, 12, U)
    lens[U - 1] = 0
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate([np.sort(rng.choice(I - 1, n, replace=False)) for n in lens]).astype(np.int32)
    nnz = len(items)
    rows = T.csr_rows(rowptr)
    order, perm = T.transpose_order(rowptr, items)
    val = rng.standard_normal(nnz)
    k1, k2 = (rng.random(nnz) < 0.6).astype(np.uint8), (rng.random(nnz) < 0.6).astype(np.uint8)
    # the square masked matrix, built entry by entry as the reference masks it: user rows then item rows, row-major
    N = U + I
    S = np.zeros((N, N))
    S[rows, U + items] = val * k1
    S[U + items[order], rows[order]] = val[order] * k2
    assert not np.array_equal(S, S.T)
    fu, fi, bu, bi = T.mirror_keeps(perm, k1, k2)

    def csr_dense(r, c, v, shape):
        A = np.zeros(shape)
        A[r, c] = v
        return A
    fwd_u = csr_dense(rows, items, val * fu, (U, I))                       # a run of A with fu
    fwd_i = csr_dense(items[order], rows[order], val[order] * fi, (I, U))  # a run of At with fi
    bwd_u = csr_dense(rows, items, val * bu, (U, I))
    bwd_i = csr_dense(items[order], rows[order], val[order] * bi, (I, U))
    assert np.array_equal(fwd_u, S[:U, U:]) and np.array_equal(fwd_i, S[U:, :U])
    assert np.array_equal(bwd_u, S.T[:U, U:]) and np.array_equal(bwd_i, S.T[U:, :U])
    # and the twin's blocks are the same matrix
    R1, R2t = T.masked_blocks(rowptr, items, I, val, k1, k2, 1.0)
    assert np.array_equal(R1, S[:U, U:]) and np.array_equal(R2t, S[U:, :U])


def test_folded_score_equals_the_reference_score():
    rng = np.random.default_rng(11)
    Mu, Mi = T.t64(rng.standard_normal((30, 20))), T.t64(rng.standard_normal((50, 20)))
    W, b = T.t64(rng.standard_normal((20, 20))), T.t64(rng.standard_normal(20))
    users = [0, 7, 7, 29]
    want, got = T.scores_f64(Mu, Mi, W, b, users).numpy(), T.folded_scores_f64(Mu, Mi, W, b, users).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
