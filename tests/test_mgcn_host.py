"""CPU suite of MGCN (skrec/recommender/MGCN.py, skrec/utils/item_graph.py's weighted builder, tests/mgcn_twin.py,
tests/golden/golden_mgcn.npz): the twin's replay of the fixture, the twin's hand-derived backward against central differences,
the graph builder against the reference's recorded values, the config and the limits, the registry, the schedule."""
import numpy as np
import pytest

import mgcn_twin as T


# ---------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replay(golden):
    g = golden("golden_mgcn")
    R, S = T.fixture_graphs(g)
    cfg = T.fixture_config(g)
    return g, cfg, T.replay_f64(R, S, T.fixture_params(g, 0), T.fixture_steps(g), cfg, 3, g["test_users"])


def test_fixture_meets_its_conditions(golden):
    g = golden("golden_mgcn")
    assert int(g["seed"]) == T.SEED
    cfg = T.fixture_config(g)
    assert cfg == dict(lr=1e-2, reg=1e-2, cl_loss=0.1, n_ui_layers=2, n_layers=2, knn_k=10, lr_scheduler=[0.5, 1], batch_size=256, epochs=3)
    assert max(g["f64_dev_params"].max(), g["f64_dev_scores"].max(), float(g["f64_dev_loss"]), g["f64_dev_graph"].max()) <= 1e-5
    assert g["close_users"].max() <= 3 and len(g["test_users"]) == 63
    for m in ("image", "text"):
        assert (g[m + "_knn_sims"].sum(1) > 0).all()
    assert list(g["step_sizes"]) == [256, 256, 251] * 3
    assert g["loss"][0] > g["loss"][-1]


def test_twin_replays_the_fixture(replay):
    g, cfg, (P, losses, scores) = replay
    final = T.fixture_params(g, 1)
    for k, name in enumerate(T.NAMES):
        diff = np.abs(P[name] - final[name]).max()
        assert diff <= g["f64_dev_params"][k] * (1 + 1e-9) + 1e-15, (name, diff, g["f64_dev_params"][k])
    for e, sc in enumerate(scores):
        assert np.abs(sc - g["pred"][e]).max() <= g["f64_dev_scores"][e] * (1 + 1e-9)
    assert np.abs(losses / g["loss"].astype(np.float64) - 1).max() <= float(g["f64_dev_loss"]) * (1 + 1e-9)


def test_twin_graphs_equal_the_recorded_ones(golden):
    g = golden("golden_mgcn")
    dev = g["f64_dev_graph"]
    val = T.norm_adj_values(g["adj_rowptr"], g["adj_cols"], int(g["shape"][1]))
    assert np.abs(val - g["adj_val"]).max() <= dev[0] * (1 + 1e-9)
    for k, (m, key) in enumerate((("image", "image_embedding_weight_0"), ("text", "text_embedding_weight_0"))):
        ids, sims = T.knn_f64(g[key], 10)
        assert np.array_equal(np.sort(ids, 1), np.sort(g[m + "_knn_ids"], 1))
        want = T.dense_graph(g[m + "_knn_ids"], g[m + "_graph_val"])
        assert np.abs(T.dense_graph(ids, T.weighted_graph_values(ids, sims)) - want).max() <= dev[1 + k] * (1 + 1e-9)


def test_twin_backward_equals_central_differences():
    """every parameter group, on 5 users x 7 items, a batch with a repeated user, pos == neg in one row and an id out of range"""
    P, R, S, cfg = T.tiny_case()
    u, p, q = np.array([0, 1, 1, 4, 2, 1]), np.array([1, 2, 2, 6, 0, 3]), np.array([3, 2, 5, 0, 4, 9])
    comps, G = T.gradients_f64(P, R, S, u, p, q, cfg)
    assert all(c > 0 for c in comps)
    h, rng = 1e-6, np.random.default_rng(1)
    for name in T.NAMES:
        flat, grad = P[name].reshape(-1), G[name].reshape(-1)
        assert np.abs(grad).max() > 0, name
        for e in rng.choice(flat.size, min(flat.size, 10), replace=False):
            old = flat[e]
            flat[e] = old + h
            lp = sum(T.losses_f64(P, R, S, u, p, q, cfg))
            flat[e] = old - h
            lm = sum(T.losses_f64(P, R, S, u, p, q, cfg))
            flat[e] = old
            # central differences of a smooth function of O(1) curvature: h^2 truncation, 1e-16 / h rounding
            assert abs((lp - lm) / (2 * h) - grad[e]) <= 1e-8 + 1e-6 * abs(grad[e]), (name, e)


def test_twin_switches_change_the_run(golden):
    g = golden("golden_mgcn")
    R, S = T.fixture_graphs(g)
    cfg, init, steps = T.fixture_config(g), T.fixture_params(g, 0), T.fixture_steps(g)[:4]
    base, _, _ = T.replay_f64(R, S, init, steps, cfg, 3, g["test_users"])
    for kw in (dict(use_cl=False), dict(use_reg=False), dict(use_schedule=False)):
        other, _, _ = T.replay_f64(R, S, init, steps, cfg, 3, g["test_users"], **kw)
        assert max(np.abs(other[k] - base[k]).max() for k in T.NAMES) > 100 * g["f64_dev_params"].max(), kw


# ---------------------------------------------------------------------------------------------------------------------
# the graph builder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modality", ["image", "text"])
def test_weighted_item_graph_equals_the_reference_bit_for_bit(golden, modality):
    import torch
    from skrec.utils.item_graph import build_weighted_item_graph
    g = golden("golden_mgcn")
    ids, sims, want = g[modality + "_knn_ids"], g[modality + "_knn_sims"], g[modality + "_graph_val"]
    ni, k = ids.shape
    (rp, col, val), (rpt, colt, valt) = build_weighted_item_graph(torch.from_numpy(ids), torch.from_numpy(sims))
    assert rp.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert np.array_equal(rp.numpy(), np.arange(ni + 1) * k)
    order = np.argsort(ids, axis=1, kind="stable")
    assert np.array_equal(col.numpy().reshape(ni, k), np.take_along_axis(ids, order, 1))
    assert np.array_equal(val.numpy().reshape(ni, k), np.take_along_axis(want, order, 1))          # the reference's bits
    # the transpose holds the same entries
    S = np.zeros((ni, ni), np.float32)
    S[np.repeat(np.arange(ni), k), col.numpy()] = val.numpy()
    St = np.zeros((ni, ni), np.float32)
    rows_t = np.repeat(np.arange(ni), np.diff(rpt.numpy()))
    St[rows_t, colt.numpy()] = valt.numpy()
    assert int(rpt[-1]) == ni * k and np.array_equal(St, S.T)
    for r in range(ni):
        assert (np.diff(colt.numpy()[rpt[r]:rpt[r + 1]]) > 0).all()
    assert not np.array_equal(S, S.T)                                                            # directed


def test_weighted_item_graph_rejects_bad_ids_and_zero_rows():
    import torch
    from skrec.utils.item_graph import build_weighted_item_graph
    with pytest.raises(ValueError):
        build_weighted_item_graph(torch.tensor([[0, 2], [1, 0]]), torch.ones(2, 2))
    # a row whose kept similarities sum to zero: its inverse root is inf -> 0, as in the reference
    (_, _, val), _ = build_weighted_item_graph(torch.tensor([[0, 1], [1, 0]]), torch.tensor([[1.0, 0.5], [0.0, 0.0]]))
    d0 = torch.tensor(1.5).pow(-0.5)
    assert torch.equal(val, torch.stack([d0 * 1.0 * d0, torch.tensor(0.0), torch.tensor(0.0), torch.tensor(0.0)]))
    assert abs(float(val[0]) - 1.0 / 1.5) < 1e-7


# ---------------------------------------------------------------------------------------------------------------------
# the config, the limits, the registry, the schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    from skrec.recommender.MGCN import MGCNConfig
    c = MGCNConfig()
    assert (c.lr, c.reg, c.embed_dim, c.n_ui_layers, c.n_layers, c.lambda_coeff, c.knn_k, c.cl_loss) == (1e-3, 1e-4, 64, 2, 1, 0.9, 10, 0.001)
    assert (list(c.lr_scheduler), c.batch_size, c.epochs, c.early_stop) == ([0.96, 50], 2048, 1000, 200)
    assert MGCNConfig.param_space() == {"cl_loss": [0.001, 0.01, 0.1]}
    assert MGCNConfig(lambda_coeff=0.5).lambda_coeff == 0.5         # accepted and unused
    for bad in (dict(lr=0.0), dict(reg=-1.0), dict(embed_dim=0), dict(n_layers=-1), dict(knn_k=0), dict(cl_loss=-0.1),
                dict(lr_scheduler=[0.5]), dict(batch_size=0)):
        with pytest.raises(AssertionError):
            MGCNConfig(**bad)


@pytest.mark.parametrize("kw, word", [(dict(embed_dim=65), "embed_dim"), (dict(n_ui_layers=5), "n_ui_layers"), (dict(n_layers=5), "n_layers"),
                                      (dict(batch_size=2049), "batch_size"), (dict(knn_k=33), "knn_k")])
def test_limits_by_name(kw, word):
    from skrec.recommender.MGCN import MGCN, MGCNConfig, check_limits
    with pytest.raises(NotImplementedError, match=word):
        check_limits(MGCNConfig(**kw))
    with pytest.raises(NotImplementedError, match=word):
        MGCN(None, dict(kw))
    with pytest.raises(NotImplementedError, match=word):
        MGCN.detached(8, 8, dict(kw), img=np.zeros((8, 4), np.float32), txt=np.zeros((8, 4), np.float32))


def test_limits_of_the_features_and_the_ranks():
    from skrec.recommender.MGCN import MGCN, MGCNConfig, check_limits
    check_limits(MGCNConfig(embed_dim=20, n_ui_layers=4, n_layers=4, batch_size=2048, knn_k=32), img_dim=4096, txt_dim=1)
    check_limits(MGCNConfig(n_ui_layers=0, n_layers=0))
    with pytest.raises(NotImplementedError, match="feature width"):
        check_limits(MGCNConfig(), img_dim=4097)
    with pytest.raises(NotImplementedError, match="feature width"):
        MGCN.detached(8, 8, {}, img=np.zeros((8, 4), np.float32), txt=np.zeros((8, 4097), np.float32))
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(MGCNConfig(), world=2)


def test_a_missing_modality_is_a_value_error():
    from skrec.recommender.MGCN import MGCN
    for kw in (dict(), dict(img=np.zeros((8, 4), np.float32)), dict(txt=np.zeros((8, 4), np.float32))):
        with pytest.raises(ValueError, match="missing"):
            MGCN.detached(8, 8, {}, **kw)


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.MGCN import MGCN, MGCNConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("MGCN")
    assert reg.get_model("MGCN") == (MGCN, MGCNConfig)


def test_schedule_is_the_reference_expression():
    from skrec.recommender.MGCN import MGCNConfig, learning_rate
    for cfg in (MGCNConfig(), MGCNConfig(lr=1e-2, lr_scheduler=[0.5, 1]), MGCNConfig(lr=3e-3, lr_scheduler=[0.9, 7])):
        g, s = cfg.lr_scheduler
        for e in (0, 1, 2, 49, 50, 333):
            assert learning_rate(cfg, e) == cfg.lr * g ** (e / s)
            assert learning_rate(cfg, e) == T.schedule_lr(dict(lr=cfg.lr, lr_scheduler=cfg.lr_scheduler), e)
    assert learning_rate(MGCNConfig(lr=1e-2, lr_scheduler=[0.5, 1]), 2) == 2.5e-3


def test_init_parameters_equal_the_reference(golden):
    """the draws of MGCN.py:138-206 under the golden's seed"""
    import random
    import torch
    from skrec.recommender.MGCN import NAMES, init_parameters
    g = golden("golden_mgcn")
    assert NAMES == T.NAMES
    np.random.seed(T.SEED)
    random.seed(T.SEED)
    torch.manual_seed(T.SEED)
    P = init_parameters(64, 96, 64, 100, 37)
    want = T.fixture_params(g, 0)
    for name, t in P.items():
        assert np.array_equal(t.numpy(), want[name]), name


def test_library_exports_and_checks_without_a_gpu():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 17
    assert (_hip.SKR_MGCN_MAX_BATCH, _hip.SKR_MGCN_MAX_LAYERS, _hip.SKR_MGCN_MAX_FEAT, _hip.SKR_MGCN_GROUPS) == (2048, 4, 4096, 8)
    assert L.skr_mgcn_workspace(0, 10, 4) == 0 and L.skr_mgcn_workspace(2049, 10, 4) == 0 and L.skr_mgcn_workspace(16, 10, 4100) == 0
    assert L.skr_mgcn_workspace(16, 10, 4) > 0
    assert [L.skr_mgcn_row_block(n) for n in (1, 256, 16384, 16385, 100000)] == [256, 256, 256, 272, 1568]
    assert L.skr_mgcn_step(None, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_mgcn_project(None, 1, 1, 4, None, None, None) == -1
    assert L.skr_mgcn_fuse(None, None, None, None, None, None, 1, 64, None, None, None) == -1
