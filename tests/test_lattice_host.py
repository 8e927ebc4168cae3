"""CPU suite of LATTICE (skrec/recommender/LATTICE.py, tests/lattice_twin.py, tests/golden/golden_lattice.npz): the twin's
replay of the fixture, the twin's hand-derived backward against central differences, the union-pattern builder against a dense
restatement, the config and the limits, the registry, the schedule, the library's argument checks."""
import numpy as np
import pytest

import lattice_twin as T


# ---------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replay(golden):
    g = golden("golden_lattice")
    cfg, tcfg = T.fixture_config(g)
    args = (T.fixture_adjacency(g), T.fixture_frozen(g), T.fixture_params(g, 0), T.fixture_steps(g), tcfg, 3, g["test_users"])
    return g, tcfg, args, T.replay_f64(*args, knn_builds=T.fixture_knn(g, cfg["knn_k"]))


def test_fixture_meets_its_conditions(golden):
    g = golden("golden_lattice")
    assert int(g["seed"]) == T.SEED
    cfg, tcfg = T.fixture_config(g)
    assert cfg == dict(lr=1e-2, reg=1e-2, lambda_coeff=0.5, n_layers=2, knn_k=10, lr_scheduler=[0.5, 1], batch_size=256, epochs=3)
    assert tcfg["n_ui_layers"] == 2 and tcfg["cf_model"] == "lightgcn"
    assert max(g["f64_dev_params"].max(), g["f64_dev_scores"].max(), float(g["f64_dev_loss"])) <= 1e-5
    assert g["close_users"].max() <= 3 and len(g["test_users"]) == 63
    k = cfg["knn_k"]
    assert g["knn_ids"].shape == (6, 2, 96, k + 1)
    sims = g["knn_sims"]
    assert (sims[..., k - 1] - sims[..., k]).min() > 1e-5 and float(g["min_gap"]) > 1e-5        # another exact kNN returns these sets
    assert (sims[..., :k].sum(-1) > 0).all()
    for m in ("image", "text"):
        assert (g[m + "_frozen_sims"].sum(1) > 0).all()
    assert list(g["step_sizes"]) == [256, 256, 251] * 3
    assert list(g["adam_steps"]) == [3, 9, 9, 3, 3, 3, 3, 3, 3]            # torch's Adam skips a tensor without a gradient
    assert g["loss"][0] > g["loss"][-1]


def test_twin_replays_the_fixture(replay):
    g, tcfg, _, (P, losses, scores, ts) = replay
    final = T.fixture_params(g, 1)
    for k, name in enumerate(T.NAMES):
        diff = np.abs(P[name] - final[name]).max()
        assert diff <= g["f64_dev_params"][k] * (1 + 1e-9) + 1e-15, (name, diff, g["f64_dev_params"][k])
    for e, sc in enumerate(scores):
        assert np.abs(sc - g["pred"][e]).max() <= g["f64_dev_scores"][e] * (1 + 1e-9)
    assert np.abs(losses / g["loss"].astype(np.float64) - 1).max() <= float(g["f64_dev_loss"]) * (1 + 1e-9)
    assert ts == (9, 3)


def test_twin_finds_the_recorded_neighbour_sets(golden):
    """the float64 kNN of the twin's own projected rows at the first build returns the reference's sets, and its frozen
    graphs the reference's values"""
    g = golden("golden_lattice")
    P = {k: v.astype(np.float64) for k, v in T.fixture_params(g, 0).items()}
    for m, F in enumerate(T.project(P)):
        ids, sims = T.knn_f64(F, 10)
        assert np.array_equal(np.sort(ids, 1), np.sort(g["knn_ids"][0][m][:, :10], 1))
        assert np.abs(sims - g["knn_sims"][0][m][:, :10]).max() <= 1e-6
    for m, (name, tab) in enumerate((("image", "image_embedding.weight"), ("text", "text_embedding.weight"))):
        ids, vals = T.frozen_lists(P[tab], 10)
        want_ids, want_vals = T.fixture_frozen(g)[m]
        assert np.array_equal(ids, want_ids) and np.abs(vals - want_vals).max() <= 1e-6
    rp, items = g["adj_rowptr"], g["adj_cols"]
    assert np.abs(T.norm_adj_dense(rp, items, 96) - T.fixture_adjacency(g)).max() <= 1e-7
    A = T.fixture_adjacency(g)
    assert np.allclose(A.sum(1), 1.0, atol=1e-6) and (np.diag(A) > 0).all() and not np.allclose(A, A.T)     # D^-1 (A + I)


@pytest.mark.parametrize("kw", [dict(), dict(cf_model="mf", n_layers=1), dict(n_layers=1), dict(n_layers=0), dict(n_layers=3, n_ui_layers=1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default")
def test_twin_backward_equals_central_differences(kw):
    """every parameter group, on 5 users x 9 items, a batch with a repeated user, pos == neg in one row and an id out of
    range; the neighbour sets are those of the point, where every k-th / (k+1)-th pair is 2e-5 or more apart: a step of
    h = 1e-6 in one parameter of O(1) rows moves a cosine by a few 1e-6 at most, so no set changes between the two evaluations"""
    P, A, frozen, cfg = T.tiny_case(**kw)
    u, p, q = np.array([0, 1, 1, 4, 2, 1]), np.array([1, 2, 2, 6, 0, 3]), np.array([3, 2, 5, 0, 4, 9])
    knn = []
    for F in T.project(P):
        ids, _ = T.knn_f64(F, cfg["knn_k"] + 1)
        sims = T.cosine_at(F, ids)
        assert (sims[:, -2] - sims[:, -1]).min() > 2e-5
        knn.append(ids[:, :-1])
    comps, G, _, _ = T.gradients_f64(P, A, frozen, u, p, q, cfg, knn=knn)
    assert all(c > 0 for c in comps)
    h, rng = 1e-6, np.random.default_rng(1)
    for name in T.NAMES:
        flat, grad = P[name].reshape(-1), G[name].reshape(-1)
        if name in T.ROWS or cfg["n_layers"] > 0:
            assert np.abs(grad).max() > 0, name
        else:
            assert np.abs(grad).max() == 0, name          # without a layer the graph is unused
        for e in rng.choice(flat.size, min(flat.size, 10), replace=False):
            old = flat[e]
            flat[e] = old + h
            lp = sum(T.losses_f64(P, A, frozen, u, p, q, cfg, knn=knn))
            flat[e] = old - h
            lm = sum(T.losses_f64(P, A, frozen, u, p, q, cfg, knn=knn))
            flat[e] = old
            # central differences of a smooth function of O(1) curvature: h^2 truncation, 1e-16 / h rounding
            assert abs((lp - lm) / (2 * h) - grad[e]) <= 1e-8 + 1e-6 * abs(grad[e]), (name, e)


def test_an_ordinary_step_leaves_the_modal_tensors_alone():
    P, A, frozen, cfg = T.tiny_case()
    u, p, q = np.array([0, 1, 3]), np.array([1, 2, 8]), np.array([3, 5, 0])
    G0 = T.build_graph(P, frozen, cfg)
    _, Gb, _, _ = T.gradients_f64(P, A, frozen, u, p, q, cfg, build=True)
    _, Go, _, _ = T.gradients_f64(P, A, frozen, u, p, q, cfg, build=False, G=G0)
    for name in T.NAMES:
        if name in T.ROWS:
            assert np.array_equal(Gb[name], Go[name]), name       # the same graph, the same rows' gradient
        else:
            assert np.abs(Gb[name]).max() > 0 and np.abs(Go[name]).max() == 0, name


def test_twin_switches_change_the_run(replay):
    g, tcfg, args, (base, _, _, _) = replay
    knn = T.fixture_knn(g, tcfg["knn_k"])
    for kw in (dict(use_learned=False), dict(use_reg=False), dict(use_schedule=False), dict(skip_modal_on_ordinary_steps=False)):
        other = T.replay_f64(*args, knn_builds=knn, **kw)[0]
        assert max(np.abs(other[k] - base[k]).max() for k in T.NAMES) > 100 * g["f64_dev_params"].max(), kw
    assert T.replay_f64(*args, knn_builds=knn, skip_modal_on_ordinary_steps=False)[3] == (9, 9)


# ---------------------------------------------------------------------------------------------------------------------
# the union-pattern builder
# ---------------------------------------------------------------------------------------------------------------------
def _dense_restatement(lists, w, lam, I):
    """LATTICE.py:212-228 on dense matrices: scatter every list, mix, normalise, mix again"""
    mats = []
    for l in lists:
        Mx = np.zeros((I, I))
        if l is not None:
            for i in range(I):
                for p in range(l[0].shape[1] - 1, -1, -1):          # of a repeated id the first counts
                    if 0 <= l[0][i, p] < I:
                        Mx[i, l[0][i, p]] = l[1][i, p]
        mats.append(Mx)
    learned = w[0] * mats[0] + w[1] * mats[1]
    r = learned.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(r > 0, np.power(np.where(r > 0, r, 1.0), -0.5), 0.0)
    return (1 - lam) * q[:, None] * learned * q[None, :] + lam * (w[0] * mats[2] + w[1] * mats[3])


@pytest.mark.parametrize("absent", [(), (1, 3), (0, 2)])
def test_union_graph_equals_the_dense_restatement(absent):
    rng = np.random.default_rng(len(absent))
    I, k = 23, 4
    lists = []
    for t in range(4):
        ids = np.stack([rng.permutation(I)[:k] for _ in range(I)])
        lists.append(None if t in absent else (ids, rng.random((I, k)) + 0.1))
    if not absent:
        lists[1][0][3, 2] = lists[1][0][3, 0]        # a repeated id inside a list
        lists[0][0][5, 1] = -1                       # ids out of range
        lists[2][0][5, 0] = I
        lists[0][1][7], lists[1][1][7] = 0.0, 0.0    # r_7 = 0
    w = np.array([0.3, 0.7]) if not absent else np.array([0.0 if 0 in absent else 1.0, 0.0 if 1 in absent else 1.0])
    G = T.union_graph(lists, w, 0.4)
    want = _dense_restatement(lists, w, 0.4, I)
    assert np.abs(T.dense_S(G) - want).max() <= 1e-15
    assert set(zip(*np.nonzero(want))) <= set(zip(G["rows"], G["col"]))
    for r in range(I):
        cols = G["col"][G["rowptr"][r]:G["rowptr"][r + 1]]
        assert (np.diff(cols) > 0).all() and len(cols) <= 4 * k          # ascending, merged
    for t in range(4):                                                    # the slots name the entry's place in every list
        if lists[t] is None:
            assert (G["slots"][:, t] == -1).all()
            continue
        m = G["slots"][:, t] >= 0
        assert np.array_equal(lists[t][0][G["rows"][m], G["slots"][m, t]], G["col"][m])
    if not absent:
        assert G["r"][7] == 0 and G["q"][7] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the config, the limits, the registry, the schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    from skrec.recommender.LATTICE import LATTICEConfig
    c = LATTICEConfig()
    assert (c.lr, c.reg, c.embed_dim, c.feat_embed_dim, c.weight_size, c.lambda_coeff, c.mess_dropout) == (1e-4, 0.0, 64, 64, [64, 64], 0.9, [0.1, 0.1])
    assert (c.n_layers, c.knn_k, c.cf_model, list(c.lr_scheduler), c.batch_size, c.epochs, c.early_stop) == (1, 10, "lightgcn", [0.96, 50], 2048, 1000, 200)
    assert LATTICEConfig.param_space() == {"lr": [0.0001, 0.0005, 0.001, 0.005], "reg": [0.0, 1e-05, 1e-04, 1e-03]}
    for bad in (dict(lr=0.0), dict(reg=-1.0), dict(embed_dim=0), dict(feat_embed_dim=0), dict(n_layers=-1), dict(knn_k=0), dict(cf_model="gcn"),
                dict(lr_scheduler=[0.5]), dict(batch_size=0), dict(lambda_coeff=1.5)):
        with pytest.raises(AssertionError):
            LATTICEConfig(**bad)


@pytest.mark.parametrize("kw, word", [(dict(embed_dim=65), "embed_dim"), (dict(feat_embed_dim=65), "feat_embed_dim"),
                                      (dict(weight_size=[64] * 5), "weight_size"), (dict(n_layers=5), "n_layers"),
                                      (dict(batch_size=2049), "batch_size"), (dict(knn_k=33), "knn_k"), (dict(cf_model="ngcf"), "cf_model")])
def test_limits_by_name(kw, word):
    from skrec.recommender.LATTICE import LATTICE, LATTICEConfig, check_limits
    with pytest.raises(NotImplementedError, match=word):
        check_limits(LATTICEConfig(**kw))
    with pytest.raises(NotImplementedError, match=word):
        LATTICE(None, dict(kw))
    with pytest.raises(NotImplementedError, match=word):
        LATTICE.detached(8, 8, dict(kw), img=np.zeros((8, 4), np.float32), txt=np.zeros((8, 4), np.float32))


def test_limits_of_the_features_and_the_ranks():
    from skrec.recommender.LATTICE import LATTICE, LATTICEConfig, check_limits
    check_limits(LATTICEConfig(embed_dim=20, feat_embed_dim=1, weight_size=[1] * 4, n_layers=4, batch_size=2048, knn_k=32), img_dim=4096, txt_dim=1)
    check_limits(LATTICEConfig(weight_size=[], n_layers=0, cf_model="mf"))
    with pytest.raises(NotImplementedError, match="feature width"):
        check_limits(LATTICEConfig(), img_dim=4097)
    with pytest.raises(NotImplementedError, match="feature width"):
        LATTICE.detached(8, 8, {}, txt=np.zeros((8, 4097), np.float32))
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(LATTICEConfig(), world=2)
    with pytest.raises(ValueError, match="no modality"):
        LATTICE.detached(8, 8, {})


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.LATTICE import LATTICE, LATTICEConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("LATTICE")
    assert reg.get_model("LATTICE") == (LATTICE, LATTICEConfig)


def test_schedule_is_the_reference_expression():
    from skrec.recommender.LATTICE import LATTICEConfig, learning_rate
    for cfg in (LATTICEConfig(), LATTICEConfig(lr=1e-2, lr_scheduler=[0.5, 1]), LATTICEConfig(lr=3e-3, lr_scheduler=[0.9, 7])):
        g, s = cfg.lr_scheduler
        for e in (0, 1, 2, 49, 50, 333):
            assert learning_rate(cfg, e) == cfg.lr * g ** (e / s)
            assert learning_rate(cfg, e) == T.schedule_lr(dict(lr=cfg.lr, lr_scheduler=cfg.lr_scheduler), e)
    assert learning_rate(LATTICEConfig(lr=1e-2, lr_scheduler=[0.5, 1]), 2) == 2.5e-3


def test_init_parameters_equal_the_reference(golden):
    """the draws of LATTICE.py:116-165 under the golden's seed"""
    import random
    import torch
    from skrec.recommender.LATTICE import NAMES, init_parameters
    g = golden("golden_lattice")
    assert NAMES == T.NAMES
    np.random.seed(T.SEED)
    random.seed(T.SEED)
    torch.manual_seed(T.SEED)
    P = init_parameters(64, 96, 64, 64, 100, 37)
    want = T.fixture_params(g, 0)
    for name, t in P.items():
        assert np.array_equal(t.numpy(), want[name]), name
    assert set(P) == set(T.NAMES) - {"image_embedding.weight", "text_embedding.weight"}


def test_library_exports_and_checks_without_a_gpu():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 18
    assert (_hip.SKR_LATTICE_MAX_BATCH, _hip.SKR_LATTICE_MAX_LAYERS, _hip.SKR_LATTICE_GROUPS) == (2048, 4, 7)
    assert L.skr_lattice_workspace(0, 10) == 0 and L.skr_lattice_workspace(2049, 10) == 0 and L.skr_lattice_workspace(16, 0) == 0
    assert L.skr_lattice_workspace(16, 10) > 0 and L.skr_lattice_graph_workspace(10) >= 40 and L.skr_lattice_graph_workspace(0) == 0
    assert L.skr_lattice_graph_bwd_workspace(10, 40) > 0 and L.skr_lattice_graph_bwd_workspace(0, 40) == 0
    assert L.skr_lattice_step(None, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_lattice_graph(10, 2, None, None, None, 0.5, None, None, None, None, None, None, None, 0, None) == -1
    assert L.skr_lattice_sddmm(10, 10, None, None, None, 0, None, 0, 1, None, 0, None, None) == -1
    assert L.skr_lattice_add_normalized(None, 1, None, None) == -1
    import ctypes
    a = _hip.LatticeStepArgs()
    assert L.skr_lattice_step_timed(ctypes.byref(a), None, None) == -1
