"""CPU suite of SLMRec (skrec/recommender/SLMRec.py, csrc/slmrec.hip's argument checks, tests/slmrec_twin.py,
tests/golden/golden_slmrec.npz): the library's exports and argument checks, the limits by name, the draws and the adjacency
against the reference's recorded bits, the twin's hand-derived backward against torch autograd, the twin's replay of the fixture."""
import ctypes

import numpy as np
import pytest

import slmrec_twin as T


# ---------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entries():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 19
    for name in ("skr_slmrec_step", "skr_slmrec_step_timed", "skr_slmrec_workspace", "skr_slmrec_fuse", "skr_slmrec_project_bwd_w"):
        assert name in _hip.SIGNATURES and hasattr(L, name), name
    assert (_hip.SKR_SLMREC_MAX_BATCH, _hip.SKR_SLMREC_MAX_LAYERS, _hip.SKR_SLMREC_MAX_FEAT, _hip.SKR_SLMREC_GROUPS) == (2048, 4, 4096, 8)
    assert (_hip.SKR_SLMREC_GATE_FLOATS, _hip.SKR_SLMREC_FUSION_FLOATS) == (4160, 12352)
    assert L.skr_slmrec_workspace(0, 10, 4) == 0 and L.skr_slmrec_workspace(2049, 10, 4) == 0 and L.skr_slmrec_workspace(16, 10, 4100) == 0
    assert 0 < L.skr_slmrec_workspace(1, 10, 4) == L.skr_slmrec_workspace(16, 10, 4) < L.skr_slmrec_workspace(17, 10, 4)


def _args(**kw):
    """a skr_slmrec_step_args whose every pointer is a distinct non-NULL, 16-byte aligned address: the checks below fail before any
    of them is read"""
    from skrec import _hip
    a = _hip.SLMRecStepArgs()
    addr = iter(range(0x1000, 0x100000, 0x100))
    for name, ctype in a._fields_:
        if ctype is _hip.vp:
            setattr(a, name, next(addr))
        elif hasattr(ctype, "_length_") and ctype._type_ is _hip.vp:
            for k in range(ctype._length_):
                getattr(a, name)[k] = next(addr)
    a.n_users, a.n_items, a.dim, a.n_layers, a.n = 8, 8, 64, 2, 4
    a.feat_dim[0], a.feat_dim[1], a.feat_ld[0], a.feat_ld[1] = 5, 3, 8, 4
    a.temp, a.ssl_temp, a.ssl_alpha = 0.2, 0.1, 0.5
    a.work_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw, word", [(dict(plan_a=None), b"plan"), (dict(plan_at=None), b"plan"), (dict(n=2049), b"2048"),
                                      (dict(dim=65), b"dim"), (dict(dim=0), b"dim"), (dict(n_layers=5), b"n_layers"),
                                      (dict(work=0x1004), b"aligned"), (dict(loss=None), b"NULL"), (dict(ssl_temp=0.0), b"ssl_temp")])
def test_step_checks_its_arguments(kw, word):
    from skrec import _hip
    L = _hip.lib()
    rc = L.skr_slmrec_step(ctypes.byref(_args(**kw)), None)
    assert rc == -1 and word in L.skr_last_error(), L.skr_last_error()
    with pytest.raises(ValueError):
        _hip.check(rc)


def test_step_checks_the_arguments_of_an_empty_batch_and_launches_nothing():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_slmrec_step(ctypes.byref(_args(n=0)), None) == 0          # nothing is launched: no GPU is needed
    assert L.skr_slmrec_step(ctypes.byref(_args(n=0, plan_a=None)), None) == -1
    assert L.skr_slmrec_step(None, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_slmrec_step_timed(ctypes.byref(_args(n=0)), None, None) == -1
    a = _args(n=0)
    a.feat_ld[1] = 3
    assert L.skr_slmrec_step(ctypes.byref(a), None) == -1 and b"feat_ld" in L.skr_last_error()


def test_fuse_and_weight_backward_check_their_arguments():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_slmrec_fuse(None, None, None, None, 1, 64, None, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_slmrec_fuse(16, 32, 48, 64, 1, 65, 80, None) == -1 and b"dim" in L.skr_last_error()
    assert L.skr_slmrec_fuse(16, 32, 48, 64, 0, 64, 80, None) == -1
    assert L.skr_slmrec_fuse(16, 32, 48, 68, 1, 64, 80, None) == -1 and b"aligned" in L.skr_last_error()
    assert L.skr_slmrec_project_bwd_w(None, None, 1, 1, 4, None, None, 0, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_slmrec_project_bwd_w(16, 32, 1, 5, 4, 48, 64, 1 << 20, None) == -1 and b"feat_ld" in L.skr_last_error()
    assert L.skr_slmrec_project_bwd_w(16, 32, 1, 4, 4, 48, 64, 8, None) == -1 and b"work" in L.skr_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the config, the limits, the registry, the schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_param_space():
    from skrec.recommender.SLMRec import SLMRecConfig
    c = SLMRecConfig()
    assert (c.lr, c.reg, c.rec_dim, c.layer_num, c.ssl_alpha, c.ssl_temp, c.dropout_rate, c.temp, c.weight_decay) == \
        (1e-4, 1e-4, 64, 3, 0.01, 0.1, 0.3, 0.2, 1e-4)
    assert (c.mm_fusion_mode, c.adj_type, c.ssl_task, c.init, c.batch_size, c.epochs, c.early_stop) == ("concat", "pre", "FAC", "xavier", 2048, 1000, 200)
    assert SLMRecConfig.param_space() == {"lr": [0.0001, 0.001, 0.01, 0.1], "ssl_temp": [0.1, 0.2, 0.5, 1.0],
                                          "ssl_alpha": [0.01, 0.05, 0.1, 0.5, 1.0], "reg": [0.0001, 0.001, 0.01, 0.1]}
    for bad in (dict(lr=0.0), dict(rec_dim=0), dict(layer_num=-1), dict(ssl_temp=0.0), dict(temp=0.0), dict(batch_size=0)):
        with pytest.raises(AssertionError):
            SLMRecConfig(**bad)


@pytest.mark.parametrize("kw, word", [(dict(ssl_task="FD"), "ssl_task"), (dict(ssl_task="FM"), "a_dense_emb"), (dict(ssl_task="FD+FM"), "ssl_task"),
                                      (dict(mm_fusion_mode="mean"), "mm_fusion_mode"), (dict(init="normal"), "embedding_item_ID"),
                                      (dict(adj_type="norm"), "adj_type"), (dict(adj_type="plain"), "adj_type"), (dict(rec_dim=65), "rec_dim"),
                                      (dict(layer_num=5), "layer_num"), (dict(batch_size=2049), "batch_size")])
def test_limits_by_name(kw, word):
    from skrec.recommender.SLMRec import SLMRec, SLMRecConfig, check_limits
    with pytest.raises(NotImplementedError, match=word):
        check_limits(SLMRecConfig(**kw))
    with pytest.raises(NotImplementedError, match=word):
        SLMRec(None, dict(kw))
    with pytest.raises(NotImplementedError, match=word):
        SLMRec.detached(8, 8, dict(kw), img=np.zeros((8, 4), np.float32), txt=np.zeros((8, 4), np.float32))


def test_limits_of_the_data_the_features_and_the_ranks():
    from skrec.recommender.SLMRec import SLMRec, SLMRecConfig, check_limits
    check_limits(SLMRecConfig(rec_dim=37, layer_num=4, batch_size=2048), img_dim=4096, txt_dim=1, data_name="tiny")
    check_limits(SLMRecConfig(layer_num=0))
    with pytest.raises(NotImplementedError, match="kwai"):
        check_limits(SLMRecConfig(), data_name="kwai")
    with pytest.raises(NotImplementedError, match="feature width"):
        check_limits(SLMRecConfig(), txt_dim=4097)
    with pytest.raises(NotImplementedError, match="feature width"):
        SLMRec.detached(8, 8, {}, img=np.zeros((8, 4097), np.float32), txt=np.zeros((8, 4), np.float32))
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(SLMRecConfig(), world=2)


def test_a_missing_modality_is_a_value_error():
    from skrec.recommender.SLMRec import SLMRec
    for kw in (dict(), dict(img=np.zeros((8, 4), np.float32)), dict(txt=np.zeros((8, 4), np.float32))):
        with pytest.raises(ValueError, match="missing"):
            SLMRec.detached(8, 8, {}, **kw)


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.SLMRec import SLMRec, SLMRecConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("SLMRec")
    assert reg.get_model("SLMRec") == (SLMRec, SLMRecConfig)


def test_schedule_is_the_reference_expression():
    from skrec.recommender.SLMRec import SLMRecConfig, learning_rate
    for cfg in (SLMRecConfig(), SLMRecConfig(lr=1e-2)):
        for e in (0, 1, 49, 50, 333):
            assert learning_rate(cfg, e) == cfg.lr * 1.0 ** (e / 50) == cfg.lr == T.schedule_lr(dict(lr=cfg.lr), e)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's recorded bits
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_meets_its_conditions(golden):
    g = golden("golden_slmrec")
    assert int(g["seed"]) == T.SEED
    cfg = T.fixture_config(g)
    assert (cfg["lr"], cfg["ssl_alpha"], cfg["layer_num"], cfg["batch_size"], cfg["epochs"]) == (1e-2, 0.5, 2, 256, 3)
    assert (cfg["ssl_task"], cfg["mm_fusion_mode"], cfg["adj_type"], cfg["init"], cfg["rec_dim"]) == ("FAC", "concat", "pre", "xavier", 64)
    dev = dict(zip(T.NAMES, g["f64_dev_params"]))
    assert max(v for k, v in dev.items() if k not in T.NOISE_DRIVEN) <= 1e-5
    assert max(g["f64_dev_scores"].max(), float(g["f64_dev_loss"])) <= 1e-5
    assert g["close_users"].max() <= 3 and len(g["test_users"]) == 63
    assert list(g["step_sizes"]) == [256, 256, 251] * 3
    for name in T.UNTRAINED:          # g_a_iva after training equals g_a_iva before, bit for bit
        assert np.array_equal(g[T._key(name, 0)], g[T._key(name, 1)]) and np.abs(g[T._key(name, 0)]).max() > 0
    for e in range(3):                # predict() is the fp32 sigmoid of the raw scores
        import torch
        assert np.array_equal(g["pred"][e], torch.sigmoid(torch.from_numpy(g["raw"][e])).numpy())


def test_init_parameters_equal_the_reference(golden):
    """the draws of SLMRec.py:106-119, 434-486 under the golden's seed"""
    import random
    import torch
    from skrec.recommender.SLMRec import NAMES, UNTRAINED, init_parameters
    g = golden("golden_slmrec")
    assert NAMES == T.NAMES and UNTRAINED == T.UNTRAINED
    np.random.seed(T.SEED)
    random.seed(T.SEED)
    torch.manual_seed(T.SEED)
    P = init_parameters(64, 96, 64, 100, 37)
    want = T.fixture_params(g, 0)
    assert list(P) == list(want)
    for name, t in P.items():
        assert np.array_equal(t.numpy(), want[name]), name


def test_adjacency_values_equal_the_reference_bit_for_bit(golden):
    from skrec.recommender.SLMRec import adjacency_values, inverse_root_degrees
    g = golden("golden_slmrec")
    val = adjacency_values(g["adj_rowptr"], g["adj_cols"], int(g["shape"][1]))
    assert val.dtype == np.float32 and np.array_equal(val, g["adj_val"])
    assert np.array_equal(val, T.pre_adj_values(g["adj_rowptr"], g["adj_cols"], int(g["shape"][1])))
    assert inverse_root_degrees(np.array([0]))[0] == np.float32(1e-08) ** np.float32(-0.5)          # 1e4, not inf
    assert inverse_root_degrees(np.array([4]))[0] == np.float32(0.5)


def test_features_are_normalised_once_as_the_reference_does(golden):
    import torch
    g = golden("golden_slmrec")
    for raw, kept in (("img", "v_feat"), ("txt", "t_feat")):
        assert np.array_equal(torch.nn.functional.normalize(torch.from_numpy(g[raw]), dim=1).numpy(), g[kept])
        np.testing.assert_allclose(T.normalize_rows(g[raw].astype(np.float64)), g[kept], rtol=0, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, L", [(6, 2), (7, 0), (5, 1)])
def test_twin_backward_equals_autograd(d, L):
    """7 rows: a repeated user, a repeated item, a repeated pair and an id out of range; odd d gives d // 2 = 3 / 2 wide layers"""
    P, R, V, Tt, cfg, _, _ = T.random_case(seed=d, nu=6, ni=9, d=d, L=L)
    u, p = np.array([0, 1, 1, 4, 2, 1, 5]), np.array([1, 2, 2, 6, 0, 3, 9])
    comps, G, _ = T.gradients_f64(P, R, V, Tt, u, p, cfg)
    comps_t, G_t = T.gradients_torch(P, R, V, Tt, u, p, cfg)
    np.testing.assert_allclose(comps, comps_t, rtol=1e-12)
    assert all(c > 0 for c in comps)
    for name in T.TRAINED:
        scale = max(np.abs(G_t[name]).max(), 1.0)
        assert np.abs(G[name] - G_t[name]).max() <= 1e-12 * scale, name
        if name not in T.NOISE_DRIVEN:
            assert np.abs(G[name]).max() > 1e-6, name
    for name in T.NOISE_DRIVEN:       # zero in exact arithmetic: what is left is the rounding of sums of O(1) terms
        assert np.abs(G[name]).max() <= 1e-13 and np.abs(G_t[name]).max() <= 1e-13, name
    for name in T.UNTRAINED:
        assert not G[name].any()


def test_twin_replays_the_fixture(golden):
    g = golden("golden_slmrec")
    cfg = T.fixture_config(g)
    V, Tt = T.fixture_features(g)
    P, losses, scores = T.replay_f64(T.fixture_graph(g), V, Tt, T.fixture_params(g, 0), T.fixture_steps(g), cfg, 3, g["test_users"])
    final = T.fixture_params(g, 1)
    for k, name in enumerate(T.NAMES):
        diff = np.abs(P[name] - final[name]).max()
        assert diff <= g["f64_dev_params"][k] * (1 + 1e-9) + 1e-15, (name, diff, g["f64_dev_params"][k])
    for e, sc in enumerate(scores):
        assert np.abs(sc - g["raw"][e]).max() <= g["f64_dev_scores"][e] * (1 + 1e-9)
    assert np.abs(losses / g["loss"].astype(np.float64) - 1).max() <= float(g["f64_dev_loss"]) * (1 + 1e-9)


def test_twin_switches_change_the_run(golden):
    g = golden("golden_slmrec")
    cfg, init, steps = T.fixture_config(g), T.fixture_params(g, 0), T.fixture_steps(g)[:4]
    V, Tt = T.fixture_features(g)
    R = T.fixture_graph(g)
    held = [k for k in T.NAMES if k not in T.NOISE_DRIVEN]
    bound = 100 * max(d for k, d in zip(T.NAMES, g["f64_dev_params"]) if k in held)
    base, _, _ = T.replay_f64(R, V, Tt, init, steps, cfg, 3, g["test_users"])
    for kw in (dict(use_main=False), dict(use_v=False), dict(use_t=False)):
        other, _, _ = T.replay_f64(R, V, Tt, init, steps, cfg, 3, g["test_users"], **kw)
        assert max(np.abs(other[k] - base[k]).max() for k in held) > bound, kw
