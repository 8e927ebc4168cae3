"""CPU suite of FREEDOM (skrec/recommender/FREEDOM.py, csrc/freedom.hip's argument checks, tests/golden/golden_freedom.npz):
the config and the limits, the registry, the library's exports and checks without a GPU, the initialisation against the
fixture, the fixture against the float64 twin (tests/freedom_twin.py), the sampler's law."""
import ctypes

import numpy as np
import pytest

import freedom_twin as T

SEED = T.SEED
CONFIG = dict(lr=1e-2, reg=0.5, n_mm_layers=2, n_ui_layers=2, dropout=0.8, batch_size=256, epochs=3)


# ---------------------------------------------------------------------------------------------------------------------
# the config, the limits, the registry
# ---------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    from skrec.recommender.FREEDOM import FREEDOMConfig
    c = FREEDOMConfig()
    assert dict(c.items()) == dict(lr=1e-3, reg=0.0, embed_dim=64, feat_dim=64, lambda_coeff=0.9, n_mm_layers=1, n_ui_layers=2, knn_k=10,
                                   mm_image_weight=0.1, dropout=0.8, batch_size=2048, epochs=1000, early_stop=200, draws="device")
    assert FREEDOMConfig.param_space() == {"reg": [0.0, 1e-05, 1e-04, 1e-03], "dropout": [0.8, 0.9]}
    assert FREEDOMConfig(lambda_coeff=0.5).lambda_coeff == 0.5         # accepted and unused
    assert FREEDOMConfig(dropout=0.0).dropout == 0.0                   # no pruning: the unpruned pair trains
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(reg=-0.1), dict(embed_dim=0), dict(n_ui_layers=-1), dict(n_mm_layers=2.0), dict(dropout=1.0),
                dict(knn_k=0), dict(mm_image_weight=1.5), dict(batch_size=0), dict(epochs=-1), dict(draws="reference")):
        with pytest.raises(AssertionError):
            FREEDOMConfig(**bad)


LIMITS = [(dict(embed_dim=65, feat_dim=65), "embed_dim <= 64"), (dict(n_ui_layers=5), "n_ui_layers <= 4"), (dict(n_mm_layers=5), "n_mm_layers <= 4"),
          (dict(batch_size=2049), "batch_size <= 2048"), (dict(knn_k=33), "knn_k <= 32")]


def test_limits_are_named():
    from skrec.recommender.FREEDOM import FREEDOM, FREEDOMConfig, check_limits
    check_limits(FREEDOMConfig(embed_dim=20, feat_dim=20, n_ui_layers=4, n_mm_layers=4, batch_size=2048, knn_k=32), img_dim=4096, txt_dim=1)
    check_limits(FREEDOMConfig(n_ui_layers=0, n_mm_layers=0))
    for kw, msg in LIMITS:
        with pytest.raises(NotImplementedError, match=msg):
            check_limits(FREEDOMConfig(**kw))
        with pytest.raises(NotImplementedError, match=msg):           # before the data set: there is none to read
            FREEDOM(None, dict(kw))
        with pytest.raises(NotImplementedError, match=msg):
            FREEDOM.detached(8, 8, dict(kw))
    with pytest.raises(NotImplementedError, match="feature width <= 4096.*image.*4097"):
        check_limits(FREEDOMConfig(), img_dim=4097)
    with pytest.raises(NotImplementedError, match="feature width <= 4096.*text.*4097"):
        check_limits(FREEDOMConfig(), txt_dim=4097)
    with pytest.raises(NotImplementedError, match="feature width <= 4096.*text.*4097"):
        FREEDOM.detached(8, 8, {}, txt=np.zeros((8, 4097), np.float32))
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(FREEDOMConfig(), world=2)


def test_detached_refuses_missing_modalities_and_unequal_widths(monkeypatch):
    from skrec import _hip
    from skrec.recommender.FREEDOM import FREEDOM

    def no_gpu():
        raise AssertionError("the GPU is asked for before the data is checked")
    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    with pytest.raises(ValueError, match="no modality"):
        FREEDOM.detached(8, 8, {})
    with pytest.raises(ValueError, match="feat_dim = 32 must equal embed_dim = 64"):
        FREEDOM.detached(8, 8, dict(feat_dim=32), img=np.zeros((8, 5), np.float32))
    with pytest.raises(ValueError, match="feat_dim = 32 must equal embed_dim = 64"):       # at any reg
        FREEDOM.detached(8, 8, dict(feat_dim=32, reg=0.0), txt=np.zeros((8, 5), np.float32))


def test_one_gpu_refusal_comes_before_the_data_set(monkeypatch):
    import skrec.parallel as P
    from skrec.recommender.FREEDOM import FREEDOM
    monkeypatch.setattr(P, "init_from_env", lambda: P.DistContext(0, 2))         # no WORLD_SIZE: that would start a group
    with pytest.raises(NotImplementedError, match="runs on one GPU"):
        FREEDOM(None, {})


def test_fit_is_the_scaffolds():
    from skrec.recommender.FREEDOM import FREEDOM
    from skrec.recommender.base import DeviceRecommender
    assert FREEDOM.fit is DeviceRecommender.fit and "fit" not in vars(FREEDOM)


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.FREEDOM import FREEDOM, FREEDOMConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("FREEDOM")
    assert reg.get_model("FREEDOM") == (FREEDOM, FREEDOMConfig)


# ---------------------------------------------------------------------------------------------------------------------
# the library without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 16
    for name in ("skr_freedom_keys", "skr_freedom_select_workspace", "skr_freedom_select", "skr_freedom_pruned_workspace",
                 "skr_freedom_pruned_csr", "skr_freedom_workspace", "skr_freedom_step", "skr_freedom_step_timed"):
        assert hasattr(L, name) and name in _hip.SIGNATURES
    assert (_hip.SKR_FREEDOM_MAX_BATCH, _hip.SKR_FREEDOM_MAX_LAYERS, _hip.SKR_FREEDOM_MAX_FEAT, _hip.SKR_FREEDOM_GROUPS) == (2048, 4, 4096, 7)
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    # keys
    assert L.skr_freedom_keys(None, 4, 1, 0, p, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_freedom_keys(p, -1, 1, 0, p, None) == -1 and b"nnz" in L.skr_last_error()
    assert L.skr_freedom_keys(p, 2 ** 31, 1, 0, p, None) == -1 and b"nnz" in L.skr_last_error()
    assert L.skr_freedom_keys(p, 0, 1, 0, p, None) == 0
    # select
    assert L.skr_freedom_select_workspace(0) == 0 and L.skr_freedom_select_workspace(2 ** 31) == 0
    ws = L.skr_freedom_select_workspace(70001)
    assert ws > 0 and ws % 16 == 0
    assert L.skr_freedom_select(None, 4, 2, p, p, ws, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_freedom_select(p, 4, 5, p, p, ws, None) == -1 and b"n_keep" in L.skr_last_error()
    assert L.skr_freedom_select(p, 4, -1, p, p, ws, None) == -1 and b"n_keep" in L.skr_last_error()
    assert L.skr_freedom_select(p, 70001, 5, p, p, ws - 16, None) == -1 and b"skr_freedom_select_workspace" in L.skr_last_error()
    assert L.skr_freedom_select(p, 70001, 5, p, 8, ws, None) == -1 and b"aligned" in L.skr_last_error()
    assert L.skr_freedom_select(p, 0, 0, p, p, 0, None) == 0
    # the compaction
    assert L.skr_freedom_pruned_workspace(0, 4, 4) == 0 and L.skr_freedom_pruned_workspace(4, 4, 0) == 0
    wp = L.skr_freedom_pruned_workspace(70, 45, 763)
    assert wp >= 763 + 2 * 4 * 115

    def pruned(nu=70, ni=45, nnz=763, work=p, work_bytes=wp, **kw):
        a = dict(rowptr=p, col=p, rowptr_t=p, col_t=p, perm=p, keep=p, o1=p, o2=p, o3=p, o4=p, o5=p, o6=p, kept=p)
        a.update(kw)
        return L.skr_freedom_pruned_csr(nu, ni, nnz, *a.values(), work, work_bytes, None)
    for name in ("rowptr", "perm", "keep", "o3", "kept"):
        assert pruned(**{name: None}) == -1 and b"NULL" in L.skr_last_error()
    assert pruned(nu=0) == -1 and b"n_users" in L.skr_last_error()
    assert pruned(nnz=-1) == -1 and b"nnz" in L.skr_last_error()
    assert pruned(work_bytes=wp - 16) == -1 and b"skr_freedom_pruned_workspace" in L.skr_last_error()
    assert pruned(work=8) == -1 and b"aligned" in L.skr_last_error()
    # the step
    assert L.skr_freedom_workspace(0) == 0 and L.skr_freedom_workspace(2049) == 0 and L.skr_freedom_workspace(2048) > 0

    def step(**kw):
        a = _hip.FreedomStepArgs()
        a.plan_a = a.plan_at = a.plan_s = a.plan_st = a.params = a.users = a.pos = a.neg = a.M = a.G = a.grad = a.loss = a.work = p
        a.ping[0] = a.ping[1] = p
        a.n_users, a.n_items, a.dim, a.n_ui_layers, a.n_mm_layers, a.n = 70, 45, 64, 2, 2, 16
        a.reg, a.work_bytes = 0.5, 1 << 30
        a.feat_dim[0], a.feat_ld[0] = 100, 100
        a.trs[0] = a.feat[0] = a.trs_grad[0] = a.feat_grad[0] = p
        for k, v in kw.items():
            if k in ("ping", "feat_dim", "feat_ld", "trs_grad"):
                getattr(a, k)[0] = v
            else:
                setattr(a, k, v)
        return L.skr_freedom_step(ctypes.byref(a), None)
    assert L.skr_freedom_step(None, None) == -1
    for name in ("params", "users", "pos", "neg", "M", "G", "grad", "loss", "work"):
        assert step(**{name: None}) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=2049) == -1 and b"at most 2048" in L.skr_last_error()
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(n_ui_layers=5) == -1 and b"n_ui_layers" in L.skr_last_error()
    assert step(n_mm_layers=5) == -1 and b"n_mm_layers" in L.skr_last_error()
    assert step(plan_a=None) == -1 and b"user-item graph" in L.skr_last_error()
    assert step(plan_st=None) == -1 and b"item graph" in L.skr_last_error()
    assert step(ping=None) == -1 and b"ping" in L.skr_last_error()
    assert step(reg=-1.0) == -1 and b"reg" in L.skr_last_error()
    assert step(feat_dim=4097) == -1 and b"feat_dim" in L.skr_last_error()
    assert step(feat_ld=98) == -1 and b"feat_ld" in L.skr_last_error()
    assert step(trs_grad=None) == -1 and b"four tables" in L.skr_last_error()
    assert step(n_clear=3) == -1 and b"clear_items" in L.skr_last_error()
    assert step(work_bytes=64) == -1 and b"skr_freedom_workspace" in L.skr_last_error()
    assert step(work=8) == -1 and b"aligned" in L.skr_last_error()
    assert step(n=0) == 0                     # an empty batch: nothing to launch
    assert step(n=0, reg=0.0, feat_dim=4097) == 0         # reg == 0: the modal arguments are not looked at
    assert L.skr_freedom_step_timed(None, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
def test_initialisation_equals_the_reference(golden):
    """the draws of FREEDOM.py:94-109 under the golden's seed; the feature tables are the features themselves"""
    import torch
    from skrec.recommender.FREEDOM import init_parameters
    g = golden("golden_freedom")
    want = T.fixture_params(g, 0)
    assert list(want) == list(T.param_names(True, True))
    torch.manual_seed(SEED)
    got = init_parameters(64, 96, 64, 64, 100, 37)
    assert set(got) == set(want) - {"image_embedding.weight", "text_embedding.weight"}
    for name, v in got.items():
        assert np.array_equal(v.numpy(), want[name]), name
    assert want["image_embedding.weight"].shape == (96, 100) and want["text_embedding.weight"].shape == (96, 37)
    # one modality alone draws less: the text block comes right after the item table
    torch.manual_seed(SEED)
    only_txt = init_parameters(64, 96, 64, 64, None, 37)
    assert set(only_txt) == set(T.BASE) | {"text_trs.weight", "text_trs.bias"}
    assert np.array_equal(only_txt["item_id_embedding.weight"].numpy(), want["item_id_embedding.weight"])
    assert not np.array_equal(only_txt["text_trs.weight"].numpy(), want["text_trs.weight"])


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def test_fixture_matches_the_twin(golden):
    g = golden("golden_freedom")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    nu = len(rowptr) - 1
    rows = T.csr_rows(rowptr)
    assert np.array_equal(g["adj_rows"], rows) and np.array_equal(g["adj_cols"], items) and len(items) == 763
    ig = golden("golden_item_graph")
    for k in ("mm_adj_row", "mm_adj_col", "mm_adj_val"):
        assert np.array_equal(g[k], ig[k])
    # the edge weights: the reference's fp32 _normalize_adj_m on the full graph
    w = np.power(np.float32(1e-7) + np.diff(rowptr).astype(np.float32), np.float32(-0.5))[rows] * \
        np.power(np.float32(1e-7) + np.bincount(items, minlength=ni).astype(np.float32), np.float32(-0.5))[items]
    assert _ulps(g["edge_w"], w).max() <= 4
    # every epoch's kept set and its values: each factor is correctly rounded in the twin and within 1 ulp in torch, and there
    # is one product
    keeps = T.fixture_keeps(g)
    n_keep = T.n_keep_of(763, CONFIG["dropout"])
    assert n_keep == 152 and g["keep_idx"].shape == g["keep_val"].shape == (3, n_keep)
    sets = []
    for e, keep in enumerate(keeps):
        assert keep.sum() == n_keep and np.array_equal(np.sort(g["keep_idx"][e]), np.nonzero(keep)[0])
        full = np.zeros(763, np.float32)
        full[g["keep_idx"][e]] = g["keep_val"][e]
        got = full[keep.astype(bool)]
        want = T.pruned_values_f32(rows, items, keep, nu, ni)
        print("epoch", e, "masked_adj values: largest distance", _ulps(got, want).max(), "ulps")
        assert _ulps(got, want).max() <= 4
        (rp, c, v), (rpt, ct, vt) = T.pruned_csr(rowptr, items, ni, keep)
        assert rp[-1] == rpt[-1] == n_keep and np.array_equal(v, want) and np.array_equal(np.sort(v), np.sort(vt))
        sets.append(frozenset(np.nonzero(keep)[0]))
    assert len(set(sets)) == 3
    steps = T.fixture_steps(g)
    assert [len(s["users"]) for s in steps] == [256, 256, 251] * 3
    test_users = g["test_users"]
    assert len(test_users) == 63
    names = T.param_names(True, True)
    S = T.dense_graph(g["mm_adj_row"], g["mm_adj_col"], g["mm_adj_val"], ni)
    init = T.fixture_params(g, 0)
    P, losses, scores = T.replay_f64((rowptr, items, ni), keeps, S, init, steps, CONFIG, 3, test_users)
    dev_p, dev_s, dev_l = g["f64_dev_params"], g["f64_dev_scores"], float(g["f64_dev_loss"])
    print("loss dev", np.abs(losses / g["loss"].astype(np.float64) - 1).max(), "allowed", 10 * dev_l)
    np.testing.assert_allclose(losses, g["loss"], rtol=10 * dev_l)
    final = T.fixture_params(g, 1)
    assert len(dev_p) == len(names) == 8
    drift = float(g["bias_drift"])
    for k, name in enumerate(names):
        dev = np.abs(P[name] - final[name]).max()
        if name in T.BIASES:                  # the twin's never move; the reference's drift is its own
            print(name, "drift", dev, "recorded", drift)
            assert np.array_equal(P[name], init[name]) and dev <= drift
        else:
            print(name, "dev", dev, "allowed", 10 * dev_p[k])
            assert dev <= 10 * dev_p[k]
    assert not np.array_equal(final["image_embedding.weight"], init["image_embedding.weight"])      # reg > 0: the tables train
    assert len(scores) == 3 and g["pred"].shape == (3, 63, 96)
    for s, p, lim in zip(scores, g["pred"], dev_s):
        assert np.abs(s - p).max() <= 10 * lim
    ndcg = [dict(zip(g["names"], r))["NDCG@10"] for r in g["reports"]]
    assert ndcg[0] < ndcg[-1]


def test_fixture_meets_its_own_conditions(golden):
    """BM3's conditions on a fixture: no float64 deviation above 1e-5, at most 3 near-tie users per evaluation"""
    g = golden("golden_freedom")
    print("f64_dev_params", g["f64_dev_params"], "scores", g["f64_dev_scores"], "loss", g["f64_dev_loss"], "close users", g["close_users"])
    assert max(g["f64_dev_scores"].max(), g["f64_dev_params"].max(), float(g["f64_dev_loss"])) <= 1e-5
    assert (g["close_users"] <= 3).all()
    assert [int((row >= 0).sum()) for row in g["close_ids"]] == list(g["close_users"])
    assert int(g["seed"]) == T.SEED


# ---------------------------------------------------------------------------------------------------------------------
# the sampler's law
# ---------------------------------------------------------------------------------------------------------------------
LAW_W = np.float32([0.5] * 24 + [0.1] * 24)
LAW_KEEP, LAW_TRIALS = 12, 4096
LAW_SEED = 2021                # fixed, and checked to hold on the CPU and with the device draws


def multinomial_frequencies(seed=LAW_SEED):
    """inclusion frequencies of torch.multinomial(w, 12) over 4096 seeded trials on the CPU"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    w = torch.from_numpy(LAW_W)
    count = np.zeros(len(LAW_W))
    for _ in range(LAW_TRIALS):
        count[torch.multinomial(w, LAW_KEEP, generator=gen).numpy()] += 1
    return count / LAW_TRIALS


def assert_same_law(f1, f2):
    """every entry within 5 standard errors of the difference of two binomial frequencies"""
    p = (f1 + f2) / 2
    bound = 5 * np.sqrt(2 * p * (1 - p) / LAW_TRIALS)
    print("largest |difference| / bound", (np.abs(f1 - f2) / bound).max())
    assert (np.abs(f1 - f2) <= bound).all()
    assert abs(f1.sum() - LAW_KEEP) < 1e-9 and abs(f2.sum() - LAW_KEEP) < 1e-9


def test_topk_of_weight_over_exponential_has_multinomials_law():
    rng = np.random.default_rng(LAW_SEED)
    count = np.zeros(len(LAW_W))
    for _ in range(LAW_TRIALS):
        keep = T.sample_keep(LAW_W, LAW_KEEP, rng)
        assert keep.sum() == LAW_KEEP
        count += keep
    f_twin, f_ref = count / LAW_TRIALS, multinomial_frequencies()
    assert f_ref[:24].mean() > 2 * f_ref[24:].mean()          # the draw is degree-sensitive at all
    assert_same_law(f_twin, f_ref)
