"""CPU suite of BM3 (skrec/io/dataset.py's feature loader, skrec/recommender/BM3.py, csrc/bm3.hip's argument checks,
tests/golden/golden_bm3.npz): the feature loader, the config and the limits, the registry, the library's exports and checks
without a GPU, the initialisation against the fixture, the fixture against the float64 twin (tests/bm3_twin.py)."""
import ctypes
import os

import numpy as np
import pytest

import bm3_twin as T

SEED = 2021
CONFIG = dict(lr=1e-2, reg=0.1, embed_dim=64, n_layers=2, dropout=0.3, cl_weight=2.0, batch_size=256, epochs=3)


# ---------------------------------------------------------------------------------------------------------------------
# the feature loader
# ---------------------------------------------------------------------------------------------------------------------
def _dataset(tiny_dir):
    from skrec.io import RSDataset
    lines = []
    ds = RSDataset(tiny_dir, "\t", "UIRT")
    ds._log_print = lines.append
    return ds, lines


def test_feature_loader_reads_both_one_or_no_file(tiny_dir):
    rng = np.random.default_rng(1)
    img, txt = rng.standard_normal((96, 100)).astype(np.float32), rng.standard_normal((96, 37)).astype(np.float32)
    ds, lines = _dataset(tiny_dir)
    assert ds.img_features is None and ds.txt_features is None and ds.audio_features is None
    assert ds.img_dim is None and ds.txt_dim is None and ds.audio_dim is None
    # the first array is used, whatever its key
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), zebra=img, apple=np.zeros((3, 3)))
    ds, lines = _dataset(tiny_dir)
    assert np.array_equal(ds.img_features, img) and ds.img_dim == 100 and ds.txt_features is None and ds.txt_dim is None
    np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), anything=txt)
    ds, lines = _dataset(tiny_dir)
    assert np.array_equal(ds.img_features, img) and np.array_equal(ds.txt_features, txt) and (ds.img_dim, ds.txt_dim) == (100, 37)
    assert ds.audio_features is None and ds.mm_data is ds.mm_data
    _ = ds.txt_features, ds.img_dim
    shapes = [ln for ln in lines if "features" in ln]
    assert len(shapes) == 1 and "(96, 100)" in shapes[0] and "(96, 37)" in shapes[0]          # logged once
    os.remove(os.path.join(tiny_dir, "tiny.img.npz"))
    ds, _ = _dataset(tiny_dir)
    assert ds.img_features is None and np.array_equal(ds.txt_features, txt)


def test_feature_loader_rejects_a_wrong_row_count(tiny_dir):
    np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), f=np.zeros((95, 8), np.float32))
    ds, _ = _dataset(tiny_dir)
    with pytest.raises(ValueError, match=r"95 rows.*96 items"):
        ds.txt_features


# ---------------------------------------------------------------------------------------------------------------------
# the config, the limits, the registry
# ---------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    from skrec.recommender.BM3 import BM3Config
    c = BM3Config()
    assert dict(c.items()) == dict(lr=1e-3, reg=0.1, embed_dim=64, feat_dim=64, n_layers=1, cl_weight=2.0, dropout=0.3, batch_size=2048,
                                   epochs=1000, early_stop=200, draws="device")
    assert BM3Config.param_space() == {"n_layers": [1, 2], "reg": [0.1, 0.01], "dropout": [0.3, 0.5]}
    assert BM3Config(feat_dim=7).feat_dim == 7                   # accepted and ignored
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(reg=-0.1), dict(embed_dim=0), dict(n_layers=-1), dict(n_layers=2.0), dict(dropout=1.0),
                dict(dropout=0), dict(cl_weight=-1.0), dict(batch_size=0), dict(epochs=-1), dict(draws="reference")):
        with pytest.raises(AssertionError):
            BM3Config(**bad)


def test_limits_are_named():
    from skrec.recommender.BM3 import BM3, BM3Config, check_limits
    check_limits(BM3Config(embed_dim=20, n_layers=4, batch_size=2048), img_dim=4096, txt_dim=1)
    check_limits(BM3Config(n_layers=0))
    with pytest.raises(NotImplementedError, match="embed_dim <= 64"):
        check_limits(BM3Config(embed_dim=65))
    with pytest.raises(NotImplementedError, match="n_layers <= 4"):
        check_limits(BM3Config(n_layers=5))
    with pytest.raises(NotImplementedError, match="batch_size <= 2048"):
        check_limits(BM3Config(batch_size=2049))
    with pytest.raises(NotImplementedError, match="feature width <= 4096.*image.*4097"):
        check_limits(BM3Config(), img_dim=4097)
    with pytest.raises(NotImplementedError, match="feature width <= 4096.*text.*4097"):
        check_limits(BM3Config(), txt_dim=4097)
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(BM3Config(), world=2)
    # the constructor raises before it touches the data set or the GPU
    with pytest.raises(NotImplementedError, match="embed_dim <= 64"):
        BM3(None, dict(embed_dim=128))
    with pytest.raises(NotImplementedError, match="n_layers <= 4"):
        BM3(None, dict(n_layers=7))


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.BM3 import BM3, BM3Config
    reg = ModelRegistry()
    assert reg.load_skrec_model("BM3")
    assert reg.get_model("BM3") == (BM3, BM3Config)


def test_library_exports_and_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 14
    for name in ("skr_bm3_project", "skr_bm3_draws", "skr_bm3_workspace", "skr_bm3_step", "skr_bm3_step_timed", "skr_bm3_queries"):
        assert hasattr(L, name) and name in _hip.SIGNATURES
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    assert L.skr_bm3_workspace(0) == 0 and L.skr_bm3_workspace(2049) == 0 and L.skr_bm3_workspace(2048) > 0
    assert L.skr_bm3_project(None, 4, 8, 8, p, p, 4, p, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_bm3_project(p, 4, 4097, 4100, p, p, 4, p, None) == -1 and b"feat_dim" in L.skr_last_error()
    assert L.skr_bm3_project(p, 4, 0, 4, p, p, 4, p, None) == -1 and b"feat_dim" in L.skr_last_error()
    assert L.skr_bm3_project(p, 4, 37, 37, p, p, 4, p, None) == -1 and b"multiple of 4" in L.skr_last_error()
    assert L.skr_bm3_project(p, 4, 8, 8, p, p, 2049, p, None) == -1 and b"at most 2048" in L.skr_last_error()
    assert L.skr_bm3_project(p, 4, 8, 8, p, p, 0, p, None) == 0
    assert L.skr_bm3_draws(None, 4, 0, 0.3, 1, 1, p, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_bm3_draws(p, 4, 4, 0.3, 1, 1, p, None) == -1 and b"table" in L.skr_last_error()
    assert L.skr_bm3_draws(p, 4, 0, 1.0, 1, 1, p, None) == -1 and b"rate" in L.skr_last_error()
    assert L.skr_bm3_queries(None, p, 4, 4, p, p, None) == -1 and b"NULL" in L.skr_last_error()

    def step(**kw):
        a = _hip.BM3StepArgs()
        a.plan_a = a.plan_at = a.params = a.users = a.items = a.M = a.G = a.grad = a.loss = a.work = p
        a.ping[0] = a.ping[1] = p
        a.n_users, a.n_items, a.dim, a.n_layers, a.n = 70, 45, 64, 2, 16
        a.dropout, a.reg, a.cl_weight, a.work_bytes = 0.3, 0.1, 2.0, 1 << 30
        a.feat_dim[0], a.feat_ld[0] = 100, 100
        a.trs[0] = a.feat[0] = a.trs_grad[0] = a.feat_grad[0] = p
        for k, v in kw.items():
            if k in ("ping", "keep", "feat_dim", "feat_ld", "trs_grad"):
                getattr(a, k)[0] = v
            else:
                setattr(a, k, v)
        return L.skr_bm3_step(ctypes.byref(a), None)
    assert L.skr_bm3_step(None, None) == -1
    assert step(params=None) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=2049) == -1 and b"at most 2048" in L.skr_last_error()
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(n_layers=5) == -1 and b"n_layers" in L.skr_last_error()
    assert step(plan_a=None) == -1 and b"plans" in L.skr_last_error()
    assert step(ping=None) == -1 and b"ping" in L.skr_last_error()
    assert step(dropout=1.0) == -1 and b"dropout" in L.skr_last_error()
    assert step(keep=p) == -1 and b"together" in L.skr_last_error()
    assert step(feat_dim=4097) == -1 and b"feat_dim" in L.skr_last_error()
    assert step(feat_ld=98) == -1 and b"feat_ld" in L.skr_last_error()
    assert step(trs_grad=None) == -1 and b"four tables" in L.skr_last_error()
    assert step(n_clear=3) == -1 and b"clear_items" in L.skr_last_error()
    assert step(work_bytes=64) == -1 and b"skr_bm3_workspace" in L.skr_last_error()
    assert step(work=8) == -1 and b"aligned" in L.skr_last_error()
    assert step(n=0) == 0                     # an empty batch: nothing to launch
    assert L.skr_bm3_step_timed(None, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
def test_initialisation_equals_the_reference(golden):
    """the draws of BM3.py:95-114 under the golden's seed; the feature tables are the features themselves"""
    import torch
    from skrec.recommender.BM3 import init_parameters
    g = golden("golden_bm3")
    want = T.fixture_params(g, 0)
    assert set(want) == set(T.param_names(True, True))
    torch.manual_seed(SEED)
    got = init_parameters(64, 96, 64, 100, 37)
    assert set(got) == set(want) - {"image_embedding.weight", "text_embedding.weight"}
    for name, v in got.items():
        assert np.array_equal(v.numpy(), want[name]), name
    assert want["image_embedding.weight"].shape == (96, 100) and want["text_embedding.weight"].shape == (96, 37)
    # one modality alone draws less: the text block comes right after the predictor
    torch.manual_seed(SEED)
    only_txt = init_parameters(64, 96, 64, None, 37)
    assert set(only_txt) == set(T.BASE) | {"text_trs.weight", "text_trs.bias"}
    assert np.array_equal(only_txt["predictor.weight"].numpy(), want["predictor.weight"])
    assert not np.array_equal(only_txt["text_trs.weight"].numpy(), want["text_trs.weight"])


def test_fixture_matches_the_twin(golden):
    g = golden("golden_bm3")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    steps = T.fixture_steps(g)
    assert [len(s["users"]) for s in steps] == [256, 256, 251] * 3
    rows = T.csr_rows(rowptr)
    order = np.lexsort((rows, items))
    assert np.array_equal(g["adj_rows"], rows) and np.array_equal(g["adj_cols"], items) and len(items) == 763
    assert np.array_equal(g["adj_t_rows"], items[order]) and np.array_equal(g["adj_t_cols"], rows[order])
    assert np.array_equal(g["adj_t_val"], g["adj_val"][order])
    np.testing.assert_allclose(g["adj_val"], T.normalised_values(rowptr, items, ni), rtol=2e-7)
    for s in steps:
        for k in ("ku", "ki", "kt", "kv"):
            assert s[k].shape == (len(s["users"]), 64) and 0.6 < s[k].mean() < 0.8
        # a node that occurs twice in a batch has one mask
        first = {}
        for r, i in enumerate(s["items"]):
            assert np.array_equal(s["kt"][r], s["kt"][first.setdefault(int(i), r)])
    test_users = g["test_users"]
    assert len(test_users) == 63 and 63 in test_users
    names = T.param_names(True, True)
    P, losses, scores = T.replay_f64((rowptr, items, ni), g["adj_val"], T.fixture_params(g, 0), steps, CONFIG, 3, test_users)
    dev_p, dev_s, dev_l = g["f64_dev_params"], g["f64_dev_scores"], float(g["f64_dev_loss"])
    print("loss dev", np.abs(losses / g["loss"].astype(np.float64) - 1).max(), "allowed", 10 * dev_l)
    np.testing.assert_allclose(losses, g["loss"], rtol=10 * dev_l)
    final = T.fixture_params(g, 1)
    assert len(dev_p) == len(names) == 10
    for k, name in enumerate(names):
        print(name, "dev", np.abs(P[name] - final[name]).max(), "allowed", 10 * dev_p[k])
        assert np.abs(P[name] - final[name]).max() <= 10 * dev_p[k]
    # the feature tables are trainable: rows move, also outside a step's batch (leftover momentum)
    assert not np.array_equal(final["image_embedding.weight"], T.fixture_params(g, 0)["image_embedding.weight"])
    assert len(scores) == 3 and g["pred"].shape == (3, 63, 96)
    for s, p, lim in zip(scores, g["pred"], dev_s):
        assert np.abs(s - p).max() <= 10 * lim
    # the fixture's own conditions, and what the GPU tests rely on
    assert (g["close_users"] <= 3).all()
    assert max(dev_s.max(), dev_p.max(), dev_l) <= 1e-5
    ndcg = [dict(zip(g["names"], r))["NDCG@10"] for r in g["reports"]]
    assert ndcg[0] < ndcg[-1]
