"""CPU suite of the multimodal models' shared half (skrec/recommender/_multimodal.py): the layout of the modal blocks against the
arithmetic each model's ``_build`` used to spell out, the named views of a buffer, the feature intake and its messages, the
limit clauses the five ``check_limits`` share and the order in which each model raises them."""
import importlib

import numpy as np
import pytest
import torch

from skrec import _hip
from skrec.recommender._multimodal import MODALITIES, ModalLayout, feature_dims, features, lambda_lr, limit_batch, limit_features, limit_world

MODELS = ("BM3", "FREEDOM", "MGCN", "LATTICE", "SLMRec")
U, I = 5, 3
N = U + I
# where each model's modal blocks start, and whether a table follows the projection block
STARTS = {"BM3": (N * 64 + _hip.SKR_BM3_PRED_FLOATS, True), "FREEDOM": (N * 64, True), "MGCN": (N * 64, True), "LATTICE": (4, True),
          "SLMRec": (N * 64, False)}
WIDTHS = (1, 4, 5, 4096)
LD = {1: 4, 4: 4, 5: 8, 4096: 4096}
CASES = [(Fv, Ft) for Fv in WIDTHS for Ft in WIDTHS] + [(F, 0) for F in WIDTHS] + [(0, F) for F in WIDTHS]


def _module(model):
    return importlib.import_module("skrec.recommender." + model)


# ---------------------------------------------------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------------------------------------------------
def _expected(start, tables, Fv, Ft):
    """the offsets loop of the models' former ``_build``"""
    off, o = {}, start
    for key, F in (("img", Fv), ("txt", Ft)):
        if F:
            ld = (F + 3) // 4 * 4
            assert ld == LD[F]
            off[key] = (o, o + 64 * ld + 64 if tables else None)
            o += 64 * ld + 64 + (I * ld if tables else 0)
    return off, o


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("Fv,Ft", CASES)
def test_layout_offsets(model, Fv, Ft):
    start, tables = STARTS[model]
    lay = ModalLayout(I, {"img": Fv, "txt": Ft}, start, tables=tables)
    off, total = _expected(start, tables, Fv, Ft)
    assert lay.off == off and lay.total == total and list(lay.off) == [k for k, _ in MODALITIES if k in off]
    assert lay.feat_ld == {"img": (Fv + 3) // 4 * 4, "txt": (Ft + 3) // 4 * 4}


def test_layout_present_overrides_the_widths():
    lay = ModalLayout(I, {"img": 5, "txt": 4}, 7, present=["txt"])
    assert lay.off == {"txt": (7, 7 + 64 * 4 + 64)} and lay.total == 7 + 64 * 4 + 64 + I * 4
    assert ModalLayout(I, {"img": 5, "txt": 4}, 7, present=[]).total == 7


@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("Fv,Ft", CASES)
def test_named_views_are_the_expected_slices(Fv, Ft, d):
    start = 100
    lay = ModalLayout(I, {"img": Fv, "txt": Ft}, start)
    buf = torch.arange(lay.total + 10, dtype=torch.int64)
    hit = torch.zeros_like(buf)
    off, _ = _expected(start, True, Fv, Ft)
    for key, prefix in MODALITIES:
        if key not in off:
            assert key not in lay.off
            continue
        F, ld, (t, e) = lay.feat_dim[key], LD[lay.feat_dim[key]], off[key]
        trs, tab = lay.blocks(buf, key)
        assert trs.data_ptr() == buf[t:].data_ptr() and trs.numel() == 64 * ld + 64
        assert tab.data_ptr() == buf[e:].data_ptr() and tab.numel() == I * ld
        V = lay.views(buf, key, prefix, d)
        assert list(V) == [prefix + "_embedding.weight", prefix + "_trs.weight", prefix + "_trs.bias"]
        want_tab = e + ld * torch.arange(I)[:, None] + torch.arange(F)[None, :]
        want_W = t + ld * torch.arange(d)[:, None] + torch.arange(F)[None, :]
        assert torch.equal(V[prefix + "_embedding.weight"], want_tab)
        assert torch.equal(V[prefix + "_trs.weight"], want_W)
        assert torch.equal(V[prefix + "_trs.bias"], t + 64 * ld + torch.arange(d))
        W, b = lay.linear(trs, key, d)
        assert torch.equal(W, want_W) and torch.equal(b, V[prefix + "_trs.bias"])
        for v in lay.views(hit, key, prefix, d).values():
            v += 1
        assert lay.views(None, key, prefix, d) == dict.fromkeys(V)
    covered = sum(d * F + d + I * F for F in (Fv, Ft) if F)
    assert int(hit.max()) == 1 and int(hit.sum()) == covered          # disjoint
    assert not hit[:start].any() and not hit[lay.total:].any()


def test_projection_only_layout_has_no_table():
    lay = ModalLayout(I, {"img": 5, "txt": 4}, 0, tables=False)
    buf = torch.arange(lay.total)
    trs, tab = lay.blocks(buf, "txt")
    assert tab is None and trs.data_ptr() == buf[64 * 8 + 64:].data_ptr() and trs.numel() == 64 * 4 + 64 and lay.total == 64 * 12 + 128


# ---------------------------------------------------------------------------------------------------------------------
# the feature intake
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_features_messages(model):
    bad = np.zeros((4, 6), np.float32)
    for name in ("image", "text"):
        with pytest.raises(ValueError) as e:
            features(bad, 3, model, name)
        assert str(e.value) == f"{model}: the {name} feature table has shape (4, 6), the data set has 3 items"
        with pytest.raises(ValueError) as e:
            features(torch.zeros(3), 3, model, name)
        assert str(e.value) == f"{model}: the {name} feature table has shape (3,), the data set has 3 items"
        with pytest.raises(ValueError) as e:
            features(None, 3, model, name, required=True)
        assert str(e.value) == f"{model}: the {name} feature table is missing -- the model's forward uses both modalities"
        assert features(None, 3, model, name) is None


@pytest.mark.parametrize("model", MODELS)
def test_model_requires_its_tables_or_not(model):
    cls = getattr(_module(model), model)
    assert cls.required == (model in ("MGCN", "SLMRec"))
    assert cls.seeded == (model in ("BM3", "FREEDOM")) and cls.pairwise == (model in ("FREEDOM", "MGCN", "LATTICE"))
    m = cls.__new__(cls)
    m.config = cls.config_class()
    ok = np.zeros((3, 4), np.float32)
    if cls.required:
        for kw, name in ((dict(txt=ok), "image"), (dict(img=ok), "text")):
            with pytest.raises(ValueError) as e:
                m._check_data(**kw)
            assert str(e.value) == f"{model}: the {name} feature table is missing -- the model's forward uses both modalities"
    elif model != "BM3":
        with pytest.raises(ValueError) as e:
            m._check_data()
        assert str(e.value) == f"{model}: no modality at all -- the item graph needs an image or a text feature table"
    m._check_data(img=ok, txt=ok)
    with pytest.raises(NotImplementedError) as e:
        m._check_data(img=ok, txt=np.zeros((3, 0), np.float32))
    assert "(the text table has 0 columns)" in str(e.value)


def test_features_of_numpy_and_tensor_agree():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3, 5))                       # float64, as np.load gives it
    got_np, got_t = features(a, 3, "BM3", "image"), features(torch.from_numpy(a), 3, "BM3", "image")
    assert got_np.dtype == got_t.dtype == torch.float32 and got_np.shape == (3, 5) and torch.equal(got_np, got_t)
    assert torch.equal(got_np, torch.from_numpy(a.astype(np.float32)))
    assert torch.equal(features(np.asfortranarray(a), 3, "BM3", "image"), got_np)
    dim, ld, present = feature_dims({"img": got_np, "txt": None})
    assert dim == {"img": 5, "txt": 0} and ld == {"img": 8, "txt": 0} and present == [True, False]
    assert feature_dims({"img": None, "txt": torch.zeros(3, 4)}) == ({"img": 0, "txt": 4}, {"img": 0, "txt": 4}, [False, True])


# ---------------------------------------------------------------------------------------------------------------------
# the shared limit clauses
# ---------------------------------------------------------------------------------------------------------------------
class _Cfg:
    batch_size = 2049


def test_shared_clauses_messages():
    with pytest.raises(NotImplementedError) as e:
        limit_batch("SLMRec", _Cfg, 2048)
    assert str(e.value) == "SLMRec: batch_size <= 2048 (got 2049): skr_slmrec_step takes 2048 rows"
    limit_batch("SLMRec", _Cfg, 2049)
    for F, name, kw in ((4097, "image", dict(img_dim=4097, txt_dim=0)), (0, "text", dict(img_dim=None, txt_dim=0))):
        with pytest.raises(NotImplementedError) as e:
            limit_features("BM3", 4096, **kw)
        assert str(e.value) == f"BM3: 1 <= feature width <= 4096 (the {name} table has {F} columns)"
    limit_features("BM3", 4096, 1, 4096)
    limit_features("BM3", 4096, None, None)
    with pytest.raises(NotImplementedError) as e:
        limit_world("MGCN", 2)
    assert str(e.value) == "MGCN runs on one GPU (one rank): there is no sharded engine for it"
    limit_world("MGCN", 1)


@pytest.mark.parametrize("model", MODELS)
def test_check_limits_raises_the_shared_clauses_in_its_order(model):
    mod = _module(model)
    Config, check = getattr(mod, model + "Config"), mod.check_limits
    MB, MF = mod.MAX_BATCH, mod.MAX_FEAT
    assert (MB, MF) == (2048, 4096)
    low = model.lower()
    msg_batch = f"{model}: batch_size <= {MB} (got {MB + 1}): skr_{low}_step takes {MB} rows"
    msg_world = f"{model} runs on one GPU (one rank): there is no sharded engine for it"

    def raised(cfg, *a):
        with pytest.raises(NotImplementedError) as e:
            check(cfg, *a)
        return str(e.value)
    check(Config(), 1, 1, MF)
    assert raised(Config(batch_size=MB + 1)) == msg_batch
    assert raised(Config(), 1, MF + 1, None) == f"{model}: 1 <= feature width <= {MF} (the image table has {MF + 1} columns)"
    assert raised(Config(), 1, 5, 0) == f"{model}: 1 <= feature width <= {MF} (the text table has 0 columns)"
    assert raised(Config(), 2) == msg_world
    # two limits at once: the batch clause before the widths, the widths before the world, the image before the text
    assert raised(Config(batch_size=MB + 1), 2, 0, 0) == msg_batch
    assert raised(Config(), 2, MF + 1, 0) == f"{model}: 1 <= feature width <= {MF} (the image table has {MF + 1} columns)"
    if hasattr(Config(), "knn_k"):         # the neighbour clause sits between the batch clause and the widths
        knn = f"{model}: knn_k <= 32 (got 33): skr_knn_topk keeps 32 neighbours per row"
        assert raised(Config(knn_k=33), 2, 0, 0) == knn
        assert raised(Config(knn_k=33, batch_size=MB + 1), 2, 0, 0) == msg_batch
    assert raised(Config(embed_dim=65) if model != "SLMRec" else Config(rec_dim=65), 2, 0, 0).startswith(
        f"{model}: {'rec_dim' if model == 'SLMRec' else 'embed_dim'} <= 64 (got 65)")


def test_lambda_lr_is_the_reference_expression():
    for lr, g, s, epoch in ((1e-3, 0.96, 50, 7), (1e-4, 1.0, 50, 3), (1e-2, 0.5, 1, 2)):
        assert lambda_lr(lr, [g, s], epoch) == lr * g ** (epoch / s)
    from skrec.recommender import LATTICE, MGCN, SLMRec
    assert MGCN.learning_rate(MGCN.MGCNConfig(lr=1e-3, lr_scheduler=(0.96, 50)), 7) == 1e-3 * 0.96 ** (7 / 50)
    assert LATTICE.learning_rate(LATTICE.LATTICEConfig(lr=1e-3, lr_scheduler=(0.9, 10)), 3) == 1e-3 * 0.9 ** (3 / 10)
    assert SLMRec.learning_rate(SLMRec.SLMRecConfig(lr=1e-3), 9) == 1e-3 * 1.0 ** (9 / 50)
