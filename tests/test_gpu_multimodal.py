"""GPU suite of the multimodal models' shared half (skrec/recommender/_multimodal.py) under each of the five models: the
reference's parameter names in order, ``load_parameters(parameters())`` as the identity on every parameter buffer, the shapes of
``gradients()`` after a ``gradient_step``, and a second ``train_step`` behind the first.  U = 5, I = 7, d = 8; the image table is 5
wide (padded to 8), the text table 4 (exact)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U, I, D, FV, FT = 5, 7, 8, 5, 4
ROWS = [sorted({u, (u + 3) % I}) for u in range(U)]           # every user has two items, every item a user
ROWPTR = np.concatenate([[0], np.cumsum([len(r) for r in ROWS])]).astype(np.int64)
ITEMS = np.concatenate(ROWS).astype(np.int32)
USERS, POS, NEG = np.array([1, 3, 1], np.int32), np.array([2, 2, 5], np.int32), np.array([6, 0, 6], np.int32)     # a user and an item twice


def _modal(prefixes):
    return [f"{p}_{s}" for p in prefixes for s in ("embedding.weight", "trs.weight", "trs.bias")]


def _mgcn_names(prefixes):
    gates = [f"{g}.0.{p}" for g in ("gate_v", "gate_t", "gate_image_prefer", "gate_text_prefer") for p in ("weight", "bias")]
    return (["user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight", "image_trs.weight",
             "image_trs.bias", "text_trs.weight", "text_trs.bias", "query_common.0.weight", "query_common.0.bias", "query_common.2.weight"] + gates)


def _lattice_names(prefixes):
    return (["modal_weight", "user_embedding.weight", "item_id_embedding.weight"] + [p + "_embedding.weight" for p in prefixes]
            + [f"{p}_trs.{s}" for p in prefixes for s in ("weight", "bias")])


def _slmrec_names(prefixes):
    linears = ("v_dense", "t_dense", "embedding_item_after_GCN", "embedding_user_after_GCN", "g_i_iv", "g_v_iv", "g_iv_iva", "g_a_iva",
               "g_iva_ivat", "g_t_ivat")
    return ["embedding_user.weight", "embedding_item.weight"] + [f"{m}.{p}" for m in linears for p in ("weight", "bias")]


# model -> (config, the reference's names for the present prefixes, the lists of a batch)
MODELS = {
    "BM3": (dict(embed_dim=D, n_layers=1, batch_size=3),
            lambda pre: ["user_embedding.weight", "item_id_embedding.weight", "predictor.weight", "predictor.bias"] + _modal(pre), (USERS, POS)),
    "FREEDOM": (dict(embed_dim=D, feat_dim=D, n_ui_layers=1, n_mm_layers=1, knn_k=2, reg=1e-3, batch_size=3),
                lambda pre: ["user_embedding.weight", "item_id_embedding.weight"] + _modal(pre), (USERS, POS, NEG)),
    "MGCN": (dict(embed_dim=D, n_ui_layers=1, n_layers=1, knn_k=2, batch_size=3), _mgcn_names, (USERS, POS, NEG)),
    "LATTICE": (dict(embed_dim=D, feat_embed_dim=D, weight_size=(D,), n_layers=1, knn_k=2, batch_size=3), _lattice_names, (USERS, POS, NEG)),
    "SLMRec": (dict(rec_dim=D, layer_num=1, batch_size=3), _slmrec_names, (USERS, POS)),
}
CASES = [(m, True, {}) for m in MODELS] + [(m, False, {}) for m in ("BM3", "FREEDOM", "LATTICE")] + [("FREEDOM", True, dict(reg=0.0))]


def _build(model, image, extra):
    cls = getattr(importlib.import_module("skrec.recommender." + model), model)
    cfg, names, batch = MODELS[model]
    rng = np.random.default_rng(7)
    img, txt = rng.standard_normal((I, FV)).astype(np.float32), rng.standard_normal((I, FT)).astype(np.float32)
    torch.manual_seed(11)
    kw = dict(seed=5) if cls.seeded else {}
    m = cls.detached(U, I, dict(cfg, **extra), (ROWPTR, ITEMS), img=img if image else None, txt=txt, **kw)
    return m, names(["image", "text"] if image else ["text"]), batch


def _buffers(m):
    """every parameter buffer of the model"""
    return [b for b in (m._flat, getattr(m, "_mflat", None), getattr(m, "_const", None)) if b is not None]


@pytest.mark.parametrize("model,image,extra", CASES, ids=[f"{m}{'' if i else '-text_only'}{'-reg0' if e else ''}" for m, i, e in CASES])
def test_shared_half_under_each_model(model, image, extra):
    m, names, batch = _build(model, image, extra)
    mod = importlib.import_module("skrec.recommender." + model)
    assert m.feat_dim == {"img": FV if image else 0, "txt": FT} and m.feat_ld == {"img": 8 if image else 0, "txt": 4}
    assert m.present == [image, True]
    # the reference's names, in its order, in its shapes
    P = m.parameters()
    assert list(P) == names
    for prefix, dense, F in (("image", "v_dense", FV), ("text", "t_dense", FT)):
        if prefix == "text" or image:
            lin = dense if model == "SLMRec" else prefix + "_trs"
            assert tuple(P[lin + ".weight"].shape) == (D, F) and tuple(P[lin + ".bias"].shape) == (D,)
            if model != "SLMRec":          # its tables are constants, not parameters
                assert tuple(P[prefix + "_embedding.weight"].shape) == (I, F)
    # load_parameters(parameters()) is the identity on every buffer, the padding included
    bufs = _buffers(m)
    assert len(bufs) == {"LATTICE": 2}.get(model, 2 if model == "FREEDOM" and extra else 1)
    assert all(bool(b.any()) for b in bufs)
    before = [b.clone() for b in bufs]
    m.load_parameters(P)
    for b, want in zip(_buffers(m), before):
        assert torch.equal(b, want)
    for k, v in m.parameters().items():
        assert torch.equal(v, P[k]), k
    # gradients() after one gradient_step: the shapes of parameters()
    kw = dict(build=True) if model == "LATTICE" else {}
    loss = m.gradient_step(*batch, **kw)
    assert loss.shape == (m.LOSS_LEN,) and bool(torch.isfinite(loss).all())
    G = m.gradients()
    untrained = getattr(mod, "UNTRAINED", ())
    assert list(G) == [k for k in names if k not in untrained]
    for k, g in G.items():
        assert g.shape == P[k].shape and g.dtype == torch.float32 and g.is_contiguous() and bool(torch.isfinite(g).all()), k
    assert bool(G[names[1]].any())
    clears = model in ("BM3", "FREEDOM") and not extra
    if clears:         # the step left the item ids whose feature-gradient rows it wrote
        want = POS if model == "BM3" else np.concatenate([POS, NEG])
        assert np.array_equal(m._prev_items.cpu().numpy(), want)
    else:
        assert m._prev_items is None
    # two train_steps: the first one's gradient rows are not the second one's to clear
    l1 = m.train_step(*batch, **kw).cpu().numpy()
    assert m._prev_items is None
    l2 = m.train_step(*batch).cpu().numpy()
    assert m._prev_items is None and len(m.step_losses) == 2
    assert np.isfinite(l1).all() and np.isfinite(l2).all()
    moved = m.parameters()
    assert not torch.equal(moved[names[1]], P[names[1]])
    if model == "FREEDOM" and extra:       # reg == 0: the modal blocks are constants
        for k in _modal(["image", "text"]):
            assert torch.equal(moved[k], P[k]), k
    torch.cuda.synchronize()
