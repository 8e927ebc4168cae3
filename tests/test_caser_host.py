"""CPU suite of Caser: the float64 twin (tests/caser_twin.py) replays the reference's fit() from the fixture's batches and
keep flags; the twin's rule for pooling ties and relu'(0) against torch's own ops; the config and the registry; the limits;
the initialisation and the parameter views against the reference's shapes; the argument checks of the entry points (no GPU
needed)."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)
import caser_twin as T

SEED = 2021


def _golden_params(g, sfx, L):
    return {k: g[k + sfx] for k in T.param_names(L)}


@pytest.fixture(scope="module")
def replay(golden):
    """the twin's run over the fixture's 9 steps: (losses [9, 2], parameters afterwards, the fixture)"""
    import torch
    g = golden("golden_caser")
    cfg = T.CONFIG
    L, Tn = cfg["seq_L"], cfg["seq_T"]
    P = T.to_torch(_golden_params(g, "0", L))
    opt = torch.optim.Adam(list(P.values()), lr=cfg["lr"], weight_decay=cfg["l2_reg"])
    keep = T.unpack_bits(g["keep_bits"], g["keep_shape"])
    b = g["step_bounds"]
    losses = []
    for s in range(len(b) - 1):
        sl = slice(int(b[s]), int(b[s + 1]))
        u, seq, it = (torch.from_numpy(g[k][sl]).long() for k in ("batch_users", "batch_seqs", "batch_items"))
        lp, ln, loss = T.step_losses(P, u, seq, it[:, :Tn], it[:, Tn:], torch.from_numpy(keep[sl]), cfg["dropout"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append((lp.item(), ln.item()))
    return np.array(losses), {k: v.detach().numpy() for k, v in P.items()}, g


def test_twin_replays_the_reference_fit(replay):
    losses, P, g = replay
    print("bce sums", losses.ravel(), "golden", g["bce_sums"].ravel())
    assert losses.shape == g["bce_sums"].shape == (9, 2)
    np.testing.assert_allclose(losses, g["bce_sums"], rtol=1e-5)
    dev = {k: float(np.abs(P[k] - g[k + "1"]).max()) for k in P}
    for k, d in dev.items():
        print(f'    "{k}": {d:.3g},   # step {float(np.abs(g[k + "1"] - g[k + "0"]).max()):.3g}')
    assert set(dev) == set(T.TWIN_DEVIATION)
    for k, d in dev.items():
        assert d <= T.TWIN_DEVIATION[k], (k, d)
        # ... and the recorded bound is the reference's fp32 noise, not slack: within a factor of 1.5 of what is measured
        assert T.TWIN_DEVIATION[k] <= 1.5 * d + 1e-12, (k, d)


def test_twin_predicts_what_the_reference_predicts(replay):
    import torch
    _, P, g = replay
    Pt = T.to_torch(P, requires_grad=False)
    users = [int(u) for u in g["pred_users"]]
    win = {int(u): s for u, s in zip(g["trunc_users"], g["trunc_seqs"])}
    x = T.query_rows(Pt, torch.tensor(users), torch.from_numpy(np.stack([win[u] for u in users])).long())
    pred = (x @ Pt["W2"].T + Pt["b2"].squeeze(-1)).numpy()
    assert pred.shape == g["pred"].shape == (4, 97)
    print("pred max abs diff", np.abs(pred - g["pred"]).max())
    np.testing.assert_allclose(pred, g["pred"], rtol=1e-4, atol=1e-6)
    assert g["min_top_gap"][0] >= 1e-7


def _torch_ops_loss(P, u, seq, pos, neg):
    """the same forward with torch's own conv2d / max_pool1d / relu, as the reference composes them"""
    import torch
    import torch.nn.functional as F
    L = seq.shape[1]
    emb = P["item_embeddings"][seq].unsqueeze(1)
    out_v = F.conv2d(emb, P["conv_v_weight"], P["conv_v_bias"]).view(seq.shape[0], -1)
    hs = []
    for i in range(L):
        c = F.relu(F.conv2d(emb, P[f"conv_h_weight_{i}"], P[f"conv_h_bias_{i}"]).squeeze(3))
        hs.append(F.max_pool1d(c, c.size(2)).squeeze(2))
    out = torch.cat([out_v] + hs, 1)
    z = F.relu(F.linear(out, P["fc1_weight"], P["fc1_bias"]))
    x = torch.cat([z, P["user_embeddings"][u]], 1)
    it = torch.cat([pos, neg], 1)
    y = torch.baddbmm(P["b2"][it], P["W2"][it], x.unsqueeze(2)).squeeze(-1)
    yp, yn = torch.split(y, [pos.shape[1], neg.shape[1]], dim=1)
    bce = F.binary_cross_entropy_with_logits
    return (bce(yp, torch.ones_like(yp), reduction="none") + bce(yn, torch.zeros_like(yn), reduction="none")).mean()


@pytest.mark.parametrize("window", [[9, 9, 3, 1, 4], [2, 7, 2, 7, 2], [9, 9, 9, 9, 5], [1, 2, 3, 4, 5]])
def test_twin_ties_and_relu_follow_torch(window):
    """windows with two (and four) padding positions and with a repeated item: equal sub-windows tie exactly; the bias of
    some filters is set so that the best pre-activation is exactly zero (relu'(0) = 0)"""
    import torch
    rng = np.random.default_rng(5)
    nU, nI, e, L, nv, nh = 3, 9, 8, 5, 2, 6
    raw = T.random_params(rng, nU, nI, e, L, nv, nh)
    # integer-valued rows and filters: every pre-activation is exact, so ties and zeros are exact in both programs
    for k in raw:
        if k.startswith("conv_h_weight") or k == "item_embeddings":
            raw[k] = np.round(raw[k] * 4).astype(np.float32)
    seq = torch.tensor([window, window[::-1]])
    u, pos, neg = torch.tensor([0, 2]), torch.tensor([[1, 2], [3, 1]]), torch.tensor([[4, 5], [5, 0]])
    for i in range(L):
        raw[f"conv_h_bias_{i}"] = (np.round(raw[f"conv_h_bias_{i}"] * 8) / 8).astype(np.float32)
    _, a, _ = T.forward_x(T.to_torch(raw, requires_grad=False), u, seq, return_parts=True)
    for i in range(L):                                     # filter 0 of every height: instance 0's best pre-activation is exactly 0
        raw[f"conv_h_bias_{i}"][0] -= np.float32(a[i][0, 0].max().item())
    Pa, Pb = T.to_torch(raw), T.to_torch(raw)
    _, a, _ = T.forward_x(Pa, u, seq, return_parts=True)
    assert all(float(a[i][0, 0].detach().max()) == 0.0 for i in range(L))
    if len(set(window)) < L:                               # at least one pool has an exact tie at its maximum
        ties = sum(int(((t == t.max(-1, keepdim=True).values).sum(-1) > 1).sum()) for t in a)
        assert ties > 0
    la = T.step_losses(Pa, u, seq, pos, neg)[2]
    lb = _torch_ops_loss(Pb, u, seq, pos, neg)
    la.backward()
    lb.backward()
    assert abs(la.item() - lb.item()) < 1e-12
    for k in Pa:
        ga, gb = Pa[k].grad, Pb[k].grad
        assert float((ga - gb).abs().max()) <= 1e-12 * max(1.0, float(gb.abs().max())), k


def test_registry_finds_caser_with_reference_defaults():
    from skrec import ModelRegistry
    reg = ModelRegistry()
    assert reg.load_skrec_model("Caser") is True
    model_class, config_class = reg.get_model("Caser")
    assert model_class.__name__ == "Caser" and config_class.__name__ == "CaserConfig"
    cfg = config_class()
    want = dict(lr=1e-3, l2_reg=1e-6, embed_size=64, seq_L=5, seq_T=3, nv=4, nh=16, dropout=0.5, batch_size=1024, epochs=500,
                early_stop=100)
    for k, v in want.items():
        got = getattr(cfg, k)
        assert got == v and type(got) is type(v), (k, got, v)
    cfg._validate()
    for bad in (dict(l2_reg=-1.0), dict(lr=1), dict(seq_L=0), dict(seq_T=0), dict(seq_L=2.0), dict(embed_size=0), dict(nv=0),
                dict(nh=0), dict(nh=1.5), dict(dropout=1), dict(batch_size=0), dict(epochs=-1), dict(early_stop=1.5)):
        with pytest.raises(AssertionError):
            config_class(**bad)._validate()


@pytest.mark.parametrize("kw,exc,match", [
    (dict(embed_size=65), NotImplementedError, "embed_size <= 64"), (dict(seq_L=9), ValueError, "seq_L <= 8"),
    (dict(seq_T=17), ValueError, "seq_T <= 16"), (dict(nv=9), ValueError, "nv <= 8"), (dict(nh=33), ValueError, "nh <= 32"),
    (dict(batch_size=2049), ValueError, "batch_size <= 2048"), (dict(dropout=1.0), ValueError, "dropout < 1")])
def test_limits_are_refused_by_name(kw, exc, match):
    from skrec.recommender.Caser import Caser, CaserConfig
    m = Caser.__new__(Caser)
    m.config = CaserConfig(**kw)
    with pytest.raises(exc, match=match):
        m._check_limits(1)
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.config = CaserConfig()
        m._check_limits(2)
    m._check_limits(1)


def test_initialisation_has_the_reference_bits(golden):
    import random
    import torch
    from skrec.recommender.Caser import _init_tables
    g = golden("golden_caser")
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)
    nu, ni = g["user_embeddings0"].shape[0], g["item_embeddings0"].shape[0]
    t = _init_tables(nu, ni, 64, 5, 4, 16)
    assert set(t) == set(T.param_names(5))
    for k, v in t.items():
        assert v.shape == g[k + "0"].shape and np.array_equal(v.numpy(), g[k + "0"]), k
    assert ni == 97 and g["item_embeddings0"][96].any() and g["W2"+ "0"][96].any()      # the padding item: an ordinary row


@pytest.mark.parametrize("e,L,nv,nh", [(64, 5, 4, 16), (16, 5, 4, 16), (40, 8, 8, 32), (7, 1, 1, 1)])
def test_parameter_views_have_the_reference_shapes(e, L, nv, nh):
    import torch
    from skrec import _hip
    from skrec.recommender.Caser import _Layout, _init_tables, pack_parameters, parameter_views
    torch.manual_seed(3)
    nu, ni = 11, 70
    t = _init_tables(nu, ni, e, L, nv, nh)
    with torch.no_grad():
        t["b2"].normal_()
    lay = _Layout(nu, ni, L, nv, nh)
    assert lay.ns == _hip.caser_shared_floats(L, nv, nh) == T.shared_offsets(L, nv, nh)["total"]
    assert all(o % 64 == 0 for o in (lay.U, lay.E, lay.W2, lay.b2, lay.shared, lay.total, lay.s_bv, lay.s_wh, lay.s_bh, lay.s_w1, lay.s_b1))
    flat = pack_parameters(t, lay, e)
    # the shared block as the twin's own packer lays it out (written from the header, independently)
    assert np.array_equal(flat[lay.shared:].numpy(), T.shared_block({k: v.numpy() for k, v in t.items()}, e, L, nv, nh))
    assert np.array_equal(flat[lay.W2:lay.b2].view(ni, 128).numpy(), T.w2_rows(t["W2"].numpy(), e))
    v = parameter_views(flat, lay, e)
    F = nv * e + nh * L
    want = {"user_embeddings": (nu, e), "item_embeddings": (ni, e), "conv_v_weight": (nv, 1, L, 1), "conv_v_bias": (nv,),
            "fc1_weight": (e, F), "fc1_bias": (e,), "W2": (ni, 2 * e), "b2": (ni, 1)}
    for i in range(L):
        want[f"conv_h_weight_{i}"], want[f"conv_h_bias_{i}"] = (nh, 1, i + 1, e), (nh,)
    assert set(v) == set(want)
    for k, shape in want.items():
        assert tuple(v[k].shape) == shape, k
        assert torch.equal(v[k], t[k]), k
    copies = {"fc1_weight", "W2"} if e < 64 else set()
    for k in v:                                            # views: a write through them lands in the flat buffer
        is_view = v[k].untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        assert is_view == (k not in copies), k
    # what the views do not cover is zero
    back, rest = T.unpack_shared(flat[lay.shared:].numpy(), e, L, nv, nh)
    assert not rest.any()
    for k, a in back.items():
        assert np.array_equal(a, t[k].numpy()), k


def test_caser_symbols_are_declared_exported_and_bound():
    from skrec import _hip
    from test_abi import _declared
    declared = _declared()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    L = _hip.lib()
    for name in ("skr_caser_workspace", "skr_caser_step", "skr_caser_step_timed", "skr_caser_queries"):
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _hip.SIGNATURES and getattr(L, name).argtypes is not None, name
    assert len(_hip.SIGNATURES["skr_caser_step_timed"][1]) == len(_hip.SIGNATURES["skr_caser_step"][1]) + 1
    assert _hip.caser_shared_floats(5, 4, 16) == 128 + 64 * 240 + 128 + 64 * 384 + 64
    assert _hip.caser_fp(8, 8, 32) == 768 and _hip.caser_rows(8, 32) == 1152
    assert L.skr_caser_workspace(1024, 5, 4, 16) > 2 * 1024 * 384 * 4
    for bad in ((0, 5, 4, 16), (2049, 5, 4, 16), (8, 9, 4, 16), (8, 5, 9, 16), (8, 5, 4, 33), (8, 0, 4, 16)):
        assert L.skr_caser_workspace(*bad) == 0


def _err(L):
    return L.skr_last_error().decode()


def test_caser_entry_points_reject_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    b = (ctypes.c_float * 64)()

    def step(tabs=(b,) * 9, n=4, nu=2, nr=3, pad=2, dim=64, width=64, sl=5, stt=3, nv=4, nh=16, rate=0.5, outs=(b,) * 6, wb=1 << 30,
             slots=1, timed=False):
        fn = L.skr_caser_step_timed if timed else L.skr_caser_step
        extra = (None,) if timed else ()
        return fn(*tabs, n, nu, nr, pad, dim, width, sl, stt, nv, nh, rate, None, None, 1, 1, *outs, wb, b, slots, None, *extra)
    assert step(tabs=(None,) + (b,) * 8) == -1 and "NULL" in _err(L)
    assert step(outs=(b,) * 5 + (None,)) == -1 and "NULL" in _err(L)            # the workspace
    assert step(n=-1) == -1 and "n <= 2048" in _err(L)
    assert step(n=2049) == -1 and "n <= 2048" in _err(L)
    assert step(pad=3) == -1 and "pad_idx" in _err(L)
    assert step(dim=128) == -1 and "dim" in _err(L)
    assert step(width=65) == -1 and "width" in _err(L)
    assert step(sl=0) == -1 and "seq_L" in _err(L)
    assert step(sl=9) == -1 and "seq_L <= 8" in _err(L)
    assert step(stt=17) == -1 and "seq_T <= 16" in _err(L)
    assert step(nv=9) == -1 and "nv <= 8" in _err(L)
    assert step(nh=33) == -1 and "nh <= 32" in _err(L)
    assert step(rate=1.0) == -1 and "dropout" in _err(L)
    assert step(slots=3) == -1 and "loss_slots" in _err(L)
    assert step(wb=64) == -1 and "skr_caser_workspace" in _err(L)
    assert step(timed=True) == -1 and "NULL" in _err(L)                          # h_ms
    assert step(n=0) == 0

    def queries(tabs=(b, b, b), users=None, n=2, win=b, nu=2, nr=3, pad=-1, dim=64, width=64, sl=5, nv=4, nh=16, work=b, wb=1 << 30,
                out=b):
        return L.skr_caser_queries(*tabs, users, n, win, nu, nr, pad, dim, width, sl, nv, nh, work, wb, out, None)
    assert queries(win=None) == -1 and "NULL" in _err(L)
    assert queries(work=None) == -1 and "NULL" in _err(L)
    assert queries(n=3) == -1 and "user list" in _err(L)
    assert queries(dim=16) == -1 and "dim" in _err(L)
    assert queries(sl=9) == -1 and "seq_L" in _err(L)
    assert queries(nh=0) == -1 and "nh" in _err(L)
    assert queries(wb=1000) == -1 and "64 users" in _err(L)
    assert queries(n=0) == 0
