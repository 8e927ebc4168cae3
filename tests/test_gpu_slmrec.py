"""GPU suite of SLMRec (csrc/slmrec.hip, skrec/recommender/SLMRec.py): ``gradient_step`` against the float64 twin's hand-derived
gradient (tests/slmrec_twin.py) over the batch sizes, widths, depths and feature widths at which the kernels take another path;
the edge batches; logits of +-200; bit-reproducibility; the untouched g_a_iva; the row-local fusion and the weight-only
projection backward; the golden replay of the reference's fit() from its recorded batches; fit() through the registry; the
ranking on the pre-update fusion weights.

Tolerances of the step: the project's own from test_gpu_mgcn.py, rtol = 1e-4 and atol = 2e-5 * max|want| per gradient tensor,
rtol = 1e-5 for the loss components.  Two tensors get another absolute bound in EVERY case: g_v_iv.bias and g_t_ivat.bias, whose
gradient is zero in exact arithmetic (slmrec_twin.NOISE_DRIVEN says why) -- the twin's value is 1e-17 and max|want| gives no
scale.  What an fp32 evaluation leaves there is the rounding of a column sum over n rows whose terms cancel.  Their bound is
atol = 2e-5 times the largest element of the SAME KIND of sum on the other side of the same term, whose terms do not cancel
(g_i_iv.bias for g_v_iv.bias, g_iva_ivat.bias for g_t_ivat.bias: the same n, the same factor ssl_alpha / (ssl_temp n)), or, as
test_gpu_mgcn.py's WIDENED set has it, 4 x the error of a torch-CPU fp32 evaluation of the same gradient on the same inputs,
measured in the test (never the device's own output), where that is more."""
import ctypes

import numpy as np
import pytest

import slmrec_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = T.SEED
RTOL, ATOL = 1e-4, 2e-5
WIDENED = {"g_v_iv.bias": "g_i_iv.bias", "g_t_ivat.bias": "g_iva_ivat.bias"}
assert tuple(WIDENED) == T.NOISE_DRIVEN


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad(a, cols=64):
    out = np.zeros((a.shape[0], cols), np.float32)
    out[:, :a.shape[1]] = a
    return out


def _graph(rng, nu, ni, empty_user=None, empty_item=None):
    """a seeded random bipartite graph as (rowptr, items); ``empty_user`` has no entry, ``empty_item`` appears in no row"""
    rows = []
    for u in range(nu):
        k = 0 if u == empty_user else int(rng.integers(1, 12))
        c = np.sort(rng.choice(ni, k, replace=False))
        rows.append(c[c != empty_item] if empty_item is not None else c)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32)


def _model(nu, ni, rowptr, items, d=64, L=2, Fv=9, Ft=5, seed=0, **kw):
    from skrec.recommender.SLMRec import SLMRec
    rng = np.random.default_rng(seed)
    cfg = dict(lr=1e-2, ssl_alpha=0.5, layer_num=L, rec_dim=d, batch_size=2048, **kw)
    _seed()
    m = SLMRec.detached(nu, ni, cfg, (rowptr, items), img=rng.standard_normal((ni, Fv)).astype(np.float32),
                        txt=rng.standard_normal((ni, Ft)).astype(np.float32))
    # biases away from nn.Linear's small draws, so that a dropped or misplaced bias shows
    P = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    for k in P:
        if k.endswith(".bias"):
            P[k] = (rng.standard_normal(P[k].shape) * 0.1).astype(np.float32)
    m.load_parameters(P)
    return m


def _twin_inputs(m):
    """(P, R, V, T, cfg) in float64 from the model's own arrays: the comparison is of the step, not of the graph"""
    nu, ni = m.num_users, m.num_items
    rp, col, val = m.adj.rowptr.cpu().numpy(), m.adj.col.cpu().numpy(), m.adj.val.cpu().numpy().astype(np.float64)
    R = np.zeros((nu, ni), np.float64)
    R[np.repeat(np.arange(nu), np.diff(rp)), col] = val
    V, Tt = (m.feat[k][:, :m.feat_dim[k]].cpu().numpy().astype(np.float64) for k in ("img", "txt"))
    P = {k: v.cpu().numpy().astype(np.float64) for k, v in m.parameters().items()}
    c = m.config
    return P, R, V, Tt, dict(lr=c.lr, layer_num=c.layer_num, ssl_alpha=c.ssl_alpha, ssl_temp=c.ssl_temp, temp=c.temp)


def _compare_step(m, users, pos, what, floor=None):
    """``floor`` ({name: a gradient}): a batch at which exact cancellation leaves some gradients zero takes each tensor's scale
    from max|want| or from that tensor's gradient at a batch without the cancellation, whichever is more"""
    P, R, V, Tt, cfg = _twin_inputs(m)
    comps, G, _ = T.gradients_f64(P, R, V, Tt, users, pos, cfg)
    loss = m.gradient_step(users, pos).cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    print(what, "loss", loss, "twin", comps)
    assert np.isfinite(loss).all()
    np.testing.assert_allclose(loss[:3], np.array(comps), rtol=1e-5, atol=0)
    np.testing.assert_allclose(loss[3], sum(comps), rtol=1e-5, atol=0)
    _, G32 = T.gradients_torch(P, R, V, Tt, users, pos, cfg, "float32")
    assert set(got) == set(T.TRAINED)
    for name in T.TRAINED:            # every tensor is measured before the assertion
        want = np.asarray(G[name], np.float64)
        err32, scale = float(np.abs(G32[name] - want).max()), float(np.abs(G[WIDENED.get(name, name)]).max())
        if floor is not None:
            scale = max(scale, float(np.abs(floor[WIDENED.get(name, name)]).max()))
        assert np.isfinite(got[name]).all(), name
        err = np.abs(got[name].astype(np.float64) - want)
        print(f"{what}: {name}: max abs err {err.max():.3e}, scale {scale:.3e}, fp32-CPU err {err32:.3e}")
        atol = max(ATOL * scale, 4 * err32) if name in WIDENED else ATOL * scale
        assert np.all(err <= atol + RTOL * np.abs(want)), (what, name, float(err.max()), scale, err32)
    return loss, got


def _padding_is_zero(m):
    """beyond dim, beyond the feature width and beyond d // 2 every element of the gradient buffer is exactly zero"""
    d, nu, ni = m.config.rec_dim, m.num_users, m.num_items
    assert (m._grad[:(nu + ni) * 64].view(-1, 64)[:, d:] == 0).all()
    for key, name, _ in (("img", "v_dense", 0), ("txt", "t_dense", 0)):
        F, ld = m.feat_dim[key], m.feat_ld[key]
        b = m._block(name, True)
        W = b[:64 * ld].view(64, ld)
        assert (W[d:] == 0).all() and (W[:, F:] == 0).all() and (b[64 * ld + d:] == 0).all()
    for name in ("embedding_item_after_GCN", "embedding_user_after_GCN"):
        b = m._block(name, True)
        W = b[:64 * 192].view(64, 3, 64)
        assert (W[d:] == 0).all() and (W[:, :, d:] == 0).all() and (b[64 * 192 + d:] == 0).all()
    for name in ("g_i_iv", "g_v_iv", "g_iv_iva", "g_iva_ivat", "g_t_ivat"):
        do = d // 2 if name in ("g_iva_ivat", "g_t_ivat") else d
        b = m._block(name, True)
        W = b[:4096].view(64, 64)
        assert (W[do:] == 0).all() and (W[:, d:] == 0).all() and (b[4096 + do:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 1. gradient_step against the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """150 users x 170 items, d = 64, L = 2; user 7 has no interaction, item 11 none"""
    rng = np.random.default_rng(150)
    rowptr, items = _graph(rng, 150, 170, empty_user=7, empty_item=11)
    return _model(150, 170, rowptr, items, seed=150)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 251])
def test_step_equals_the_twin_over_batch_sizes(small, n):
    """below, at and above one 16-row tile; 251: four 64-row workgroups, the last ragged"""
    rng = np.random.default_rng(n)
    _compare_step(small, rng.integers(0, 150, n), rng.integers(0, 170, n), f"n = {n}")
    _padding_is_zero(small)


def test_step_equals_the_twin_on_a_full_batch():
    """n = 2048 on a seeded random 2100 x 2100 graph: 8 row blocks of the weight gradients' reductions, 32 column tiles"""
    rng = np.random.default_rng(2100)
    rowptr, items = _graph(rng, 2100, 2100)
    m = _model(2100, 2100, rowptr, items, seed=2100)
    _compare_step(m, rng.integers(0, 2100, 2048), rng.integers(0, 2100, 2048), "n = 2048")
    with pytest.raises(NotImplementedError, match="2048"):
        m.gradient_step(np.zeros(2049, np.int32), np.zeros(2049, np.int32))


@pytest.mark.parametrize("L", [0, 1, 4])
@pytest.mark.parametrize("d", [64, 50, 37, 32])
def test_step_equals_the_twin_over_widths_and_depths(d, L):
    """d // 2 = 32, 25, 18, 16: one not a multiple of 4, one from an odd d; L = 0 takes the copies instead of the plan runs"""
    rng = np.random.default_rng(100 * d + L)
    rowptr, items = _graph(rng, 90, 110)
    m = _model(90, 110, rowptr, items, d=d, L=L, seed=d + L)
    _compare_step(m, rng.integers(0, 90, 77), rng.integers(0, 110, 77), f"d = {d}, L = {L}")
    _padding_is_zero(m)


@pytest.mark.parametrize("Fv, Ft, ni", [(37, 3, 300), (4096, 1, 40), (130, 4096, 40)])
def test_step_equals_the_twin_over_feature_widths(Fv, Ft, ni):
    """widths that are no multiple of 4 (ld = 40, 4, 132), the widest table, and 300 items: two row blocks of dW's reduction"""
    rng = np.random.default_rng(Fv + Ft)
    rowptr, items = _graph(rng, 60, ni)
    m = _model(60, ni, rowptr, items, d=37, L=1, Fv=Fv, Ft=Ft, seed=Fv)
    _compare_step(m, rng.integers(0, 60, 50), rng.integers(0, ni, 50), f"Fv = {Fv}, Ft = {Ft}")
    _padding_is_zero(m)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
def test_every_row_the_same_user(small):
    rng = np.random.default_rng(3)
    _compare_step(small, np.full(37, 3), rng.integers(0, 170, 37), "one user")


def test_every_row_the_same_item(small):
    """all FAC rows are equal, every logit row is uniform: v_loss = t_loss = log n; the main term's item columns are equal too.
    Every gradient of the two FAC terms, and the main term's with respect to the users' side, is then zero in exact arithmetic
    (P = 1 / n: sum_k P_rk b_k - b_r = 0), and the device leaves the rounding of that cancellation, about 1e-7 of the terms.  The
    tensors' scales are therefore taken from the same users with random items (``floor``): 2e-5 of a gradient of this batch size"""
    rng = np.random.default_rng(4)
    n = 37
    users = rng.integers(0, 150, n)
    P, R, V, Tt, cfg = _twin_inputs(small)
    _, floor, _ = T.gradients_f64(P, R, V, Tt, users, rng.integers(0, 170, n), cfg)
    loss, _ = _compare_step(small, users, np.full(n, 5), "one item", floor=floor)
    np.testing.assert_allclose(loss, np.log(n) * np.array([1.0, 0.5, 0.5, 2.0]), rtol=1e-5)


def test_duplicates_of_both_kinds(small):
    rng = np.random.default_rng(5)
    users, pos = rng.integers(0, 150, 60), rng.integers(0, 170, 60)
    users[10:20], pos[15:30] = users[0], pos[1]          # rows 15 .. 19 are one repeated pair
    users[40], pos[40] = users[41], pos[42]
    _compare_step(small, users, pos, "duplicates")


def test_a_user_and_an_item_without_interactions(small):
    rng = np.random.default_rng(6)
    users, pos = rng.integers(0, 150, 40), rng.integers(0, 170, 40)
    users[[0, 17, 39]], pos[[3, 17]] = 7, 11
    assert small.adj.rowptr[8] == small.adj.rowptr[7] and not (small.adj.col == 11).any()
    _compare_step(small, users, pos, "no interactions")


def test_ids_out_of_range_contribute_nothing(small):
    """the result is that of the batch without those rows, with n = 70 as the divisor"""
    rng = np.random.default_rng(7)
    users, pos = rng.integers(0, 150, 70), rng.integers(0, 170, 70)
    users[3], pos[17], users[40], pos[40], users[69] = 150, -1, -7, 170, 2 ** 31 - 1
    loss, got = _compare_step(small, users, pos, "ids out of range")
    ok = (users >= 0) & (users < 150) & (pos >= 0) & (pos < 170)
    assert ok.sum() == 66
    loss2 = small.gradient_step(users[ok], pos[ok]).cpu().numpy()
    got2 = {k: v.cpu().numpy() for k, v in small.gradients().items()}
    np.testing.assert_allclose(loss, loss2 * 66 / 70, rtol=1e-5)
    for k in T.TRAINED:
        if k not in T.NOISE_DRIVEN:
            scale = np.abs(got[k]).max()
            np.testing.assert_allclose(got[k], got2[k] * np.float32(66 / 70), rtol=RTOL, atol=ATOL * scale, err_msg=k)


def test_an_empty_batch_writes_nothing(small):
    import torch
    from skrec import _hip
    m = small
    loss = torch.full((4,), 7.0, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    a = m._step_args(ids, ids, loss)
    a.n = 0
    m._grad.fill_(3.0)
    before = [t.clone() for t in m.M] + [m._work.clone()]
    _hip.check(_hip.lib().skr_slmrec_step(ctypes.byref(a), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (m._grad == 3.0).all()
    assert all(torch.equal(x, y) for x, y in zip(before, list(m.M) + [m._work]))
    # through the class: a zero loss, a zero gradient
    assert not m.gradient_step(np.zeros(0, np.int32), np.zeros(0, np.int32)).any() and not m._grad.any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. large logits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_logits_of_two_hundred(sign):
    """g_i_iv and g_v_iv scaled until the FAC logits over ssl_temp reach +200 (sign = 1: exp of such a logit overflows fp32, so a
    log-sum-exp that does not take the running maximum off first gives inf) or -200 (sign = -1, g_v_iv negated: such an exp
    underflows to 0); through x the logits of the t term grow too"""
    rng = np.random.default_rng(200)
    rowptr, items = _graph(rng, 90, 110)
    m = _model(90, 110, rowptr, items, seed=200)
    users, pos = rng.integers(0, 90, 100), rng.integers(0, 110, 100)

    def logits(P, R, V, Tt, cfg):
        M = T.forward_f64(P, R, V, Tt, cfg["layer_num"])["M"]
        x, y = T._lin(P, "g_i_iv", M[0][1][pos]), T._lin(P, "g_v_iv", M[1][1][pos])
        return x @ y.T / cfg["ssl_temp"]
    s = np.sqrt(200.0 / logits(*_twin_inputs(m)).max())
    Q = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    for k in ("g_i_iv.weight", "g_i_iv.bias"):
        Q[k] = (Q[k] * s).astype(np.float32)
    for k in ("g_v_iv.weight", "g_v_iv.bias"):
        Q[k] = (Q[k] * (s * sign)).astype(np.float32)
    m.load_parameters(Q)
    lg = logits(*_twin_inputs(m))
    print("FAC logits over ssl_temp: min", lg.min(), "max", lg.max())
    if sign > 0:
        assert 199 < lg.max() < 201 and np.exp(np.float32(lg.max())) == np.inf
    else:
        assert -201 < lg.min() < -199 and np.exp(np.float32(lg.min())) == 0
    _compare_step(m, users, pos, "logits of 200")


# ---------------------------------------------------------------------------------------------------------------------
# 4. reproducibility, the untouched parameters
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(small):
    import torch
    rng = np.random.default_rng(8)
    users, pos = rng.integers(0, 150, 251), rng.integers(0, 170, 251)
    users[5:9] = users[4]
    l1 = small.gradient_step(users, pos).clone()
    g1, M1 = small._grad.clone(), [t.clone() for t in small.M]
    small._grad.fill_(3.0)            # every element is written again
    small._work.fill_(255)
    for t in small.M + small._G + small._ping + small._D:
        t.fill_(float("nan"))
    l2 = small.gradient_step(users, pos)
    assert torch.equal(l1, l2) and torch.equal(g1, small._grad)
    assert all(torch.equal(a, b) for a, b in zip(M1, small.M))


def test_g_a_iva_is_never_stepped():
    import torch
    rng = np.random.default_rng(9)
    rowptr, items = _graph(rng, 90, 110)
    m = _model(90, 110, rowptr, items, seed=9)
    o, size = m._off["g_a_iva"]
    assert o == m._trained and o + size == m._flat.numel() and m._grad.numel() == m._trained
    before, trained = m._flat[o:].clone(), m._flat[:o].clone()
    assert before.abs().max() > 0
    for _ in range(5):
        m.train_step(rng.integers(0, 90, 64), rng.integers(0, 110, 64))
    assert torch.equal(m._flat[o:], before)
    assert not torch.equal(m._flat[:o], trained)
    assert list(m.gradients()) == list(T.TRAINED) and list(m.parameters()) == list(T.NAMES)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the row-local fusion, the weight-only projection backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 37])
@pytest.mark.parametrize("n_rows", [1, 17, 1000])
def test_fuse_equals_float64(n_rows, d):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(13 * n_rows + d)
    M = [rng.standard_normal((n_rows, d)).astype(np.float32) for _ in range(3)]
    W, b = (rng.standard_normal((d, 3, d)) / np.sqrt(3 * d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    blk = np.zeros(64 * 192 + 64, np.float32)
    blk[:64 * 192].reshape(64, 3, 64)[:d, :, :d] = W
    blk[64 * 192:64 * 192 + d] = b
    tabs = [_dev(_pad(a)) for a in M] + [_dev(blk)]
    out = torch.full((n_rows, 64), 7.0, device="cuda")
    _hip.check(_hip.lib().skr_slmrec_fuse(*[_hip.ptr(t) for t in tabs], n_rows, d, _hip.ptr(out), _hip.stream()))
    out = out.cpu().numpy()
    cat, W2 = np.hstack(M).astype(np.float64), W.reshape(d, 3 * d).astype(np.float64)
    want, mass = cat @ W2.T + b, np.abs(cat) @ np.abs(W2).T + np.abs(b)
    err = np.abs(out[:, :d] - want)
    print("fuse", n_rows, d, "max err / mass", (err / mass).max())
    assert np.all(err <= 1e-6 * mass) and np.all(out[:, d:] == 0)


@pytest.mark.parametrize("I, F", [(17, 37), (300, 64), (257, 130), (17, 4096)])
def test_weight_backward_equals_the_full_one_bit_for_bit(I, F):
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    rng = np.random.default_rng(I + F)
    ld = (F + 3) // 4 * 4
    X, dF = _dev(_pad(rng.standard_normal((I, F)).astype(np.float32), ld)), _dev(_pad(rng.standard_normal((I, 50)).astype(np.float32)))
    trs = _dev((rng.standard_normal(64 * ld + 64) * 0.1).astype(np.float32))
    ws = int(L.skr_mgcn_project_bwd_workspace(I, ld))
    work = torch.full((ws,), 255, dtype=torch.uint8, device="cuda")
    full, dX = torch.full((64 * ld + 64,), 7.0, device="cuda"), torch.empty((I, ld), device="cuda")
    _hip.check(L.skr_mgcn_project_bwd(p(dF), p(X), I, F, ld, p(trs), p(full), p(dX), p(work), ws, st))
    work.fill_(255)
    mine = torch.full((64 * ld + 64,), 7.0, device="cuda")
    _hip.check(L.skr_slmrec_project_bwd_w(p(dF), p(X), I, F, ld, p(mine), p(work), ws, st))
    assert torch.equal(full, mine) and not (mine == 7.0).any()
    want = dF.cpu().numpy().astype(np.float64).T @ X.cpu().numpy().astype(np.float64)
    got = mine.cpu().numpy()[:64 * ld].reshape(64, ld)
    assert np.abs(got - want).max() <= ATOL * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the golden replay, fit(), the ranking on the pre-update weights
# ---------------------------------------------------------------------------------------------------------------------
def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="SLMRec", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED, sampler_mode="exact")


def _write_features(tiny_dir, g):
    import os
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), features=g["img"])
    np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), features=g["txt"])


def _given(g):
    import json
    return json.loads(str(g["config_given"]))


class _Recorded(object):
    """the reference's evaluator contract on recorded scores: predict() -> ndarray (the generic path)"""

    def __init__(self, users, scores):
        self.row = {int(u): r for r, u in enumerate(users)}
        self.scores = scores

    def predict(self, users):
        return self.scores[[self.row[int(u)] for u in users]]


def _check_evaluation(m, g, e, report):
    """evaluation ``e`` of a model on the reference's trajectory: raw scores and predict() within 6 x f64_dev_scores; the metric
    rows of the users outside close_ids equal to the reference's; the report at rtol 1e-5 where no near-tie user's row differs"""
    ev = m.evaluator
    test_users = g["test_users"]
    dev_s = g["f64_dev_scores"]
    raw = m.raw_scores(test_users).cpu().numpy()
    print("evaluation", e, "max raw score diff", np.abs(raw - g["raw"][e]).max(), "allowed", 6 * dev_s[e])
    assert np.abs(raw - g["raw"][e]).max() <= 6 * dev_s[e]
    pred = m.predict(test_users)
    assert pred.dtype == np.float32 and np.abs(pred - g["pred"][e]).max() <= 6 * dev_s[e] and pred.min() > 0 and pred.max() < 1
    rows, _, n = ev.per_user_rows(m, test_users)
    rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, g["pred"][e]), test_users)
    ok = ~np.isin(test_users, g["close_ids"][e])
    print("near-tie users left out", int((~ok).sum()))
    assert n == 63 and (~ok).sum() == g["close_users"][e]
    assert np.array_equal(rows[ok], rows_ref[ok])
    np.testing.assert_allclose(rows[ok].mean(0), rows_ref[ok].mean(0), rtol=1e-5, atol=0)
    if np.array_equal(rows, rows_ref):
        np.testing.assert_allclose(report, g["reports"][e], rtol=1e-5, atol=0, err_msg=str(g["names"]))
    return np.array_equal(rows, rows_ref)


def _public_model(g, tiny_dir):
    from skrec.recommender.SLMRec import SLMRec
    _write_features(tiny_dir, g)
    _seed()
    return SLMRec(_run_config(tiny_dir), _given(g))


def test_replays_reference(golden, tiny_dir, monkeypatch, tmp_path):
    """The reference's recorded run, step by step, with test_gpu_mgcn.py's multiples of the fixture's own deviations: 6 x
    f64_dev_params per tensor, 6 x f64_dev_scores on the raw scores, rtol 1e-5 on the losses.  For g_v_iv.bias and g_t_ivat.bias
    the recorded deviation is itself some lr (slmrec_twin.NOISE_DRIVEN): the factor is the same, the bound it gives is wide."""
    monkeypatch.chdir(tmp_path)
    g = golden("golden_slmrec")
    m = _public_model(g, tiny_dir)
    assert (m.num_users, m.num_items) == (64, 96) and m.feat_dim == {"img": 100, "txt": 37}
    P0, want0 = m.parameters(), T.fixture_params(g, 0)
    assert list(P0) == list(want0)
    for name, want in want0.items():
        assert np.array_equal(P0[name].cpu().numpy(), want), name        # same init, same seed
    assert np.array_equal(m.adj.col.cpu().numpy(), g["adj_cols"]) and np.array_equal(m.adj.val.cpu().numpy(), g["adj_val"])
    assert np.array_equal(m.feat["img"][:, :100].cpu().numpy(), g["v_feat"]) and np.array_equal(m.feat["txt"][:, :37].cpu().numpy(), g["t_feat"])
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    assert np.array_equal(np.fromiter(ev.user_pos_test.keys(), dtype=np.int32), g["test_users"])
    steps = T.fixture_steps(g)
    assert len(steps) == 9
    losses, n_eval = [], 0
    for s, st in enumerate(steps):
        if s % 3 == 0:
            assert m.set_epoch(s // 3) == 1e-2
        losses.append(m.train_step(st["users"], st["pos"]).cpu().numpy())
        if (s + 1) % 3 == 0:
            _check_evaluation(m, g, n_eval, np.array(list(m.evaluate().values()), np.float32))
            n_eval += 1
    losses = np.stack(losses)
    print("loss", losses[:, 3], "golden", g["loss"], "largest relative difference", np.abs(losses[:, 3] / g["loss"] - 1).max())
    np.testing.assert_allclose(losses[:, 3], g["loss"], rtol=1e-5)
    P1 = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    final, dev_p = T.fixture_params(g, 1), g["f64_dev_params"]
    missed = []
    for k, name in enumerate(T.NAMES):        # every tensor is measured before the assertion
        diff = np.abs(P1[name] - final[name]).max()
        print(name, "max abs diff", diff, "allowed", 6 * dev_p[k])
        if not diff <= 6 * dev_p[k]:
            missed.append((name, float(diff), float(6 * dev_p[k])))
    assert not missed, missed
    for name in T.UNTRAINED:
        assert np.array_equal(P1[name], final[name])


def test_fit_ends_with_the_recorded_best_report(golden, tiny_dir, monkeypatch, tmp_path):
    """fit() on the tiny set as run_skrec.py starts it -- the class from the registry, the run config, the model config: the
    reference's batches (its losses), its evaluations, its best report"""
    import torch
    from skrec.utils.registry import ModelRegistry
    monkeypatch.chdir(tmp_path)
    g = golden("golden_slmrec")
    _write_features(tiny_dir, g)
    registry = ModelRegistry()
    assert registry.load_skrec_model("SLMRec")
    model_class, config_class = registry.get_model("SLMRec")
    _seed()
    m = model_class(_run_config(tiny_dir), _given(g))
    assert isinstance(m.config, config_class)
    same, losses, orig_eval = [], [], m.evaluate

    def evaluate(tu=None):
        losses.extend(torch.stack(m.step_losses).cpu().numpy()[:, 3])
        r = orig_eval(tu)
        same.append(_check_evaluation(m, g, len(same), np.array(list(r.values()), np.float32)))
        return r
    m.evaluate = evaluate
    best = np.array(list(m.fit().values()), np.float32)
    assert len(same) == 3
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-5)
    e_best = int(np.argmax([dict(zip(g["names"], r))["NDCG@10"] for r in g["reports"]]))
    np.testing.assert_allclose(g["reports"][e_best], g["best"], rtol=0, atol=0)
    # a near-tie user moves a mean over 63 users by at most 1 / 63 per metric; without one that differs the report is the recorded one
    if same[e_best]:
        np.testing.assert_allclose(best, g["best"], rtol=1e-5, atol=0)
    else:
        assert np.abs(best - g["best"]).max() <= g["close_users"][e_best] / 63.0


def test_evaluation_ranks_on_the_weights_before_the_update(golden, tiny_dir, monkeypatch, tmp_path):
    """after three steps the reference's scores are those of the third step's forward: the kept tables and the fusion blocks as
    they were BEFORE the third Adam update.  A second model whose snapshot holds the updated blocks leaves the bound"""
    monkeypatch.chdir(tmp_path)
    g = golden("golden_slmrec")
    models = [_public_model(g, tiny_dir) for _ in range(2)]
    for m in models:
        m.set_epoch(0)
        for st in T.fixture_steps(g)[:3]:
            m.train_step(st["users"], st["pos"])
    good, bad = models
    assert not np.array_equal(bad._fusion_snapshot.cpu().numpy(), bad._fusion.cpu().numpy())
    bad._fusion_snapshot.copy_(bad._fusion)
    ref, bound = g["raw"][0], 6 * g["f64_dev_scores"][0]
    d_good = np.abs(good.raw_scores(g["test_users"]).cpu().numpy() - ref).max()
    d_bad = np.abs(bad.raw_scores(g["test_users"]).cpu().numpy() - ref).max()
    print("pre-update snapshot", d_good, "post-update snapshot", d_bad, "allowed", bound)
    assert d_good <= bound < d_bad


def test_evaluation_before_any_step_is_a_forward_of_the_current_parameters(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    g = golden("golden_slmrec")
    m = _public_model(g, tiny_dir)
    P = {k: v.astype(np.float64) for k, v in T.fixture_params(g, 0).items()}
    V, Tt = T.fixture_features(g)
    want = T.scores_f64(P, T.forward_f64(P, T.fixture_graph(g), V, Tt, 2), g["test_users"])
    got = m.raw_scores(g["test_users"]).cpu().numpy()
    assert np.abs(got - want).max() <= ATOL * np.abs(want).max()
    assert np.isfinite(np.array(list(m.evaluate().values()))).all()
