"""GPU suite of MGCN (csrc/mgcn.hip, skrec/recommender/MGCN.py): the full-table projection forward and backward, the purifier
forward and backward and the dense fuser against the float64 twin (tests/mgcn_twin.py) at the edges of their tiles and row
blocks; ``gradient_step`` against the twin's hand-derived gradient; bit-reproducibility; the golden replay of the reference's
fit() from its recorded batches; fit() through the registry with the learning-rate schedule; the limits.

Tolerances of the kernel-level comparisons: the project's own for FREEDOM's gradients, rtol = 1e-4 and atol = 2e-5 * max|want|
per tensor."""
import numpy as np
import pytest

import mgcn_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = T.SEED
RTOL, ATOL = 1e-4, 2e-5


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, want, what, rtol=RTOL, atol=ATOL):
    want = np.asarray(want, np.float64)
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want)
    print(what, "max abs err", err.max() if err.size else 0.0, "max|want|", scale, "allowed atol", atol * scale)
    assert np.all(err <= atol * scale + rtol * np.abs(want)), (what, float(err.max()), float(scale))


def _pad(a, cols=64):
    out = np.zeros((a.shape[0], cols), np.float32)
    out[:, :a.shape[1]] = a
    return out


def _ld(F):
    return (F + 3) // 4 * 4


def _trs_block(W, b, ld):
    blk = np.zeros(64 * ld + 64, np.float32)
    blk[:64 * ld].reshape(64, ld)[:W.shape[0], :W.shape[1]] = W
    blk[64 * ld:64 * ld + len(b)] = b
    return blk


def _gate_block(W, b):
    return _trs_block(W, b, 64)


def _row_block(n):
    from skrec import _hip
    return int(_hip.lib().skr_mgcn_row_block(n))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the full-table projection, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
def _project_case(I, F, d, seed):
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    rng = np.random.default_rng(seed)
    ld = _ld(F)
    X = rng.standard_normal((I, F)).astype(np.float32)
    W = (rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32)
    b = rng.standard_normal(d).astype(np.float32)
    dF = rng.standard_normal((I, d)).astype(np.float32)
    dX_, dtrs_, dF_ = _dev(_pad(X, ld)), _dev(_trs_block(W, b, ld)), _dev(_pad(dF))
    Y = torch.full((I, 64), 7.0, device="cuda")
    _hip.check(L.skr_mgcn_project(p(dX_), I, F, ld, p(dtrs_), p(Y), st))
    X64, W64, dF64 = X.astype(np.float64), W.astype(np.float64), dF.astype(np.float64)
    Y = Y.cpu().numpy()
    _close(Y[:, :d], X64 @ W64.T + b, f"project I={I} F={F} d={d}")
    assert np.all(Y[:, d:] == 0)
    ws = int(L.skr_mgcn_project_bwd_workspace(I, ld))
    work = torch.full((ws,), 255, dtype=torch.uint8, device="cuda")
    gtrs = torch.full((64 * ld + 64,), 7.0, device="cuda")
    gX = torch.full((I, ld), 7.0, device="cuda")
    _hip.check(L.skr_mgcn_project_bwd(p(dF_), p(dX_), I, F, ld, p(dtrs_), p(gtrs), p(gX), p(work), ws, st))
    gtrs, gX = gtrs.cpu().numpy(), gX.cpu().numpy()
    gW, gb = gtrs[:64 * ld].reshape(64, ld), gtrs[64 * ld:]
    _close(gW[:d, :F], dF64.T @ X64, f"dW I={I} F={F} d={d}")
    _close(gb[:d], dF64.sum(0), f"db I={I} F={F} d={d}")
    _close(gX[:, :F], dF64 @ W64, f"dX I={I} F={F} d={d}")
    assert np.all(gW[d:] == 0) and np.all(gW[:, F:] == 0) and np.all(gb[d:] == 0) and np.all(gX[:, F:] == 0)    # every element written, padding zero


def _project_rows():
    rb = 256                      # skr_mgcn_row_block below 16 385 rows: asserted in the test
    return [1, 15, 16, 17, rb - 1, rb, rb + 1, 2 * rb + 1]


@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("I", _project_rows())
def test_project_and_backward_equal_the_twin(I, d):
    assert _row_block(I) == 256
    for F in (1, 3, 64, 65):
        _project_case(I, F, d, 1000 * I + F)


@pytest.mark.parametrize("d", [64, 20])
def test_project_and_backward_at_the_widest_table(d):
    _project_case(17, 4096, d, 4096)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the purifier and the dense fuser
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("I", [1, 16, 17, 65])
def test_purify_forward_and_backward_equal_the_twin(I, d):
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    rng = np.random.default_rng(7 * I + d)
    F, E, dX, dE0 = (rng.standard_normal((I, d)).astype(np.float32) for _ in range(4))
    Wg, bg = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    F_, E_, gate_, dX_ = _dev(_pad(F)), _dev(_pad(E)), _dev(_gate_block(Wg, bg)), _dev(_pad(dX))
    G = torch.full((I, 64), 7.0, device="cuda")
    X = torch.full((I, 64), 7.0, device="cuda")
    _hip.check(L.skr_mgcn_purify(p(F_), p(E_), p(gate_), I, d, p(G), p(X), st))
    F64, E64, dX64, Wg64 = (a.astype(np.float64) for a in (F, E, dX, Wg))
    g64 = T.sigmoid(F64 @ Wg64.T + bg)
    Gh, Xh = G.cpu().numpy(), X.cpu().numpy()
    _close(Gh[:, :d], g64, "gate")
    _close(Xh[:, :d], E64 * g64, "purified rows")
    assert np.all(Gh[:, d:] == 0) and np.all(Xh[:, d:] == 0)
    ws = int(L.skr_mgcn_purify_bwd_workspace(I))
    work = torch.full((ws,), 255, dtype=torch.uint8, device="cuda")
    dE = _dev(_pad(dE0))
    dF = torch.full((I, 64), 7.0, device="cuda")
    dgate = torch.full((4160,), 7.0, device="cuda")
    _hip.check(L.skr_mgcn_purify_bwd(p(dX_), p(E_), p(G), p(F_), p(gate_), I, p(dE), p(dF), p(dgate), p(work), ws, st))
    dz = dX64 * E64 * g64 * (1 - g64)
    dE, dF, dgate = dE.cpu().numpy(), dF.cpu().numpy(), dgate.cpu().numpy()
    _close(dE[:, :d], dE0.astype(np.float64) + dX64 * g64, "dE (accumulated)")
    _close(dF[:, :d], dz @ Wg64, "dF")
    _close(dgate[:4096].reshape(64, 64)[:d, :d], dz.T @ F64, "dWg")
    _close(dgate[4096:4096 + d], dz.sum(0), "dbg")
    assert np.all(dE[:, d:] == 0) and np.all(dF[:, d:] == 0) and np.all(dgate[4096 + d:] == 0)
    Wpad = dgate[:4096].reshape(64, 64)
    assert np.all(Wpad[d:] == 0) and np.all(Wpad[:, d:] == 0)


def _fuser_params(rng, d):
    P = {}
    for name in ("query_common.0", "gate_image_prefer.0", "gate_text_prefer.0"):
        P[name + ".weight"] = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
        P[name + ".bias"] = rng.standard_normal(d).astype(np.float32)
    P["query_common.2.weight"] = rng.standard_normal((1, d)).astype(np.float32)
    return P


def _fuse_f64(M, Zv, Zt, P):
    """the twin's fuser on handed-in tables"""
    Wc, bc, q = (P[k].astype(np.float64) for k in ("query_common.0.weight", "query_common.0.bias", "query_common.2.weight"))
    h = [np.tanh(Z @ Wc.T + bc) for Z in (Zv, Zt)]
    a = [hh @ q.reshape(-1) for hh in h]
    mx = np.maximum(a[0], a[1])
    e = [np.exp(a[0] - mx), np.exp(a[1] - mx)]
    w = [e[0] / (e[0] + e[1]), e[1] / (e[0] + e[1])]
    c = w[0][:, None] * Zv + w[1][:, None] * Zt
    p = [T.sigmoid(M @ P[k + ".weight"].astype(np.float64).T + P[k + ".bias"]) for k in ("gate_image_prefer.0", "gate_text_prefer.0")]
    side = (p[0] * (Zv - c) + p[1] * (Zt - c) + c) / 3.0
    return M + side, w


@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("n", [1, 16, 17, 65])
def test_fuse_equals_the_twin(n, d):
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    rng = np.random.default_rng(11 * n + d)
    M, Zv, Zt = (rng.standard_normal((n, d)).astype(np.float32) for _ in range(3))
    Zv[n // 2], Zt[n // 2] = 0.0, 0.0            # a user without train items: both modality rows are zero
    P = _fuser_params(rng, d)
    query = np.concatenate([_gate_block(P["query_common.0.weight"], P["query_common.0.bias"]), _pad(P["query_common.2.weight"])[0]])
    out = torch.full((n, 64), 7.0, device="cuda")
    tabs = [_dev(a) for a in (_pad(M), _pad(Zv), _pad(Zt), query, _gate_block(P["gate_image_prefer.0.weight"], P["gate_image_prefer.0.bias"]),
                              _gate_block(P["gate_text_prefer.0.weight"], P["gate_text_prefer.0.bias"]))]      # alive across the launch
    w_dev = torch.full((n, 2), 7.0, device="cuda")
    _hip.check(L.skr_mgcn_fuse(*[p(t) for t in tabs], n, d, p(out), p(w_dev), st))
    want, w = _fuse_f64(M.astype(np.float64), Zv.astype(np.float64), Zt.astype(np.float64), P)
    out = out.cpu().numpy()
    assert np.isfinite(out).all()
    _close(out[:, :d], want, f"fuse n={n} d={d}")
    assert np.all(out[:, d:] == 0)
    # the softmax weights the DEVICE used: a pair of fp32 values of a two-way softmax, within a few ulp of 1 of the twin's
    w_dev = w_dev.cpu().numpy()
    np.testing.assert_allclose(w_dev, np.stack(w, 1), rtol=0, atol=1e-6)
    # the zero row: equal attention logits, w = (0.5, 0.5) exactly on the device too, c = 0, side = 0, out = M exactly
    assert w[0][n // 2] == 0.5 and w[1][n // 2] == 0.5
    assert w_dev[n // 2, 0] == 0.5 and w_dev[n // 2, 1] == 0.5
    assert np.array_equal(out[n // 2, :d], M[n // 2])


# ---------------------------------------------------------------------------------------------------------------------
# 3. gradient_step against the twin
# ---------------------------------------------------------------------------------------------------------------------
def _detached(g, cfg):
    from skrec.recommender.MGCN import MGCN
    nu, ni = int(g["shape"][0]), int(g["shape"][1])
    _seed()
    m = MGCN.detached(nu, ni, dict(cfg), (g["adj_rowptr"], g["adj_cols"]), img=g["image_embedding_weight_0"], txt=g["text_embedding_weight_0"])
    m.load_parameters(T.fixture_params(g, 0))
    return m


def _device_graphs(m):
    """(R, (S_v, S_t)) dense float64 from the model's own arrays: the comparison is of the step, not of the graphs"""
    def dense(csr, shape):
        rp, col, val = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy(), csr.val.cpu().numpy().astype(np.float64)
        A = np.zeros(shape, np.float64)
        A[np.repeat(np.arange(shape[0]), np.diff(rp)), col] = val
        return A
    nu, ni = m.num_users, m.num_items
    return dense(m.adj, (nu, ni)), (dense(m.mm_adj["img"], (ni, ni)), dense(m.mm_adj["txt"], (ni, ni)))


# Where FREEDOM's tolerance is not enough: {case: {tensor: the torch-CPU fp32 evaluation's error as a fraction of the tensor's
# largest element, as measured}}.  query_common.0.bias is, in every case, a sum of hundreds of terms of either sign that cancels
# to 1e-8 or less (first batch: 763 terms, largest element 8.6e-9).  In the one-user case all 37 rows add into one row of
# user_embedding.weight, whose fp32 evaluation is off by 1.1e-5 of its largest element.
WIDENED = {"first batch": {"query_common.0.bias": 2.4e-4}, "n = 1": {"query_common.0.bias": 1.6e-4},
           "one user": {"query_common.0.bias": 1.2e-4, "user_embedding.weight": 1.1e-5},
           "ids out of range": {"query_common.0.bias": 5.4e-4}, "n = 2048": {"query_common.0.bias": 9.8e-4}}


def _compare_step(m, cfg, users, pos, neg, what):
    R, S = _device_graphs(m)
    P = {k: v.cpu().numpy().astype(np.float64) for k, v in m.parameters().items()}
    comps, G = T.gradients_f64(P, R, S, users, pos, neg, cfg)
    loss = m.gradient_step(users, pos, neg).cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    print(what, "loss", loss, "twin", comps)
    # FREEDOM's rtol for the losses.  The InfoNCE component is cl_loss * (lse - <a, b> / tau) summed: two fp32 values of up to
    # 1 / tau = 5 subtracted, so it carries cl_loss * 2 ulp(5) = 0.1 * 2 * 4.8e-7 = 1e-7 whatever its size (at n = 1 it is 0)
    np.testing.assert_allclose(loss[:3], np.array(comps), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(loss[3], sum(comps), rtol=1e-5)
    # The project's tolerance for FREEDOM's gradients (rtol 1e-4, atol 2e-5 max|want|) for every tensor but those of WIDENED:
    # there, 4 x the error of a torch-CPU fp32 evaluation of the same gradient against the twin on the same inputs
    # (T.gradients_f32_torch, computed here; never the device's own output) where that is more.
    G32 = T.gradients_f32_torch(P, R, S, users, pos, neg, cfg)
    for name in T.NAMES:
        want = np.asarray(G[name], np.float64)
        err32, scale = float(np.abs(G32[name] - want).max()), float(np.abs(want).max())
        err = np.abs(got[name].astype(np.float64) - want)
        print(f"{what}: {name}: max abs err {err.max():.3e}, max|want| {scale:.3e}, fp32-CPU err {err32:.3e}")
        atol = max(ATOL * scale, 4 * err32) if name in WIDENED.get(what, ()) else ATOL * scale
        assert np.all(err <= atol + RTOL * np.abs(want)), (what, name, float(err.max()), scale, err32)
    return loss, got


@pytest.fixture(scope="module")
def tiny_model(golden):
    g = golden("golden_mgcn")
    cfg = T.fixture_config(g)
    return g, cfg, _detached(g, cfg)


def test_gradient_step_on_the_first_batch(tiny_model):
    g, cfg, m = tiny_model
    st = T.fixture_steps(g)[0]
    _compare_step(m, cfg, st["users"], st["pos"], st["neg"], "first batch")
    # the padding of every block of the gradient buffer is exactly zero
    nu, ni = m.num_users, m.num_items
    for key in ("img", "txt"):
        F, ld = m.feat_dim[key], m.feat_ld[key]
        trs, tab = m._blocks(key, True)
        assert (tab.view(ni, ld)[:, F:] == 0).all() and (trs[:64 * ld].view(64, ld)[:, F:] == 0).all()


def test_gradient_step_on_one_row(tiny_model):
    g, cfg, m = tiny_model
    _compare_step(m, cfg, np.array([5]), np.array([7]), np.array([50]), "n = 1")


def test_gradient_step_on_one_user_with_equal_items(tiny_model):
    """every row names user 3; one row has pos == neg: the ordered adds, and an InfoNCE over the users with n equal columns"""
    g, cfg, m = tiny_model
    rng = np.random.default_rng(3)
    n = 37
    pos, neg = rng.integers(0, 96, n), rng.integers(0, 96, n)
    neg[11] = pos[11]
    pos[20] = pos[4]
    _compare_step(m, cfg, np.full(n, 3), pos, neg, "one user")


def test_gradient_step_ignores_rows_out_of_range(tiny_model):
    g, cfg, m = tiny_model
    st = T.fixture_steps(g)[1]
    users, pos, neg = st["users"][:70].copy(), st["pos"][:70].copy(), st["neg"][:70].copy()
    users[3], pos[17], neg[40], users[69] = 64, -1, 96, -5
    _compare_step(m, cfg, users, pos, neg, "ids out of range")


def test_gradient_step_on_a_full_batch():
    """n = 2048 on a seeded random 2100 x 2100 graph with F = 8"""
    from skrec.recommender.MGCN import MGCN
    rng = np.random.default_rng(2100)
    nu = ni = 2100
    deg = rng.integers(1, 20, nu)
    items = np.concatenate([np.sort(rng.choice(ni, k, replace=False)) for k in deg]).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    cfg = dict(lr=1e-2, reg=1e-2, cl_loss=0.1, n_ui_layers=2, n_layers=2, knn_k=10, batch_size=2048)
    _seed()
    m = MGCN.detached(nu, ni, cfg, (rowptr, items), img=rng.standard_normal((ni, 8)).astype(np.float32),
                      txt=rng.standard_normal((ni, 8)).astype(np.float32))
    users, pos, neg = rng.integers(0, nu, 2048), rng.integers(0, ni, 2048), rng.integers(0, ni, 2048)
    _compare_step(m, cfg, users, pos, neg, "n = 2048")
    with pytest.raises(NotImplementedError, match="2048"):
        m.gradient_step(np.zeros(2049, np.int32), np.zeros(2049, np.int32), np.zeros(2049, np.int32))


def test_gradient_step_is_bit_reproducible(tiny_model):
    import torch
    g, cfg, m = tiny_model
    st = T.fixture_steps(g)[2]
    l1 = m.gradient_step(st["users"], st["pos"], st["neg"]).clone()
    g1 = m._grad.clone()
    m._grad.fill_(3.0)            # every element is written again
    m._work.fill_(255)
    l2 = m.gradient_step(st["users"], st["pos"], st["neg"])
    assert torch.equal(l1, l2) and torch.equal(g1, m._grad)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the golden replay, fit()
# ---------------------------------------------------------------------------------------------------------------------
def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="MGCN", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED, sampler_mode="exact")


def _write_features(tiny_dir, g):
    import os
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), features=g["image_embedding_weight_0"])
    np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), features=g["text_embedding_weight_0"])


class _Recorded(object):
    """the reference's evaluator contract on recorded scores: predict() -> ndarray (the generic path)"""

    def __init__(self, users, scores):
        self.row = {int(u): r for r, u in enumerate(users)}
        self.scores = scores

    def predict(self, users):
        return self.scores[[self.row[int(u)] for u in users]]


def test_replays_reference(golden, tiny_dir, monkeypatch, tmp_path):
    """The reference's recorded run, step by step, with test_gpu_freedom.py's multiples of the fixture's own deviations.

    The tightest tensor is gate_v.0.weight: 6 x f64_dev_params = 1.58e-6, and its element [8][31] has a first gradient of
    6.3014e-8, beside Adam's eps, where the first update has a slope of lr eps / (|g| + eps)^2 = 1.9e4 in g: the bound asks for
    that gradient to within about 8e-11, which is what an fp32 evaluation of it is off by in the root mean square over the
    tensor (the device 7.8e-11, torch-CPU fp32 8.9e-11; the device's own graph values, within 1.2e-7 of the reference's, move
    it by 5.0e-11).  With fp32 accumulators in the products the device was off by 1.07e-10 there and the tensor ended 2.07e-6
    from the reference; with the float64 accumulators of csrc/mgcn.hip it is off by 4.3e-11 and ends 8.7e-7 away."""
    from skrec.recommender.MGCN import MGCN
    monkeypatch.chdir(tmp_path)
    g = golden("golden_mgcn")
    cfg = T.fixture_config(g)
    _write_features(tiny_dir, g)
    _seed()
    m = MGCN(_run_config(tiny_dir), dict(cfg))
    assert (m.num_users, m.num_items) == (64, 96) and m.feat_dim == {"img": 100, "txt": 37}
    P0 = m.parameters()
    want0 = T.fixture_params(g, 0)
    assert list(P0) == list(want0)
    for name, want in want0.items():
        assert np.array_equal(P0[name].cpu().numpy(), want), name        # same init, same seed
    # the graphs against the twin's, within 4 x f64_dev_graph (floor: one fp32 ulp of the largest value)
    dev_g = g["f64_dev_graph"]
    assert np.array_equal(m.adj.col.cpu().numpy(), g["adj_cols"])
    val64 = T.norm_adj_values(g["adj_rowptr"], g["adj_cols"], 96)
    tol = max(4 * dev_g[0], float(np.spacing(np.float32(val64.max()))))
    print("adjacency max diff", np.abs(m.adj.val.cpu().numpy() - val64).max(), "allowed", tol)
    assert np.abs(m.adj.val.cpu().numpy() - val64).max() <= tol
    for k, (key, name) in enumerate((("img", "image"), ("txt", "text"))):
        ids, sims = m.knn[key]
        ids = ids.cpu().numpy()
        assert np.array_equal(np.sort(ids, 1), np.sort(g[name + "_knn_ids"], 1)), name          # the reference's neighbour sets
        ids64, sims64 = T.knn_f64(g[name + "_embedding_weight_0"], 10)
        want = T.dense_graph(ids64, T.weighted_graph_values(ids64, sims64))
        S = m.mm_adj[key]
        got = np.zeros((96, 96), np.float64)
        got[np.repeat(np.arange(96), np.diff(S.rowptr.cpu().numpy())), S.col.cpu().numpy()] = S.val.cpu().numpy()
        tol = max(4 * dev_g[1 + k], float(np.spacing(np.float32(want.max()))))
        print(name, "graph max diff", np.abs(got - want).max(), "allowed", tol)
        assert np.abs(got - want).max() <= tol
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    steps = T.fixture_steps(g)
    assert len(steps) == 9
    losses, n_eval = [], 0
    for s, st in enumerate(steps):
        if s % 3 == 0:
            assert m.set_epoch(s // 3) == T.schedule_lr(cfg, s // 3)
        losses.append(m.train_step(st["users"], st["pos"], st["neg"]).cpu().numpy())
        if (s + 1) % 3:
            continue
        report = np.array(list(m.evaluate().values()), np.float32)
        pred = m.predict(test_users)
        ref = g["pred"][n_eval]
        print("evaluation", n_eval, "max score diff", np.abs(pred - ref).max(), "allowed", 6 * dev_s[n_eval])
        assert np.abs(pred - ref).max() <= 6 * dev_s[n_eval]
        rows, _, n = ev.per_user_rows(m, test_users)
        rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, ref), test_users)
        ok = ~np.isin(test_users, g["close_ids"][n_eval])
        print("near-tie users left out", int((~ok).sum()))
        assert n == 63 and (~ok).sum() == g["close_users"][n_eval]
        assert np.array_equal(rows[ok], rows_ref[ok])
        np.testing.assert_allclose(rows[ok].mean(0), rows_ref[ok].mean(0), rtol=1e-5, atol=0)
        if ok.all():
            np.testing.assert_allclose(report, g["reports"][n_eval], rtol=1e-5, atol=0, err_msg=str(g["names"]))
        n_eval += 1
    assert n_eval == 3
    losses = np.stack(losses)
    print("loss", losses[:, 3], "golden", g["loss"], "largest relative difference", np.abs(losses[:, 3] / g["loss"] - 1).max())
    np.testing.assert_allclose(losses[:, 3], g["loss"], rtol=1e-5)
    P1 = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    final = T.fixture_params(g, 1)
    missed = []
    for k, name in enumerate(T.NAMES):        # every tensor is measured before the assertion
        diff = np.abs(P1[name] - final[name]).max()
        print(name, "max abs diff", diff, "allowed", 6 * dev_p[k])
        if not diff <= 6 * dev_p[k]:
            missed.append((name, float(diff), float(6 * dev_p[k])))
    assert not missed, missed


def test_fit_follows_the_schedule(golden, tiny_dir, monkeypatch, tmp_path):
    """fit() on the tiny set as run_skrec.py starts it -- the class from the registry, the run config, the model config"""
    import torch
    from skrec.utils.registry import ModelRegistry
    monkeypatch.chdir(tmp_path)
    g = golden("golden_mgcn")
    cfg = T.fixture_config(g)
    _write_features(tiny_dir, g)
    registry = ModelRegistry()
    assert registry.load_skrec_model("MGCN")
    model_class, config_class = registry.get_model("MGCN")
    _seed()
    m = model_class(_run_config(tiny_dir), dict(cfg))
    assert isinstance(m.config, config_class)
    lrs, orig_step = [], m.optimizer.step

    def step():
        lrs.append(m.optimizer.lr)
        orig_step()
    m.optimizer.step = step
    first = None
    orig_eval = m.evaluate

    def evaluate(tu=None):
        nonlocal first
        if first is None:
            first = torch.stack(m.step_losses).cpu().numpy()
        return orig_eval(tu)
    m.evaluate = evaluate
    best = m.fit()
    assert np.isfinite(np.array(list(best.values()))).all()
    assert lrs == [T.schedule_lr(cfg, e) for e in range(3) for _ in range(3)] and lrs[-1] == 1e-2 * 0.25
    last = torch.stack(m.step_losses).cpu().numpy()
    assert np.isfinite(first).all() and np.isfinite(last).all() and last[:, 3].mean() < first[:, 3].mean()
