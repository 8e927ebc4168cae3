"""GPU suite of the wide fused evaluator: skr_eval_fused_topk on rows of 128 / 192 / 256 floats (split_sweep_wide in
csrc/eval_fused.hip), in both split arithmetics, through the C ABI, RankingEvaluator and the models that reach it."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from helpers import random_csr

pytestmark = pytest.mark.gpu

METRICS = ["Precision", "Recall", "MAP", "NDCG", "MRR"]


@pytest.fixture(params=["f16x2", "bf16x3"])
def mode(request, monkeypatch):
    monkeypatch.setenv("SKR_FUSED_MODE", request.param)
    return request.param


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fused_topk(Ut, users, It, bias, rowptr, items, K, dim, pad_rows=0):
    """one call through the C ABI.  pad_rows > 0: the outputs are the middle of a canary-filled buffer of B + 2 pad_rows rows and
    the workspace is followed by a canary; returns (ids, scores, outside_untouched)"""
    import torch
    from skrec import _hip
    assert Ut.shape[1] == dim and It.shape[1] == dim
    ut, it = _dev(Ut), _dev(It)
    bs = _dev(bias) if bias is not None else None
    du = _dev(np.asarray(users, np.int32))
    B = len(users)
    tp = _dev(rowptr) if rowptr is not None else None
    ti = _dev(items if len(items) else np.zeros(1, np.int32)) if rowptr is not None else None
    ids_all = torch.full((B + 2 * pad_rows, K), -7, dtype=torch.int32, device="cuda")
    sc_all = torch.full((B + 2 * pad_rows, K), -123.0, dtype=torch.float32, device="cuda")
    ids, sc = ids_all[pad_rows:pad_rows + B], sc_all[pad_rows:pad_rows + B]
    ws = int(_hip.lib().skr_eval_fused_workspace(B, K))
    tail = 4096 if pad_rows else 0
    work = torch.full((ws + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    _hip.check(_hip.lib().skr_eval_fused_topk(_hip.ptr(ut), _hip.ptr(du), B, _hip.ptr(it), _hip.ptr(bs), It.shape[0], dim,
                                              _hip.ptr(tp), _hip.ptr(ti), K, _hip.ptr(ids), _hip.ptr(sc), _hip.ptr(work), ws,
                                              _hip.stream()))
    torch.cuda.synchronize()
    if not pad_rows:
        return ids.cpu().numpy(), sc.cpu().numpy()
    clean = bool((ids_all[:pad_rows] == -7).all() and (ids_all[pad_rows + B:] == -7).all()
                 and (sc_all[:pad_rows] == -123.0).all() and (sc_all[pad_rows + B:] == -123.0).all()
                 and (work[ws:] == 0xA5).all())
    return ids.cpu().numpy(), sc.cpu().numpy(), clean


def _rejected():
    from skrec import _hip
    n = ctypes.c_int32(-1)
    _hip.check(_hip.lib().skr_eval_fused_rejected(ctypes.byref(n), _hip.stream()))
    return n.value


def _masked_fp64(Ut, users, It, bias, rowptr, items):
    sc = Ut[users].astype(np.float64) @ It.astype(np.float64).T
    if bias is not None:
        sc = sc + bias.astype(np.float64)
    if rowptr is not None:
        for r, u in enumerate(users):
            sc[r, items[rowptr[u]:rowptr[u + 1]]] = -np.inf
    return sc


def _noise(Ut, users, It, bias, dim):
    """the fp32 chain's worst case: dim roundings of 2^-24 each, relative to the largest sum |u v| (+ |bias|) of the case"""
    mag = np.abs(Ut[users].astype(np.float64)) @ np.abs(It.astype(np.float64)).T
    if bias is not None:
        mag = mag + np.abs(bias.astype(np.float64))
    return dim * 2.0 ** -24 * mag.max()


def _reference(Ut, users, It, bias, rowptr, items, K):
    sc = _masked_fp64(Ut, users, It, bias, rowptr, items)
    order = np.argsort(-sc, axis=1, kind="stable")[:, :K + 1]
    top = np.take_along_axis(sc, order, 1)
    return order[:, :K], top[:, :K], -np.diff(top, axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. against float64
# ---------------------------------------------------------------------------------------------------------------------
VS64 = [(1, 40, 5, 128), (17, 17, 9, 128), (33, 49, 7, 128), (65, 1000, 20, 128), (257, 3000, 10, 128),
        (130, 33, 3, 192), (16, 16, 4, 192), (70, 6000, 100, 192),
        (15, 5, 4, 256), (31, 48, 10, 256), (64, 4097, 50, 256), (300, 20011, 128, 256)]


@functools.lru_cache(maxsize=None)
def _vs64_case(B, I, K, dim, with_bias, with_mask, long_row):
    rng = np.random.default_rng(B + I + K + dim)
    nU = B + 17
    Ut = (rng.standard_normal((nU, dim)) * 0.3).astype(np.float32)
    It = (rng.standard_normal((I, dim)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(I) * 0.1).astype(np.float32) if with_bias else None
    users = rng.permutation(nU)[:B].astype(np.int32)
    if long_row:                                     # beyond SPLIT_ROWBUF: the searches run on global memory
        rowptr, items = random_csr(rng, nU, I, 0, long_row)
        lens = np.diff(rowptr)
        if lens.max() < long_row:
            u = int(users[0])
            row = np.sort(rng.choice(I, long_row, replace=False)).astype(np.int32)
            items = np.concatenate([items[:rowptr[u]], row, items[rowptr[u + 1]:]])
            lens[u] = long_row
            rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert np.diff(rowptr).max() == long_row
    elif with_mask:
        rowptr, items = random_csr(rng, nU, I, 0, max(0, min(I - K - 1, 120)))
    else:
        rowptr, items = None, np.zeros(0, np.int32)
    want_ids, want_sc, gaps = _reference(Ut, users, It, bias, rowptr, items, K)
    noise = _noise(Ut, users, It, bias, dim)
    return Ut, It, bias, users, rowptr, items, want_ids, want_sc, gaps, noise


def _check_vs64(B, I, K, dim, with_bias, with_mask, long_row=0):
    Ut, It, bias, users, rowptr, items, want_ids, want_sc, gaps, noise = _vs64_case(B, I, K, dim, with_bias, with_mask, long_row)
    ids, sc = fused_topk(Ut, users, It, bias, rowptr, items, K, dim)
    clear = gaps > noise
    pos_ok = clear[:, 1:] if K == 1 else np.concatenate([clear[:, :1], clear[:, :-1] & clear[:, 1:]], axis=1)[:, :K]
    pos_ok[:, 0] = clear[:, 0]
    set_ok = clear[:, K - 1]                        # the K / K+1 boundary decides the id SET
    print(f"noise {noise:.3e}  comparable positions {pos_ok.mean():.3f}  boundaries {set_ok.mean():.3f}")
    assert pos_ok.mean() > 0.9 and set_ok.mean() > 0.9
    assert np.array_equal(ids[pos_ok], want_ids[pos_ok])
    for r in np.flatnonzero(set_ok):
        assert set(ids[r]) == set(want_ids[r]), r
    np.testing.assert_allclose(np.sort(sc, axis=1), np.sort(want_sc, axis=1), rtol=0, atol=noise)
    for r in range(B):
        assert len(set(ids[r])) == K and ids[r].min() >= 0 and ids[r].max() < I
        assert np.all(np.diff(sc[r]) <= 0)
        if rowptr is not None:
            u = users[r]
            assert not np.isin(ids[r], items[rowptr[u]:rowptr[u + 1]]).any()


@pytest.mark.parametrize("with_bias,with_mask", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("B,I,K,dim", VS64)
def test_wide_topk_vs_fp64(B, I, K, dim, with_bias, with_mask, mode):
    _check_vs64(B, I, K, dim, with_bias, with_mask)


def test_wide_topk_vs_fp64_with_a_train_row_beyond_the_staging_buffer(mode):
    _check_vs64(40, 2000, 10, 128, True, True, long_row=300)


# ---------------------------------------------------------------------------------------------------------------------
# 5. exact on integer scores
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I,K,dim", [(96, 777, 12, 128), (65, 3000, 64, 192), (70, 6000, 100, 256), (130, 9000, 128, 256)])
def test_wide_exact_on_integer_scores(B, I, K, dim, mode):
    """every product and every partial sum is exact in fp32 and in both splits: ids AND score bits equal the oracle's, ties
    included (lower id first)"""
    rng = np.random.default_rng(4 + K + dim)
    Ut = rng.integers(-3, 4, (B, dim)).astype(np.float32)
    It = rng.integers(-3, 4, (I, dim)).astype(np.float32)
    bias = rng.integers(-5, 6, I).astype(np.float32)
    rowptr, items = random_csr(rng, B, I, 0, 100)
    ids, sc = fused_topk(Ut, np.arange(B, dtype=np.int32), It, bias, rowptr, items, K, dim)
    full = Ut @ It.T + bias
    for r in range(B):
        full[r, items[rowptr[r]:rowptr[r + 1]]] = -np.inf
        want = O.topk_ids_lowid(full[r], K)
        assert np.array_equal(ids[r], want), r
        assert np.array_equal(sc[r].view(np.uint32), full[r, want].view(np.uint32)), r


# ---------------------------------------------------------------------------------------------------------------------
# 6. slices are where they belong
# ---------------------------------------------------------------------------------------------------------------------
def _slice_case():
    rng = np.random.default_rng(606)
    B, I, K = 40, 200, 10
    U = (rng.standard_normal((B, 256)) * 0.3).astype(np.float32)
    V = (rng.standard_normal((I, 256)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(I) * 0.1).astype(np.float32)
    rowptr, items = random_csr(rng, B, I, 0, 60)
    return B, I, K, U, V, bias, rowptr, items


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_a_table_living_in_one_slice_ranks_like_its_64_columns(c, mode):
    from gpu_utils import fused_topk as fused_topk_64
    B, I, K, U, V, bias, rowptr, items = _slice_case()
    users = np.arange(B, dtype=np.int32)
    U1, V1 = np.zeros_like(U), np.zeros_like(V)
    U1[:, 64 * c:64 * c + 64] = U[:, 64 * c:64 * c + 64]
    V1[:, 64 * c:64 * c + 64] = V[:, 64 * c:64 * c + 64]
    ids, sc = fused_topk(U1, users, V1, bias, rowptr, items, K, 256)
    U64, V64 = np.ascontiguousarray(U[:, 64 * c:64 * c + 64]), np.ascontiguousarray(V[:, 64 * c:64 * c + 64])
    ids64, sc64 = fused_topk_64(U64, users, V64, bias, rowptr, items, K)
    assert np.array_equal(ids, ids64)
    np.testing.assert_allclose(sc, sc64, rtol=0, atol=_noise(U64, users, V64, bias, 64))


@pytest.mark.parametrize("with_bias", [True, False])
def test_users_and_items_in_different_slices_score_the_bias_alone(with_bias, mode):
    B, I, K, U, V, bias, rowptr, items = _slice_case()
    users = np.arange(B, dtype=np.int32)
    U1, V1 = np.zeros_like(U), np.zeros_like(V)
    U1[:, :64] = U[:, :64]
    V1[:, 64:128] = V[:, 64:128]
    b = bias if with_bias else None
    ids, sc = fused_topk(U1, users, V1, b, rowptr, items, K, 256)
    full = np.tile(bias if with_bias else np.zeros(I, np.float32), (B, 1))
    for r in range(B):
        full[r, items[rowptr[r]:rowptr[r + 1]]] = -np.inf
        want = O.topk_ids_lowid(full[r], K)          # without a bias: the K lowest unmasked ids
        assert np.array_equal(ids[r], want), r
        assert np.array_equal(sc[r], full[r, want]), r


def test_zero_padded_rows_rank_like_their_own_columns(mode):
    B, I, K, U, V, bias, rowptr, items = _slice_case()
    users = np.arange(B, dtype=np.int32)
    U1, V1 = U.copy(), V.copy()
    U1[:, 70:] = 0.0
    V1[:, 70:] = 0.0
    ids, sc = fused_topk(U1, users, V1, bias, rowptr, items, K, 256)
    U70, V70 = U[:, :70], V[:, :70]
    want_ids, want_sc, gaps = _reference(U70, users, V70, bias, rowptr, items, K)
    noise = _noise(U70, users, V70, bias, 70)
    rows = (gaps > noise).all(axis=1)
    assert rows.mean() > 0.9
    assert np.array_equal(ids[rows], want_ids[rows])
    np.testing.assert_allclose(np.sort(sc, axis=1), np.sort(want_sc, axis=1), rtol=0, atol=noise)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the guard at width
# ---------------------------------------------------------------------------------------------------------------------
def _rel_err(sc, ids, U, V, b):
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    exact = np.einsum("bkd,bd->bk", V64[ids], U64)
    denom = np.einsum("bkd,bd->bk", np.abs(V64)[ids], np.abs(U64))
    if b is not None:
        exact, denom = exact + b.astype(np.float64)[ids], denom + np.abs(b.astype(np.float64))[ids]
    return np.abs(sc - exact) / denom


def _fp32_chain(ids, U, V, b):
    """the fp32 chain in ascending k, seeded with the bias: an fp32 product and an fp32 add per column"""
    acc = b[ids].astype(np.float32).copy() if b is not None else np.zeros(ids.shape, np.float32)
    Vg = V[ids]                                      # [B, K, d]
    for k in range(U.shape[1]):
        acc = (acc + Vg[:, :, k] * U[:, k:k + 1]).astype(np.float32)
    return acc


@pytest.mark.parametrize("dim", [128, 256])
def test_f16x2_guard_accepts_wide_tables_of_one_magnitude(dim, monkeypatch):
    monkeypatch.setenv("SKR_FUSED_MODE", "f16x2")
    rng = np.random.default_rng(7 + dim)
    B, I, K = 96, 3000, 20
    for scale in (1e-3, 1.0, 30.0):
        U = (rng.standard_normal((B, dim)) * scale).astype(np.float32)
        V = (rng.standard_normal((I, dim)) * scale).astype(np.float32)
        b = (rng.standard_normal(I) * scale * scale).astype(np.float32)
        ids, sc = fused_topk(U, np.arange(B, dtype=np.int32), V, b, None, np.zeros(0, np.int32), K, dim)
        assert _rejected() == 0
        err = _rel_err(sc, ids, U, V, b).max()
        err32 = _rel_err(_fp32_chain(ids, U, V, b), ids, U, V, b).max()
        print(f"dim {dim} scale {scale}: f16x2 {err:.3e}  fp32 chain {err32:.3e}")
        assert err <= 2.0 * err32, (scale, err, err32)


def test_f16x2_guard_hands_small_wide_rows_to_bf16x3(monkeypatch):
    monkeypatch.setenv("SKR_FUSED_MODE", "f16x2")
    rng = np.random.default_rng(11)
    B, I, K, dim = 300, 3000, 10, 128
    U = (rng.standard_normal((B, dim)) * 0.3).astype(np.float32)
    V = (rng.standard_normal((I, dim)) * 0.3).astype(np.float32)
    users = np.arange(B, dtype=np.int32)
    ids0, sc0 = fused_topk(U, users, V, None, None, np.zeros(0, np.int32), K, dim)
    assert _rejected() == 0
    small = np.sort(rng.permutation(B)[:37])
    U2 = U.copy()
    U2[small] *= np.float32(2.0 ** -22)
    ids, sc = fused_topk(U2, users, V, None, None, np.zeros(0, np.int32), K, dim)
    assert _rejected() == 37
    assert _rel_err(sc[small], ids[small], U2[small], V, None).max() < 4e-7
    want_ids, _, gaps = _reference(U2, users, V, None, None, np.zeros(0, np.int32), K)
    mag = np.abs(U2.astype(np.float64)) @ np.abs(V.astype(np.float64)).T
    clear = (gaps > dim * 2.0 ** -24 * mag.max(axis=1, keepdims=True)).all(axis=1)     # per user: the rows differ by 2^22
    assert clear[small].mean() > 0.5
    assert np.array_equal(ids[clear], want_ids[clear])
    others = np.setdiff1d(users, small)
    assert np.array_equal(ids[others], ids0[others])
    assert np.array_equal(sc[others].view(np.uint32), sc0[others].view(np.uint32))
    V2 = V.copy()
    V2[5, 3] = np.inf
    fused_topk(np.abs(U), users, V2, None, None, np.zeros(0, np.int32), K, dim)
    assert _rejected() == B


# ---------------------------------------------------------------------------------------------------------------------
# 8. determinism and containment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("B", [1, 17, 65])
def test_wide_calls_are_deterministic_and_stay_inside_their_buffers(B, dim, mode):
    rng = np.random.default_rng(B + dim)
    I, K = 1500, 20
    U = (rng.standard_normal((B + 3, dim)) * 0.3).astype(np.float32)
    V = (rng.standard_normal((I, dim)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(I) * 0.1).astype(np.float32)
    users = rng.permutation(B + 3)[:B].astype(np.int32)
    rowptr, items = random_csr(rng, B + 3, I, 0, 150)
    a = fused_topk(U, users, V, bias, rowptr, items, K, dim, pad_rows=5)
    b = fused_topk(U, users, V, bias, rowptr, items, K, dim, pad_rows=5)
    assert a[2] and b[2]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert (a[0] >= 0).all() and (a[0] < I).all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. RankingEvaluator end to end
# ---------------------------------------------------------------------------------------------------------------------
class _Calls(object):
    """skr_eval_fused_topk of the loaded library, wrapped with a record of the widths it was called with"""

    def __init__(self, monkeypatch):
        from skrec import _hip
        self.dims = []
        L = _hip.lib()
        real = L.skr_eval_fused_topk

        def counted(*args):
            self.dims.append(int(args[6]))
            return real(*args)

        class Proxy(object):
            def __getattr__(_, name):
                return counted if name == "skr_eval_fused_topk" else getattr(L, name)
        proxy = Proxy()
        monkeypatch.setattr(_hip, "lib", lambda: proxy)


def _stubs(Ut, It, bias):
    import torch
    dU, dI = torch.from_numpy(Ut).cuda(), torch.from_numpy(It).cuda()
    dB = torch.from_numpy(bias).cuda() if bias is not None else None
    dense = Ut.astype(np.float64) @ It.astype(np.float64).T + (bias.astype(np.float64) if bias is not None else 0.0)

    class Factors(object):
        def predict_factors(self):
            return dU, dI, dB

        def predict(self, users):
            raise AssertionError("the fused route must not ask for dense scores")

    class PredictOnly(object):
        def predict(self, users):
            return dense[np.asarray(users)].astype(np.float32)
    return Factors(), PredictOnly(), dense


@pytest.mark.parametrize("dim", [128, 256])
def test_evaluator_ranks_wide_factors_fused(dim, mode, monkeypatch):
    """seed 56 + dim: float64 alone leaves 2 of the 80 users, at 128 and at 256 columns, with a gap below the noise bound inside
    their top 21 (seeds 1 .. 59 were searched on the reference alone; the cap is 5 % = 4 users)"""
    from skrec.utils.py import RankingEvaluator
    rng = np.random.default_rng(56 + dim)
    nU, nI = 80, 300
    Ut = (rng.standard_normal((nU, dim)) * 0.3).astype(np.float32)
    It = (rng.standard_normal((nI, dim)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(nI) * 0.1).astype(np.float32)
    train = {u: np.sort(rng.choice(nI, rng.integers(1, 30), replace=False)) for u in range(nU)}
    test = {u: rng.choice(nI, rng.integers(1, 6), replace=False) for u in range(nU)}
    fac, gen, dense = _stubs(Ut, It, bias)
    users = np.arange(nU, dtype=np.int32)
    ev = RankingEvaluator(train, test, metric=METRICS, top_k=[5, 10, 20], batch_size=32)
    calls = _Calls(monkeypatch)
    rows_f, _, _ = ev.per_user_rows(fac, users)
    assert calls.dims == [dim]
    rows_g, _, _ = ev.per_user_rows(gen, users)
    assert calls.dims == [dim]
    masked = dense.copy()
    for u in range(nU):
        masked[u, train[u]] = -np.inf
    top = -np.sort(-masked, axis=1)[:, :21]
    noise = _noise(Ut, users, It, bias, dim)
    ok = (-np.diff(top, axis=1) > noise).all(axis=1)
    print(f"dim {dim}: {int((~ok).sum())} of {nU} users excluded")
    assert (~ok).mean() <= 0.05
    assert np.array_equal(rows_f[ok].view(np.uint32), rows_g[ok].view(np.uint32))


def test_evaluator_reranks_structural_ties_at_128_columns(mode, monkeypatch):
    import torch
    from skrec.utils.py import RankingEvaluator
    rng = np.random.default_rng(8)
    nU, nI = 150, 400
    Ut = rng.integers(-2, 3, (nU, 128)).astype(np.float32)
    It = rng.integers(-2, 3, (nI, 128)).astype(np.float32)
    cold = rng.permutation(nU)[:10]
    Ut[cold] = 0.0                                             # ten cold users
    It[10:13] = It[30:33]                                      # three duplicated items
    train = {u: np.sort(rng.choice(nI, rng.integers(1, 30), replace=False)) for u in range(nU) if u % 11}
    test = {u: rng.choice(nI, rng.integers(1, 6), replace=False) for u in range(nU) if u % 5}
    dU, dI = torch.from_numpy(Ut).cuda(), torch.from_numpy(It).cuda()

    class M(object):
        def predict_factors(self):
            return dU, dI, None

        def predict(self, users):
            return Ut[np.asarray(users)] @ It.T
    ev = RankingEvaluator(train, test, metric=METRICS, top_k=[5, 10, 20], batch_size=32)
    calls = _Calls(monkeypatch)
    got = ev.evaluate(M())
    assert calls.dims == [128]
    _, want, _ = O.ranking_evaluate(M().predict, train, test, metric=METRICS, top_k=[5, 10, 20], batch_size=32)
    np.testing.assert_allclose(np.array(list(got.values()), np.float32), want, rtol=1e-6, atol=0)   # fp32 mean order


def test_evaluator_sees_a_tie_at_the_k_boundary_at_128_columns(mode, monkeypatch):
    import torch
    from skrec.utils.py import RankingEvaluator
    rng = np.random.default_rng(12)
    nU, nI, K = 96, 300, 10
    It = np.zeros((nI, 128), np.float32)
    Ut = np.zeros((nU, 128), np.float32)
    for u in range(nU):
        Ut[u, u % 128] = 1.0
    for d in range(128):
        col = rng.permutation(nI).astype(np.float32)             # all distinct: no tie anywhere ...
        srt = np.argsort(-col)
        if d % 2 == 0:
            col[srt[K]] = col[srt[K - 1]]                         # ... except exactly at the K / K+1 boundary
        It[:, d] = col
    train = {u: np.sort(rng.choice(nI, 3, replace=False)) for u in range(nU)}
    test = {u: rng.choice(nI, 4, replace=False) for u in range(nU)}
    dU, dI = torch.from_numpy(Ut).cuda(), torch.from_numpy(It).cuda()

    class M(object):
        def predict_factors(self):
            return dU, dI, None

        def predict(self, users):
            return Ut[np.asarray(users)] @ It.T
    ev = RankingEvaluator(train, test, metric=METRICS, top_k=K, batch_size=32)
    calls = _Calls(monkeypatch)
    rows, _, _ = ev.per_user_rows(M(), list(test.keys()))
    assert calls.dims == [128]
    _, _, want_rows = O.ranking_evaluate(M().predict, train, test, metric=METRICS, top_k=K, batch_size=32)
    assert np.array_equal(rows.view(np.uint32), want_rows.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 10. the models
# ---------------------------------------------------------------------------------------------------------------------
class _PredictOnly(object):
    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def _values(report):
    return np.array(list(report.values()), np.float32)


def test_caser_is_ranked_fused_without_its_score_rows(golden, tmp_path, monkeypatch):
    import test_gpu_caser as TC
    seq = TC._write_set(golden("tiny_seq_dataset"), tmp_path / "tiny_seq")
    monkeypatch.chdir(tmp_path)
    m = TC._model(seq, epochs=1)
    m.fit()
    ev = m.evaluator
    users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)

    class ScoreRowsOnly(object):                     # the dense score-row route of the same model
        num_items = m.num_items

        def predict(self, users):
            raise AssertionError

        def score_rows(self, d_users, out):
            return m.score_rows(d_users, out)
    dense = ev.evaluate(ScoreRowsOnly(), users)

    def refuse(*a, **k):
        raise AssertionError("score_rows was called: the evaluator did not take the fused route")
    monkeypatch.setattr(m, "score_rows", refuse)
    calls = _Calls(monkeypatch)
    fused = m.evaluate()
    assert calls.dims == [128]
    assert list(fused.metrics()) == list(dense.metrics())
    assert np.array_equal(_values(fused).view(np.uint32), _values(dense).view(np.uint32))


@pytest.mark.parametrize("n_dim,width", [(128, 128), (200, 256)])
def test_bprmf_at_wide_rows_is_ranked_fused(n_dim, width, tiny_dir, tmp_path, monkeypatch):
    from skrec import RunConfig
    from skrec.recommender.BPRMF import BPRMF
    monkeypatch.chdir(tmp_path)
    rc = RunConfig(recommender="BPRMF", data_dir=tiny_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                   metric=tuple(METRICS), top_k=(5, 10, 20), test_batch_size=64, test_thread=4, seed=2021)
    m = BPRMF(rc, dict(lr=1e-3, reg=1e-3, n_dim=n_dim, batch_size=1024, epochs=2))
    m.fit()
    ut, it, _ = m.predict_factors()
    assert ut.shape[1] == width and it.shape[1] == width and ut.is_contiguous() and it.is_contiguous()
    assert ut.stride(0) == width and it.stride(0) == width
    calls = _Calls(monkeypatch)
    fused = m.evaluate()
    assert calls.dims == [width]
    generic = m.evaluator.evaluate(_PredictOnly(m))
    assert calls.dims == [width]
    assert np.array_equal(_values(fused).view(np.uint32), _values(generic).view(np.uint32))


def test_gru_at_128_units_is_ranked_fused(tiny_dir, tmp_path, monkeypatch):
    from skrec import RunConfig
    from skrec.recommender.GRU4RecPlus import GRU4RecPlus
    monkeypatch.chdir(tmp_path)
    rc = RunConfig(recommender="GRU4RecPlus", data_dir=tiny_dir, file_column="UIRT", sep="\t",
                   metric=tuple(METRICS), top_k=(5, 10, 20), test_batch_size=16, seed=2021)
    m = GRU4RecPlus(rc, dict(lr=0.01, layers=[128], batch_size=16, n_sample=64, epochs=2, early_stop=10))
    m.fit()
    assert m.predict_factors() is not None and m.predict_factors()[1].shape[1] == 128
    calls = _Calls(monkeypatch)
    fused = m.evaluate()
    assert calls.dims == [128]
    generic = m.evaluator.evaluate(_PredictOnly(m))
    np.testing.assert_allclose(_values(fused), _values(generic), rtol=1e-5, atol=2e-4)
