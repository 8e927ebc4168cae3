"""GPU suite of the kNN kernel (csrc/knn.hip, skrec/utils/item_graph.py): the neighbour lists against float64 similarities at the
tile edges, the tie rule, duplicated and all-zero rows, padded tables, the optional similarities, the guard rows, determinism, the
reference's recorded neighbour sets and its item graph from lists computed on the device.

The criterion.  With S the float64 cosine similarities and s_k a row's k-th largest value, a result is accepted iff the ids are
in range and distinct within a row, every returned j has S[i, j] >= s_k - tau, every j with S[i, j] > s_k + tau is returned, and
the returned similarities are within tau of S and non-increasing.  tau = max(2e-6, 4 x the largest error of torch-CPU's fp32
div + mm on the same input), measured per case: the rule of test_project_matches_float64 (tests/test_gpu_bm3.py).  It needs no
excluded rows and holds under exact ties."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def _run(X, F, k, sims=True):
    """skr_knn_topk on the padded table X [n, ld]; one guard row behind both outputs must stay as it was"""
    import torch
    from gpu_utils import dev, to_dev
    from skrec import _hip
    L = _hip.lib()
    n, ld = X.shape
    dX = to_dev(X)
    ws = int(L.skr_knn_workspace(n, k))
    assert ws >= 4 * n
    work = torch.empty(ws, dtype=torch.uint8, device=dev())
    ids = torch.full((n + 1, k), -7, dtype=torch.int32, device=dev())
    sm = torch.full((n + 1, k), 7.0, dtype=torch.float32, device=dev()) if sims else None
    _hip.check(L.skr_knn_topk(_hip.ptr(dX), n, F, ld, k, _hip.ptr(ids), _hip.ptr(sm), _hip.ptr(work), ws, _hip.stream()))
    torch.cuda.synchronize()
    ids = ids.cpu().numpy()
    assert (ids[n] == -7).all()
    if sims:
        sm = sm.cpu().numpy()
        assert (sm[n] == 7.0).all()
        return ids[:n], sm[:n]
    return ids[:n], None


def _float64_sims(X):
    x = X.astype(np.float64)
    xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return xn @ xn.T


def _tau(X, S):
    import torch
    t = torch.from_numpy(X)
    tn = t.div(torch.norm(t, p=2, dim=-1, keepdim=True).clamp_min(1e-12))
    err = float(np.abs(torch.mm(tn, tn.T).numpy().astype(np.float64) - S).max())
    return max(2e-6, 4 * err), err


def _accept(X, k, ids, sims, what=""):
    n = len(X)
    S = _float64_sims(X)
    tau, err = _tau(X, S)
    sk = -np.sort(-S, axis=1)[:, k - 1]
    assert ids.shape == (n, k) and ids.min() >= 0 and ids.max() < n
    assert all(len(set(r)) == k for r in ids.tolist()), "ids are distinct within a row"
    got = np.take_along_axis(S, ids.astype(np.int64), axis=1)
    worst_in = float((sk[:, None] - got).max())
    returned = np.zeros((n, n), bool)
    returned[np.repeat(np.arange(n), k), ids.reshape(-1)] = True
    missed = np.where(returned, -np.inf, S - sk[:, None])
    worst_out = float(missed.max()) if k < n else -np.inf
    print(what, "n", n, "k", k, "torch-CPU fp32 error", err, "tau", tau, "worst returned deficit", worst_in, "worst missed excess", worst_out)
    assert worst_in <= tau, "a returned neighbour lies more than tau below the k-th similarity"
    assert worst_out <= tau, "a row more than tau above the k-th similarity was not returned"
    if sims is not None:
        assert np.isfinite(sims).all()
        print(what, "similarity error", float(np.abs(sims - got).max()))
        assert np.abs(sims - got).max() <= tau
        assert (np.diff(sims, axis=1) <= 0).all(), "similarities are non-increasing"
    return S


def _table(n, F, seed, ld=None):
    ld = (F + 3) // 4 * 4 if ld is None else ld
    X = np.zeros((n, ld), np.float32)
    X[:, :F] = np.random.default_rng(seed).standard_normal((n, F))
    return X


# (I, F, k): one row; one feature; k at its limit on a partial tile; more than one column block (256 rows, merged in quarters of
# 64) and more than one workgroup (64 rows) with ragged edges; the widest table (128 chunks of 32 features); k = 32 over several
# blocks; k = 1 behind 2048 = 8 full column blocks plus one row; k = I; two workgroups and a ragged third quarter
@pytest.mark.parametrize("n,F,k", [(1, 1, 1), (17, 1, 10), (33, 3, 32), (257, 100, 10), (300, 4096, 10), (1000, 37, 32), (2049, 64, 1),
                                   (20, 8, 20), (129, 33, 5)])
def test_lists_match_float64(n, F, k):
    X = _table(n, F, 7 * n + F)
    ids, sims = _run(X, F, k)
    _accept(X, k, ids, sims)
    if k == 1 and F > 1:
        assert (ids[:, 0] == np.arange(n)).all()                # a row is its own nearest neighbour


def test_equal_similarities_rank_by_ascending_id():
    """one feature: every similarity is +1 or -1.  The inputs are signed powers of two, on which every fp32 operation of the kernel
    (the product, the norm, the reciprocal, the two scalings) is exact, so the similarities are exactly +-1 and the order of a list is
    decided by the id rule alone"""
    n, k = 17, 10
    rng = np.random.default_rng(5)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    sign[:2] = (1.0, -1.0)
    X = np.zeros((n, 4), np.float32)
    X[:, 0] = sign * np.exp2(rng.integers(-3, 4, n))
    ids, sims = _run(X, 1, k)
    _accept(X, k, ids, sims)
    for i in range(n):
        same = np.flatnonzero(sign == sign[i])
        other = np.flatnonzero(sign != sign[i])
        want = np.concatenate([same, other])[:k]                # +1 in ascending id, then -1 in ascending id
        assert np.array_equal(ids[i], want), i
        assert np.array_equal(sims[i], np.where(sign[want] == sign[i], 1.0, -1.0).astype(np.float32))
    # k = I: the whole order
    ids, _ = _run(X, 1, n)
    for i in range(n):
        assert np.array_equal(ids[i], np.concatenate([np.flatnonzero(sign == sign[i]), np.flatnonzero(sign != sign[i])]))


def test_duplicated_rows_and_an_all_zero_row():
    n, F, k = 150, 20, 12
    X = _table(n, F, 11)
    X[140] = X[3]
    X[77] = X[3]
    X[131] = X[60]
    X[99] = 0.0
    ids, sims = _run(X, F, k)
    _accept(X, k, ids, sims)
    assert np.isfinite(sims).all()
    # the all-zero row: similarity 0 to every row, so its list is the k lowest ids; nobody else's similarity to it is a NaN
    assert np.array_equal(ids[99], np.arange(k)) and (sims[99] == 0.0).all()
    # copies have bit-equal similarities to every row: wherever a copy is listed, the lower ids of its group come before it
    for group in ([3, 77, 140], [60, 131]):
        for i in range(n):
            row = ids[i].tolist()
            pos = [row.index(j) if j in row else None for j in group]
            seen = [p for p in pos if p is not None]
            assert pos[:len(seen)] == sorted(seen), (i, pos)                 # a prefix of the group, in ascending id
            if len(seen) > 1:
                assert len(set(sims[i][seen].tolist())) == 1
    assert ids[3, 0] == 3 and ids[77, 0] == 3 and ids[140, 0] == 3 and ids[140, 1] == 77 and ids[140, 2] == 140


def test_padded_table_null_sims_and_determinism():
    n, F, k = 200, 37, 10
    X = _table(n, F, 3)
    ids, sims = _run(X, F, k)
    wide = _table(n, F, 3, ld=48)                               # feat_ld > feat_dim rounded up: zero columns change nothing
    assert np.array_equal(wide[:, :40], X)
    ids_w, sims_w = _run(wide, F, k)
    assert np.array_equal(ids_w, ids) and np.array_equal(sims_w, sims)
    ids_n, none = _run(X, F, k, sims=False)                     # d_sims = NULL
    assert none is None and np.array_equal(ids_n, ids)
    ids2, sims2 = _run(X, F, k)                                 # two calls: the same bits
    assert np.array_equal(ids2, ids) and np.array_equal(sims2.view(np.uint32), sims.view(np.uint32))


def test_reference_sets_and_item_graph_from_device_lists(golden):
    """the fixture's features: every row's set equals the reference's recorded set, through the raw entry and through knn_topk on the
    unpadded table; build_item_graph on the device lists is the reference's mm_adj bit for bit"""
    import torch
    from gpu_utils import to_dev
    from skrec.utils.item_graph import build_item_graph, knn_topk
    g, bm3 = golden("golden_item_graph"), golden("golden_bm3")
    k = int(g["knn_k"])
    lists = {}
    for key, name in (("img", "image_embedding_weight_0"), ("txt", "text_embedding_weight_0")):
        feats = bm3[name]
        n, F = feats.shape
        X = np.zeros((n, (F + 3) // 4 * 4), np.float32)
        X[:, :F] = feats
        ids, sims = _run(X, F, k)
        _accept(X, k, ids, sims, key)
        want = g[f"knn_ind_{key}"]
        assert all(set(a) == set(b) for a, b in zip(ids.tolist(), want.tolist())), key
        assert (ids[:, 0] == np.arange(n)).all()
        d_ids, d_sims = knn_topk(to_dev(feats), k, return_sims=True)            # [96, 37] is copied into the padded layout
        assert d_ids.dtype == torch.int32 and np.array_equal(d_ids.cpu().numpy(), ids)
        assert np.array_equal(d_sims.cpu().numpy(), sims)
        lists[key] = d_ids
    S, St = build_item_graph(lists["img"], lists["txt"], k, float(g["mm_image_weight"]))
    assert S[1].is_cuda
    rowptr, col, val = (t.cpu().numpy() for t in S)
    assert np.array_equal(np.repeat(np.arange(96), np.diff(rowptr)), g["mm_adj_row"])
    assert np.array_equal(col, g["mm_adj_col"]) and np.array_equal(val, g["mm_adj_val"])
    dense = np.zeros((96, 96), np.float32)
    dense[g["mm_adj_row"], g["mm_adj_col"]] = g["mm_adj_val"]
    rp, c, v = (t.cpu().numpy() for t in St)
    dt = np.zeros((96, 96), np.float32)
    dt[np.repeat(np.arange(96), np.diff(rp)), c] = v
    assert np.array_equal(dt, dense.T)


def test_wrapper_limits():
    import torch
    from gpu_utils import dev
    from skrec.utils.item_graph import knn_topk
    x = torch.ones((40, 8), device=dev())
    with pytest.raises(NotImplementedError, match="knn_k <= 32"):
        knn_topk(x, 33)
    with pytest.raises(ValueError, match="number of rows = 40"):
        knn_topk(x, 41)
    with pytest.raises(ValueError, match="number of rows = 40"):
        knn_topk(x, 0)
    with pytest.raises(NotImplementedError, match="feature width <= 4096"):
        knn_topk(torch.ones((4, 4100), device=dev()), 2)
    assert knn_topk(x, 3).shape == (40, 3)
