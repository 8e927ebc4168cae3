"""CPU suite of the kNN item graph (csrc/knn.hip's argument checks, skrec/utils/item_graph.py, tests/golden/golden_item_graph.npz):
the library's exports and checks without a GPU, the limits, ``build_item_graph`` on CPU tensors against the reference's recorded
graph, its transpose, the fixture's own conditions."""
import numpy as np
import pytest


def test_library_exports_and_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    assert L.skr_abi_version() >= 15
    for name, n_args in (("skr_knn_workspace", 2), ("skr_knn_topk", 10)):
        assert hasattr(L, name) and len(_hip.SIGNATURES[name][1]) == n_args
    assert _hip.SKR_KNN_MAX_K == 32
    # the workspace: n_rows floats, rounded up to 256 bytes; 0 outside the ranges
    assert L.skr_knn_workspace(100, 10) == 512 and L.skr_knn_workspace(64, 32) == 256 and L.skr_knn_workspace(1, 1) == 256
    for bad in ((0, 1), (-3, 1), (100, 0), (100, -1), (100, 33), (5, 6)):
        assert L.skr_knn_workspace(*bad) == 0, bad
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    big = 1 << 20
    assert L.skr_knn_topk(None, 8, 4, 4, 2, p, p, p, big, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4, 4, 2, None, p, p, big, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4, 4, 2, p, p, None, big, None) == -1 and b"NULL" in L.skr_last_error()
    assert L.skr_knn_topk(p, 0, 4, 4, 1, p, p, p, big, None) == -1 and b"n_rows" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4, 4, 0, p, p, p, big, None) == -1 and b"<= k <=" in L.skr_last_error()
    assert L.skr_knn_topk(p, 100, 4, 4, 33, p, p, p, big, None) == -1 and b"<= k <=" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4, 4, 9, p, p, p, big, None) == -1 and b"n_rows = 8" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 0, 4, 2, p, p, p, big, None) == -1 and b"feat_dim" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4097, 4100, 2, p, p, p, big, None) == -1 and b"feat_dim" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 37, 37, 2, p, p, p, big, None) == -1 and b"multiple of 4" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 37, 36, 2, p, p, p, big, None) == -1 and b"feat_ld" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4, 4100, 2, p, p, p, big, None) == -1 and b"feat_ld" in L.skr_last_error()
    assert L.skr_knn_topk(8, 8, 4, 4, 2, p, p, p, big, None) == -1 and b"16-byte aligned" in L.skr_last_error()     # a misaligned table
    assert L.skr_knn_topk(p, 8, 4, 4, 2, p, p, 8, big, None) == -1 and b"16-byte aligned" in L.skr_last_error()
    assert L.skr_knn_topk(p, 8, 4, 4, 2, 18, p, p, big, None) == -1 and b"4-byte aligned" in L.skr_last_error()
    assert L.skr_knn_topk(p, 100, 4, 4, 2, p, p, p, 511, None) == -1 and b"skr_knn_workspace" in L.skr_last_error()  # a short workspace


def test_limits_are_named():
    from skrec.utils.item_graph import check_knn_limits
    check_knn_limits(32, 4096)
    check_knn_limits(1)
    with pytest.raises(NotImplementedError, match="knn_k <= 32"):
        check_knn_limits(33, 64)
    with pytest.raises(NotImplementedError, match=r"feature width <= 4096.*image.*4097"):
        check_knn_limits(10, 4097, "image")


def _dense(csr, n):
    rowptr, col, val = (t.numpy() for t in csr)
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float32
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(val)
    out = np.zeros((n, n), np.float32)
    for r in range(n):
        c = col[rowptr[r]:rowptr[r + 1]]
        assert (np.diff(c) > 0).all(), "columns ascend and are distinct within a row"
        out[r, c] = val[rowptr[r]:rowptr[r + 1]]
    return out


def test_build_item_graph_reproduces_the_reference_exactly(golden):
    import torch
    from skrec.utils.item_graph import build_item_graph
    g = golden("golden_item_graph")
    k, w, n = int(g["knn_k"]), float(g["mm_image_weight"]), 96
    img, txt = torch.from_numpy(g["knn_ind_img"]), torch.from_numpy(g["knn_ind_txt"])
    S, St = build_item_graph(img, txt, k, w)
    rowptr, col, val = (t.numpy() for t in S)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    assert np.array_equal(rows, g["mm_adj_row"]) and np.array_equal(col, g["mm_adj_col"])
    assert np.array_equal(val, g["mm_adj_val"])                         # bit for bit
    per_row = np.diff(rowptr)
    assert per_row.min() >= k and per_row.max() <= 2 * k and per_row.max() > k
    dense = _dense(S, n)
    assert np.array_equal(_dense(St, n), dense.T)
    assert not np.array_equal(dense, dense.T)                           # directed: not symmetric
    # the order of a row's list does not matter, int64 and int32 lists are the same thing
    perm = torch.from_numpy(np.random.default_rng(0).permutation(k))
    S2, _ = build_item_graph(img[:, perm].to(torch.int64), txt, k, w)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(S, S2))


def test_one_modality_alone_is_its_own_normalised_graph(golden):
    import torch
    from skrec.utils.item_graph import build_item_graph
    g = golden("golden_item_graph")
    k, n = int(g["knn_k"]), 96
    for key, args in (("img", lambda t: (t, None)), ("txt", lambda t: (None, t))):
        ind = g[f"knn_ind_{key}"]
        S, St = build_item_graph(*args(torch.from_numpy(ind)), k, 0.1)
        want = np.zeros((n, n), np.float32)
        want[np.repeat(np.arange(n), k), ind.reshape(-1)] = g[f"adj_val_{key}"]
        assert np.array_equal(_dense(S, n), want) and np.array_equal(_dense(St, n), want.T)
        # every row has knn_k ones, so every value is the one fp32 number (10 + 1e-7)^-0.5 squared, about 1 / knn_k
        r = np.float32(np.float32(k) + np.float32(1e-7)) ** np.float32(-0.5)
        assert set(S[2].numpy().tolist()) == {float(np.float32(r * r))}
        assert (np.diff(S[0].numpy()) == k).all()
    with pytest.raises(ValueError, match="no modality"):
        build_item_graph(None, None, k, 0.1)
    with pytest.raises(ValueError, match="outside"):
        build_item_graph(torch.full((4, 2), 4, dtype=torch.int32), None, 2, 0.1)


def test_fixture_conditions(golden):
    """what the GPU test of the recorded sets relies on: the float64 gap behind the 10th neighbour dwarfs any fp32 error"""
    g = golden("golden_item_graph")
    assert float(g["gap_img"]) >= 1e-5 and float(g["gap_txt"]) >= 1e-5
    assert max(float(g["sim_err_img"]), float(g["sim_err_txt"])) < 1e-6
    bm3 = golden("golden_bm3")
    for key, name in (("img", "image_embedding_weight_0"), ("txt", "text_embedding_weight_0")):
        x = bm3[name].astype(np.float64)
        xn = x / np.linalg.norm(x, axis=1, keepdims=True)
        s = xn @ xn.T
        want = np.argsort(-s, axis=1, kind="stable")[:, :10]
        ind = g[f"knn_ind_{key}"]
        assert ind.shape == (96, 10) and (ind[:, 0] == np.arange(96)).all()          # an item is its own nearest neighbour
        assert all(set(a) == set(b) for a, b in zip(want.tolist(), ind.tolist()))
