"""The item-item k-nearest-neighbour graph of the multimodal models (reference: recommender/FREEDOM.py:102-147; LATTICE and
MGCN start from the same construction).

``knn_topk`` is the device half: the ``k`` most cosine-similar rows of every row of a feature table, computed by
``skr_knn_topk`` (csrc/knn.hip) on the fp32 matrix pipe without ever forming the [I, I] similarity matrix the reference
builds with ``torch.mm`` + ``torch.topk``.  There is no fallback: without the library or a GPU it raises.

``build_weighted_item_graph`` is MGCN's (and LATTICE's) variant of the host half: one modality, entries weighted by the
similarities themselves (MGCN.py:67-80, 101-111).

``build_item_graph`` is the host half, pure torch on whatever device its inputs live on (CPU tensors included): neighbour
lists -> the reference's normalised, weighted, coalesced graph ``S`` and its transpose, both as CSR triples.  Nothing is
cached: the reference stores the graph in the data set's cache directory under a name that ignores the features, here it is
recomputed on every call.
"""
import torch

from skrec import _hip

__all__ = ["knn_topk", "build_item_graph", "build_weighted_item_graph", "check_knn_limits"]


def check_knn_limits(knn_k, feat_dim=None, what="feature"):
    """the limits of skr_knn_topk, raised by name as the models raise theirs"""
    if int(knn_k) > _hip.SKR_KNN_MAX_K:
        raise NotImplementedError(f"skr_knn_topk is built for knn_k <= {_hip.SKR_KNN_MAX_K} (got {knn_k})")
    if feat_dim is not None and int(feat_dim) > _hip.SKR_BM3_MAX_FEAT:
        raise NotImplementedError(f"skr_knn_topk is built for a feature width <= {_hip.SKR_BM3_MAX_FEAT} ({what}: {feat_dim})")


def knn_topk(features, k, feat_dim=None, return_sims=False):
    """ids [I, k] int32 (and sims [I, k] float32): for every row of ``features`` the ``k`` rows with the largest cosine
    similarity, the row itself included, in descending order; equal similarities rank by ascending id.

    ``features``: a float32 device tensor [I, ld].  ``feat_dim`` (default ld) columns are features, the columns beyond are
    zero; a table whose width is no multiple of 4, or that is not contiguous, is copied into the padded layout first (the
    models' own tables already have it and are used in place).  A row's norm is clamped at 1e-12: an all-zero row has
    similarity 0 to every row, where the reference's division gives NaN."""
    dev = _hip.require_gpu()
    assert features.dim() == 2 and features.dtype == torch.float32 and features.device.type == "cuda", \
        "knn_topk: features must be a float32 [I, F] tensor on the GPU"
    n, ld = int(features.shape[0]), int(features.shape[1])
    F = ld if feat_dim is None else int(feat_dim)
    k = int(k)
    if k < 1 or k > n:
        raise ValueError(f"knn_topk: 1 <= k <= the number of rows = {n} (got {k})")
    if not 1 <= F <= ld:
        raise ValueError(f"knn_topk: 1 <= feat_dim <= the table's width = {ld} (got {F})")
    check_knn_limits(k, F)
    if ld % 4 != 0 or not features.is_contiguous() or features.data_ptr() % 16 != 0:
        padded = torch.zeros((n, (F + 3) // 4 * 4), dtype=torch.float32, device=dev)
        padded[:, :F] = features[:, :F]
        features, ld = padded, int(padded.shape[1])
    L = _hip.lib()
    ws = int(L.skr_knn_workspace(n, k))
    work = torch.empty(ws, dtype=torch.uint8, device=dev)
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    sims = torch.empty((n, k), dtype=torch.float32, device=dev) if return_sims else None
    _hip.check(L.skr_knn_topk(_hip.ptr(features), n, F, ld, k, _hip.ptr(ids), _hip.ptr(sims), _hip.ptr(work), ws, _hip.stream()))
    return (ids, sims) if return_sims else ids


def _normalised_entries(knn_ids, n_items):
    """(keys = row * I + col, values) of one modality's graph: ones on the neighbour entries, then r[row] * r[col] with
    r = (rowsum + 1e-7)^-0.5, in the reference's fp32 operations (FREEDOM.py:140-147)"""
    ids = knn_ids.to(torch.int64)
    assert ids.dim() == 2 and ids.shape[0] == n_items, "build_item_graph: one neighbour list per item"
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_items):
        raise ValueError("build_item_graph: a neighbour id is outside [0, n_items)")
    rows = torch.arange(n_items, dtype=torch.int64, device=ids.device).unsqueeze(1).expand_as(ids).reshape(-1)
    cols = ids.reshape(-1)
    ones = torch.ones(rows.numel(), dtype=torch.float32, device=ids.device)
    row_sum = 1e-7 + torch.zeros(n_items, dtype=torch.float32, device=ids.device).index_add_(0, rows, ones)
    r_inv_sqrt = torch.pow(row_sum, -0.5)
    return rows * n_items + cols, r_inv_sqrt[rows] * r_inv_sqrt[cols]


def _csr(keys, vals, n_items):
    rows = torch.div(keys, n_items, rounding_mode="floor")
    rowptr = torch.zeros(n_items + 1, dtype=torch.int64, device=keys.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_items), 0)
    return rowptr, (keys - rows * n_items).to(torch.int32), vals


def build_item_graph(knn_ids_img, knn_ids_txt, knn_k, weight):
    """The frozen item graph ``S`` [I, I] of FREEDOM.py:111-147 from the neighbour lists ([I, knn_k] integer tensors, or None
    for an absent modality): per modality ones on the neighbour entries normalised as r[row] r[col]; with both modalities
    ``weight * image + (1 - weight) * text``, duplicates coalesced (an entry of both lists is the fp32 sum of its two
    terms).  ``S`` is directed and not symmetric; a row has between knn_k and 2 knn_k entries.

    Returns ``((rowptr, col, val), (rowptr_t, col_t, val_t))``: ``S`` and ``S^T`` as CSR with ascending columns, rowptr
    int64, col int32, val float32, on the inputs' device.  Pure torch: it runs on CPU tensors as well."""
    present = [x for x in (knn_ids_img, knn_ids_txt) if x is not None]
    if not present:
        raise ValueError("build_item_graph: no modality at all -- the item graph needs image or text neighbour lists")
    n_items = int(present[0].shape[0])
    for x in present:
        assert x.dim() == 2 and int(x.shape[0]) == n_items and int(x.shape[1]) == int(knn_k), \
            f"build_item_graph: neighbour lists must be [n_items, knn_k = {knn_k}]"
    if len(present) == 1:
        keys, vals = _normalised_entries(present[0], n_items)
    else:
        k_img, v_img = _normalised_entries(knn_ids_img, n_items)
        k_txt, v_txt = _normalised_entries(knn_ids_txt, n_items)
        keys, vals = torch.cat([k_img, k_txt]), torch.cat([weight * v_img, (1.0 - weight) * v_txt])
    # coalesce: ascending (row, col); an entry occurs at most once per modality, and a sum of two fp32 terms has one value
    ukeys, inverse = torch.unique(keys, sorted=True, return_inverse=True)
    uvals = torch.zeros(ukeys.numel(), dtype=torch.float32, device=keys.device).index_add_(0, inverse, vals)
    rows = torch.div(ukeys, n_items, rounding_mode="floor")
    cols = ukeys - rows * n_items
    tkeys = cols * n_items + rows
    order = torch.argsort(tkeys)                # the keys are distinct: any sort gives the one order
    return _csr(ukeys, uvals, n_items), _csr(tkeys[order], uvals[order], n_items)


def build_weighted_item_graph(knn_ids, knn_sims):
    """One modality's graph ``S`` [I, I] of MGCN.py:101-111 (sparse branch, 'sym') from the neighbour lists ``knn_ids``
    [I, k] and their cosine similarities ``knn_sims`` [I, k]: the entry (i, j) of a kept neighbour is
    ``deg_i^-0.5 * s_ij * deg_j^-0.5`` with ``deg`` the ROW sums of the kept similarities (inf -> 0), in the reference's fp32
    operations.  ``S`` is directed, weighted, has exactly k entries per row and is not symmetric.

    Returns ``((rowptr, col, val), (rowptr_t, col_t, val_t))``: ``S`` and ``S^T`` as CSR with ascending columns, rowptr
    int64, col int32, val float32, on the inputs' device.  Pure torch: it runs on CPU tensors as well."""
    ids = knn_ids.to(torch.int64)
    assert ids.dim() == 2 and knn_sims.shape == ids.shape, "build_weighted_item_graph: ids and sims must both be [n_items, k]"
    n_items = int(ids.shape[0])
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_items):
        raise ValueError("build_weighted_item_graph: a neighbour id is outside [0, n_items)")
    rows = torch.arange(n_items, dtype=torch.int64, device=ids.device).unsqueeze(1).expand_as(ids).reshape(-1)
    cols = ids.reshape(-1)
    v = knn_sims.to(torch.float32).reshape(-1)
    deg = torch.zeros(n_items, dtype=torch.float32, device=ids.device).index_add_(0, rows, v)
    deg_inv_sqrt = deg.pow(-0.5)
    deg_inv_sqrt.masked_fill_(deg_inv_sqrt == float("inf"), 0)
    vals = deg_inv_sqrt[rows] * v * deg_inv_sqrt[cols]
    keys = rows * n_items + cols
    order = torch.argsort(keys)                 # a row's neighbours are distinct: the keys are, too
    tkeys = cols * n_items + rows
    order_t = torch.argsort(tkeys)
    return _csr(keys[order], vals[order], n_items), _csr(tkeys[order_t], vals[order_t], n_items)
