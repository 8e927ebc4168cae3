"""Generate the golden vectors of the kNN item graph by RUNNING THE REFERENCE's own construction on the seeded features of
make_golden_bm3.py (seed 20260302, image [96, 100], text [96, 37]):

    python tests/golden/make_golden_item_graph.py

Same rules as the other generators: a fresh process, the reference is imported from where it lies, only data is written.  The
reference's ``_FREEDOM.get_knn_adj_mat`` and ``compute_normalized_laplacian`` (recommender/FREEDOM.py:126-147) are called as
they stand, on a bare namespace that carries the three attributes they read (``knn_k``, ``device`` and the second method):
no data set, no cache directory and no training are involved, so nothing is written outside this fixture.  The two graphs are
then combined by the expression of FREEDOM.py:121 with the reference's default ``mm_image_weight`` and coalesced.

Recorded: ``knn_k``, ``mm_image_weight``, per modality ``knn_ind`` [96, 10] and the normalised values in list order, the
coalesced ``mm_adj`` (row, col, value), the features' smallest float64 gap between the 10th and the 11th neighbour per
modality and torch-CPU's largest fp32 similarity error.

No fixture is written if any row's gap is below 1e-5: the neighbour SETS must be unambiguous at fp32.
"""
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
from make_golden_bm3 import FEATURE_SEED, IMG_SHAPE, TXT_SHAPE, _shims  # noqa: E402

KNN_K, IMAGE_WEIGHT = 10, 0.1           # FREEDOMConfig's defaults (recommender/FREEDOM.py:24-61)
MIN_GAP = 1e-5


def _features():
    rng = np.random.default_rng(FEATURE_SEED)
    img = rng.standard_normal(IMG_SHAPE).astype(np.float32)
    txt = rng.standard_normal(TXT_SHAPE).astype(np.float32)
    return img, txt


def _gap_and_error(x, knn_ind):
    """the smallest float64 gap between the k-th and the (k + 1)-th similarity of a row; the reference's sets against float64;
    torch-CPU's fp32 error"""
    import torch
    x64 = x.astype(np.float64)
    xn = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    s = xn @ xn.T
    srt = -np.sort(-s, axis=1)
    gap = float((srt[:, KNN_K - 1] - srt[:, KNN_K]).min())
    want = np.argsort(-s, axis=1, kind="stable")[:, :KNN_K]
    assert all(set(a) == set(b) for a, b in zip(want.tolist(), knn_ind.tolist())), "the reference's sets differ from float64's"
    t = torch.from_numpy(x)
    tn = t.div(torch.norm(t, p=2, dim=-1, keepdim=True))
    err = float(np.abs(torch.mm(tn, tn.T).numpy().astype(np.float64) - s).max())
    return gap, err


def make_item_graph():
    img, txt = _features()
    G._install()
    import torch
    torch.set_num_threads(1)
    _shims()
    import skrec.recommender.FREEDOM as M
    assert M.FREEDOMConfig().knn_k == KNN_K and M.FREEDOMConfig().mm_image_weight == IMAGE_WEIGHT
    net = types.SimpleNamespace(knn_k=KNN_K, device=torch.device("cpu"))
    net.compute_normalized_laplacian = lambda indices, size: M._FREEDOM.compute_normalized_laplacian(net, indices, size)
    out = dict(knn_k=np.int32(KNN_K), mm_image_weight=np.float64(IMAGE_WEIGHT))
    adj = {}
    for key, x in (("img", img), ("txt", txt)):
        indices, a = M._FREEDOM.get_knn_adj_mat(net, torch.from_numpy(x))
        knn_ind = indices[1].reshape(len(x), KNN_K).numpy()
        assert np.array_equal(indices[0].numpy(), np.repeat(np.arange(len(x)), KNN_K))
        assert np.array_equal(a._indices().numpy(), indices.numpy())
        gap, err = _gap_and_error(x, knn_ind)
        print(key, "smallest gap between the neighbours", KNN_K, "and", KNN_K + 1, ":", gap, " torch-CPU fp32 error:", err)
        if gap < MIN_GAP:
            raise SystemExit(f"{key}: a row's gap is {gap} < {MIN_GAP}: fixture NOT written")
        out[f"knn_ind_{key}"] = knn_ind.astype(np.int32)
        out[f"adj_val_{key}"] = a._values().numpy().astype(np.float32)
        out[f"gap_{key}"], out[f"sim_err_{key}"] = np.float64(gap), np.float64(err)
        adj[key] = a
    mm_adj = (IMAGE_WEIGHT * adj["img"] + (1.0 - IMAGE_WEIGHT) * adj["txt"]).coalesce()
    idx, val = mm_adj.indices().numpy(), mm_adj.values().numpy()
    assert val.dtype == np.float32 and (np.diff(idx[0].astype(np.int64) * len(img) + idx[1]) > 0).all()
    per_row = np.bincount(idx[0], minlength=len(img))
    assert per_row.min() >= KNN_K and per_row.max() <= 2 * KNN_K
    print("mm_adj:", len(val), "entries, per row", per_row.min(), "..", per_row.max(), " values", val.min(), "..", val.max())
    out.update(mm_adj_row=idx[0].astype(np.int32), mm_adj_col=idx[1].astype(np.int32), mm_adj_val=val)
    np.savez_compressed(os.path.join(HERE, "golden_item_graph.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        make_item_graph()
    else:   # a fresh process, as the other generators
        subprocess.run([sys.executable, os.path.abspath(__file__), "run"], check=True)
