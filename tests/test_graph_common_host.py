"""CPU suite of the graph models' shared module (skrec/recommender/_graph.py): the two adjacency builders on CPU tensors against
scipy's transpose and their value formulas restated in numpy, the keep permutation, the train CSR helpers, the linear-block
views."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from helpers import graph_70x45

U, I = 70, 45


@pytest.fixture(scope="module")
def graph():
    rowptr, items = graph_70x45()
    rowdeg = np.diff(rowptr)
    coldeg = np.bincount(items, minlength=I)
    assert 250 <= len(items) <= 350 and rowdeg[17] == 0 and coldeg[44] == 0 and (np.delete(rowdeg, 17) > 0).all()
    rows = np.repeat(np.arange(U), rowdeg)
    return dict(rowptr=rowptr, items=items, rows=rows, rowdeg=rowdeg, coldeg=coldeg)


def _prim(np_fn, torch_fn, x):
    """``np_fn(x)`` -- unless this machine's torch CPU kernel rounds the primitive differently on these very operands: then
    torch's result.  Casts, products, sums and quotients are exact IEEE operations in both libraries; torch hands sqrt and
    pow of a contiguous CPU tensor to a vendor vector library that on some CPUs is accurate to an ulp but not correctly
    rounded (seen on one host: the float32 sqrt of 22 of this matrix' 315 degree products and the float64 power of 28 of
    its 115 degrees differ from numpy's, 1 / sqrt(42) comes out one ulp low).  The restatement still pins the dtypes, the order of the operations and
    where the one rounding to float32 happens."""
    want, got = np_fn(x), torch_fn(torch.from_numpy(x)).numpy()
    if not np.array_equal(want, got):
        print("torch's CPU primitive differs from numpy's on", int((want != got).sum()), "of", want.size, "operands")
    return got


def _values(name, g):
    """the value formulas in numpy, in the dtypes the models' references use"""
    rd, cd = g["rowdeg"][g["rows"]], g["coldeg"][g["items"]]
    if name == "normalized":          # LightGCL, DENS: 1 / sqrt(fp32 * fp32)
        return np.float32(1.0) / _prim(np.sqrt, torch.sqrt, rd.astype(np.float32) * cd.astype(np.float32))
    rsqrt = lambda deg: _prim(lambda x: x ** -0.5, lambda x: x.pow(-0.5), deg.astype(np.float64) + 1e-7)    # noqa: E731
    du, di = rsqrt(g["rowdeg"]), rsqrt(g["coldeg"])               # SelfCF, BM3: float64 powers and product, rounded once
    return (du[g["rows"]] * di[g["items"]]).astype(np.float32)


def _scipy(m):
    return sp.csr_matrix((m.val.numpy()[:m.nnz], m.col.numpy()[:m.nnz], m.rowptr.numpy()), shape=m.shape)


@pytest.mark.parametrize("name", ["normalized", "selfcf"])
def test_adjacency_and_transpose(graph, name):
    from skrec.recommender import _graph as G
    fn = G.normalized_adjacency if name == "normalized" else G.selfcf_adjacency
    rp, col = G.upload_csr(graph["rowptr"], graph["items"], "cpu")
    out = fn(rp, col, U, I)
    assert len(out) == (2 if name == "normalized" else 3)
    A, At = out[0], out[1]
    nnz = len(graph["items"])
    assert A.shape == (U, I) and At.shape == (I, U) and A.nnz == At.nnz == nnz
    assert A.rowptr.dtype == At.rowptr.dtype == torch.int64 and A.col.dtype == At.col.dtype == torch.int32
    assert A.val.dtype == At.val.dtype == torch.float32
    want = _values(name, graph)
    assert np.array_equal(A.rowptr.numpy(), graph["rowptr"]) and np.array_equal(A.col.numpy(), graph["items"])
    assert np.array_equal(A.val.numpy().view(np.int32), want.view(np.int32))                 # bit for bit
    ref_t = sp.csr_matrix((want, graph["items"], graph["rowptr"]), shape=(U, I)).T.tocsr()
    ref_t.sort_indices()
    assert np.array_equal(At.rowptr.numpy(), ref_t.indptr) and np.array_equal(At.col.numpy(), ref_t.indices)
    assert np.array_equal(At.val.numpy().view(np.int32), ref_t.data.view(np.int32))
    assert (_scipy(A).T != _scipy(At)).nnz == 0                                              # entry for entry
    if name == "selfcf":
        perm = out[2].numpy()
        assert out[2].dtype == torch.int32 and sorted(perm) == list(range(nnz))
        order = np.lexsort((graph["rows"], graph["items"]))                                  # the transpose: by column, then by row
        assert np.array_equal(perm[order], np.arange(nnz))                                   # its inverse
        assert np.array_equal(At.col.numpy()[perm], graph["rows"]) and np.array_equal(At.val.numpy()[perm], A.val.numpy())


def test_empty_matrix_keeps_one_padding_entry():
    from skrec.recommender._graph import selfcf_adjacency
    A, At, perm = selfcf_adjacency(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 3, 2)
    assert A.nnz == At.nnz == perm.numel() == 0 and A.col.numel() == A.val.numel() == At.col.numel() == 1
    assert At.rowptr.tolist() == [0, 0, 0]


def test_the_models_still_export_the_moved_names():
    from skrec.recommender import LightGCL as M
    from skrec.recommender import _graph as G
    assert M.normalized_adjacency is G.normalized_adjacency and M.selfcf_adjacency is G.selfcf_adjacency
    assert M._device_csr is G._device_csr and M.DeviceCSR is G.DeviceCSR
    for name in ("svd_lowrank_device", "_times", "init_tables"):
        assert hasattr(M, name)


def test_train_csr_and_upload_csr(graph):
    from skrec.recommender._graph import train_csr, upload_csr
    rows, cols = graph["rows"], graph["items"].astype(np.int64)
    shuffle = np.random.default_rng(3).permutation(len(rows))
    dup = np.concatenate([shuffle, shuffle[:25]])                     # unsorted, 25 interactions twice

    class Train:
        def to_csr_matrix(self):
            return sp.coo_matrix((np.ones(len(dup), np.float32), (rows[dup], cols[dup])), shape=(U, I))

    class Dataset:
        train_data = Train()

    indptr, indices = train_csr(Dataset())
    assert np.array_equal(indptr, graph["rowptr"]) and np.array_equal(indices, graph["items"])
    for rp_in, it_in in ((graph["rowptr"], graph["items"]), (graph["rowptr"].astype(np.int32), graph["items"].astype(np.int64)),
                         (torch.from_numpy(graph["rowptr"]).to(torch.int32), torch.from_numpy(graph["items"]).to(torch.int64)),
                         (torch.from_numpy(graph["rowptr"])[::1], torch.from_numpy(np.repeat(graph["items"], 2))[::2])):
        rp, col = upload_csr(rp_in, it_in, "cpu")
        assert rp.dtype == torch.int64 and col.dtype == torch.int32 and rp.is_contiguous() and col.is_contiguous()
        assert np.array_equal(rp.numpy(), graph["rowptr"]) and np.array_equal(col.numpy(), graph["items"])


@pytest.mark.parametrize("d", [64, 20])
def test_linear_block_views(d):
    from skrec.recommender._graph import linear_block
    flat = torch.zeros(100 + 2 * 4160)
    W, b = linear_block(flat[100 + 4160:100 + 2 * 4160], d)
    assert W.shape == (d, d) and b.shape == (d,)
    Wv = torch.arange(1, d * d + 1, dtype=torch.float32).view(d, d)
    W.copy_(Wv)
    b.copy_(-torch.arange(1, d + 1, dtype=torch.float32))
    got = flat.numpy()
    assert not got[:100 + 4160].any()                                 # the buffer in front of the block
    blk = got[100 + 4160:]
    want = np.zeros(4160, np.float32)
    want[:4096].reshape(64, 64)[:d, :d] = Wv.numpy()                  # W[r][c] at 64 r + c
    want[4096:4096 + d] = -np.arange(1, d + 1)
    assert np.array_equal(blk, want)                                  # the padding stays zero
    assert got[100 + 4160 + 64 * 3 + 5] == 3 * d + 5 + 1 and got[100 + 4160 + 4096 + d - 1] == -d
