"""GPU suite of skrec/recommender/_sparse.py: a rectangular block built from COO triples on the device multiplies as the same
block built from scipy does -- the same bits, both within test_gpu_train.py's bound of float64 numpy -- and a block without
entries, which holds one padding entry, returns the addend."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROWS, COLS, VALS = np.array([4, 0, 2, 0, 1, 2]), np.array([1, 2, 0, 0, 1, 2]), np.array([0.5, -1.25, 2.0, 0.75, -3.0, 1.5], np.float32)


@pytest.mark.parametrize("plan", ["0", "1"])
def test_a_block_from_coo_multiplies_as_the_scipy_one(plan, monkeypatch):
    import torch
    from gpu_utils import dev
    from skrec.recommender._sparse import DeviceCSR
    monkeypatch.setenv("SKR_SPMM_PLAN", plan)
    A = sp.csr_matrix((VALS, (ROWS, COLS)), shape=(5, 3))                 # row 3 is empty
    rng = np.random.default_rng(5)
    X, add = rng.standard_normal((3, 64)).astype(np.float32), rng.standard_normal((5, 64)).astype(np.float32)
    dX, dadd = torch.from_numpy(X).to(dev()), torch.from_numpy(add).to(dev())
    to = lambda a, t: torch.from_numpy(a).to(dev(), t)      # noqa: E731
    built = {"coo": DeviceCSR.from_coo(to(ROWS, torch.int64), to(COLS, torch.int64), to(VALS, torch.float32), 5, 3),
             "scipy": DeviceCSR(A, dev())}
    want = A.astype(np.float64) @ X.astype(np.float64)
    tol = 2e-6 * (abs(A).astype(np.float64) @ np.abs(X).astype(np.float64)) + 1e-6        # test_gpu_train.py::test_csr_spmm_vs_scipy
    got = {}
    for how, m in built.items():
        assert m.shape == (5, 3) and m.nnz == 6 and m.uses_plan() == (plan == "1")
        Y, Ya = torch.full((5, 64), 7.0, device=dev()), torch.full((5, 64), 7.0, device=dev())
        m.spmm(dX, Y)
        m.spmm(dX, Ya, addend=dadd)
        torch.cuda.synchronize()
        got[how] = (Y.cpu().numpy(), Ya.cpu().numpy())
        for g, ref in zip(got[how], (want, want + add)):
            assert np.all(np.abs(g - ref) <= tol + 2e-6 * np.abs(ref)), (how, np.abs(g - ref).max())
        assert np.array_equal(got[how][0][3], np.zeros(64, np.float32)) and np.array_equal(got[how][1][3], add[3])
    for a, b in zip(got["coo"], got["scipy"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))                      # the same bits


@pytest.mark.parametrize("plan", ["0", "1"])
def test_a_block_without_entries_returns_the_addend(plan, monkeypatch):
    import torch
    from gpu_utils import dev
    from skrec.recommender._sparse import DeviceCSR
    monkeypatch.setenv("SKR_SPMM_PLAN", plan)
    none = torch.zeros(0, dtype=torch.int64, device=dev())
    m = DeviceCSR.from_coo(none, none, torch.zeros(0, device=dev()), 3, 2)
    assert m.shape == (3, 2) and m.nnz == 0 and m.col.numel() == m.val.numel() == 1 and m.rowptr.tolist() == [0, 0, 0, 0]
    X = torch.ones((2, 64), device=dev())
    add = torch.arange(3 * 64, dtype=torch.float32, device=dev()).view(3, 64)
    Y = torch.full((3, 64), 7.0, device=dev())
    m.spmm(X, Y, addend=add)
    torch.cuda.synchronize()
    assert torch.equal(Y, add)
    m.spmm(X, Y)
    torch.cuda.synchronize()
    assert not Y.any()
