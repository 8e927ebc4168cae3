"""GPU suite of the graph models' shared propagation (skrec/recommender/_graph.py: propagate_mean through run_plan): the ping
form (SelfCF, BM3) and the hops form (DENS) against each other bit for bit and against a dense float64 restatement, on dirty
buffers."""
import numpy as np
import pytest

from helpers import graph_70x45

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
U, I = 70, 45
N = U + I


@pytest.fixture(scope="module")
def case():
    """the 70 x 45 matrix' adjacency pairs in HBM, their dense float64 square forms, one X_0 with zero padding columns"""
    from gpu_utils import dev, to_dev
    from skrec.recommender import _graph as G
    rowptr, items = graph_70x45()
    rp, col = G.upload_csr(rowptr, items, dev())
    adj = {"normalized": G.normalized_adjacency(rp, col, U, I), "selfcf": G.selfcf_adjacency(rp, col, U, I)[:2]}
    rows = np.repeat(np.arange(U), np.diff(rowptr))
    dense = {}
    for name, (A, _) in adj.items():
        S = np.zeros((N, N))
        S[rows, U + items] = S[U + items, rows] = A.val.cpu().numpy().astype(np.float64)
        dense[name] = S
    X0 = np.zeros((N, 64), np.float32)
    X0[:, :40] = np.random.default_rng(11).standard_normal((N, 40)).astype(np.float32)
    return dict(adj=adj, dense=dense, X0=X0, dX0=to_dev(X0))


@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])       # 3: both ping tables are in use; 4: the first one is written twice
@pytest.mark.parametrize("name", ["normalized", "selfcf"])
def test_propagate_mean_ping_and_hops(case, name, L):
    """Every launch is a plan product held to test_gpu_selfcf.py's bound for one: |y - want| <= 2e-6 mass + 1e-6, and
    2e-6 (mass + |accum before|) + 1e-6 for what it accumulates, mass = |A| |X|.  Against the float64 chain from X_0 the bound
    of layer k also carries the earlier layers' through |A|:  E_k = |A| E_(k-1) + 2e-6 mass_k + 1e-6."""
    import torch
    from gpu_utils import dev
    from skrec.recommender._graph import propagate_mean
    A, At = case["adj"][name]
    dirty = lambda: torch.full((N, 64), float("nan"), device=dev())          # noqa: E731
    p_ping, p_hops = dirty(), dirty()
    ping = (dirty(), dirty()) if L > 1 else (None, None)                     # as the models allocate them
    hops = [dirty() for _ in range(L)]
    assert propagate_mean(A, At, case["dX0"], U, L, p_ping, ping=ping) is p_ping
    assert propagate_mean(A, At, case["dX0"], U, L, p_hops, hops=hops) is p_hops
    torch.cuda.synchronize()
    got, got_h = p_ping.cpu().numpy(), p_hops.cpu().numpy()
    assert np.array_equal(got.view(np.int32), got_h.view(np.int32))
    for k in range(1, L):                                                    # the ping tables hold the last layers written there
        if k + 2 >= L:
            assert np.array_equal(ping[(k - 1) & 1].cpu().numpy().view(np.int32), hops[k - 1].cpu().numpy().view(np.int32))
    assert np.array_equal(case["dX0"].cpu().numpy(), case["X0"])             # the input is left alone
    S, X = case["dense"][name], case["X0"].astype(np.float64)
    s = 1.0 / (L + 1)
    want, tol, E = s * X, np.zeros((N, 64)), np.zeros((N, 64))
    for k in range(1, L + 1):
        mass = np.abs(S) @ np.abs(X)
        carried = np.abs(S) @ E                                              # E_(k-1) through this product
        tol += s * carried + 2e-6 * (mass + np.abs(want)) + 1e-6             # want: what the table held before this launch
        E = carried + 2e-6 * mass + 1e-6
        X = S @ X
        want = want + s * X
        err = np.abs(hops[k - 1].cpu().numpy() - X)
        print(name, "L", L, "layer", k, "max err", err.max(), "bound at it", E.flat[err.argmax()])
        assert np.all(err <= E)
    err = np.abs(got - want)
    print(name, "L", L, "pooled max err", err.max(), "bound at it", tol.flat[err.argmax()] if L else 0.0)
    assert np.all(err <= tol)                                                # L == 0: the copy, exactly
    assert not got[:, 40:].any()
