"""GPU suite of LightGCL (csrc/lightgcl.hip, skrec/recommender/LightGCL.py): the fused InfoNCE term and the whole step against
float64 autograd of a restatement (tests/lightgcl_twin.py), the step's determinism, the golden replay of the reference's fit()
from its recorded batches and factors, the model's own SVD, the evaluator's fused path against its generic one, the CLI."""
import numpy as np
import pytest

import lightgcl_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
CONFIG = dict(lr=1e-2, lambda1=0.2, d=64, gnn_layer=2, batch_size=256, svd_q=5, dropout=0.0, temp=0.2, lambda2=1e-4, epochs=3)


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="LightGCL", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, svd_factors=None, **kw):
    from skrec.recommender.LightGCL import LightGCL
    cfg = dict(CONFIG)
    cfg.update(kw)
    _seed()
    return LightGCL(_run_config(data_dir), cfg, svd_factors=svd_factors)


def _check_grad(name, got, want):
    """the tolerances of test_gpu_multvae.py::test_step_matches_float64_autograd"""
    print(name, "max abs err", np.abs(got - want).max(), "max |grad|", np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * np.abs(want).max(), err_msg=name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the InfoNCE kernels against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def _cl_case(rng, n, N, d, variant, inv_temp):
    """queries with repeated rows, a table; ``wide``: logits spanning +-60; ``small``: logits near log(1e-8 / N), so that
    sum exp is within a factor 10 of the 1e-8 inside the log"""
    base = (rng.standard_normal((max(2, (2 * n) // 3), d)) * 0.3).astype(np.float32)
    Q = base[rng.integers(0, len(base), n)]                  # about a third of the rows are repeats
    E = (rng.standard_normal((N, d)) * 0.3).astype(np.float32)
    s = Q.astype(np.float64) @ E.astype(np.float64).T * inv_temp
    if variant == "wide":
        E = (E * (60.0 / np.abs(s).max())).astype(np.float32)
    elif variant == "small":
        Q, E = Q * np.float32(0.2), E.copy()
        Q[:, 0], E[:, 0] = 1.0, np.float32(np.log(1e-8 / N) / inv_temp)
    return Q, E


def _cl(Q, E, inv_temp, weight):
    import torch
    from skrec import _hip
    L = _hip.lib()
    n, d = Q.shape
    N = E.shape[0]
    qp, ep = np.zeros((n, 64), np.float32), np.zeros((N, 64), np.float32)
    qp[:, :d], ep[:, :d] = Q, E
    dq, de = torch.from_numpy(qp).cuda(), torch.from_numpy(ep).cuda()
    gq, ge = torch.full((n + 1, 64), 7.0, device="cuda"), torch.full((N + 1, 64), 7.0, device="cuda")
    nb = int(L.skr_lightgcl_cl_workspace(n, N))
    assert nb > 0
    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    _hip.check(L.skr_lightgcl_cl(_hip.ptr(dq), n, _hip.ptr(de), N, inv_temp, weight, _hip.ptr(gq), _hip.ptr(ge), _hip.ptr(loss),
                                 _hip.ptr(work), nb, _hip.stream()))
    torch.cuda.synchronize()
    gq, ge, loss = gq.cpu().numpy(), ge.cpu().numpy(), loss.cpu().numpy()
    assert (gq[n] == 7.0).all() and (ge[N] == 7.0).all() and loss[1] == 7.0          # nothing beyond the outputs is written
    return gq[:n], ge[:N], loss[0]


@pytest.mark.parametrize("variant", ["plain", "wide", "small"])
@pytest.mark.parametrize("n,N,d", [(3, 70, 16), (37, 1000, 64), (130, 4099, 64), (4096, 257, 40)])
def test_cl_matches_float64_autograd(n, N, d, variant):
    """shapes: n off the 64-query chunk, N off the 64-row tile, padded columns, repeated query rows"""
    import torch
    rng = np.random.default_rng(n + N + d + len(variant))
    inv_temp, weight = 5.0, 0.2 / n
    Q, E = _cl_case(rng, n, N, d, variant, inv_temp)
    gq, ge, loss = _cl(Q, E, inv_temp, weight)
    q64, e64 = T.t64(Q, True), T.t64(E, True)
    s = q64 @ e64.T * inv_temp
    if variant == "wide":
        assert 59.0 < float(s.detach().abs().max()) < 61.0
    if variant == "small":
        tot = torch.exp(s.detach()).sum(1)
        assert float(tot.min()) > 1e-9 and float(tot.max()) < 1e-7
    want = weight * torch.log(torch.exp(s).sum(1) + 1e-8).sum()
    want.backward()
    print("loss", loss, want.item())
    np.testing.assert_allclose(loss, want.item(), rtol=1e-5)
    _check_grad("dQ", gq[:, :d], q64.grad.numpy())
    _check_grad("dE", ge[:, :d], e64.grad.numpy())
    assert not gq[:, d:].any() and not ge[:, d:].any()       # padded columns are exactly zero


# ---------------------------------------------------------------------------------------------------------------------
# 2. the whole step against the twin
# ---------------------------------------------------------------------------------------------------------------------
def _step_case(U, I, B, L, q, d, seed):
    """a bipartite CSR whose last user and last item have no entry, a batch with repeated ids, random factors (the step's
    arithmetic does not need them to be an SVD), parameters scaled so that the positive scores straddle +-5"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, min(12, I - 1), U)
    lens[U - 1] = 0
    rows = [np.sort(rng.choice(I - 1, n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate(rows)
    uids = rng.integers(0, U - 1, B).astype(np.int32)
    uids[:2] = uids[2]                                       # repeated ids for certain
    pos = np.array([rows[u][rng.integers(0, len(rows[u]))] for u in uids], np.int32)
    neg = rng.integers(0, I, B).astype(np.int32)
    neg[0], neg[1] = pos[1], I - 1                           # an item that is positive and negative, the zero-degree item
    E0 = (rng.standard_normal((U + I, d)) * (1.15 / np.sqrt(d))).astype(np.float32)
    fac = [(rng.standard_normal(s) * 0.3 / np.sqrt(s[0] if k >= 2 else s[1])).astype(np.float32)
           for k, s in enumerate(((U, q), (I, q), (q, U), (q, I)))]
    return dict(U=U, I=I, B=B, L=L, q=q, d=d, rowptr=rowptr, items=items, uids=uids, pos=pos, neg=neg, E0=E0, fac=fac)


def _twin(c, temp, lambda1, lambda2):
    A = T.t64(T.dense_adjacency(c["rowptr"], c["items"], c["I"]))
    eu, ei = T.t64(c["E0"][:c["U"]], True), T.t64(c["E0"][c["U"]:], True)
    comps, Eu, Ei, ps = T.losses_f64(eu, ei, A, tuple(T.t64(f) for f in c["fac"]), c["uids"], c["pos"], c["neg"], c["L"], temp,
                                     lambda1, lambda2)
    (comps[0] + comps[1]).backward()
    return [float(x.detach()) for x in comps], Eu.detach().numpy(), Ei.detach().numpy(), eu.grad.numpy(), ei.grad.numpy(), ps


def _detached(c, temp, lambda1, lambda2):
    import torch
    from skrec.recommender.LightGCL import LightGCL
    cfg = dict(lr=1e-2, lambda1=lambda1, d=c["d"], gnn_layer=c["L"], batch_size=c["B"], svd_q=c["q"], temp=temp, lambda2=lambda2)
    m = LightGCL.detached(c["U"], c["I"], cfg, (c["rowptr"], c["items"]), svd_factors=c["fac"])
    flat = np.zeros((c["U"] + c["I"], 64), np.float32)
    flat[:, :c["d"]] = c["E0"]
    m.E0.copy_(torch.from_numpy(flat).cuda())
    return m


SHAPES = [(70, 45, 16, 1, 3, 16), (300, 1000, 256, 2, 5, 64), (1000, 257, 2048, 3, 8, 40)]


@pytest.mark.parametrize("U,I,B,L,q,d,lambda1", [s + (0.2,) for s in SHAPES] + [SHAPES[0] + (0.0,)])
def test_step_matches_the_twin(U, I, B, L, q, d, lambda1):
    """every case: a zero-degree user and item, repeated ids, positive scores on both sides of +-5, none within 1e-3"""
    temp, lambda2 = 0.2, 1e-4
    c = _step_case(U, I, B, L, q, d, U + B)
    comps, Eu, Ei, gu, gi, ps = _twin(c, temp, lambda1, lambda2)
    assert c["rowptr"][U] == c["rowptr"][U - 1] and not (c["items"] == I - 1).any()
    assert len(np.unique(c["uids"])) < B
    if lambda1 > 0:
        for s in ps:
            s = s.detach().numpy()
            assert (np.abs(s) > 5).any() and (np.abs(s) < 5).any() and np.abs(np.abs(s) - 5).min() >= 1e-3
    m = _detached(c, temp, lambda1, lambda2)
    loss = m.gradient_step(c["uids"], c["pos"], c["neg"]).cpu().numpy()
    grad, sums = m._grad.cpu().numpy(), m.sums.cpu().numpy()
    print("loss", loss, "twin", comps)
    np.testing.assert_allclose(loss[0], comps[0], rtol=1e-5)
    if lambda1 > 0:
        np.testing.assert_allclose(loss[1], comps[1], rtol=1e-5)
    else:
        assert loss[1] == 0.0
    np.testing.assert_allclose(loss[2], comps[2], rtol=1e-5)
    np.testing.assert_allclose(loss[3], sum(comps), rtol=1e-5)
    np.testing.assert_allclose(sums[:U, :d], Eu, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sums[U:, :d], Ei, rtol=1e-5, atol=1e-6)
    _check_grad("E_u_0", grad[:U, :d], gu)
    _check_grad("E_i_0", grad[U:, :d], gi)
    assert not grad[:, d:].any() and not sums[:, d:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the step is bit-reproducible
# ---------------------------------------------------------------------------------------------------------------------
def test_step_is_deterministic():
    c = _step_case(*SHAPES[2], 5)
    m = _detached(c, 0.2, 0.2, 1e-4)
    outs = []
    for _ in range(2):
        loss = m.gradient_step(c["uids"], c["pos"], c["neg"]).cpu().numpy()
        outs.append((m._grad.cpu().numpy().copy(), loss))
    (g0, l0), (g1, l1) = outs
    assert np.count_nonzero(g0[:, :40]) > 0.9 * g0[:, :40].size
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 4. golden replay of the reference's fit() from its recorded batches and factors
# ---------------------------------------------------------------------------------------------------------------------
class _Recorded(object):
    """the reference's evaluator contract on recorded scores: predict() -> ndarray (the generic path)"""

    def __init__(self, users, scores):
        self.row = {int(u): r for r, u in enumerate(users)}
        self.scores = scores

    def predict(self, users):
        return self.scores[[self.row[int(u)] for u in users]]


def _gap_ok(ev, users, scores, gap=5e-6):
    """users whose 22 best unmasked reference scores are pairwise more than ``gap`` apart"""
    ok = np.zeros(len(users), bool)
    for r, u in enumerate(users):
        row = scores[r].astype(np.float64).copy()
        row[np.asarray(ev.user_pos_train.get(int(u), []), dtype=np.int64)] = -np.inf
        top = np.sort(row)[::-1][:22]
        ok[r] = np.min(top[:-1] - top[1:]) > gap
    return ok


def test_replays_reference(golden, tiny_dir, monkeypatch, tmp_path, fused_mode):
    monkeypatch.chdir(tmp_path)
    g = golden("golden_lightgcl")
    m = _model(tiny_dir, svd_factors=T.fixture_factors(g))
    assert (m.num_users, m.num_items) == (64, 96)
    eu, ei = m.parameters()
    assert np.array_equal(eu.cpu().numpy(), g["E_u_00"]) and np.array_equal(ei.cpu().numpy(), g["E_i_00"])   # same init, same seed
    np.testing.assert_allclose(m.adj.val.cpu().numpy(), g["adj_val"], rtol=2e-7)
    assert np.array_equal(m.adj.col.cpu().numpy(), g["adj_cols"])
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    losses, n_eval = [], 0
    for s, (uids, pos, neg) in enumerate(T.fixture_steps(g)):
        losses.append(m.train_step(uids, pos, neg).cpu().numpy())
        if (s + 1) % 3:
            continue
        report = np.array(list(m.evaluate().values()), np.float32)
        pred = m.predict(test_users)                         # the sums of the step's forward, not of the updated parameters
        ref = g["pred"][n_eval]
        print("evaluation", n_eval, "max score diff", np.abs(pred - ref).max(), "allowed", 6 * dev_s[n_eval])
        assert np.abs(pred - ref).max() <= 6 * dev_s[n_eval]
        rows, _, n = ev.per_user_rows(m, test_users)
        rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, ref), test_users)
        ok = _gap_ok(ev, test_users, ref)
        print("users left out", int((~ok).sum()))
        assert n == 63 and (~ok).sum() <= 3
        assert np.array_equal(rows[ok], rows_ref[ok])
        if ok.all():
            np.testing.assert_allclose(report, g["reports"][n_eval], rtol=1e-5, atol=0, err_msg=str(g["names"]))
        n_eval += 1
    assert n_eval == 3
    losses = np.stack(losses)
    print("loss", losses[:, 3], "golden", g["loss"])
    np.testing.assert_allclose(losses[:, 3], g["loss"], rtol=1e-5)
    eu, ei = (t.cpu().numpy() for t in m.parameters())
    print("E_u_0 max abs diff", np.abs(eu - g["E_u_01"]).max(), "allowed", 6 * dev_p[0])
    print("E_i_0 max abs diff", np.abs(ei - g["E_i_01"]).max(), "allowed", 6 * dev_p[1])
    assert np.abs(eu - g["E_u_01"]).max() <= 6 * dev_p[0]
    assert np.abs(ei - g["E_i_01"]).max() <= 6 * dev_p[1]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the model's own SVD
# ---------------------------------------------------------------------------------------------------------------------
def test_own_svd_on_the_tiny_set(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(tiny_dir)
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    A = T.dense_adjacency(rowptr, items, ni)
    ums, vms, ut, vt = (t.cpu().numpy().astype(np.float64) for t in (m.u_mul_s, m.v_mul_s, m.ut, m.vt))
    assert ums.shape == (64, 5) and vms.shape == (96, 5) and ut.shape == (5, 64) and vt.shape == (5, 96)
    for f in (ut, vt):                                       # orthonormal (the reference's own factors: <= 1.2e-6)
        print("orthonormality", np.abs(f @ f.T - np.eye(5)).max())
        assert np.abs(f @ f.T - np.eye(5)).max() <= 1e-5
    sv = np.linalg.svd(A, compute_uv=False)
    best = np.sqrt((sv[5:] ** 2).sum())                      # the optimum of a rank-5 approximation
    err = np.linalg.norm(A - ums @ vt)
    print("|A - u_mul_s vt|_F", err, "optimum", best, "ratio", err / best)
    # the reference's own factors: 1.0136-1.0146 x the optimum over three seeds; the bound is twice that excess
    assert err <= 1.03 * best
    assert np.abs(ums @ vt - (vms @ ut).T).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 6. the evaluator's fused path against its generic path, evaluate() before training, the command line
# ---------------------------------------------------------------------------------------------------------------------
class _PredictOnly(object):
    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def test_fused_path_equals_generic_path(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SKR_FUSED_MODE", "fp32")
    m = _model(tiny_dir, epochs=1)
    # evaluate() before any training step: one forward propagation of the initial parameters
    first = m.evaluate()
    assert np.isfinite(np.array(list(first.values()))).all()
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    A = T.t64(T.dense_adjacency(rowptr, items, ni))
    eu, ei = (T.t64(t.cpu().numpy()) for t in m.parameters())
    Eu, Ei, _, _ = T.forward_f64(eu, ei, A, tuple(T.t64(t.cpu().numpy()) for t in (m.u_mul_s, m.v_mul_s, m.ut, m.vt)), 2)
    np.testing.assert_allclose(m.sums[:64].cpu().numpy(), Eu.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m.sums[64:].cpu().numpy(), Ei.numpy(), rtol=1e-5, atol=1e-6)
    best = m.fit()
    assert np.isfinite(np.array(list(best.values()))).all() and len(m.step_losses) == 3
    ev = m.evaluator
    users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    rows_dev, _, n_dev = ev.per_user_rows(m, users)
    rows_gen, _, n_gen = ev.per_user_rows(_PredictOnly(m), users)
    assert n_dev == n_gen == len(users) == 63
    assert np.array_equal(rows_dev, rows_gen)


def test_run_skrec_cli(tiny_dir, tmp_path):
    import os
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "LightGCL", "--data_dir", tiny_dir, "--d", "32", "--epochs", "1",
                        "--batch_size", "128", "--top_k", "[5,10]", "--metric", "['Recall','NDCG']", "--seed", "7"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 0:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# 7. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
RTOL, ATOL = 1e-4, 2e-5        # _check_grad's
TEMP, LAMBDA1, LAMBDA2 = 0.2, 0.2, 1e-4


def _twin_run(c, dtype, valid=None):
    """the twin in ``dtype`` -> ((bpr, cl, reg), gradient of bpr + cl with respect to E_0 [U + I, d] in float64, the user
    side's and the item side's contrastive logits over temp)"""
    import torch
    U = c["U"]
    A = torch.tensor(T.dense_adjacency(c["rowptr"], c["items"], c["I"]), dtype=dtype)
    eu, ei = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (c["E0"][:U], c["E0"][U:]))
    fac = tuple(torch.tensor(f, dtype=dtype) for f in c["fac"])
    comps, Eu, Ei, _ = T.losses_f64(eu, ei, A, fac, c["uids"], c["pos"], c["neg"], c["L"], TEMP, LAMBDA1, LAMBDA2, valid=valid)
    (comps[0] + comps[1]).backward()
    with torch.no_grad():
        _, _, Gu, Gi = T.forward_f64(eu, ei, A, fac, c["L"])
        ok_u = np.ones(c["B"], bool) if valid is None else valid[0]
        ok_i = np.ones(2 * c["B"], bool) if valid is None else np.concatenate(valid[1:])
        iids = np.concatenate([c["pos"], c["neg"]])
        logits = ((Gu[c["uids"][ok_u]] @ Eu.T / TEMP).numpy(), (Gi[iids[ok_i]] @ Ei.T / TEMP).numpy())
    return [x.item() for x in comps], np.vstack([eu.grad.numpy(), ei.grad.numpy()]).astype(np.float64), logits


def _edge_compare(c, what, valid=None, floor=None, widen=False, m=None):
    """The device step on the batch of ``c`` against the float64 twin, which skips the ids that ``valid`` marks as out of range.
    ``floor``: each side's scale is max|want| or that of a batch without the exact cancellation, whichever is more.  ``widen``:
    allow max(ATOL * scale, 4 x the error of the same twin in float32 on the CPU), both printed"""
    import torch
    U, d = c["U"], c["d"]
    comps, G, _ = _twin_run(c, torch.float64, valid)
    comps32, G32, _ = _twin_run(c, torch.float32, valid) if widen else (comps, None, None)
    m = _detached(c, TEMP, LAMBDA1, LAMBDA2) if m is None else m
    loss = m.gradient_step(c["uids"], c["pos"], c["neg"]).cpu().numpy()
    want, want32 = (np.array(x + [sum(x)], np.float64) for x in (comps, comps32))
    print(what, "loss", loss, "twin", want, "abs err", np.abs(loss - want), "fp32-CPU err", np.abs(want32 - want))
    assert np.isfinite(loss).all()
    assert np.all(np.abs(loss - want) <= np.maximum(1e-5 * np.abs(want), 4 * np.abs(want32 - want)))
    grad = m._grad.cpu().numpy()
    assert np.isfinite(grad).all() and not grad[:, d:].any()
    for name, rows in (("E_u_0", slice(0, U)), ("E_i_0", slice(U, None))):     # both tensors are measured before the assertion
        w = G[rows]
        scale = float(np.abs(w).max())
        if floor is not None:
            scale = max(scale, float(np.abs(floor[rows]).max()))
        err = np.abs(grad[rows, :d].astype(np.float64) - w)
        atol = ATOL * scale
        if widen:
            err32 = float(np.abs(G32[rows] - w).max())
            atol = max(atol, 4 * err32)
            print(f"{what}: {name}: max abs err {err.max():.3e}, scale {scale:.3e}, fp32-CPU err {err32:.3e}")
        else:
            print(f"{what}: {name}: max abs err {err.max():.3e}, scale {scale:.3e}")
        assert np.all(err <= atol + RTOL * np.abs(w)), (what, name, float(err.max()), scale)
    return loss, grad, m


@pytest.mark.parametrize("d", [64, 40])
@pytest.mark.parametrize("B", [15, 16, 17, 63, 64, 65])
def test_batch_sizes_around_the_tiles(B, d):
    """below, at and above 16 and 64 pairs: the item side's 2 B queries cross the 64-query chunk of the InfoNCE passes at B = 32
    and again here at 2 B = 126, 128, 130"""
    c = _step_case(150, 130, B, 2, 5, d, 1000 + B + d)
    assert len(np.unique(c["uids"])) < B and (c["neg"] == 129).any()
    _edge_compare(c, f"B = {B}, d = {d}")


def test_full_batch_at_sixteen_factors():
    """B = 2048 at q = SKR_LIGHTGCL_MAX_Q = 16 and L = 3 on a 2100 x 2100 graph: 4096 item-side queries =
    SKR_LIGHTGCL_MAX_QUERIES; then the same call again: the same bits; one pair more is refused"""
    import time
    import torch
    from skrec import _hip
    t0 = time.time()
    assert _hip.SKR_LIGHTGCL_MAX_Q == 16 and _hip.SKR_LIGHTGCL_MAX_QUERIES == 4096
    c = _step_case(2100, 2100, 2048, 3, 16, 64, 2100)
    loss, _, m = _edge_compare(c, "B = 2048", widen=True)
    g1, s1 = m._grad.clone(), m.sums.clone()
    m._work.fill_(255)
    m._grad.fill_(3.0)
    loss2 = m.gradient_step(c["uids"], c["pos"], c["neg"]).cpu().numpy()
    assert np.array_equal(loss.view(np.uint32), loss2.view(np.uint32)) and torch.equal(g1, m._grad) and torch.equal(s1, m.sums)
    z = np.zeros(2049, np.int32)
    with pytest.raises(NotImplementedError, match="at most 2048"):
        m.gradient_step(z, z, z)
    print("full batch: wall time", time.time() - t0)


def test_one_factor():
    """q = 1: one column of the [N, 16] factor tables is in use"""
    _edge_compare(_step_case(150, 130, 37, 2, 1, 64, 1100), "q = 1")


@pytest.mark.parametrize("B", [37, 300])
@pytest.mark.parametrize("which", ["user", "item"])
def test_one_id_in_every_row(which, B):
    """the longest segment: all B ranks of the user list, or all 2 B ranks of the item list (pos and neg together), name one id,
    so one wavefront of seg_add walks them all and the prep kernel counts B (2 B) equal keys.  With pos = neg every BPR argument
    is 0 and the term's gradients cancel exactly: the scales are floored by the same users with the case's random items"""
    import torch
    c = _step_case(150, 130, B, 2, 5, 64, 3000 + B)
    floor = _twin_run(c, torch.float64)[1]
    if which == "user":
        c["uids"][:] = c["uids"][B - 1]
    else:
        c["pos"][:] = c["pos"][B - 1]
        c["neg"][:] = c["pos"][B - 1]
    loss, _, _ = _edge_compare(c, f"one {which}, B = {B}", floor=floor)
    if which == "item":
        np.testing.assert_allclose(loss[0], np.log(2.0), rtol=1e-5)


def test_ids_out_of_range_are_skipped():
    """each id on its own, as the header says: a pair's BPR term needs its three ids, a user's (an item's) log-sum-exp and
    positive score that id alone, and 70 and 140 stay the divisors.  Then rows whose three ids are all out of range: the
    device's own result on the batch without them, scaled by 65 / 70"""
    U, I, B = 150, 130, 70
    c = _step_case(U, I, B, 2, 5, 64, 4000)
    uids, pos, neg = c["uids"], c["pos"], c["neg"]
    keep = uids.copy(), pos.copy(), neg.copy()
    uids[3], pos[17], uids[40], neg[40], neg[69] = U, -1, -7, I, 2 ** 31 - 1
    valid = ((uids >= 0) & (uids < U), (pos >= 0) & (pos < I), (neg >= 0) & (neg < I))
    assert [int(v.sum()) for v in valid] == [68, 69, 68] and (valid[0] & valid[1] & valid[2]).sum() == 66
    _, _, m = _edge_compare(c, "ids out of range", valid=valid)
    bad = np.array([3, 17, 40, 41, 69])
    c["uids"], c["pos"], c["neg"] = keep
    keep[0][bad], keep[1][bad], keep[2][bad] = (U, -1, -7, U + 5, 2 ** 31 - 1), (I, -1, -7, I + 5, 2 ** 31 - 1), (-3, I, I + 1, -1, 2 ** 31 - 1)
    ok = np.ones(B, bool)
    ok[bad] = False
    loss = m.gradient_step(*keep).cpu().numpy()
    g = m._grad.cpu().numpy().copy()
    loss2 = m.gradient_step(*(a[ok] for a in keep)).cpu().numpy()
    g2 = m._grad.cpu().numpy()
    np.testing.assert_allclose(loss[:2], loss2[:2] * 65 / 70, rtol=1e-5)
    np.testing.assert_allclose(g, g2 * np.float32(65 / 70), rtol=RTOL, atol=ATOL * np.abs(g).max())


def test_an_empty_batch_writes_nothing():
    import ctypes
    import torch
    from skrec import _hip
    c = _step_case(150, 130, 17, 2, 5, 64, 5000)
    m = _detached(c, TEMP, LAMBDA1, 0.0)
    loss = torch.full((4,), 7.0, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    a = m._step_args(ids, ids, ids, loss)
    a.n = 0
    m._grad.fill_(3.0)
    m._work.fill_(5)
    tabs = [m.sums, m._below, m._ping[0], m._ping[1], m._gsum, m._addend]
    for t in tabs:
        t.fill_(2.0)
    before = [t.clone() for t in tabs] + [m._work.clone(), m._flat.clone()]
    _hip.check(_hip.lib().skr_lightgcl_step(ctypes.byref(a), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (m._grad == 3.0).all()
    assert all(torch.equal(x, y) for x, y in zip(before, tabs + [m._work, m._flat]))
    # through the class: a zero loss, a zero gradient, and the sums are not claimed to be those of the parameters
    z = np.zeros(0, np.int32)
    loss = m.gradient_step(z, z, z)
    assert loss.shape == (4,) and not loss.any() and not m._grad.any() and not m._sums_current
    m.gradient_step(c["uids"], c["pos"], c["neg"])
    assert m._grad.any() and m._sums_current
    assert not m.gradient_step(z, z, z).any() and not m._grad.any()
    # train_step: the zero gradient through Adam, as MGCN, LATTICE and SLMRec do it; with no moments yet and no weight decay
    # (lambda2 = 0: the decay term does not depend on the batch) nothing moves
    m.gradient_step(c["uids"], c["pos"], c["neg"])
    flat = m._flat.clone()
    assert not m.train_step(z, z, z).any()
    assert torch.equal(flat, m._flat)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_contrastive_logits_of_two_hundred(sign):
    """E_0 scaled (the logits are quadratic in the factor) until the user side's logits over temp reach +200 (exp overflows fp32:
    a log-sum-exp that does not take the running maximum off first gives inf) or -200 (such an exp underflows to 0)"""
    import torch
    c = _step_case(150, 130, 100, 2, 5, 64, 6000)
    lg = _twin_run(c, torch.float64)[2][0]
    c["E0"] = (c["E0"] * np.sqrt(200.0 / (lg.max() if sign > 0 else -lg.min()))).astype(np.float32)
    lu, li = _twin_run(c, torch.float64)[2]
    print("logits over temp: users min", lu.min(), "max", lu.max(), "items min", li.min(), "max", li.max())
    if sign > 0:
        assert 199 < lu.max() < 201 and np.isinf(np.exp(np.float32(lu.max())))
    else:
        assert -201 < lu.min() < -199 and np.exp(np.float32(lu.min())) == 0
    _edge_compare(c, f"logits of {sign * 200}", widen=True)
