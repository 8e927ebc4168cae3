"""GPU suite of SelfCF (csrc/selfcf.hip, skr_spmm_plan_run_dropped of csrc/spmm.hip, skrec/recommender/SelfCF.py): the dropped
plan run against the float64 product of the masked matrix, the keep arrays against their numpy mirror, the whole step against
float64 autograd of a restatement (tests/selfcf_twin.py), the step's determinism, the golden replay of the reference's fit()
from its recorded batches, rates and masks, fit() with device draws, the CLI, the limits."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import selfcf_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
CONFIG = dict(lr=1e-2, reg=1e-3, embed_dim=64, n_layers=2, dropout=0.5, batch_size=256, epochs=3)


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="SelfCF", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    from skrec.recommender.SelfCF import SelfCF
    cfg = dict(CONFIG)
    cfg.update(kw)
    _seed()
    return SelfCF(_run_config(data_dir), cfg)


def _check_grad(name, got, want):
    """the tolerances of test_gpu_dens.py / test_gpu_lightgcl.py for a gradient against float64 autograd"""
    print(name, "max abs err", np.abs(got - want).max(), "max |grad|", np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * np.abs(want).max(), err_msg=name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the dropped plan run
# ---------------------------------------------------------------------------------------------------------------------
def _epilogue(addend=None, Y=None, accum=None, accum_scale=1.0, mode=0):
    from skrec import _hip
    ep = _hip.SpmmEpilogue()
    ep.mode = mode
    ep.addend, ep.Y, ep.accum = _hip.ptr(addend), _hip.ptr(Y), _hip.ptr(accum)
    ep.accum_scale = accum_scale
    return ep


@pytest.mark.parametrize("n_rows,n_cols,long_from", [(300, 40_000, 2), (64, 200_000, 100), (7, 5, 2)])
def test_dropped_run_matches_the_masked_product(n_rows, n_cols, long_from):
    """the matrices of test_gpu_train.py::test_spmm_plan_rectangular_blocks_and_determinism (long rows across several column
    blocks, tasks of every length, rows at the threshold, empty rows; the first case has rows dense enough for the plan's
    LDS-streamed path, which a dropped run must not take) at keep rates 0.5 and 0.1, one row fully dropped, one long row
    fully kept"""
    import torch
    from gpu_utils import dev, to_dev
    from skrec import _hip
    L = _hip.lib()
    rng = np.random.default_rng(n_rows * 7 + long_from)
    lens = np.minimum(rng.integers(0, 40, n_rows) ** 2 // 3, n_cols)
    lens[rng.integers(0, n_rows, max(1, n_rows // 50))] = min(n_cols, 3000)          # long rows across many blocks
    lens[0] = 0
    if long_from >= 2 and n_rows > 3:
        lens[1], lens[2] = min(long_from, n_cols), min(long_from, n_cols) - 1          # exactly at / just under the threshold
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(n_cols, l, replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    if n_rows > 5 and lens[5] > 0:
        b, e = rowptr[5], rowptr[6]
        col[b:e] = np.arange(n_cols - (e - b), n_cols)                                 # only the last columns
    val = rng.standard_normal(len(col)).astype(np.float32)
    nnz = len(col)
    X = rng.standard_normal((n_cols, 64)).astype(np.float32)
    add = rng.standard_normal((n_rows, 64)).astype(np.float32)
    acc0 = rng.standard_normal((n_rows, 64)).astype(np.float32)
    d_rp, d_col, d_val = to_dev(rowptr), to_dev(col), to_dev(val)
    dX, dadd = to_dev(X), to_dev(add)
    h = C.c_void_p()
    _hip.check(L.skr_spmm_plan_create(n_rows, n_cols, _hip.ptr(d_rp), _hip.ptr(d_col), _hip.ptr(d_val), nnz, long_from, C.byref(h), _hip.stream()))
    info = (C.c_int64 * 4)()
    _hip.check(L.skr_spmm_plan_info(h, info))
    thr = long_from or 512
    assert (info[0] & 0xffffffff) == int((lens >= thr).sum()) > 0
    if n_rows == 300:
        assert (info[0] >> 32) > 0                           # the plan has hot rows
    longest = int(np.argmax(lens))
    dropped = int([r for r in np.flatnonzero(lens > 0) if r != longest][-1])
    assert lens[longest] >= thr
    X64 = X.astype(np.float64)
    for rate in (0.5, 0.9):
        keep = (rng.random(nnz) >= rate).astype(np.uint8)
        keep[rowptr[dropped]:rowptr[dropped + 1]] = 0        # one row fully dropped
        keep[rowptr[longest]:rowptr[longest + 1]] = 1        # one long row fully kept
        scale = np.float32(1.0 / (1.0 - rate))
        d_keep = to_dev(keep)
        outs = []
        for rep in range(3):
            Y = torch.full((n_rows, 64), 7.0, device=dev())
            acc = to_dev(acc0.copy())
            ep = _epilogue(addend=dadd, Y=Y, accum=acc, accum_scale=0.5)
            _hip.check(L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 64, C.byref(ep), _hip.ptr(d_keep), float(scale), _hip.stream()))
            torch.cuda.synchronize()
            outs.append((Y.cpu().numpy(), acc.cpu().numpy()))
        for y, a in outs[1:]:
            assert np.array_equal(y.view(np.int32), outs[0][0].view(np.int32)) and np.array_equal(a.view(np.int32), outs[0][1].view(np.int32))
        A = sp.csr_matrix(((val * scale).astype(np.float64) * keep, col, rowptr), shape=(n_rows, n_cols))   # one fp32 multiply
        want = A @ X64 + add
        mass = abs(A) @ np.abs(X64) + np.abs(add)
        y, a = outs[0]
        print("rate", rate, "max err", np.abs(y - want).max(), "kept", keep.mean())
        assert np.all(np.abs(y - want) <= 2e-6 * mass + 1e-6)
        assert np.all(np.abs(a - (acc0 + 0.5 * want)) <= 2e-6 * (mass + np.abs(acc0)) + 1e-6)
        assert np.array_equal(y[dropped], add[dropped]) and np.array_equal(y[0], add[0])     # nothing kept / empty: y = addend
    # all-ones keep with scale 1 against the plain run: the same sums, possibly in another order (the hot rows)
    ones = to_dev(np.ones(max(nnz, 1), np.uint8))
    Yd, Yp = torch.full((n_rows, 64), 7.0, device=dev()), torch.full((n_rows, 64), 7.0, device=dev())
    accd, accp = to_dev(acc0.copy()), to_dev(acc0.copy())
    epd, epp = _epilogue(addend=dadd, Y=Yd, accum=accd, accum_scale=0.5), _epilogue(addend=dadd, Y=Yp, accum=accp, accum_scale=0.5)
    _hip.check(L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 64, C.byref(epd), _hip.ptr(ones), 1.0, _hip.stream()))
    _hip.check(L.skr_spmm_plan_run_ex(h, _hip.ptr(dX), 64, C.byref(epp), None, None, _hip.stream()))
    torch.cuda.synchronize()
    A1 = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n_rows, n_cols))
    mass1 = abs(A1) @ np.abs(X64) + np.abs(add)
    assert np.all(np.abs(Yd.cpu().numpy() - Yp.cpu().numpy()) <= 1e-6 * mass1 + 1e-7)
    assert np.all(np.abs(accd.cpu().numpy() - accp.cpu().numpy()) <= 1e-6 * (mass1 + np.abs(acc0)) + 1e-7)
    # accum alone (no Y), and the argument checks
    acc = to_dev(acc0.copy())
    ep = _epilogue(accum=acc, accum_scale=0.5)
    _hip.check(L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 64, C.byref(ep), _hip.ptr(ones), 1.0, _hip.stream()))
    torch.cuda.synchronize()
    want1, mass0 = A1 @ X64, abs(A1) @ np.abs(X64)
    assert np.all(np.abs(acc.cpu().numpy() - (acc0 + 0.5 * want1)) <= 2e-6 * (mass0 + np.abs(acc0)) + 1e-6)
    Y = torch.empty((n_rows, 64), device=dev())
    for mode in (1, 2, 3):
        ep = _epilogue(Y=Y, mode=mode)
        assert L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 64, C.byref(ep), _hip.ptr(ones), 1.0, _hip.stream()) == -1
        assert b"plain" in L.skr_last_error()
    ep = _epilogue(Y=Y)
    assert L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 32, C.byref(ep), _hip.ptr(ones), 1.0, _hip.stream()) == -1
    assert L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 64, C.byref(ep), None, 1.0, _hip.stream()) == -1
    ep = _epilogue(Y=dX)
    assert L.skr_spmm_plan_run_dropped(h, _hip.ptr(dX), 64, C.byref(ep), _hip.ptr(ones), 1.0, _hip.stream()) == -1
    _hip.check(L.skr_spmm_plan_destroy(h))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the keep arrays
# ---------------------------------------------------------------------------------------------------------------------
def _graph(U, I, rng, max_len=10):
    """a bipartite CSR whose last user and last item have no entry"""
    lens = rng.integers(1, max_len, U)
    lens[U - 1] = 0
    rows = [np.sort(rng.choice(I - 1, n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    return rowptr, np.concatenate(rows), rows


def _keeps(perm, nnz, k1, k2, rate, seed, step):
    import torch
    from gpu_utils import dev, to_dev
    from skrec import _hip
    out = torch.full((4, nnz + 1), 9, dtype=torch.uint8, device=dev())
    d_perm = to_dev(np.asarray(perm, np.int32))
    d1, d2 = (None, None) if k1 is None else (to_dev(k1), to_dev(k2))
    _hip.check(_hip.lib().skr_selfcf_keeps(_hip.ptr(d_perm), nnz, _hip.ptr(d1), _hip.ptr(d2), rate, seed, step, _hip.ptr(out[0]),
                                           _hip.ptr(out[1]), _hip.ptr(out[2]), _hip.ptr(out[3]), _hip.stream()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:, nnz] == 9).all()                          # nothing beyond the outputs is written
    return out[:, :nnz]


def test_keeps_equal_the_mirror_and_device_draws_follow_the_rate():
    rng = np.random.default_rng(3)
    rowptr, items, _ = _graph(48, 40, rng)
    nnz = len(items)
    _, perm = T.transpose_order(rowptr, items)
    k1, k2 = (rng.random(nnz) < 0.6).astype(np.uint8), (rng.random(nnz) < 0.6).astype(np.uint8)
    got = _keeps(perm, nnz, k1, k2, 0.0, 0, 0)
    for g, w in zip(got, T.mirror_keeps(perm, k1, k2)):
        assert np.array_equal(g, w)
    # device draws: the kept share at rate 0.3 over 200 k entries (sigma of the share: 1e-3), equal for equal (seed, step)
    n = 200_000
    perm = rng.permutation(n)
    a = _keeps(perm, n, None, None, 0.3, 17, 5)
    for arr in a:
        assert set(np.unique(arr)) == {0, 1}
        print("kept share", arr.mean())
        assert abs(arr.mean() - 0.7) <= 0.005
    assert np.array_equal(a[2], a[1][perm])                  # k2 in A's order
    assert np.array_equal(a[3][perm], a[0])                  # k1 in At's order
    assert not np.array_equal(a[0], a[1])                    # the two halves are drawn independently
    assert abs((a[0] & a[1]).mean() - 0.49) <= 0.01
    assert np.array_equal(a, _keeps(perm, n, None, None, 0.3, 17, 5))
    b = _keeps(perm, n, None, None, 0.3, 17, 6)
    assert not np.array_equal(a[0], b[0]) and abs((a[0] == b[0]).mean() - 0.58) <= 0.01     # 0.7^2 + 0.3^2
    assert not np.array_equal(a[0], _keeps(perm, n, None, None, 0.3, 18, 5)[0])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the whole step against the twin
# ---------------------------------------------------------------------------------------------------------------------
def _step_case(n, L, d, seed, U=48, I=40):
    """U = 48, I = 40, the last user and the last item isolated; a batch with repeated users and items, the isolated user and
    item (n >= 3), one user whose edges are all dropped, one target row with all 64 flags zero"""
    rng = np.random.default_rng(seed)
    rowptr, items, rows = _graph(U, I, rng)
    nnz = len(items)
    users = rng.integers(0, U - 1, n).astype(np.int32)
    its = np.array([rows[u][rng.integers(0, len(rows[u]))] for u in users], np.int32)
    if n >= 3:
        users[1], its[1] = U - 1, I - 1                      # the isolated user and the isolated item
        users[2], its[2] = users[0], its[0]                  # a repeated user and a repeated item for certain
    rate = 0.3
    k1, k2 = (rng.random(nnz) >= rate).astype(np.uint8), (rng.random(nnz) >= rate).astype(np.uint8)
    k1[rowptr[users[0]]:rowptr[users[0] + 1]] = 0            # every edge of the first row's user is dropped
    ku, ki = (rng.random((n, 64)) >= 0.5).astype(np.uint8), (rng.random((n, 64)) >= 0.5).astype(np.uint8)
    ki[0] = 0                                                # a zero target: both norms' clamp, a zero gradient
    P = {"user_emb": (rng.standard_normal((U, d)) * 0.3).astype(np.float32), "item_emb": (rng.standard_normal((I, d)) * 0.3).astype(np.float32),
         "predictor.weight": (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32),
         "predictor.bias": (rng.standard_normal(d) * 0.1).astype(np.float32)}
    return dict(U=U, I=I, n=n, L=L, d=d, rowptr=rowptr, items=items, users=users, its=its, rate=rate, k1=k1, k2=k2, ku=ku, ki=ki, P=P)


def _detached(c, reg=1e-2, dropout=0.5):
    from skrec.recommender.SelfCF import SelfCF
    cfg = dict(lr=1e-2, reg=reg, embed_dim=c["d"], n_layers=c["L"], dropout=dropout, batch_size=max(c["n"], 1))
    m = SelfCF.detached(c["U"], c["I"], cfg, (c["rowptr"], c["items"]), seed=SEED)
    m.load_parameters(c["P"])
    return m


@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("L", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 3, 64, 300])
def test_step_matches_float64_autograd(n, L, d):
    reg, dropout = 1e-2, 0.5
    c = _step_case(n, L, d, 100 * n + 10 * L + d)
    U, I = c["U"], c["I"]
    assert c["rowptr"][U] == c["rowptr"][U - 1] and not (c["items"] == I - 1).any()
    if n >= 3:
        assert len(np.unique(c["users"])) < n and len(np.unique(c["its"])) < n and (c["users"] == U - 1).any() and (c["its"] == I - 1).any()
    m = _detached(c, reg, dropout)
    val = m.adj.val.cpu().numpy()[:len(c["items"])]
    np.testing.assert_allclose(val, T.normalised_values(c["rowptr"], c["items"], I), rtol=2e-7)
    assert np.array_equal(m.perm.cpu().numpy(), T.transpose_order(c["rowptr"], c["items"])[1])
    scale = float(np.float32(1.0 / (1.0 - c["rate"])))
    R1, R2t = (T.t64(a) for a in T.masked_blocks(c["rowptr"], c["items"], I, val, c["k1"], c["k2"], scale))
    P = {k: T.t64(v, True) for k, v in c["P"].items()}
    (cos, regl), Mu, Mi = T.losses_f64(P["user_emb"], P["item_emb"], P["predictor.weight"], P["predictor.bias"], R1, R2t, c["users"],
                                       c["its"], c["ku"][:, :d], c["ki"][:, :d], L, dropout, reg)
    (cos + regl).backward()
    if L > 0:
        assert not R1[c["users"][0]].any()                   # the user whose edges are all dropped
    loss = m.gradient_step(c["users"], c["its"], rate=c["rate"], edge_keep=(c["k1"], c["k2"]), target_keep=(c["ku"], c["ki"])).cpu().numpy()
    print("loss", loss, "twin", cos.item(), regl.item())
    np.testing.assert_allclose(loss[0], cos.item(), rtol=1e-5)
    np.testing.assert_allclose(loss[1], regl.item(), rtol=1e-5)
    np.testing.assert_allclose(loss[2], cos.item() + regl.item(), rtol=1e-5)
    Mg = m.M.cpu().numpy()
    np.testing.assert_allclose(Mg[:U, :d], Mu.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(Mg[U:, :d], Mi.detach().numpy(), rtol=1e-5, atol=1e-6)
    G = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    for name in T.PARAMS:
        _check_grad(name, G[name], P[name].grad.numpy())
    # padding columns stay zero: the tables, the whole gradient buffer
    N = U + I
    flat = m._grad.cpu().numpy()
    rows, Wp, bp = flat[:N * 64].reshape(N, 64), flat[N * 64:N * 64 + 4096].reshape(64, 64), flat[N * 64 + 4096:]
    assert not rows[:, d:].any() and not Mg[:, d:].any() and not Wp[d:].any() and not Wp[:, d:].any() and not bp[d:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the step is bit-reproducible
# ---------------------------------------------------------------------------------------------------------------------
def test_step_is_deterministic():
    c = _step_case(300, 3, 64, 5)
    m = _detached(c)
    outs = []
    for _ in range(2):
        loss = m.gradient_step(c["users"], c["its"], rate=c["rate"], edge_keep=(c["k1"], c["k2"]), target_keep=(c["ku"], c["ki"])).cpu().numpy()
        outs.append((m._grad.cpu().numpy().copy(), loss))
    (g0, l0), (g1, l1) = outs
    assert np.count_nonzero(g0) > 0.8 * g0.size
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 5. golden replay of the reference's fit() from its recorded batches, rates and masks
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
    g = golden("golden_selfcf")
    m = _model(tiny_dir)
    assert (m.num_users, m.num_items) == (64, 96)
    P0 = m.parameters()
    for name, want in T.fixture_params(g, 0).items():
        assert np.array_equal(P0[name].cpu().numpy(), want), name        # same init, same seed
    np.testing.assert_allclose(m.adj.val.cpu().numpy(), g["adj_val"], rtol=2e-7)
    np.testing.assert_allclose(m.adj_t.val.cpu().numpy(), g["adj_t_val"], rtol=2e-7)
    assert np.array_equal(m.adj.col.cpu().numpy(), g["adj_cols"]) and np.array_equal(m.adj_t.col.cpu().numpy(), g["adj_t_cols"])
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    losses, n_eval = [], 0
    for s, st in enumerate(T.fixture_steps(g)):
        losses.append(m.train_step(st["users"], st["items"], rate=st["rate"], edge_keep=(st["k1"], st["k2"]),
                                   target_keep=(st["ku"], st["ki"])).cpu().numpy())
        if (s + 1) % 3:
            continue
        report = np.array(list(m.evaluate().values()), np.float32)
        pred = m.predict(test_users)
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
    print("loss", losses[:, 2], "golden", g["loss"])
    np.testing.assert_allclose(losses[:, 2], g["loss"], rtol=1e-5)
    P1 = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    for k, (name, want) in enumerate(T.fixture_params(g, 1).items()):
        print(name, "max abs diff", np.abs(P1[name] - want).max(), "allowed", 6 * dev_p[k])
        assert np.abs(P1[name] - want).max() <= 6 * dev_p[k]


# ---------------------------------------------------------------------------------------------------------------------
# 6. fit() with device draws, the command line, the limits
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_with_device_draws_learns(tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(tiny_dir)
    reports = []
    orig = m.evaluate

    def evaluate(tu=None):
        r = orig(tu)
        reports.append(dict(r.items()))
        return r
    m.evaluate = evaluate
    best = m.fit()
    assert np.isfinite(np.array(list(best.values()))).all() and len(reports) == 3 and len(m.step_losses) == 3
    import torch
    assert torch.isfinite(torch.stack(m.step_losses)).all()
    print("NDCG@10", [r["NDCG@10"] for r in reports])
    assert reports[-1]["NDCG@10"] > reports[0]["NDCG@10"]


def test_run_skrec_cli(tiny_dir, tmp_path):
    import os
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "SelfCF", "--data_dir", tiny_dir, "--embed_dim", "32", "--epochs", "1",
                        "--batch_size", "128", "--top_k", "[5,10]", "--metric", "['Recall','NDCG']", "--seed", "7"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 0:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout


@pytest.mark.parametrize("kw,msg", [(dict(embed_dim=65), "embed_dim <= 64"), (dict(n_layers=5), "n_layers <= 4"),
                                    (dict(batch_size=2049), "batch_size <= 2048")])
def test_each_limit_raises(tiny_dir, monkeypatch, tmp_path, kw, msg):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match=msg):
        _model(tiny_dir, **kw)
    m = _model(tiny_dir)
    with pytest.raises(NotImplementedError, match="at most 2048"):
        m.gradient_step(np.zeros(2049, np.int32), np.zeros(2049, np.int32))
    from skrec.recommender.SelfCF import SelfCFConfig, check_limits
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(SelfCFConfig(**CONFIG), world=2)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
RTOL, ATOL = 1e-4, 2e-5        # _check_grad's


def _twin_run(c, m, rows, dtype, reg, dropout=0.5, n_div=None):
    """the twin in ``dtype`` on the batch rows ``rows`` of ``c``, on the model's own adjacency values
    -> ((cosine, reg part), {name: float64 gradient}, targets' norms (user side, item side))"""
    import torch
    d, I = c["d"], c["I"]
    val = m.adj.val.cpu().numpy()[:len(c["items"])]
    scale = float(np.float32(1.0 / (1.0 - c["rate"])))
    R1, R2t = (torch.tensor(a, dtype=dtype) for a in T.masked_blocks(c["rowptr"], c["items"], I, val, c["k1"], c["k2"], scale))
    P = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in c["P"].items()}
    (cos, regl), Mu, Mi = T.losses_f64(P["user_emb"], P["item_emb"], P["predictor.weight"], P["predictor.bias"], R1, R2t, c["users"][rows],
                                       c["its"][rows], c["ku"][rows][:, :d], c["ki"][rows][:, :d], c["L"], dropout, reg, n_div=n_div)
    (cos + regl).backward()
    with torch.no_grad():
        tn = ((Mu[c["users"][rows]] * torch.tensor(c["ku"][rows][:, :d], dtype=dtype) / (1 - dropout)).norm(dim=1).numpy(),
              (Mi[c["its"][rows]] * torch.tensor(c["ki"][rows][:, :d], dtype=dtype) / (1 - dropout)).norm(dim=1).numpy())
    return (cos.item(), regl.item()), {k: v.grad.numpy().astype(np.float64) for k, v in P.items()}, tn


def _edge_compare(c, what, reg=1e-2, ok=None, floor=None, widen=False, m=None):
    """The device step on the batch of ``c`` against the float64 twin on the rows ``ok`` (all when None) with n as the divisor.
    ``floor`` ({name: gradient}): each tensor's scale is max|want| or that tensor at a batch without the exact cancellation,
    whichever is more.  ``widen``: allow max(ATOL * scale, 4 x the error of the same twin in float32 on the CPU), both printed"""
    import torch
    n = c["n"]
    ok = np.ones(n, bool) if ok is None else ok
    m = _detached(c, reg) if m is None else m
    (cos, regl), G, _ = _twin_run(c, m, ok, torch.float64, reg, n_div=n)
    (cos32, regl32), G32, _ = _twin_run(c, m, ok, torch.float32, reg, n_div=n) if widen else ((cos, regl), None, None)
    loss = m.gradient_step(c["users"], c["its"], rate=c["rate"], edge_keep=(c["k1"], c["k2"]), target_keep=(c["ku"], c["ki"])).cpu().numpy()
    want, want32 = np.array([cos, regl, cos + regl]), np.array([cos32, regl32, cos32 + regl32])
    print(what, "loss", loss, "twin", want, "abs err", np.abs(loss - want), "fp32-CPU err", np.abs(want32 - want))
    assert np.isfinite(loss).all()
    assert np.all(np.abs(loss - want) <= np.maximum(1e-5 * np.abs(want), 4 * np.abs(want32 - want)))
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    for k in T.PARAMS:                # every tensor is measured before the assertion
        scale = float(np.abs(G[k]).max())
        if floor is not None:
            scale = max(scale, float(np.abs(floor[k]).max()))
        err = np.abs(got[k].astype(np.float64) - G[k])
        atol = ATOL * scale
        if widen:
            err32 = float(np.abs(G32[k] - G[k]).max())
            atol = max(atol, 4 * err32)
            print(f"{what}: {k}: max abs err {err.max():.3e}, scale {scale:.3e}, fp32-CPU err {err32:.3e}")
        else:
            print(f"{what}: {k}: max abs err {err.max():.3e}, scale {scale:.3e}")
        assert np.isfinite(got[k]).all(), k
        assert np.all(err <= atol + RTOL * np.abs(G[k])), (what, k, float(err.max()), scale)
    return loss, got, m


def _run(m, c, rows=None):
    rows = slice(None) if rows is None else rows
    return m.gradient_step(c["users"][rows], c["its"][rows], rate=c["rate"], edge_keep=(c["k1"], c["k2"]),
                           target_keep=(c["ku"][rows], c["ki"][rows]))


@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("n", [15, 16, 17, 63, 65])
def test_batch_sizes_around_the_tiles(n, d):
    """below, at and above a wavefront's 16 rows and a workgroup's 64 (n = 64 is in test_step_matches_float64_autograd)"""
    c = _step_case(n, 2, d, 1000 + n + d)
    assert len(np.unique(c["users"])) < n and len(np.unique(c["its"])) < n and (c["users"] == 47).any() and (c["its"] == 39).any()
    _edge_compare(c, f"n = {n}, d = {d}")


def test_full_batch_at_four_layers():
    """n = 2048 at L = SKR_SELFCF_MAX_LAYERS = 4 on a 2100 x 2100 graph: 32 batch workgroups, eight dropped plan runs each way;
    then the same call again: the same bits"""
    import time
    import torch
    from skrec import _hip
    t0 = time.time()
    assert _hip.SKR_SELFCF_MAX_LAYERS == 4 and _hip.SKR_SELFCF_MAX_BATCH == 2048
    c = _step_case(2048, 4, 64, 2100, U=2100, I=2100)
    loss, _, m = _edge_compare(c, "n = 2048", widen=True)
    g1, M1 = m._grad.clone(), m.M.clone()
    m._work.fill_(255)
    m._grad.fill_(3.0)
    loss2 = _run(m, c).cpu().numpy()
    assert np.array_equal(loss.view(np.uint32), loss2.view(np.uint32)) and torch.equal(g1, m._grad) and torch.equal(M1, m.M)
    print("full batch: wall time", time.time() - t0)


@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("which", ["user", "item"])
def test_one_id_in_every_row(which, n):
    """the longest segment: all n ranks of one list name one id, so one wavefront of seg_add walks them all and the rank
    kernel counts n equal keys; the scales are floored by the same batch with its random ids"""
    import torch
    c = _step_case(n, 2, 64, 3000 + n)
    m = _detached(c, 1e-2)
    floor = _twin_run(c, m, np.ones(n, bool), torch.float64, 1e-2, n_div=n)[1]
    key = "users" if which == "user" else "its"
    c[key][:] = c[key][n - 1]
    _edge_compare(c, f"one {which}, n = {n}", floor=floor, m=m)


def test_ids_out_of_range_contribute_nothing():
    """the result is that of the batch without those rows with n = 70 as the divisor of the two cosine means; the regulariser
    is a sum over the remaining rows"""
    U, I, n = 48, 40, 70
    c = _step_case(n, 2, 64, 4000)
    users, its = c["users"], c["its"]
    users[3], its[17], users[40], its[40], users[69] = U, -1, -7, I, 2 ** 31 - 1
    ok = (users >= 0) & (users < U) & (its >= 0) & (its < I)
    assert ok.sum() == 66
    _edge_compare(c, "ids out of range", ok=ok)
    # the device's own result on the filtered batch, scaled by 66 / 70 (without the regulariser, which does not scale)
    m = _detached(c, 0.0)
    loss = _run(m, c).cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    loss2 = _run(m, c, ok).cpu().numpy()
    got2 = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    assert loss[1] == 0 and loss2[1] == 0
    np.testing.assert_allclose(loss, loss2 * 66 / 70, rtol=1e-5)
    for k in T.PARAMS:
        np.testing.assert_allclose(got[k], got2[k] * np.float32(66 / 70), rtol=RTOL, atol=ATOL * np.abs(got[k]).max(), err_msg=k)


def test_an_empty_batch_writes_nothing():
    import torch
    from skrec import _hip
    c = _step_case(17, 2, 64, 5000)
    m = _detached(c)
    loss = torch.full((3,), 7.0, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    a = m._step_args(ids, ids, 0.3, None, None, None, loss)
    a.n = 0
    m._grad.fill_(3.0)
    m._work.fill_(5)
    tabs = [m.M, m._G, m._ping[0], m._ping[1]]
    for t in tabs:
        t.fill_(2.0)
    before = [t.clone() for t in tabs] + [m._work.clone(), m._flat.clone()]
    _hip.check(_hip.lib().skr_selfcf_step(C.byref(a), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (m._grad == 3.0).all()
    assert all(torch.equal(x, y) for x, y in zip(before, tabs + [m._work, m._flat]))
    # through the class: a zero loss, a zero gradient whatever the last step left there; the draws' step counter stays
    _run(m, c)
    assert m._grad.any()
    z, step = np.zeros(0, np.int32), m._step
    loss = m.gradient_step(z, z)
    assert loss.shape == (3,) and not loss.any() and not m._grad.any() and m._step == step
    # train_step: the zero gradient through Adam, as MGCN, LATTICE and SLMRec do it; with no moments yet nothing moves
    _run(m, c)
    flat = m._flat.clone()
    assert not m.train_step(z, z).any()
    assert torch.equal(flat, m._flat)


def test_a_predictor_output_of_exact_zeros():
    """W = 0 and b = 0: every P row is zero, |P| takes the 1e-8 clamp, every cosine is 0 and the predictor's gradient is
    -t / (1e-8 max(|t|, 1e-8)) / (2 n): of the order 1e8 / n, finite"""
    c = _step_case(70, 2, 64, 6000)
    c["P"]["predictor.weight"][:] = 0
    c["P"]["predictor.bias"][:] = 0
    loss, got, _ = _edge_compare(c, "P = 0", widen=True)
    assert loss[0] == 0 and np.abs(got["predictor.bias"]).max() > 1e4


def test_target_rows_with_a_norm_under_the_clamp():
    """the isolated user's and the isolated item's embedding rows scaled by 1e-9: their target rows (rows 1 of the batch) have
    0 < |t| < 1e-8, the max(|t|, 1e-8) branch of the cosine; the reference is the twin's own clamp"""
    import torch
    c = _step_case(70, 2, 64, 6001)
    U, I = c["U"], c["I"]
    assert c["users"][1] == U - 1 and c["its"][1] == I - 1
    c["ku"][1], c["ki"][1] = 1, 1
    c["P"]["user_emb"][U - 1] *= np.float32(1e-9)
    c["P"]["item_emb"][I - 1] *= np.float32(1e-9)
    m = _detached(c, 1e-2)
    tn = _twin_run(c, m, np.ones(70, bool), torch.float64, 1e-2)[2]
    print("target norms of row 1:", tn[0][1], tn[1][1])
    assert 0 < tn[0][1] < 1e-8 and 0 < tn[1][1] < 1e-8
    _edge_compare(c, "small targets", widen=True, m=m)
