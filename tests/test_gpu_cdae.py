"""GPU suite of CDAE (csrc/cdae.hip, skrec/recommender/CDAE.py): the fused step against float64 autograd of a restatement
(tests/cdae_twin.py), its determinism, the exact negatives and the device layout against the host layout function, the
blocked against the dense Adam, the golden replay of the reference's fit() from its recorded draws, the query rows, the
evaluator's fused path against its generic one, the device draws, fit() and the command line."""
import numpy as np
import pytest

import cdae_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = 2021
CONFIG = dict(lr=1e-2, reg=1e-3, hidden_dim=64, dropout=0.5, num_neg=2, hidden_act="sigmoid", batch_size=24, epochs=3)


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="CDAE", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    from skrec.recommender.CDAE import CDAE
    from skrec.utils.py.random import DeviceSampler
    cfg = dict(CONFIG)
    cfg.update(kw)
    _seed()
    m = CDAE(_run_config(data_dir), cfg)
    m.sampler = DeviceSampler(2020)           # the stream of a fresh process, whatever ran before in this one
    return m


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step kernel against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def _case(rng, B, I, d, act, keep_prob=0.5, num_neg=2, lens=(2, 12), long_rows=True):
    """parameters of width d, a CSR of B + 2 users (the batch is B of them, not in id order), raw negatives and keep
    flags.  Batch position 0: a user with a single training item; 1 (B > 1): every entry dropped; 2: more than 64 pairs;
    3: more than 256 pairs (``long_rows``).  Item 7 is a positive of every user; the bias of the last item block is
    exercised by the catalogue's last item, a positive of position 0's neighbour.  ``lens``: the rows' lengths, [lo, hi)."""
    nU = B + 2
    lens = rng.integers(lens[0], lens[1], nU)
    lens[0] = 1
    if B > 3 and long_rows:
        lens[2], lens[3] = 30, min(140, I // 3)
    rows = []
    for n in lens:
        r = rng.choice(np.setdiff1d(np.arange(I), [7]), n, replace=False)
        r[0] = 7
        rows.append(np.sort(r).astype(np.int32))
    if B > 1:
        rows[1][-1] = I - 1
        rows[1] = np.unique(rows[1]).astype(np.int32)
        lens[1] = len(rows[1])
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate(rows)
    users = np.concatenate([np.arange(min(4, B)), 4 + rng.permutation(nU - 4)])[:B].astype(np.int32) if B > 4 \
        else np.arange(B, dtype=np.int32)
    negs = [rng.choice(np.setdiff1d(np.arange(I), rows[u]), num_neg * lens[u], replace=True).astype(np.int32) for u in users]
    pu, pi, pl = T.pairs(rowptr, items, users, negs)
    keep = (rng.random(len(pi)) < keep_prob).astype(np.uint8) if keep_prob < 1 else np.ones(len(pi), np.uint8)
    keep[pu == 0] = 1
    if B > 1:
        keep[pu == 1] = 0
    par = dict(en_embeddings=rng.standard_normal((I, d)) * 0.2, en_offset=rng.standard_normal(d) * 0.2,
               de_embeddings=rng.standard_normal((I, d)) * 0.3, de_bias=rng.standard_normal((I, 1)) * 0.3,
               user_embeddings=rng.standard_normal((nU, d)) * 0.2)
    par = {k: v.astype(np.float32) for k, v in par.items()}
    return dict(nU=nU, I=I, d=d, B=B, act=act, keep_prob=keep_prob, rowptr=rowptr, items=items, users=users, negs=negs,
                pu=pu, pi=pi, pl=pl, keep=keep, par=par)


def _device_tables(c):
    """the kernel's layout of a case's parameters: E_en, E_de [I, 64], bias [ceil(I / 64) * 64], offset [64], U [nU, 64]"""
    import torch
    d, I, p = c["d"], c["I"], c["par"]
    pad = lambda a: np.pad(a, ((0, 0), (0, 64 - d)))            # noqa: E731
    bias = np.zeros((I + 63) // 64 * 64, np.float32)
    bias[:I] = p["de_bias"][:, 0]
    off = np.zeros(64, np.float32)
    off[:d] = p["en_offset"]
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
            (pad(p["en_embeddings"]), pad(p["de_embeddings"]), bias, off, pad(p["user_embeddings"]))]


LAYOUT_KEYS = ("uptr", "pitem", "plabel", "puser", "ditems", "iptr", "ipair")


def _launch(c, tabs, lay, users, keep, reg=1e-3, n=None, P=None, J=None, u0=0, j0=0):
    """one skr_cdae_step on the layout ``lay`` as it stands (a test may have broken single entries of it), the workspace
    filled with 0xFF bytes, gradients zeroed before -> (gE_en, gE_de, gbias, goffset, gU on the host, loss).  ``u0`` / ``j0``:
    the batch starts at users[u0], uptr[u0], ditems[j0], iptr[j0] of a longer block and holds n users, P pairs, J items"""
    import torch
    from skrec import _hip
    L = _hip.lib()
    dev = {k: torch.from_numpy(np.ascontiguousarray(lay[k])).cuda() for k in LAYOUT_KEYS}
    assert all(dev[k].dtype == torch.int32 for k in ("uptr", "pitem", "puser", "ditems", "iptr", "ipair"))
    du = torch.from_numpy(np.ascontiguousarray(users, dtype=np.int32)).cuda()
    dk = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).cuda()
    grads = [torch.zeros_like(t) for t in tabs]
    n = len(users) if n is None else n
    P, J = len(lay["pitem"]) if P is None else P, len(lay["ditems"]) if J is None else J
    nb = int(L.skr_cdae_workspace(n, P))
    assert nb > 0
    work = torch.full((nb + 64,), 255, dtype=torch.uint8, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    act = _hip.SKR_CDAE_SIGMOID if c["act"] == "sigmoid" else _hip.SKR_CDAE_IDENTITY
    _hip.check(L.skr_cdae_step(*[_hip.ptr(t) for t in tabs], du.data_ptr() + 4 * u0, dev["uptr"].data_ptr() + 4 * u0,
                               _hip.ptr(dev["pitem"]), _hip.ptr(dev["plabel"]), _hip.ptr(dk), _hip.ptr(dev["puser"]),
                               dev["ditems"].data_ptr() + 4 * j0, dev["iptr"].data_ptr() + 4 * j0, _hip.ptr(dev["ipair"]), n, P, J,
                               c["nU"], c["I"], c["d"], act, c["keep_prob"], reg, *[_hip.ptr(g) for g in grads], _hip.ptr(work),
                               nb, _hip.ptr(loss), _hip.stream()))
    torch.cuda.synchronize()
    assert (work[nb:] == 255).all()                              # nothing past the workspace
    return [g.cpu().numpy() for g in grads], loss.cpu().numpy()


def _step(c, tabs, reg=1e-3):
    """one skr_cdae_step on the host layout, gradients zeroed before -> (gE_en, gE_de, gbias, goffset, gU on the host, loss)"""
    from skrec.recommender.CDAE import batch_layout
    lay = batch_layout(c["rowptr"], c["items"], c["users"], c["negs"])
    assert np.array_equal(lay["pitem"], c["pi"]) and np.array_equal(lay["puser"], c["pu"])
    return _launch(c, tabs, lay, c["users"], c["keep"], reg)


@pytest.mark.parametrize("B,I,d,act", [(1, 70, 20, "sigmoid"), (9, 459, 64, "sigmoid"), (9, 459, 20, "identity"),
                                       (37, 459, 64, "identity"), (37, 1030, 40, "sigmoid")])
def test_step_matches_float64_autograd(B, I, d, act):
    """shapes: catalogues that are no multiple of 64 (the bias block's tail), padded columns, both activations, a batch
    of one user, more users than a workgroup holds; every larger case holds a user with a single item, one whose every
    entry is dropped, users with more than 64 and more than 256 pairs, an item every user holds and items held once"""
    import torch
    rng = np.random.default_rng(B + I + d)
    reg = 1e-3
    c = _case(rng, B, I, d, act)
    per_user = np.bincount(c["pu"], minlength=B)
    held = np.bincount(c["pi"], minlength=I)
    assert I % 64 and held[7] == B and (held == 1).any() and (held == 0).any()
    if B > 3:
        assert per_user[0] <= 3 and 64 < per_user[2] <= 256 < per_user[3] and not c["keep"][c["pu"] == 1].any()
    tabs = _device_tables(c)
    (gen, gde, gb, goff, gU), loss = _step(c, tabs, reg)
    t64 = [torch.tensor(c["par"][k], dtype=torch.float64, requires_grad=True) for k in T.PARAMS]
    bce, l2 = T.losses_f64(t64, c["users"], c["pu"], c["pi"], c["pl"], c["keep"], c["keep_prob"], act)
    (bce + reg * l2).backward()
    print("bce", loss[0], bce.item(), "l2", loss[1], l2.item())
    np.testing.assert_allclose(loss[0], bce.item(), rtol=1e-5)
    np.testing.assert_allclose(loss[1], l2.item(), rtol=1e-5)
    want = [t.grad.numpy() for t in t64]
    checks = [("en_embeddings", gen[:, :d], want[0]), ("en_offset", goff[:d], want[1]), ("de_embeddings", gde[:, :d], want[2]),
              ("de_bias", gb[:I], want[3][:, 0]), ("user_embeddings", gU[:, :d], want[4])]
    for name, got, w in checks:
        print(name, "max abs err", np.abs(got - w).max(), "max |grad|", np.abs(w).max())
    for name, got, w in checks:
        np.testing.assert_allclose(got, w, rtol=1e-4, atol=2e-5 * np.abs(w).max(), err_msg=name)
    # padded columns, padded bias entries, and the rows the batch does not name are exactly zero
    assert not gen[:, d:].any() and not gde[:, d:].any() and not gU[:, d:].any() and not goff[d:].any() and not gb[I:].any()
    assert not gen[held == 0].any() and not gde[held == 0].any() and not gb[:I][held == 0].any()
    assert not gU[np.setdiff1d(np.arange(c["nU"]), c["users"])].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism
# ---------------------------------------------------------------------------------------------------------------------
def _synth_csr(rng, nU, I, lo=3, hi=20):
    lens = rng.integers(lo, hi, nU)
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate([np.sort(rng.choice(I, n, replace=False)).astype(np.int32) for n in lens])
    return rowptr, items


def test_step_is_deterministic():
    c = _case(np.random.default_rng(5), 300, 2053, 64, "sigmoid")
    tabs = _device_tables(c)
    (g0, l0), (g1, l1) = _step(c, tabs), _step(c, tabs)
    assert np.count_nonzero(g0[1]) > 0 and np.isfinite(l0).all()
    for a, b in zip(g0, g1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    # ... and so are the parameters after training steps on the same draws
    from skrec.recommender.CDAE import CDAE
    from skrec.utils.py.random import DeviceSampler
    import torch
    rng = np.random.default_rng(6)
    nU, I = 200, 333
    csr = _synth_csr(rng, nU, I)
    flats, losses = [], []
    for _ in range(2):
        torch.manual_seed(3)
        m = CDAE.detached(nU, I, dict(CONFIG, hidden_dim=48), csr, seed=9)
        m.sampler = DeviceSampler(2020)
        ls = [m.train_step(np.arange(s * 50, s * 50 + 50, dtype=np.int32)).cpu().numpy() for s in range(3)]
        flats.append(m._flat.cpu().numpy())
        losses.append(np.stack(ls))
    assert np.array_equal(flats[0].view(np.uint32), flats[1].view(np.uint32))
    assert np.array_equal(losses[0].view(np.uint32), losses[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the exact negatives and the device layout
# ---------------------------------------------------------------------------------------------------------------------
def _block_step(B, s):
    """step s of a device block in the host layout function's form"""
    h = lambda t: t.cpu().numpy()             # noqa: E731
    u0, u1, p0, p1, j0, j1 = B.ustart[s], B.ustart[s + 1], B.pstart[s], B.pstart[s + 1], B.jstart[s], B.jstart[s + 1]
    iptr = h(B.iptr)[j0:j1 + 1].astype(np.int64)
    return dict(users=h(B.users)[u0:u1], uptr=h(B.uptr)[u0:u1 + 1] - p0, pitem=h(B.pitem)[p0:p1], plabel=h(B.plabel)[p0:p1],
                puser=h(B.puser)[p0:p1], ditems=h(B.ditems)[j0:j1], iptr=iptr - iptr[0], ipair=h(B.ipair)[iptr[0]:iptr[-1]])


def test_negatives_and_device_layout(golden, tiny_dir, monkeypatch, tmp_path):
    import torch
    from skrec.recommender.CDAE import batch_layout
    from skrec.utils.py.random import DeviceSampler
    monkeypatch.chdir(tmp_path)
    g = golden("golden_cdae")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    steps = T.fixture_steps(g)
    # the raw draws of the whole run, for the users in the order they were visited
    order = g["step_users"].astype(np.int64)
    lens = rowptr[order + 1] - rowptr[order]
    rp = np.concatenate([[0], np.cumsum(lens)])
    excl = np.concatenate([items[rowptr[u]:rowptr[u + 1]] for u in order]).astype(np.int32)
    d_rp, d_ex, d_dp = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, excl, rp * 2))
    out = torch.empty(int(rp[-1]) * 2, dtype=torch.int32, device="cuda")
    DeviceSampler(2020).sample_epoch_exact_counts(ni, len(order), d_rp, d_ex, int(rp[-1]), d_dp, out.numel(), out)
    assert np.array_equal(out.cpu().numpy(), g["neg_raw"]) and np.array_equal(g["neg_sizes"], 2 * lens)
    # the model's own preparation: blocks of 4, 4 and 1 steps on one stream
    m = _model(tiny_dir)
    at = 0
    for k in (4, 4, 1):
        B = m._prepare([s[0] for s in steps[at:at + k]])
        assert len(B.ustart) == k + 1 and B.ids.numel() == k * B.per
        ids = B.ids.view(k, B.per).cpu().numpy()
        for s in range(k):
            users, negs, _, _ = steps[at + s]
            lay, got = batch_layout(rowptr, items, users, negs), _block_step(B, s)
            assert np.array_equal(got["users"], users)
            for key in ("uptr", "pitem", "plabel", "puser", "ditems", "iptr", "ipair"):
                assert np.array_equal(got[key], lay[key]), (at + s, key)
            J = lay["ditems"].astype(np.int64)
            want = np.concatenate([m._blk_user + users, J, m._blk_de + J, m._blk_bias + J // 64, [m._blk_off]])
            assert set(ids[s][ids[s] >= 0]) == set(want.tolist()) and ids[s].max() < m._flat.numel() // 64
        m.update_count += k
        at += k
    with pytest.raises(ValueError, match="positive integer"):
        _model(tiny_dir, num_neg=0).train_step(steps[0][0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. blocked against dense Adam
# ---------------------------------------------------------------------------------------------------------------------
def test_blocked_adam_equals_dense(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    batches = [s[0] for s in T.fixture_steps(golden("golden_cdae"))]
    assert len(batches) == 9
    res = []
    for k in ("4", "1"):
        monkeypatch.setenv("SKR_ADAM_BLOCK", k)
        m = _model(tiny_dir)
        assert m.adam_block == int(k)
        losses = m.train_epoch(batches).cpu().numpy()
        res.append((m._flat.cpu().numpy(), losses, m.optimizer.m.cpu().numpy(), m.optimizer.v.cpu().numpy()))
        left = np.flatnonzero(m.optimizer.grad.cpu().numpy())
        print("SKR_ADAM_BLOCK", k, "t", m.optimizer.t, "steps", m.update_count, "gradient elements left", len(left), left[:8] // 64)
        assert m.optimizer.t == 9 and m.update_count == 9 and len(left) == 0
    assert np.isfinite(res[0][1]).all() and (res[0][1] != 0).all()
    for name, a, b in zip(("parameters", "losses", "m", "v"), *res):
        diff = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
        print(name, "elements that differ", len(diff), "first blocks", np.unique(diff // 64)[:8] if name != "losses" else diff)
    for a, b in zip(*res):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 5. golden replay of the reference's fit() from its recorded draws
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
    g = golden("golden_cdae")
    m = _model(tiny_dir)
    assert (m.num_users, m.num_items, m.d) == (64, 96, 64)
    for k, t in zip(T.PARAMS, m.parameters()):
        assert np.array_equal(t.cpu().numpy(), g[k + "0"]), k          # same init under the same seed
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    losses, n_eval = [], 0
    for s, (users, _, keep, flat) in enumerate(T.fixture_steps(g)):
        losses.append(m.train_step(users, flat, keep).cpu().numpy())
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
    print("bce", losses[:, 0], "golden", g["bce"], "\nl2", losses[:, 1], "golden", g["l2"])
    np.testing.assert_allclose(losses[:, 0], g["bce"], rtol=1e-5)
    np.testing.assert_allclose(losses[:, 1], g["l2"], rtol=1e-5)
    for k, t, lim in zip(T.PARAMS, m.parameters(), dev_p):
        print(k, "max abs diff", np.abs(t.cpu().numpy() - g[k + "1"]).max(), "allowed", 6 * lim)
    for k, t, lim in zip(T.PARAMS, m.parameters(), dev_p):
        assert np.abs(t.cpu().numpy() - g[k + "1"]).max() <= 6 * lim, k
    # padded bias entries stay zero
    assert not m._flat[m._blk_bias * 64 + 96:m._blk_off * 64].any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. query rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("d,act", [(64, "sigmoid"), (24, "identity")])
def test_queries_match_float64(d, act, with_list):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(d)
    nU, I = 301, 1000
    lens = rng.integers(1, 60, nU)
    lens[7], lens[11] = 0, 700                            # an empty row, a long row
    rowptr = np.zeros(nU + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    items = np.concatenate([np.sort(rng.choice(I, n, replace=False)).astype(np.int32) for n in lens])
    par = dict(en_embeddings=rng.standard_normal((I, d)) * 0.1, en_offset=rng.standard_normal(d) * 0.2,
               de_embeddings=np.zeros((I, d)), de_bias=np.zeros((I, 1)), user_embeddings=rng.standard_normal((nU, d)) * 0.2)
    c = dict(d=d, I=I, par={k: v.astype(np.float32) for k, v in par.items()})
    en, _, _, off, U = _device_tables(c)
    users = np.concatenate([[7, 11], 12 + rng.permutation(nU - 12)[:75]]).astype(np.int32) if with_list \
        else np.arange(nU, dtype=np.int32)
    Q = torch.full((nU + 1, 64), 7.0, device="cuda")
    drp, dit, du = (torch.from_numpy(a).cuda() for a in (rowptr, items, users))
    _hip.check(_hip.lib().skr_cdae_queries(_hip.ptr(en), _hip.ptr(off), _hip.ptr(U), _hip.ptr(drp), _hip.ptr(dit),
                                           _hip.ptr(du) if with_list else None, len(users), nU, I, d,
                                           _hip.SKR_CDAE_SIGMOID if act == "sigmoid" else _hip.SKR_CDAE_IDENTITY, _hip.ptr(Q),
                                           _hip.stream()))
    got = Q.cpu().numpy()
    assert (got[nU] == 7.0).all() and (got[np.setdiff1d(np.arange(nU), users)] == 7.0).all()
    p64 = {k: v.astype(np.float64) for k, v in c["par"].items()}
    pre = np.stack([p64["en_embeddings"][items[rowptr[u]:rowptr[u + 1]]].sum(0) for u in users]) \
        + p64["user_embeddings"][users] + p64["en_offset"]
    want = 1 / (1 + np.exp(-pre)) if act == "sigmoid" else pre
    print("max abs err", np.abs(got[users, :d] - want).max())
    np.testing.assert_allclose(got[users, :d], want, rtol=1e-5, atol=2e-6)
    assert not got[users, d:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the evaluator's fused path against its generic path
# ---------------------------------------------------------------------------------------------------------------------
class _PredictOnly(object):
    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def test_fused_path_equals_generic_path(tiny_dir, monkeypatch, tmp_path):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SKR_FUSED_MODE", "fp32")
    m = _model(tiny_dir, epochs=1)
    m.fit()
    ev = m.evaluator
    users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert 63 in users and m._rowptr_host[64] == m._rowptr_host[63]          # the cold user is ranked like anyone else
    rows_dev, _, n_dev = ev.per_user_rows(m, users)
    rows_gen, _, n_gen = ev.per_user_rows(_PredictOnly(m), users)
    assert n_dev == n_gen == len(users) == 63
    assert np.array_equal(rows_dev, rows_gen)
    Q, _, _ = m.predict_factors()
    np.testing.assert_allclose(Q[63].cpu().numpy(), torch.sigmoid(m._user[63] + m._off).cpu().numpy(), rtol=1e-6)
    # the query rows are kept between evaluations and dropped by a training step
    assert m._q_current
    q0 = Q.clone()
    m.train_step(np.arange(24, dtype=np.int32))
    assert not m._q_current
    assert not np.array_equal(m.predict_factors()[0].cpu().numpy(), q0.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 8. device draws
# ---------------------------------------------------------------------------------------------------------------------
def _draws(users, puser, pitem, keep_prob, seed, step):
    import torch
    from skrec import _hip
    du, dp, di = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (users, puser, pitem))
    keep = torch.full((len(pitem) + 1,), 9, dtype=torch.uint8, device="cuda")
    _hip.check(_hip.lib().skr_cdae_draws(_hip.ptr(du), _hip.ptr(dp), _hip.ptr(di), None, len(pitem), len(users), keep_prob, seed,
                                         step, _hip.ptr(keep), _hip.stream()))
    k = keep.cpu().numpy()
    assert k[-1] == 9
    return k[:-1]


def test_device_draws():
    rng = np.random.default_rng(3)
    nU, I, p = 512, 5000, 0.3
    rowptr, items = _synth_csr(rng, nU, I, 100, 200)
    users = np.arange(nU, dtype=np.int32)
    puser = np.repeat(users, np.diff(rowptr))
    keep = _draws(users, puser, items, p, 11, 4)
    n = len(keep)
    assert n > 5e4 and set(np.unique(keep)) == {0, 1}
    assert abs(keep.mean() - p) <= 4 * np.sqrt(p * (1 - p) / n)
    assert np.array_equal(keep, _draws(users, puser, items, p, 11, 4))              # the same (seed, step)
    assert not np.array_equal(keep, _draws(users, puser, items, p, 11, 5))          # another step
    assert not np.array_equal(keep, _draws(users, puser, items, p, 12, 4))          # another seed
    sub = rng.permutation(nU)[:60].astype(np.int32)                                # another batch: the users' flags are the same
    pu = np.repeat(np.arange(60), rowptr[sub + 1] - rowptr[sub])
    pi = np.concatenate([items[rowptr[u]:rowptr[u + 1]] for u in sub])
    ks = _draws(sub, pu, pi, p, 11, 4)
    assert np.array_equal(ks, np.concatenate([keep[rowptr[u]:rowptr[u + 1]] for u in sub]))


def test_model_keep_flags_are_keyed_by_step_user_and_item(golden, tiny_dir, monkeypatch, tmp_path):
    """the flags the model prepares for a block of steps are skr_cdae_draws' for (seed, global step, user, item),
    whatever the block's partition into steps"""
    monkeypatch.chdir(tmp_path)
    batches = [s[0] for s in T.fixture_steps(golden("golden_cdae"))][:5]
    m = _model(tiny_dir)
    m.update_count = 3
    flags = {}
    for part in ((0, 2), (2, 5)):
        B = m._prepare(batches[part[0]:part[1]])
        keep = B.pkeep.cpu().numpy()
        for s in range(part[1] - part[0]):
            got = _block_step(B, s)
            want = _draws(got["users"], got["puser"], got["pitem"], 0.5, SEED, m.update_count + s)
            assert np.array_equal(keep[B.pstart[s]:B.pstart[s + 1]], want), (part, s)
            flags[part[0] + s] = want
        m.update_count += part[1] - part[0]
    assert 0.3 < np.concatenate(list(flags.values())).mean() < 0.7


# ---------------------------------------------------------------------------------------------------------------------
# 9. the training loop and the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_runs_end_to_end(tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(tiny_dir, epochs=2, batch_size=8, hidden_dim=32, num_neg=3)
    epochs = []
    te = m.train_epoch

    def train_epoch(batches):
        r = te(batches)
        epochs.append((sorted(np.concatenate(batches).tolist()), [len(b) for b in batches], r.cpu().numpy()))
        return r
    m.train_epoch = train_epoch
    best = m.fit()
    assert len(epochs) == 2 and m.update_count == 16
    for users, sizes, losses in epochs:
        assert users == list(range(63)) and sizes == [8] * 7 + [7] and np.isfinite(losses).all()     # users with history
    assert epochs[1][2][:, 0].sum() < epochs[0][2][:, 0].sum()
    assert np.isfinite(np.array(list(best.values()))).all()
    assert not m._flat[:96 * 64].view(96, 64)[:, 32:].any() and not m._user[:, 32:].any()         # padded columns


def test_run_skrec_cli(tiny_dir, tmp_path):
    import os
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "CDAE", "--data_dir", tiny_dir, "--hidden_dim", "32",
                        "--epochs", "2", "--batch_size", "16", "--num_neg", "2", "--top_k", "[5,10]",
                        "--metric", "['Recall','NDCG']", "--seed", "7"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 1:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# 10. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
REG = 1e-3
NAMES = ("en_embeddings", "en_offset", "de_embeddings", "de_bias", "user_embeddings")


def _layout(c):
    from skrec.recommender.CDAE import batch_layout
    lay = batch_layout(c["rowptr"], c["items"], c["users"], c["negs"])
    assert np.array_equal(lay["pitem"], c["pi"]) and np.array_equal(lay["puser"], c["pu"])
    return {k: lay[k].copy() for k in LAYOUT_KEYS}


def _layout_of_pairs(pu, pi, n):
    """the layout of a pair list given user-major (items ascending inside a user); the labels are the caller's"""
    pu, pi = np.asarray(pu, np.int64), np.asarray(pi, np.int64)
    uptr = np.concatenate([[0], np.cumsum(np.bincount(pu, minlength=n))]).astype(np.int32)
    ditems, counts = np.unique(pi, return_counts=True)
    return dict(uptr=uptr, pitem=pi.astype(np.int32), puser=pu.astype(np.int32), ditems=ditems.astype(np.int32),
                iptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), ipair=np.argsort(pi, kind="stable").astype(np.int32))


def _edge_compare(c, what, got, pair_ok=None, user_ok=None, l2_items=None, adjust=None, users=None, pairs=None, keep=None):
    """The device's (gradients, loss) against float64 autograd of the twin on the pairs ``pair_ok`` and the users ``user_ok``
    (all when None), with the suite's bounds.  ``adjust(want, detail)`` changes the expected gradients where the contract
    has the item side leave a pair out.  Then: the rows no valid pair or user names, and the padded columns, are exactly zero.
    Prints one ``edge-error`` line per tensor (collected into profiles/scaffold_edges_errors.txt)"""
    import torch
    grads, loss = got
    d, I, nU = c["d"], c["I"], c["nU"]
    users = c["users"] if users is None else users
    pu, pi, pl = (c["pu"], c["pi"], c["pl"]) if pairs is None else pairs
    keep = c["keep"] if keep is None else keep
    ok = np.ones(len(pu), bool) if pair_ok is None else pair_ok
    uok = np.ones(len(users), bool) if user_ok is None else user_ok
    t64 = [torch.tensor(c["par"][k], dtype=torch.float64, requires_grad=True) for k in T.PARAMS]
    detail = {}
    bce, l2 = T.losses_f64(t64, users, pu, pi, pl, keep, c["keep_prob"], c["act"], pair_ok=ok, user_ok=uok, l2_items=l2_items,
                           detail=detail)
    (bce + REG * l2).backward()
    want = [np.zeros(t.shape) if t.grad is None else t.grad.numpy().copy() for t in t64]
    if adjust is not None:
        adjust(want, detail)
    assert np.isfinite(bce.item()) and np.isfinite(l2.item()) and all(np.isfinite(w).all() for w in want)
    print(what, "bce", loss[0], bce.item(), "l2", loss[1], l2.item())
    assert np.isfinite(loss).all() and all(np.isfinite(g).all() for g in grads), what
    np.testing.assert_allclose(loss[0], bce.item(), rtol=1e-5, err_msg=what)
    np.testing.assert_allclose(loss[1], l2.item(), rtol=1e-5, err_msg=what)
    gen, gde, gb, goff, gU = grads
    checks = [(NAMES[0], gen[:, :d], want[0]), (NAMES[1], goff[:d], want[1]), (NAMES[2], gde[:, :d], want[2]),
              (NAMES[3], gb[:I], want[3][:, 0]), (NAMES[4], gU[:, :d], want[4])]
    for name, g, w in checks:                       # every tensor is measured before the assertion
        scale = np.abs(w).max()
        print(f"edge-error CDAE | {what} | {name} | {np.abs(g - w).max():.3e} | {scale:.3e}")
    for name, g, w in checks:
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=2e-5 * np.abs(w).max(), err_msg=f"{what}: {name}")
    # the rows no valid pair (user) names, the padded columns and the padded bias entries are exactly zero
    named = np.zeros(I, bool)
    named[np.unique(np.asarray(pi)[ok]) if l2_items is None else l2_items] = True
    named_u = np.zeros(nU, bool)
    named_u[np.asarray(users)[uok]] = True
    assert not gen[~named].any() and not gde[~named].any() and not gb[:I][~named].any(), what
    assert not gU[~named_u].any(), what
    assert not gen[:, d:].any() and not gde[:, d:].any() and not gU[:, d:].any() and not goff[d:].any() and not gb[I:].any(), what
    return named, named_u, detail


@pytest.mark.parametrize("B", [2, 4, 5, 15, 16, 17, 63, 65])
def test_batch_sizes_around_the_workgroups(B):
    """users below, at and above the item side's four wavefronts and the finish kernel's 16 strided parts and 64 columns"""
    d, act = (64, "sigmoid") if B % 2 else (24, "identity")
    c = _case(np.random.default_rng(100 + B), B, 203, d, act)
    _edge_compare(c, f"B = {B}", _step(c, _device_tables(c), REG))


def test_full_batch_and_the_batch_over_the_limit():
    """B = SKR_CDAE_MAX_BATCH with rows of 2 to 4 items and one negative per positive on 1100 items: more than 1024 distinct
    items, so the finish kernel's loops over n and over n_distinct both take a second trip; twice: the same bits.  Then
    1025 users: refused by name, and the workspace size is 0"""
    from skrec import _hip
    B = _hip.SKR_CDAE_MAX_BATCH
    assert B == 1024
    c = _case(np.random.default_rng(1024), B, 1100, 64, "sigmoid", num_neg=1, lens=(2, 5), long_rows=False)
    lay = _layout(c)
    assert len(lay["ditems"]) > 1024 and len(c["users"]) == 1024 and np.bincount(c["pu"]).max() <= 8
    tabs = _device_tables(c)
    got = _step(c, tabs, REG)
    _edge_compare(c, "B = 1024", got)
    again = _step(c, tabs, REG)
    for a, b in zip(got[0] + [got[1]], again[0] + [again[1]]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert _hip.lib().skr_cdae_workspace(B + 1, len(c["pi"])) == 0
    over = np.concatenate([c["users"], [0]]).astype(np.int32)
    lay["uptr"] = np.concatenate([lay["uptr"], lay["uptr"][-1:]])
    import torch
    args = [torch.zeros(64, device="cuda") for _ in range(3)]
    L = _hip.lib()
    dev = {k: torch.from_numpy(lay[k]).cuda() for k in LAYOUT_KEYS}
    du, dk = torch.from_numpy(over).cuda(), torch.from_numpy(c["keep"]).cuda()
    grads = [torch.zeros_like(t) for t in tabs]
    rc = L.skr_cdae_step(*[_hip.ptr(t) for t in tabs], _hip.ptr(du), *[_hip.ptr(dev[k]) for k in ("uptr", "pitem", "plabel")],
                         _hip.ptr(dk), *[_hip.ptr(dev[k]) for k in ("puser", "ditems", "iptr", "ipair")], B + 1, len(c["pi"]),
                         len(lay["ditems"]), c["nU"], c["I"], 64, _hip.SKR_CDAE_SIGMOID, 0.5, REG, *[_hip.ptr(g) for g in grads],
                         _hip.ptr(args[0]), 256, _hip.ptr(args[1]), _hip.stream())
    with pytest.raises(ValueError, match="at most 1024"):
        _hip.check(rc)
    torch.cuda.synchronize()
    assert not any(g.any() for g in grads)


def test_a_step_inside_a_block():
    """three batches laid out as one block (CDAE._prepare's form: uptr and iptr run on, ipair is relative to the batch's
    first pair); the kernel entry takes the middle one: uptr[0] != 0, iptr[0] != 0, users / uptr / ditems / iptr offset"""
    from skrec.recommender.CDAE import batch_layout
    c = _case(np.random.default_rng(77), 27, 203, 40, "sigmoid")
    parts = [batch_layout(c["rowptr"], c["items"], c["users"][s:s + 9], c["negs"][s:s + 9]) for s in (0, 9, 18)]
    p0 = np.concatenate([[0], np.cumsum([len(p["pitem"]) for p in parts])])
    blk = {k: np.concatenate([p[k] for p in parts]) for k in ("pitem", "plabel", "puser", "ditems", "ipair")}
    blk["uptr"] = np.concatenate([parts[0]["uptr"]] + [p["uptr"][1:] + o for p, o in zip(parts[1:], p0[1:])]).astype(np.int32)
    blk["iptr"] = np.concatenate([parts[0]["iptr"]] + [p["iptr"][1:] + o for p, o in zip(parts[1:], p0[1:])]).astype(np.int32)
    j0 = len(parts[0]["ditems"])
    assert blk["uptr"][9] == p0[1] > 0 and blk["iptr"][j0] == p0[1]
    keep = c["keep"]                                        # flags in pair order: the block's pair order is the case's
    assert np.array_equal(blk["pitem"], c["pi"])
    mid = parts[1]
    got = _launch(c, _device_tables(c), blk, c["users"], keep, REG, n=9, P=len(mid["pitem"]), J=len(mid["ditems"]), u0=9, j0=j0)
    sl = slice(p0[1], p0[2])
    named, named_u, _ = _edge_compare(c, "the middle step of a block", got, users=c["users"][9:18],
                                      pairs=(mid["puser"], mid["pitem"], mid["plabel"]), keep=keep[sl])
    others = np.zeros(c["I"], bool)
    others[np.concatenate([parts[0]["ditems"], parts[2]["ditems"]])] = True
    assert (others & ~named).sum() > 5 and not named_u[c["users"][:9]].any() and not named_u[c["users"][18:]].any()


def _held_once_by(c, b):
    """an item that batch position b alone holds, with the number of its pair"""
    held = np.bincount(c["pi"], minlength=c["I"])
    mine = np.flatnonzero((c["pu"] == b) & (held[c["pi"]] == 1))
    assert len(mine) > 0
    return int(c["pi"][mine[0]]), int(mine[0])


@pytest.mark.parametrize("where", [0, 5, 16])
@pytest.mark.parametrize("bad", ["below", "n_users"])
def test_a_user_out_of_range_is_skipped(bad, where):
    """its pairs are not scored, not counted in the BCE sum and not followed by the item side; no U row; the items it
    alone holds are not named.  Positions: the first, one inside, the last"""
    c = _case(np.random.default_rng({0: 201, 5: 200, 16: 200}[where]), 17, 203, 64, "sigmoid", long_rows=False)
    item, _ = _held_once_by(c, where)                      # (the seeds: cases in which that position holds such an item)
    users = c["users"].copy()
    lost = int(users[where])
    users[where] = -3 if bad == "below" else c["nU"]
    ok = c["pu"] != where
    uok = np.arange(17) != where
    assert item not in c["pi"][ok] and lost not in users
    named, named_u, _ = _edge_compare(c, f"user {bad} at {where}", _launch(c, _device_tables(c), _layout(c), users, c["keep"], REG),
                                      pair_ok=ok, user_ok=uok, users=users)
    assert not named[item] and not named_u[lost]


@pytest.mark.parametrize("held", ["once", "by others"])
@pytest.mark.parametrize("bad", ["below", "n_items"])
def test_a_pair_item_out_of_range_is_skipped_alone(bad, held):
    """a KEPT pair's d_pitem: nothing goes into the user's h, dr = 0, and the item side does not follow it (a kept pair would
    otherwise put the user's dpre into the gradient of the encoder row that lists it)"""
    c = _case(np.random.default_rng(300), 9, 203, 64, "sigmoid")
    cnt = np.bincount(c["pi"], minlength=c["I"])
    cand = np.flatnonzero((c["keep"] != 0) & ((cnt[c["pi"]] == 1) if held == "once" else (cnt[c["pi"]] > 2)) & (c["pu"] > 1))
    p = int(cand[0])
    item = int(c["pi"][p])
    lay = _layout(c)
    lay["pitem"][p] = -1 if bad == "below" else c["I"]
    ok = np.arange(len(c["pi"])) != p
    assert c["keep"][p] and (item in c["pi"][ok]) == (held == "by others")
    named, _, _ = _edge_compare(c, f"pair item {bad}, held {held}", _launch(c, _device_tables(c), lay, c["users"], c["keep"], REG),
                                pair_ok=ok)
    assert named[item] == (held == "by others")


def _item_side_leaves_out(c, pairs_out, rows_out=()):
    """adjust() of _edge_compare: the item side does not follow the pairs ``pairs_out`` (numbers in the full pair list), the
    user side does: their dr h, dr and kept dpre / keep_prob are missing from their items' rows; ``rows_out``: items that
    get no row at all"""
    def adjust(want, detail):
        row = {int(p): k for k, p in enumerate(detail["rows"])}
        dr, denc, h = detail["r"].grad.numpy(), detail["enc"].grad.numpy(), detail["h"].detach().numpy()
        for p in pairs_out:
            k, it, b = row[int(p)], int(c["pi"][p]), int(c["pu"][p])
            want[2][it] -= dr[k] * h[b]
            want[3][it, 0] -= dr[k]
            if c["keep"][p]:
                want[0][it] -= denc[b] / c["keep_prob"]
        for it in rows_out:
            want[0][it], want[2][it], want[3][it] = 0.0, 0.0, 0.0
    return adjust


@pytest.mark.parametrize("bad", ["below", "n_items"])
def test_a_distinct_item_out_of_range_writes_no_row(bad):
    """a d_ditems entry: its pairs stay in the user side's sums; the item gets no gradient row and no l2 term"""
    c = _case(np.random.default_rng(400), 9, 203, 64, "sigmoid")
    lay = _layout(c)
    j = 3
    item = int(lay["ditems"][j])
    lay["ditems"][j] = -1 if bad == "below" else c["I"]
    J = np.delete(np.unique(c["pi"]), j)
    assert item not in J
    named, _, _ = _edge_compare(c, f"distinct item {bad}", _launch(c, _device_tables(c), lay, c["users"], c["keep"], REG),
                                l2_items=J, adjust=_item_side_leaves_out(c, (), (item,)))
    assert not named[item]


@pytest.mark.parametrize("which,value", [("ipair", "below"), ("ipair", "n_pairs"), ("puser", "below"), ("puser", "n")])
def test_item_side_entries_out_of_range_are_not_followed(which, value):
    """one d_ipair entry / the d_puser entry of one pair: the item side leaves that pair out of its item's three sums (the
    user side needs neither array); the item, held by other pairs too, keeps its row"""
    c = _case(np.random.default_rng(500), 9, 203, 64, "sigmoid")
    lay = _layout(c)
    cnt = np.bincount(c["pi"], minlength=c["I"])
    q = int(np.flatnonzero((cnt[c["pi"][lay["ipair"]]] > 2) & (c["keep"][lay["ipair"]] != 0))[1])     # a slot of the item-major list
    p = int(lay["ipair"][q])
    if which == "ipair":
        lay["ipair"][q] = -1 if value == "below" else len(c["pi"])
    else:
        lay["puser"][p] = -1 if value == "below" else 9
    named, _, _ = _edge_compare(c, f"{which} {value}", _launch(c, _device_tables(c), lay, c["users"], c["keep"], REG),
                                adjust=_item_side_leaves_out(c, (p,)))
    assert named[c["pi"][p]]


@pytest.mark.parametrize("how", ["descending", "past n_pairs"])
def test_a_broken_user_pointer_is_an_empty_row(how):
    """d_uptr[n] below d_uptr[n - 1], or beyond the pair list: the last user's row is empty -- none of its pairs is scored,
    and the item side, which still finds them through d_ipair, does not read the dr nobody wrote (the workspace is 0xFF
    bytes: NaN).  The user keeps its U row and its l2 term"""
    c = _case(np.random.default_rng(600), 9, 203, 64, "sigmoid")
    item, _ = _held_once_by(c, 8)
    lay = _layout(c)
    lay["uptr"][9] = lay["uptr"][8] - 1 if how == "descending" else lay["uptr"][9] + 5
    ok = c["pu"] != 8
    assert (~ok).sum() > 1 and item not in c["pi"][ok]
    named, named_u, _ = _edge_compare(c, f"uptr {how}", _launch(c, _device_tables(c), lay, c["users"], c["keep"], REG), pair_ok=ok)
    assert not named[item] and named_u[c["users"][8]]


@pytest.mark.parametrize("how", ["descending", "past n_pairs"])
def test_a_broken_item_pointer_is_an_empty_list(how):
    """d_iptr[J] below d_iptr[J - 1], or beyond the pair list: the last distinct item's pairs are not followed, so it is not
    named (no row, no l2 term); the user side still scores them"""
    c = _case(np.random.default_rng(700), 9, 203, 64, "sigmoid")
    lay = _layout(c)
    J = len(lay["ditems"])
    item = int(lay["ditems"][J - 1])
    lay["iptr"][J] = lay["iptr"][J - 1] - 1 if how == "descending" else lay["iptr"][J] + 3
    named, _, _ = _edge_compare(c, f"iptr {how}", _launch(c, _device_tables(c), lay, c["users"], c["keep"], REG),
                                l2_items=lay["ditems"][:J - 1], adjust=_item_side_leaves_out(c, (), (item,)))
    assert not named[item]


@pytest.mark.parametrize("n", [37, 300])
def test_one_item_in_every_row(n):
    """every pair names item 7, a positive of the even and a negative of the odd batch positions: n_distinct = 1,
    iptr = [0, P], one wavefront of the item side sums all P pairs"""
    c = _case(np.random.default_rng(800 + n), n, 203, 64, "sigmoid")
    pu, pi, pl = np.arange(n), np.full(n, 7), (np.arange(n) % 2 == 0).astype(np.uint8)
    keep = (np.arange(n) % 3 != 0).astype(np.uint8)
    lay = dict(_layout_of_pairs(pu, pi, n), plabel=pl)
    assert len(lay["ditems"]) == 1 and list(lay["iptr"]) == [0, n]
    _edge_compare(c, f"one item, n = {n}", _launch(c, _device_tables(c), lay, c["users"], keep, REG), pairs=(pu, pi, pl), keep=keep)


def test_one_pair_for_every_item():
    """no item is named twice: n_distinct = P, every item-side wavefront walks one pair"""
    n, I = 37, 203
    c = _case(np.random.default_rng(900), n, I, 64, "identity")
    rng = np.random.default_rng(901)
    per = rng.integers(1, 6, n)
    P = int(per.sum())
    assert P <= I
    pu = np.repeat(np.arange(n), per)
    pi = rng.permutation(I)[:P]
    pi = np.concatenate([np.sort(pi[pu == b]) for b in range(n)])
    pl, keep = (rng.random(P) < 0.5).astype(np.uint8), (rng.random(P) < 0.5).astype(np.uint8)
    lay = dict(_layout_of_pairs(pu, pi, n), plabel=pl)
    assert len(lay["ditems"]) == P
    _edge_compare(c, "one pair per item", _launch(c, _device_tables(c), lay, c["users"], keep, REG), pairs=(pu, pi, pl), keep=keep)


@pytest.mark.parametrize("act", ["sigmoid", "identity"])
@pytest.mark.parametrize("what", ["dim = 1", "keep_prob = 1"])
def test_one_column_and_no_dropout(what, act):
    c = _case(np.random.default_rng(1000), 5, 203, 1 if what == "dim = 1" else 40, act, keep_prob=1.0 if what == "keep_prob = 1" else 0.5)
    assert what != "keep_prob = 1" or c["keep"][c["pu"] != 1].all()       # (position 1 is the user whose every entry is dropped)
    _edge_compare(c, f"{what}, {act}", _step(c, _device_tables(c), REG))


def test_saturated_logits():
    """E_de scaled until |r| passes 88 for the positives and for the negatives (expf(-|r|) underflows, sigmoid(r) rounds to 0
    or 1): the loss stays finite and dr keeps its digits in the -sigmoid(-r) form"""
    import torch
    c = _case(np.random.default_rng(1100), 17, 203, 64, "sigmoid")
    c["par"]["de_bias"][:] = 0.0

    def logits():
        detail = {}
        with torch.no_grad():
            bce, _ = T.losses_f64([torch.tensor(c["par"][k], dtype=torch.float64) for k in T.PARAMS], c["users"], c["pu"], c["pi"],
                                  c["pl"], c["keep"], 0.5, "sigmoid", detail=detail)
        return detail["r"].numpy(), bce.item()
    r, _ = logits()
    s = 90.0 / min(np.abs(r[c["pl"] == 1]).max(), np.abs(r[c["pl"] == 0]).max())
    c["par"]["de_embeddings"] = (c["par"]["de_embeddings"].astype(np.float64) * s).astype(np.float32)
    r, bce = logits()
    print("max |r| of the positives", np.abs(r[c["pl"] == 1]).max(), "of the negatives", np.abs(r[c["pl"] == 0]).max(), "bce", bce)
    assert np.isfinite(bce) and np.abs(r[c["pl"] == 1]).max() > 88 and np.abs(r[c["pl"] == 0]).max() > 88
    assert r[c["pl"] == 1].min() < -88 or r[c["pl"] == 0].max() > 88            # a saturated pair on the wrong side: |dr| = 1
    _edge_compare(c, "logits of 90", _step(c, _device_tables(c), REG))


def test_an_empty_batch_writes_a_zero_loss_and_nothing_else():
    import torch
    from skrec import _hip
    from skrec.recommender.CDAE import CDAE
    c = _case(np.random.default_rng(1200), 5, 203, 64, "sigmoid")
    tabs = _device_tables(c)
    lay = _layout(c)
    dev = {k: torch.from_numpy(lay[k]).cuda() for k in LAYOUT_KEYS}
    du, dk = torch.from_numpy(c["users"]).cuda(), torch.from_numpy(c["keep"]).cuda()
    grads = [torch.full_like(t, 3.0) for t in tabs]
    work = torch.full((4096,), 255, dtype=torch.uint8, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    _hip.check(_hip.lib().skr_cdae_step(*[_hip.ptr(t) for t in tabs], _hip.ptr(du), *[_hip.ptr(dev[k]) for k in ("uptr", "pitem", "plabel")],
                                        _hip.ptr(dk), *[_hip.ptr(dev[k]) for k in ("puser", "ditems", "iptr", "ipair")], 0, 0, 0,
                                        c["nU"], c["I"], 64, _hip.SKR_CDAE_SIGMOID, 0.5, REG, *[_hip.ptr(g) for g in grads],
                                        _hip.ptr(work), work.numel(), _hip.ptr(loss), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 0.0).all() and all((g == 3.0).all() for g in grads) and (work == 255).all()
    # through the class: a zero pair, and a fresh model (zero moments) keeps its bits
    rng = np.random.default_rng(1201)
    m = CDAE.detached(40, 90, dict(CONFIG, hidden_dim=48), _synth_csr(rng, 40, 90), seed=9)
    flat = m._flat.clone()
    out = m.train_step(np.zeros(0, np.int32))
    assert out.shape == (2,) and not out.any() and torch.equal(flat, m._flat) and m.update_count == 1
    assert not m.optimizer.grad.any() and not m.optimizer.m.any() and not m.optimizer.v.any()


def test_queries_skip_what_is_out_of_range():
    """d_users with an id below 0, one at n_users and a valid id twice; a train row holding items out of range (skipped).
    Rows nobody names, the skipped ids' would-be rows among them, keep the sentinel bit for bit; n = 0 is allowed"""
    import torch
    from skrec import _hip
    rng = np.random.default_rng(1300)
    nU, I, d = 30, 90, 24
    rowptr, items = _synth_csr(rng, nU, I)
    items = items.copy()
    row5 = slice(rowptr[5], rowptr[5 + 1])
    assert rowptr[6] - rowptr[5] >= 3
    items[rowptr[5]], items[rowptr[5] + 1] = -1, I                  # (the row is no longer ascending: queries do not need it)
    par = dict(en_embeddings=rng.standard_normal((I, d)) * 0.1, en_offset=rng.standard_normal(d) * 0.2,
               de_embeddings=np.zeros((I, d)), de_bias=np.zeros((I, 1)), user_embeddings=rng.standard_normal((nU, d)) * 0.2)
    c = dict(d=d, I=I, par={k: v.astype(np.float32) for k, v in par.items()})
    en, _, _, off, U = _device_tables(c)
    users = np.array([5, -1, 12, nU, 5, 0, nU - 1], np.int32)
    Q = torch.full((nU + 1, 64), 7.0, device="cuda")
    drp, dit, du = (torch.from_numpy(a).cuda() for a in (rowptr, items, users))
    args = (_hip.ptr(en), _hip.ptr(off), _hip.ptr(U), _hip.ptr(drp), _hip.ptr(dit), _hip.ptr(du))
    _hip.check(_hip.lib().skr_cdae_queries(*args, 0, nU, I, d, _hip.SKR_CDAE_SIGMOID, _hip.ptr(Q), _hip.stream()))
    torch.cuda.synchronize()
    assert (Q == 7.0).all()
    _hip.check(_hip.lib().skr_cdae_queries(*args, len(users), nU, I, d, _hip.SKR_CDAE_SIGMOID, _hip.ptr(Q), _hip.stream()))
    got = Q.cpu().numpy()
    valid = np.array([5, 12, 0, nU - 1])
    assert (got[np.setdiff1d(np.arange(nU + 1), valid)] == 7.0).all()
    p64 = {k: v.astype(np.float64) for k, v in c["par"].items()}
    rows = [items[rowptr[u]:rowptr[u + 1]] for u in valid]
    pre = np.stack([p64["en_embeddings"][r[(r >= 0) & (r < I)]].sum(0) for r in rows]) + p64["user_embeddings"][valid] + p64["en_offset"]
    assert len(rows[0]) - ((rows[0] >= 0) & (rows[0] < I)).sum() == 2 and items[row5].size == len(rows[0])
    np.testing.assert_allclose(got[valid, :d], 1 / (1 + np.exp(-pre)), rtol=1e-5, atol=2e-6)
    assert not got[valid, d:].any()
