"""GPU suite of FREEDOM (csrc/freedom.hip, skrec/recommender/FREEDOM.py): the select on hand-made keys, the keys and their law,
the compacted CSR pair against the reference's recorded ``masked_adj``, the whole step against float64 autograd of a
restatement (tests/freedom_twin.py), the golden replay of the reference's fit() from its recorded keep sets and batches, fit()
with device draws, the limits."""
import os

import numpy as np
import pytest

import freedom_twin as T
from test_freedom_host import LAW_KEEP, LAW_SEED, LAW_TRIALS, LAW_W, assert_same_law, multinomial_frequencies

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = T.SEED
CONFIG = dict(lr=1e-2, reg=0.5, n_mm_layers=2, n_ui_layers=2, dropout=0.8, batch_size=256, epochs=3)


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the select
# ---------------------------------------------------------------------------------------------------------------------
def _select(keys, n_keep, dirty=0):
    import torch
    from skrec import _hip
    L = _hip.lib()
    nnz = len(keys)
    d_keys = keys if torch.is_tensor(keys) else _dev(np.asarray(keys, np.float32))
    ws = int(L.skr_freedom_select_workspace(nnz))
    work = torch.full((ws,), dirty, dtype=torch.uint8, device="cuda")
    keep = torch.full((nnz,), 7, dtype=torch.uint8, device="cuda")
    _hip.check(L.skr_freedom_select(_hip.ptr(d_keys), nnz, n_keep, _hip.ptr(keep), _hip.ptr(work), ws, _hip.stream()))
    return keep.cpu().numpy()


def _key_cases(nnz, rng):
    two = np.where(rng.random(nnz) < 0.1, 2.5, 0.75).astype(np.float32)          # the threshold falls inside a run of ties
    low = (1.0 + rng.integers(0, 200, nnz) * 2.0 ** -23).astype(np.float32)      # equal but for the last digit, many ties
    wide = np.exp(rng.uniform(-40, 40, nnz)).astype(np.float32)                  # distinct, every exponent
    wide[rng.integers(0, nnz)] = 0.0
    return {"equal": np.full(nnz, 0.3, np.float32), "two": two, "low": low, "distinct": wide,
            "uniform": rng.random(nnz).astype(np.float32) + np.float32(1e-3)}


@pytest.mark.parametrize("nnz", [1, 255, 5000, 70001])
def test_select_equals_the_stable_sort(nnz):
    rng = np.random.default_rng(nnz)
    for name, keys in _key_cases(nnz, rng).items():
        for n_keep in sorted({0, 1, nnz // 5, nnz}):
            want = T.select_keys(keys, n_keep)
            got = _select(keys, n_keep)
            assert got.sum() == n_keep, (name, n_keep)
            assert np.array_equal(got, want), (name, n_keep)
            assert np.array_equal(_select(keys, n_keep, dirty=255), got), (name, n_keep)      # the same bytes, whatever the scratch held


# ---------------------------------------------------------------------------------------------------------------------
# 2. the keys
# ---------------------------------------------------------------------------------------------------------------------
def _keys(w, seed, epoch):
    import torch
    from skrec import _hip
    d_w = _dev(np.asarray(w, np.float32))
    out = torch.empty(len(w), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().skr_freedom_keys(_hip.ptr(d_w), len(w), seed, epoch, _hip.ptr(out), _hip.stream()))
    return out


def test_keys_are_finite_positive_and_keyed_by_seed_and_epoch():
    rng = np.random.default_rng(3)
    w = (rng.random(300001) * 0.9 + 1e-4).astype(np.float32)
    a, b, c, d = (_keys(w, s, e).cpu().numpy() for s, e in ((5, 0), (5, 0), (5, 1), (6, 0)))
    assert np.isfinite(a).all() and (a > 0).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)
    # w / key = the unit exponential: mean 1, variance 1 (standard errors 0.002 and 0.005 at this size)
    E = w.astype(np.float64) / a
    assert abs(E.mean() - 1) < 0.01 and abs(E.var() - 1) < 0.03 and E.min() > 0
    # at least 32 random bits: below 1e-4, E = -log(u) is 1 - u up to 1e-3 of a 24-bit step, so a 24-bit uniform would put every
    # such E at (k + 0.5) 2^-24; a finer one spreads them over the step (the fp32 key blurs E / 2^-24 by 1e-4 at most here)
    small = E[E < 1e-4]
    frac = (small / 2.0 ** -24) % 1.0
    print("E below 1e-4:", len(small), "std of their position inside a 24-bit step", frac.std())
    assert len(small) >= 10 and frac.std() > 0.1


def test_device_draw_has_multinomials_law():
    """device keys + device select over 4096 trials (the epoch is the trial) against torch.multinomial on the CPU"""
    count = np.zeros(len(LAW_W))
    for t in range(LAW_TRIALS):
        keep = _select(_keys(LAW_W, LAW_SEED, t), LAW_KEEP)
        count += keep
    f_dev, f_ref = count / LAW_TRIALS, multinomial_frequencies()
    assert_same_law(f_dev, f_ref)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the compacted pair
# ---------------------------------------------------------------------------------------------------------------------
def _pruned(rowptr, items, ni, keep):
    """skr_freedom_pruned_csr on a numpy CSR -> ((rowptr', col', val'), (the transpose's), kept), outputs pre-filled with junk"""
    import torch
    from skrec import _hip
    L = _hip.lib()
    nu, nnz = len(rowptr) - 1, len(items)
    rows = T.csr_rows(rowptr)
    order, perm = T.transpose_order(rowptr, items)
    rpt = np.zeros(ni + 1, np.int64)
    rpt[1:] = np.cumsum(np.bincount(items, minlength=ni))
    d = dict(rp=_dev(rowptr.astype(np.int64)), col=_dev(items.astype(np.int32)), rpt=_dev(rpt), colt=_dev(rows[order].astype(np.int32)),
             perm=_dev(perm.astype(np.int32)), keep=_dev(np.asarray(keep, np.uint8)))
    out = [torch.full((nu + 1,), -5, dtype=torch.int64, device="cuda"), torch.full((max(nnz, 1),), -5, dtype=torch.int32, device="cuda"),
           torch.full((max(nnz, 1),), np.nan, dtype=torch.float32, device="cuda"), torch.full((ni + 1,), -5, dtype=torch.int64, device="cuda"),
           torch.full((max(nnz, 1),), -5, dtype=torch.int32, device="cuda"), torch.full((max(nnz, 1),), np.nan, dtype=torch.float32, device="cuda")]
    kept = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    ws = int(L.skr_freedom_pruned_workspace(nu, ni, nnz))
    work = torch.full((max(ws, 16),), 255, dtype=torch.uint8, device="cuda")
    p = _hip.ptr
    _hip.check(L.skr_freedom_pruned_csr(nu, ni, nnz, p(d["rp"]), p(d["col"]), p(d["rpt"]), p(d["colt"]), p(d["perm"]), p(d["keep"]),
                                        *[p(o) for o in out], p(kept), p(work), ws, _hip.stream()))
    k = int(kept.item())
    o = [t.cpu().numpy() for t in out]
    return (o[0], o[1][:k], o[2][:k]), (o[3], o[4][:k], o[5][:k]), k


def _check_pruned(rowptr, items, ni, keep):
    (rp, c, v), (rpt, ct, vt), k = _pruned(rowptr, items, ni, keep)
    (wrp, wc, wv), (wrpt, wct, wvt) = T.pruned_csr(rowptr, items, ni, keep)
    assert k == int(np.asarray(keep).astype(bool).sum()) == rp[-1] == rpt[-1]
    assert np.array_equal(rp, wrp) and np.array_equal(c, wc) and np.array_equal(rpt, wrpt) and np.array_equal(ct, wct)
    if k:
        print("values: largest distance from the restatement", max(_ulps(v, wv).max(), _ulps(vt, wvt).max()), "ulps")
        assert _ulps(v, wv).max() <= 4 and _ulps(vt, wvt).max() <= 4
    return (rp, c, v), (rpt, ct, vt)


def test_pruned_csr_equals_the_references_masked_adj(golden):
    g = golden("golden_freedom")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    rows = T.csr_rows(rowptr)
    for e, keep in enumerate(T.fixture_keeps(g)):
        (rp, c, v), (rpt, ct, vt) = _check_pruned(rowptr, items, ni, keep)
        # the reference's kept entries and values, in both orders
        pos = np.sort(g["keep_idx"][e])
        full = np.zeros(len(items), np.float32)
        full[g["keep_idx"][e]] = g["keep_val"][e]
        assert np.array_equal(c, items[pos]) and np.array_equal(T.csr_rows(rp), rows[pos])
        order = np.lexsort((rows[pos], items[pos]))
        assert np.array_equal(ct, rows[pos][order]) and np.array_equal(T.csr_rows(rpt), items[pos][order])
        print("epoch", e, "largest distance from masked_adj", _ulps(v, full[pos]).max(), "ulps")
        assert _ulps(v, full[pos]).max() <= 4 and _ulps(vt, full[pos][order]).max() <= 4


def test_pruned_csr_edges(golden):
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    rows = T.csr_rows(rowptr)
    nnz = len(items)
    _check_pruned(rowptr, items, ni, np.zeros(nnz, np.uint8))                      # n_keep = 0
    _check_pruned(rowptr, items, ni, np.ones(nnz, np.uint8))                       # nothing dropped
    keep = (np.random.default_rng(1).random(nnz) < 0.4).astype(np.uint8)
    keep[rows == 3] = 0                                                            # an empty kept row
    keep[items == items[0]] = 0                                                    # an empty kept column
    (rp, _, _), (rpt, _, _) = _check_pruned(rowptr, items, ni, keep)
    assert rp[4] == rp[3] and rowptr[4] > rowptr[3] and rpt[items[0] + 1] == rpt[items[0]]
    # more rows than one pass of the scan, a row longer than a wavefront's stride, empty rows, flags that are not 0 / 1
    rng = np.random.default_rng(2)
    U, I = 1500, 1100
    lens = rng.integers(0, 6, U)
    lens[7], lens[1499] = 300, 130
    cols = [np.sort(rng.choice(I, n, replace=False)).astype(np.int32) for n in lens]
    rp2 = np.zeros(U + 1, np.int64)
    rp2[1:] = np.cumsum(lens)
    keep = (rng.random(int(rp2[-1])) < 0.5).astype(np.uint8) * 3
    _check_pruned(rp2, np.concatenate(cols), I, keep)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the whole step against the twin
# ---------------------------------------------------------------------------------------------------------------------
def _graph(U, I, rng, max_len=10):
    lens = rng.integers(1, max_len, U)
    rows = [np.sort(rng.choice(I, n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    return rowptr, np.concatenate(rows)


def _step_case(n, Lu, Lm, d, Fv, Ft, seed, U=48, I=40):
    """a batch with a repeated user, a repeated positive, and an item that is a positive of one row and a negative of another"""
    rng = np.random.default_rng(seed)
    rowptr, items = _graph(U, I, rng)
    users = rng.integers(0, U, n).astype(np.int32)
    pos = rng.integers(0, I, n).astype(np.int32)
    neg = rng.integers(0, I, n).astype(np.int32)
    if n >= 3:
        users[2], pos[2] = users[0], pos[0]
        neg[1] = pos[0]
    if n > 3:
        users[n - 1], pos[n - 1] = U - 1, I - 1
    keep = (rng.random(len(items)) < 0.5).astype(np.uint8)
    P = {"user_embedding.weight": (rng.standard_normal((U, d)) * 0.3).astype(np.float32),
         "item_id_embedding.weight": (rng.standard_normal((I, d)) * 0.3).astype(np.float32)}
    for prefix, F in (("image", Fv), ("text", Ft)):
        if F:
            P[prefix + "_embedding.weight"] = rng.standard_normal((I, F)).astype(np.float32)
            P[prefix + "_trs.weight"] = (rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32)
            P[prefix + "_trs.bias"] = (rng.standard_normal(d) * 0.1).astype(np.float32)
    return dict(U=U, I=I, n=n, Lu=Lu, Lm=Lm, d=d, Fv=Fv, Ft=Ft, rowptr=rowptr, items=items, users=users, pos=pos, neg=neg, keep=keep, P=P)


def _detached(c, reg):
    from skrec.recommender.FREEDOM import FREEDOM
    cfg = dict(lr=1e-2, reg=reg, embed_dim=c["d"], feat_dim=c["d"], n_ui_layers=c["Lu"], n_mm_layers=c["Lm"], dropout=0.5, knn_k=5,
               batch_size=max(c["n"], 1))
    P = c["P"]
    m = FREEDOM.detached(c["U"], c["I"], cfg, (c["rowptr"], c["items"]), img=P.get("image_embedding.weight"),
                         txt=P.get("text_embedding.weight"), seed=SEED)
    m.load_parameters({k: P[k] for k in m.parameters()})
    return m


def _dirty(m):
    """no buffer the step is documented to write may matter beforehand"""
    N = m.num_users + m.num_items
    m._work.fill_(255)
    for t in (m.M, m._G) + tuple(p for p in m._ping if p is not None):
        t.fill_(float("nan"))
    m._grad[:N * 64].fill_(float("nan"))
    if m._modal_trained:
        for key in ("img", "txt"):
            if m.feat_dim[key]:
                m._blocks(key, True)[0].fill_(float("nan"))


def _check_grad(name, got, want):
    """test_gpu_bm3.py's rule for a gradient against float64 autograd"""
    print(name, "max abs err", np.abs(got - want).max(), "max |grad|", np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * np.abs(want).max(), err_msg=name)


# (n, Lu, Lm, d, F_image, F_text, reg): every listed value of every factor, every pair (Lu, Lm) at both reg, each modality
# set at both d; the full product has 144 members
STEP_CASES = [(256, 2, 1, 64, 100, 37, 0.5), (63, 0, 0, 20, 100, 37, 0.5), (1, 1, 0, 64, 100, 0, 0.5), (256, 4, 4, 20, 0, 37, 0.5),
              (63, 2, 1, 64, 100, 37, 0.0), (256, 0, 0, 64, 100, 0, 0.0), (1, 4, 4, 64, 100, 37, 0.0), (63, 1, 0, 20, 0, 37, 0.0),
              (63, 2, 1, 20, 100, 0, 0.5), (63, 4, 4, 64, 100, 37, 0.5), (256, 0, 0, 64, 0, 37, 0.5), (256, 1, 0, 20, 100, 37, 0.5),
              (1, 2, 1, 64, 0, 37, 0.5), (3, 2, 2, 64, 4096, 1, 0.5)]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "n{}-Lu{}-Lm{}-d{}-img{}-txt{}-reg{}".format(*c))
def test_step_matches_the_twin(case):
    import torch
    n, Lu, Lm, d, Fv, Ft, reg = case
    c = _step_case(n, Lu, Lm, d, Fv, Ft, seed=7 * n + Lu)
    U, I = c["U"], c["I"]
    if n >= 3:
        assert len(np.unique(c["users"])) < n and len(np.unique(c["pos"])) < n and np.isin(c["pos"], c["neg"]).any()
    m = _detached(c, reg)
    assert m.optimizer.flat is m._flat and (m._flat.numel() == (U + I) * 64) == (reg == 0)
    keep = m.prune(0, keep=c["keep"])
    assert np.array_equal(keep.cpu().numpy(), c["keep"]) and m.adj_train.nnz == int(c["keep"].sum()) and m.adj_train is not m.adj
    P = {k: v.astype(np.float64) for k, v in c["P"].items()}
    R = T.pruned_block(c["rowptr"], c["items"], I, c["keep"])
    S = T.dense_graph(T.csr_rows(m.mm_adj.rowptr.cpu().numpy()), m.mm_adj.col.cpu().numpy()[:m.mm_adj.nnz],
                      m.mm_adj.val.cpu().numpy()[:m.mm_adj.nnz], I)
    (graph, modal), grads = T.gradients_f64(P, T.t64(R), T.t64(S), c["users"], c["pos"], c["neg"], Lu, Lm, reg)
    with torch.no_grad():
        Mu, Mi = T.forward_f64(T.t64(P["user_embedding.weight"]), T.t64(P["item_id_embedding.weight"]), T.t64(R), T.t64(S), Lu, Lm)
    _dirty(m)
    loss = m.gradient_step(c["users"], c["pos"], c["neg"]).cpu().numpy()
    print("loss", loss, "twin", graph, modal)
    np.testing.assert_allclose(loss[0], graph, rtol=1e-5)
    np.testing.assert_allclose(loss[1], modal, rtol=1e-5, atol=0)
    np.testing.assert_allclose(loss[2], graph + modal, rtol=1e-5)
    Mg = m.M.cpu().numpy()
    np.testing.assert_allclose(Mg[:U, :d], Mu.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(Mg[U:, :d], Mi.numpy(), rtol=1e-5, atol=1e-6)
    assert not Mg[:, d:].any()
    G = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    assert list(G) == list(T.param_names(bool(Fv), bool(Ft)))
    for name in G:
        if name in T.BIASES or reg == 0 and name not in T.BASE:
            assert not G[name].any(), name                  # exact zeros: the bias cancels; at reg == 0 nothing modal moves
        else:
            _check_grad(name, G[name], grads[name])
    assert not m._grad[:(U + I) * 64].view(U + I, 64)[:, d:].any()
    # two runs from the same state give the same bits everywhere (the second one clears what the first wrote)
    first = (loss, Mg, m._grad.clone())
    m._work.fill_(3)
    loss2 = m.gradient_step(c["users"], c["pos"], c["neg"]).cpu().numpy()
    assert np.array_equal(first[0], loss2) and np.array_equal(first[1], m.M.cpu().numpy()) and torch.equal(first[2], m._grad)
    # the optimiser: at reg == 0 the modal blocks stay outside it, bit-unchanged
    before = m.parameters()
    m.train_step(c["users"], c["pos"], c["neg"])
    after = m.parameters()
    assert not torch.equal(before["user_embedding.weight"], after["user_embedding.weight"])
    for name in before:
        if name in T.BIASES or reg == 0 and name not in T.BASE:
            assert torch.equal(before[name], after[name]), name
        elif name.endswith("_trs.weight"):
            assert not torch.equal(before[name], after[name]), name
    assert float(m._grad.abs().max()) == 0.0                 # the launch zeroes the gradient it has read


def test_unpruned_pair_with_no_dropout():
    c = _step_case(63, 2, 1, 64, 100, 37, seed=5)
    from skrec.recommender.FREEDOM import FREEDOM
    m = FREEDOM.detached(c["U"], c["I"], dict(dropout=0.0, knn_k=5, batch_size=63), (c["rowptr"], c["items"]),
                         img=c["P"]["image_embedding.weight"], seed=SEED)
    assert m.prune(0) is None and m.adj_train is m.adj and m.adj_train_t is m.adj_t


# ---------------------------------------------------------------------------------------------------------------------
# 5. the golden replay
# ---------------------------------------------------------------------------------------------------------------------
def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="FREEDOM", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED, sampler_mode="exact")


def _model(data_dir, **kw):
    from skrec.recommender.FREEDOM import FREEDOM
    cfg = dict(CONFIG)
    cfg.update(kw)
    _seed()
    return FREEDOM(_run_config(data_dir), cfg)


def _write_features(tiny_dir, g, text=True):
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), features=g["image_embedding_weight_0"])
    if text:
        np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), features=g["text_embedding_weight_0"])


class _Recorded(object):
    """the reference's evaluator contract on recorded scores: predict() -> ndarray (the generic path)"""

    def __init__(self, users, scores):
        self.row = {int(u): r for r, u in enumerate(users)}
        self.scores = scores

    def predict(self, users):
        return self.scores[[self.row[int(u)] for u in users]]


def test_replays_reference(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    g = golden("golden_freedom")
    _write_features(tiny_dir, g)
    m = _model(tiny_dir)
    assert (m.num_users, m.num_items) == (64, 96) and m.feat_dim == {"img": 100, "txt": 37}
    P0 = m.parameters()
    want0 = T.fixture_params(g, 0)
    assert list(P0) == list(want0)
    for name, want in want0.items():
        assert np.array_equal(P0[name].cpu().numpy(), want), name        # same init, same seed
    np.testing.assert_allclose(m.adj.val.cpu().numpy(), g["adj_val"], rtol=2e-7)
    assert np.array_equal(m.adj.col.cpu().numpy(), g["adj_cols"])
    assert _ulps(m.edge_w.cpu().numpy(), g["edge_w"]).max() <= 4
    assert np.array_equal(m.mm_adj.col.cpu().numpy(), g["mm_adj_col"]) and np.array_equal(m.mm_adj.val.cpu().numpy(), g["mm_adj_val"])
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s, drift = g["f64_dev_params"], g["f64_dev_scores"], float(g["bias_drift"])
    steps, keeps = T.fixture_steps(g), T.fixture_keeps(g)
    assert len(steps) == 9 and len(keeps) == 3
    losses, n_eval = [], 0
    for s, st in enumerate(steps):
        if s % 3 == 0:
            m.prune(s // 3, keep=keeps[s // 3])
            assert m.adj_train.nnz == 152
        losses.append(m.train_step(st["users"], st["pos"], st["neg"]).cpu().numpy())
        if (s + 1) % 3:
            continue
        report = np.array(list(m.evaluate().values()), np.float32)
        pred = m.predict(test_users)
        ref = g["pred"][n_eval]
        print("evaluation", n_eval, "max score diff", np.abs(pred - ref).max(), "allowed", 6 * dev_s[n_eval])
        assert np.abs(pred - ref).max() <= 6 * dev_s[n_eval]
        rows, _, n = ev.per_user_rows(m, test_users)
        rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, ref), test_users)
        ok = ~np.isin(test_users, g["close_ids"][n_eval])
        print("near-tie users left out", int((~ok).sum()))
        assert n == 63 and (~ok).sum() == g["close_users"][n_eval]
        assert np.array_equal(rows[ok], rows_ref[ok])
        np.testing.assert_allclose(rows[ok].mean(0), rows_ref[ok].mean(0), rtol=1e-5, atol=0)
        if ok.all():
            np.testing.assert_allclose(report, g["reports"][n_eval], rtol=1e-5, atol=0, err_msg=str(g["names"]))
        n_eval += 1
    assert n_eval == 3
    losses = np.stack(losses)
    print("loss", losses[:, 2], "golden", g["loss"], "largest relative difference", np.abs(losses[:, 2] / g["loss"] - 1).max())
    np.testing.assert_allclose(losses[:, 2], g["loss"], rtol=1e-5)
    P1 = {k: v.cpu().numpy() for k, v in m.parameters().items()}
    final = T.fixture_params(g, 1)
    for k, name in enumerate(T.param_names(True, True)):
        diff = np.abs(P1[name] - final[name]).max()
        if name in T.BIASES:
            print(name, "max abs diff", diff, "allowed (the reference's own drift)", drift)
            assert np.array_equal(P1[name], want0[name]) and diff <= drift
        else:
            print(name, "max abs diff", diff, "allowed", 6 * dev_p[k])
            assert diff <= 6 * dev_p[k]


# ---------------------------------------------------------------------------------------------------------------------
# 6. fit() with device draws, the limits
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_with_device_draws_learns(golden, tiny_dir, monkeypatch, tmp_path):
    import torch
    monkeypatch.chdir(tmp_path)
    _write_features(tiny_dir, golden("golden_freedom"))
    m = _model(tiny_dir)
    reports, kept = [], []
    orig_eval, orig_prune = m.evaluate, m.prune

    def evaluate(tu=None):
        r = orig_eval(tu)
        reports.append(dict(r.items()))
        return r

    def prune(epoch, keep=None):
        k = orig_prune(epoch, keep)
        kept.append(k.cpu().numpy().copy())
        assert m.adj_train.nnz == m.adj_train_t.nnz == int(k.sum())
        return k
    m.evaluate, m.prune = evaluate, prune
    best = m.fit()
    assert np.isfinite(np.array(list(best.values()))).all() and len(reports) == 3 and len(m.step_losses) == 3
    assert torch.isfinite(torch.stack(m.step_losses)).all()
    assert [int(k.sum()) for k in kept] == [T.n_keep_of(763, 0.8)] * 3
    assert not np.array_equal(kept[0], kept[1]) and not np.array_equal(kept[1], kept[2]) and not np.array_equal(kept[0], kept[2])
    print("NDCG@10", [r["NDCG@10"] for r in reports])
    assert reports[-1]["NDCG@10"] > reports[0]["NDCG@10"]
    # predict = M_u M_i^T of the current parameters on the UNPRUNED graph, through the twin
    g = golden("golden_freedom")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    P = {k: T.t64(v.cpu().numpy()) for k, v in m.parameters().items()}
    R = T.t64(T.pruned_block(rowptr, items, ni, None, g["adj_val"]))
    S = T.t64(T.dense_graph(g["mm_adj_row"], g["mm_adj_col"], g["mm_adj_val"], ni))
    Mu, Mi = T.forward_f64(P["user_embedding.weight"], P["item_id_embedding.weight"], R, S, 2, 2)
    users = np.arange(0, 64, 3)
    want = T.scores_f64(Mu, Mi, users).numpy()
    got = m.predict(users)
    print("predict: max abs diff", np.abs(got - want).max())
    # 64-term fp32 dot products of entries below 1 after two fp32 propagations: a few 1e-7 per score
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=4e-6)


def test_limits_raise(golden, tiny_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    _write_features(tiny_dir, golden("golden_freedom"))
    m = _model(tiny_dir)
    z = np.zeros(2049, np.int32)
    with pytest.raises(NotImplementedError, match="at most 2048"):
        m.gradient_step(z, z, z)
    np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), features=np.zeros((96, 4097), np.float32))
    with pytest.raises(NotImplementedError, match="feature width <= 4096.*text.*4097"):
        _model(tiny_dir)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the edge batches
# ---------------------------------------------------------------------------------------------------------------------
RTOL, ATOL = 1e-4, 2e-5        # _check_grad's
EDGE = (2, 1, 64, 100, 37)     # Lu, Lm, d, F_image, F_text of the small edge cases


def _pruned_model(c, reg):
    m = _detached(c, reg)
    m.prune(0, keep=c["keep"])
    return m


def _twin_run(c, m, rows, dtype, reg, n_div=None):
    """the twin in ``dtype`` on the batch rows ``rows`` of ``c``, on the model's own item graph
    -> ((graph, modal), {name: float64 gradient}, [x_g, x_text, x_image])"""
    import torch
    I = c["I"]
    P = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in c["P"].items()}
    R = torch.tensor(T.pruned_block(c["rowptr"], c["items"], I, c["keep"]), dtype=dtype)
    S = torch.tensor(T.dense_graph(T.csr_rows(m.mm_adj.rowptr.cpu().numpy()), m.mm_adj.col.cpu().numpy()[:m.mm_adj.nnz],
                                   m.mm_adj.val.cpu().numpy()[:m.mm_adj.nnz], I), dtype=dtype)
    args = []
    (g, mm), _, _ = T.losses_f64(P, R, S, c["users"][rows], c["pos"][rows], c["neg"][rows], c["Lu"], c["Lm"], reg, n_div=n_div, args=args)
    (g + mm).backward()
    return [g.item(), mm.item()], {k: np.zeros(v.shape) if v.grad is None else v.grad.numpy().astype(np.float64) for k, v in P.items()}, args


def _edge_compare(c, what, reg=0.5, ok=None, floor=None, widen=False, m=None):
    """The device step on the batch of ``c`` against the float64 twin on the rows ``ok`` (all when None) with n as the divisor.
    ``floor`` ({name: gradient}): each tensor's scale is max|want| or that tensor at a batch without the exact cancellation,
    whichever is more.  ``widen``: allow max(ATOL * scale, 4 x the error of the same twin in float32 on the CPU), both printed"""
    import torch
    n = c["n"]
    ok = np.ones(n, bool) if ok is None else ok
    m = _pruned_model(c, reg) if m is None else m
    comps, G, _ = _twin_run(c, m, ok, torch.float64, reg, n_div=n)
    comps32, G32, _ = _twin_run(c, m, ok, torch.float32, reg, n_div=n) if widen else (comps, None, None)
    _dirty(m)
    loss = m.gradient_step(c["users"], c["pos"], c["neg"]).cpu().numpy()
    want, want32 = (np.array(x + [sum(x)], np.float64) for x in (comps, comps32))
    print(what, "loss", loss, "twin", want, "abs err", np.abs(loss - want), "fp32-CPU err", np.abs(want32 - want))
    assert np.isfinite(loss).all()
    assert np.all(np.abs(loss - want) <= np.maximum(1e-5 * np.abs(want), 4 * np.abs(want32 - want)))
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    assert set(got) == set(G)
    for k in G:                       # every tensor is measured before the assertion
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


@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("n", [15, 16, 17, 64, 65])
def test_batch_sizes_around_the_tiles(n, d):
    """below, at and above 16 and 64 rows (n = 63 is in STEP_CASES): 4 rows per batch workgroup, 16 ranks per feature-gradient tile"""
    c = _step_case(n, 2, 1, d, 100, 37, seed=1000 + n + d)
    assert len(np.unique(c["users"])) < n and len(np.unique(c["pos"])) < n and np.isin(c["pos"], c["neg"]).any()
    _edge_compare(c, f"n = {n}, d = {d}")


def test_full_batch_at_four_layers_each():
    """n = 2048 at n_ui_layers = n_mm_layers = SKR_FREEDOM_MAX_LAYERS = 4 on a 2100 x 2100 graph, both modalities: the 4096 ranks
    of the item list, 128 trips of the float64 weight-gradient sum; then the same call again: the same bits"""
    import time
    import torch
    from skrec import _hip
    t0 = time.time()
    assert _hip.SKR_FREEDOM_MAX_LAYERS == 4 and _hip.SKR_FREEDOM_MAX_BATCH == 2048
    c = _step_case(2048, 4, 4, 64, 100, 37, seed=2100, U=2100, I=2100)
    loss, _, m = _edge_compare(c, "n = 2048", widen=True)
    g1, M1 = m._grad.clone(), m.M.clone()
    m._work.fill_(255)
    loss2 = m.gradient_step(c["users"], c["pos"], c["neg"]).cpu().numpy()
    assert np.array_equal(loss.view(np.uint32), loss2.view(np.uint32)) and torch.equal(g1, m._grad) and torch.equal(M1, m.M)
    print("full batch: wall time", time.time() - t0)


@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("which", ["user", "item"])
def test_one_id_in_every_row(which, n):
    """the longest segment: all n ranks of the user list, or all 2 n ranks of pos || neg, name one id, so one wavefront of
    seg_add (and of the feature rows' seg_rows) walks them all and the rank kernel counts n (2 n) equal keys.  With pos = neg
    every argument is 0 and every item-side gradient cancels exactly: the scales are floored by the same users with the case's
    random items"""
    import torch
    c = _step_case(n, *EDGE, seed=3000 + n)
    m = _pruned_model(c, 0.5)
    floor = _twin_run(c, m, np.ones(n, bool), torch.float64, 0.5, n_div=n)[1]
    if which == "user":
        c["users"][:] = c["users"][n - 1]
    else:
        c["pos"][:] = c["pos"][3]
        c["neg"][:] = c["pos"][3]
    loss, _, _ = _edge_compare(c, f"one {which}, n = {n}", floor=floor, m=m)
    if which == "item":
        np.testing.assert_allclose(loss, np.log(2.0) * np.array([1.0, 1.0, 2.0]), rtol=1e-5)


def test_ids_out_of_range_contribute_nothing():
    """the result is that of the batch without those rows, with n = 70 as the divisor of the three means"""
    U, I, n = 48, 40, 70
    c = _step_case(n, *EDGE, seed=4000)
    users, pos, neg = c["users"], c["pos"], c["neg"]
    users[3], pos[17], users[40], neg[40], neg[69] = U, -1, -7, I, 2 ** 31 - 1
    ok = (users >= 0) & (users < U) & (pos >= 0) & (pos < I) & (neg >= 0) & (neg < I)
    assert ok.sum() == 66
    loss, got, m = _edge_compare(c, "ids out of range", ok=ok)
    # the device's own result on the filtered batch, scaled by 66 / 70
    loss2 = m.gradient_step(users[ok], pos[ok], neg[ok]).cpu().numpy()
    got2 = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    np.testing.assert_allclose(loss, loss2 * 66 / 70, rtol=1e-5)
    for k in got:
        np.testing.assert_allclose(got[k], got2[k] * np.float32(66 / 70), rtol=RTOL, atol=ATOL * np.abs(got[k]).max(), err_msg=k)


def test_an_empty_batch_writes_nothing():
    import ctypes
    import torch
    from skrec import _hip
    c = _step_case(17, *EDGE, seed=5000)
    m = _pruned_model(c, 0.5)
    loss = torch.full((3,), 7.0, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    m._prev_items = ids               # rows that a step would clear first
    a = m._step_args(ids, ids, ids, loss)
    assert a.n_clear == 4
    a.n = 0
    m._grad.fill_(3.0)
    m._work.fill_(5)
    tabs = [m.M, m._G] + [p for p in m._ping if p is not None]
    for t in tabs:
        t.fill_(2.0)
    before = [t.clone() for t in tabs] + [m._work.clone(), m._flat.clone()]
    _hip.check(_hip.lib().skr_freedom_step(ctypes.byref(a), _hip.stream()))
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (m._grad == 3.0).all()
    assert all(torch.equal(x, y) for x, y in zip(before, tabs + [m._work, m._flat]))
    # through the class: a zero loss, a zero gradient whatever the last step left there, nothing left to clear
    m._prev_items = None
    m._grad.zero_()
    m.gradient_step(c["users"], c["pos"], c["neg"])
    assert m._grad.any() and m._prev_items is not None
    z = np.zeros(0, np.int32)
    loss = m.gradient_step(z, z, z)
    assert loss.shape == (3,) and not loss.any() and not m._grad.any() and m._prev_items is None
    # train_step: the zero gradient through Adam, as MGCN, LATTICE and SLMRec do it; with no moments yet nothing moves
    m.gradient_step(c["users"], c["pos"], c["neg"])
    flat = m._flat.clone()
    assert not m.train_step(z, z, z).any()
    assert torch.equal(flat, m._flat)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_bpr_arguments_of_a_hundred(sign):
    """the embeddings scaled (x_g is quadratic in the factor) until x_g reaches +100 or -100, then each projection's weight (x_m
    is linear in it) until x_m does: exp(-|x|) underflows inside log_sigmoid's log1p, sigmoid_neg gives 0 or 1"""
    import torch
    c = _step_case(100, *EDGE, seed=6000)
    m = _pruned_model(c, 0.5)
    rows = np.ones(100, bool)
    ext = lambda x: x.max() if sign > 0 else -x.min()       # noqa: E731
    xg = _twin_run(c, m, rows, torch.float64, 0.5)[2][0]
    for k in T.BASE:
        c["P"][k] = (c["P"][k] * np.sqrt(100.0 / ext(xg))).astype(np.float32)
    xs = _twin_run(c, m, rows, torch.float64, 0.5)[2]
    for k, x in (("text_trs.weight", xs[1]), ("image_trs.weight", xs[2])):
        c["P"][k] = (c["P"][k] * (100.0 / ext(x))).astype(np.float32)
    m.load_parameters({k: c["P"][k] for k in m.parameters()})
    xs = _twin_run(c, m, rows, torch.float64, 0.5)[2]
    print("x_g, x_text, x_image: min", [x.min() for x in xs], "max", [x.max() for x in xs])
    for x in xs:
        assert 99 < ext(x) < 101 and np.float32(1) + np.exp(np.float32(-ext(x))) == 1
    _edge_compare(c, f"arguments of {sign * 100}", widen=True, m=m)
