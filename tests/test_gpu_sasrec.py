"""GPU suite of SASRec (csrc/sasrec.hip, skrec/recommender/SASRec.py): the step against float64 autograd of the twin
(tests/sasrec_twin.py), saturated logits, determinism, the device draws, the query rows, fit() against the twin's float64
trajectory, the l2 term, the evaluator's route and the command line."""
import os

import numpy as np
import pytest

import sasrec_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
SEED = 2021
NI = 37            # items of the step cases; the padding id

# the project's bound for a step's gradients, in units of max|grad| of the parameter.  The twin evaluated in fp32 on torch-CPU
# lies up to 3.5e-3 from its float64 self on STEP_CASES (tests/test_sasrec_host.py::test_fp32_twin_distance_on_the_step_cases
# measures and prints it: torch's fp32 sigmoid backward loses the digits of 1 - s at logits near 14); 4 x that would be the
# widest bound allowed here.  The kernel does not form 1 - s, so the bound is NOT widened.
GRAD_ATOL = 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# cases of the step
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    """a few dozen of the product n x T x (d, heads) x blocks x rate: every T with every (d, heads); n, blocks and rate cycle"""
    out, i = [], 0
    for Tn in (1, 5, 17, 50, 64):
        for d, heads in ((16, 1), (50, 2), (40, 4), (64, 1), (64, 2)):
            out.append(((1, 3, 17)[i % 3], Tn, d, heads, (1, 2)[(i // 3) % 2], (0.0, 0.5)[(i // 2) % 2]))
            i += 1
    return out


STEP_CASES = _cases()


def make_batch(rng, n, Tn, I):
    """sequences with an all-padding row, a full row, a single real item, an interior padding id, one item repeated within and
    across sequences and as both pos and neg"""
    seq, pos, neg = (np.full((n, Tn), I, np.int32) for _ in range(3))
    for b in range(n):
        ln = Tn if b == 0 else int(rng.integers(1, Tn + 1))
        seq[b, Tn - ln:] = rng.integers(0, I, ln)
        pos[b, Tn - ln:] = rng.integers(0, I, ln)
        neg[b, Tn - ln:] = rng.integers(0, I, ln)
    if n >= 2:
        seq[1], pos[1], neg[1] = I, I, I                    # all padding
    if n >= 3:
        seq[2], pos[2], neg[2] = I, I, I                    # a single real item
        seq[2, -1], pos[2, -1], neg[2, -1] = 3, 4, 6
    if n >= 4 and Tn >= 3:
        seq[3, Tn - 3:] = rng.integers(0, I, 3)
        pos[3, Tn - 3:] = rng.integers(0, I, 3)
        neg[3, Tn - 3:] = rng.integers(0, I, 3)
        seq[3, Tn - 2] = I                                  # an interior padding id, under a real target
    seq[0, -1], pos[0, -1] = 5, 5                           # item 5: in seq and pos ...
    if Tn > 1:
        seq[0, 0], neg[0, 0] = 5, 5                         # ... twice in one sequence, and as a negative
    if n >= 5:
        seq[4, -1], neg[4, -1] = 5, 5                       # ... and in another sequence
    return seq, pos, neg


def step_case(n, Tn, d, heads, blocks, rate, seed, scale_out=None):
    import torch
    rng = np.random.default_rng(seed)
    raw = T.random_params(rng, NI, Tn, d, blocks)
    seq, pos, neg = make_batch(rng, n, Tn, NI)
    keep = (rng.random((n, T.keep_bytes(d, Tn, blocks, heads))) >= rate).astype(np.uint8)
    stable = False
    if scale_out is not None:
        stable = scale_out(raw, seq, pos, neg)
    P = T.to_torch(raw)
    ts, tp, tn_ = (torch.from_numpy(a).long() for a in (seq, pos, neg))
    loss, _ = T.step_loss(P, ts, tp, tn_, blocks, heads, keep, rate, stable=stable)
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return dict(n=n, T=Tn, d=d, heads=heads, blocks=blocks, rate=rate, raw=raw, ids=(seq, pos, neg), keep=keep,
                loss=loss.item(), grads=grads)


_CASES = {}


def cached_case(*key):
    if key not in _CASES:
        _CASES[key] = step_case(*key, seed=abs(hash(key)) % (2 ** 31))
    return _CASES[key]


class Device(object):
    """the tables of a case on the device, and one call of the step"""

    def __init__(self, c):
        import torch
        from skrec import _hip
        self.c = c
        raw, d = c["raw"], c["d"]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()    # noqa: E731
        E = np.zeros((NI + 1, 64), np.float32)
        E[:NI, :d] = raw["item_embeddings"]
        self.tabs = [dev(E), dev(T.pad_cols(raw["position_embeddings"])), dev(T.shared_block(raw, d, c["blocks"]))]
        assert self.tabs[2].numel() == _hip.sasrec_shared_floats(c["blocks"])
        assert c["keep"].shape[1] == _hip.sasrec_keep_bytes(d, c["T"], c["blocks"], c["heads"])
        self.nbytes = int(_hip.lib().skr_sasrec_workspace(c["n"], c["T"], c["blocks"], c["heads"]))
        assert self.nbytes > 0
        self.work = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def step(self, keep="case", keep_out=False, rate=None, seed=0, step=0, timed=False):
        """-> (loss [2 * slots], the three gradients, keep_out or None), as numpy"""
        import torch
        from skrec import _hip
        c = self.c
        n = c["n"]
        d_ids = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in c["ids"]]
        grads = [torch.zeros_like(t) for t in self.tabs]
        loss = torch.full((2 * _hip.SKR_LOSS_SLOTS,), 7.0, device="cuda")
        rate = c["rate"] if rate is None else rate
        dk = torch.from_numpy(c["keep"]).cuda() if isinstance(keep, str) else (None if keep is None else torch.from_numpy(keep).cuda())
        ko = torch.full((n, c["keep"].shape[1]), 9, dtype=torch.uint8, device="cuda") if keep_out else None
        args = [*[_hip.ptr(t) for t in self.tabs], *[_hip.ptr(t) for t in d_ids], n, NI, c["d"], c["T"], c["blocks"], c["heads"], rate,
                _hip.ptr(dk), _hip.ptr(ko), seed, step, *[_hip.ptr(g) for g in grads], _hip.ptr(self.work), self.nbytes,
                _hip.ptr(loss), _hip.SKR_LOSS_SLOTS, _hip.stream()]
        if timed:
            ms = np.zeros(_hip.SKR_SASREC_LAUNCHES, np.float32)
            _hip.check(_hip.lib().skr_sasrec_step_timed(*args, ms.ctypes.data))
            self.ms = ms
        else:
            _hip.check(_hip.lib().skr_sasrec_step(*args))
        torch.cuda.synchronize()
        return loss.cpu().numpy(), [g.cpu().numpy() for g in grads], None if ko is None else ko.cpu().numpy()


def _compare(c, loss, grads, rtol=1e-4, floor=0.0):
    gE, gP, gS = grads
    d, blocks = c["d"], c["blocks"]
    want = c["grads"]
    print("loss", loss[0], c["loss"])
    assert np.isfinite(loss).all() and all(np.isfinite(g).all() for g in grads)
    np.testing.assert_allclose(loss[0], c["loss"], rtol=1e-5)
    assert not loss[1:].any()                                        # the l2 word and the untouched slots stay 0
    shared, rest = T.unpack_shared(gS, d, blocks)
    assert not rest.any()                                            # what is padding gets no gradient
    assert not gE[NI].any() and not gE[:, d:].any() and not gP[:, d:].any()      # the padding row and the padded columns: exact zeros
    got = dict(shared, item_embeddings=gE[:NI, :d], position_embeddings=gP[:, :d])
    assert set(got) == set(want)
    for k in want:
        print(k, "max abs err", np.abs(got[k] - want[k]).max(), "max |grad|", np.abs(want[k]).max())
    for k in want:
        w = want[k]
        # bk's gradient is zero in exact arithmetic (a softmax does not see a shift of its row: the rows of dS sum to zero),
        # so what either side holds is rounding noise of the sum dS^T Q; its scale is that of Wk's gradient, the same sum
        # without the cancellation
        scale = np.abs(want["Wk" + k[2:]]).max() if k.startswith("bk_") else np.abs(w).max()
        np.testing.assert_allclose(got[k], w, rtol=rtol, atol=max(GRAD_ATOL * scale, floor), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step against float64 autograd of the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Tn,d,heads,blocks,rate", STEP_CASES)
def test_sasrec_step_matches_float64_autograd(n, Tn, d, heads, blocks, rate):
    """T: one position; less than a 16-row tile; one tile plus one row; the default; the limit.  (d, heads): odd widths, head
    widths that are no multiple of four, the full row.  n = 1, 3, 17 sequences, one workgroup each.  Tolerances: those of
    test_caser_step_matches_float64_autograd (loss rtol 1e-5; gradients rtol 1e-4 and atol 2e-5 max|grad|).  Measured for
    comparison on the CPU (tests/test_sasrec_host.py prints it): the twin evaluated in fp32 on torch-CPU lies up to 3.5e-3
    max|grad| from its float64 self on these cases (see GRAD_ATOL); the bound is not widened."""
    c = cached_case(n, Tn, d, heads, blocks, rate)
    loss, grads, _ = Device(c).step()
    _compare(c, loss, grads)


def test_sasrec_step_without_any_target():
    """a batch of padding alone: loss 0, zero gradients (unreachable through fit())"""
    c = dict(cached_case(3, 5, 16, 1, 1, 0.0))
    ids = tuple(np.full((3, 5), NI, np.int32) for _ in range(3))
    c["ids"] = ids
    loss, grads, _ = Device(c).step()
    assert not loss.any() and not any(g.any() for g in grads)


# ---------------------------------------------------------------------------------------------------------------------
# 2. saturation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mag", [30.0, 110.0])
def test_sasrec_saturated_logits(mag):
    """out rows scaled so that every logit is +-mag up to a few per cent: ln_out_beta = a unit column times mag, ln_out_gamma
    small, and the item rows' first column +-1 / sqrt(d).  Against the twin with sigmoid(-x): at 30 the literal 1 - sigmoid(x)
    carries float64's own cancellation error (1e-16 in 9e-14), at 110 both forms give -log(1e-24).  Loss rtol 1e-5;
    gradients rtol 1e-5 with the step test's absolute floor (a sum that cancels has no relative bound in fp32).  At 110 every
    gradient is of the order 1e-24 in float64 -- sigmoid(-110) = 1.7e-48 -- and exactly 0 on the device, where that is below
    fp32's smallest number: an absolute 1e-20 is allowed there."""
    def scale_out(raw, seq, pos, neg):
        d = raw["item_embeddings"].shape[1]
        rng = np.random.default_rng(1)
        raw["ln_out_gamma"] *= 1e-3
        raw["ln_out_beta"][:] = 0.0
        raw["ln_out_beta"][0] = mag
        raw["item_embeddings"][:, 0] = np.where(rng.random(NI) < 0.5, -1.0, 1.0) / np.sqrt(d)
        return True
    c = step_case(17, 17, 40, 2, 2, 0.0, seed=9, scale_out=scale_out)
    import torch
    P = T.to_torch(c["raw"], requires_grad=False)
    out = T.forward(P, torch.from_numpy(c["ids"][0]).long(), 2, 2)
    pl, nl = T.logits(P, out, torch.from_numpy(c["ids"][1]).long(), torch.from_numpy(c["ids"][2]).long())
    tgt = torch.from_numpy(c["ids"][1] != NI)
    a = pl[tgt].abs()
    print("|logit| range", float(a.min()), float(a.max()), "signs", int((pl[tgt] > 0).sum()), int((pl[tgt] < 0).sum()))
    assert float(a.min()) > 0.9 * mag and float(a.max()) < 1.1 * mag and (pl[tgt] > 0).any() and (pl[tgt] < 0).any()
    loss, grads, _ = Device(c).step()
    _compare(c, loss, grads, rtol=1e-5, floor=1e-20)


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism; 4. device draws
# ---------------------------------------------------------------------------------------------------------------------
def _bits(loss, grads):
    return [loss.view(np.uint32)] + [g.view(np.uint32) for g in grads]


@pytest.fixture(scope="module")
def big_case():
    """1 030 sequences of T = 8: more than the 256 persistent workgroups own one of each, more than one chunk of the rank
    kernel's walk; no float64 result is needed"""
    rng = np.random.default_rng(3)
    n, Tn, d, heads, blocks = 1030, 8, 40, 2, 2
    raw = T.random_params(rng, NI, Tn, d, blocks)
    ids = make_batch(rng, n, Tn, NI)
    keep = (rng.random((n, T.keep_bytes(d, Tn, blocks, heads))) >= 0.5).astype(np.uint8)
    return dict(n=n, T=Tn, d=d, heads=heads, blocks=blocks, rate=0.5, raw=raw, ids=ids, keep=keep)


def test_sasrec_step_is_deterministic(big_case):
    dev = Device(big_case)
    a = dev.step(timed=True)
    assert (dev.ms >= 0).all() and dev.ms.sum() > 0
    b = dev.step()
    assert all(np.array_equal(x, y) for x, y in zip(_bits(*a[:2]), _bits(*b[:2])))
    assert all(np.count_nonzero(g) for g in a[1]) and np.isfinite(a[0]).all()


def test_sasrec_device_draws(big_case):
    c = big_case
    dev = Device(c)
    d, Tn, blocks, heads, n = c["d"], c["T"], c["blocks"], c["heads"], c["n"]
    d1 = dev.step(keep=None, keep_out=True, seed=11, step=3)
    d2 = dev.step(keep=None, keep_out=True, seed=11, step=3)
    assert np.array_equal(d1[2], d2[2]) and set(np.unique(d1[2])) <= {0, 1}
    assert all(np.array_equal(x, y) for x, y in zip(_bits(*d1[:2]), _bits(*d2[:2])))
    d3 = dev.step(keep=d1[2], keep_out=True)                         # the recorded flags, handed in: the same bits
    assert np.array_equal(d3[2], d1[2])
    assert all(np.array_equal(x, y) for x, y in zip(_bits(*d1[:2]), _bits(*d3[:2])))
    d4 = dev.step(keep=None, keep_out=True, seed=11, step=4)         # another step: other flags
    assert not np.array_equal(d4[2], d1[2])
    sites = T.split_keeps(d1[2], d, Tn, blocks, heads)
    for name, k in sites.items():
        k = k.numpy()
        frac, sd = k.mean(), np.sqrt(0.25 / k.size)
        print(name, "kept share", frac, "sd", sd)
        assert abs(frac - 0.5) < 5 * sd, name
    assert not np.array_equal(d1[2][0], d1[2][1])                    # keyed by the sequence
    k0 = dev.step(keep=None, keep_out=True, rate=0.0, seed=11, step=3)[2]
    assert (k0 == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. query rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("Tn,d,heads,blocks", [(50, 64, 1, 2), (1, 16, 1, 1), (17, 50, 2, 2), (64, 40, 4, 1)])
def test_sasrec_queries_match_float64(Tn, d, heads, blocks, with_list):
    import torch
    from skrec import _hip
    rng = np.random.default_rng(Tn + d)
    nU = 150
    raw = T.random_params(rng, NI, Tn, d, blocks)
    win = np.full((nU, Tn), NI, np.int32)
    for u in range(nU):
        ln = Tn if u % 3 == 0 else int(rng.integers(1, Tn + 1))     # u % 3 == 0: a history of at least max_len items
        win[u, Tn - ln:] = rng.integers(0, NI, ln)
    win[5::10] = NI                                                 # users without history
    users = rng.permutation(nU)[:77].astype(np.int32) if with_list else np.arange(nU, dtype=np.int32)
    if with_list:
        users[3] = nU + 2                                           # a user out of range: skipped
        users[4] = 5                                                # a user without history is in the list
    n = len(users)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()    # noqa: E731
    E = np.zeros((NI + 1, 64), np.float32)
    E[:NI, :d] = raw["item_embeddings"]
    dE, dP, dS = dev(E), dev(T.pad_cols(raw["position_embeddings"])), dev(T.shared_block(raw, d, blocks))
    Q = torch.full((n + 1, 64), 7.0, device="cuda")
    du, dw = dev(users), dev(win)
    _hip.check(_hip.lib().skr_sasrec_queries(_hip.ptr(dE), _hip.ptr(dP), _hip.ptr(dS), _hip.ptr(du) if with_list else None, n,
                                             _hip.ptr(dw), nU, NI, d, Tn, blocks, heads, _hip.ptr(Q), _hip.stream()))
    got = Q.cpu().numpy()
    assert (got[n] == 7.0).all()
    inr = users < nU
    if with_list:
        assert (got[3] == 7.0).all()
    P = T.to_torch(raw, requires_grad=False)
    want = T.query_rows(P, torch.from_numpy(win[users[inr]]).long(), blocks, heads).numpy()
    have = got[:n][inr]
    print("max abs err", np.abs(have[:, :d] - want).max(), "max |q|", np.abs(want).max())
    np.testing.assert_allclose(have[:, :d], want, rtol=1e-5, atol=2e-6 * max(1.0, np.abs(want).max()))
    assert not have[:, d:].any()
    none = (win[users[inr]] == NI).all(1)
    assert none.sum() > 0
    np.testing.assert_allclose(have[none][:, :d], np.broadcast_to(np.sqrt(np.float32(d)) * raw["ln_out_beta"], (none.sum(), d)), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 6. fit() against the twin's float64 trajectory; 7. l2_emb; 8. the ranking route; 9. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _write_set(d, root):
    root.mkdir()
    for split in ("train", "test"):
        with open(root / f"{root.name}.{split}", "w") as f:
            for u, i, t in d[split]:
                f.write(f"{int(u)}\t{int(i)}\t1.0\t{int(t)}\n")
    return str(root)


@pytest.fixture()
def seq_dir(tmp_path, golden):
    return _write_set(golden("tiny_seq_dataset"), tmp_path / "tiny_seq")


def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="SASRec", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED)


def _model(data_dir, **kw):
    import random
    import torch
    from skrec.recommender.SASRec import SASRec
    from skrec.utils.py.random import reset_global_sampler
    cfg = dict(T.FIT_CONFIG)
    cfg.update(kw)
    reset_global_sampler(2020)
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)
    return SASRec(_run_config(data_dir), cfg)


def _load_random(m, blocks):
    """the twin's random parameters into the model (see sasrec_twin.TWIN_DEVIATION on why not the default initialisation)"""
    import torch
    cfg = m.config
    raw = T.random_params(np.random.default_rng(SEED), m.num_items, cfg.max_len, cfg.hidden_units, blocks)
    views = m.reference_parameters()
    for k, v in raw.items():
        views[k].copy_(torch.from_numpy(v))
    return raw


def _fit_against_twin(m, rate, l2_emb=0.0, keeps=None):
    cfg = m.config
    nb, nh = cfg.num_blocks, cfg.num_heads
    raw = _load_random(m, nb)
    m.record_batches = []
    losses = []
    te = m.train_epoch

    def train_epoch(it=None):
        te(it)
        losses.append(m.step_losses.cpu().numpy().copy())
    m.train_epoch = train_epoch
    m.fit()
    losses = np.concatenate(losses, 0)
    batches = [tuple(t.cpu().numpy() for t in b) for b in m.record_batches]
    assert len(batches) == 4 and [len(b[0]) for b in batches] == [32, 31, 32, 31]
    want_l, want_p = T.trajectory(raw, batches, nb, nh, cfg.lr, keeps, rate, l2_emb)
    print("losses", losses[:, 0], "twin", want_l)
    np.testing.assert_allclose(losses[:, 0], want_l, rtol=2 * T.TWIN_LOSS_DEVIATION)
    got = {k: v.cpu().numpy() for k, v in m.reference_parameters().items()}
    assert set(got) == set(want_p)
    for k in want_p:
        print(k, "max abs diff", np.abs(got[k] - want_p[k]).max(), "allowed", 2 * T.deviation_of(k))
    for k in want_p:
        np.testing.assert_allclose(got[k], want_p[k], rtol=0, atol=2 * T.deviation_of(k), err_msg=k)
    assert not m._item_rows[m.num_items].any()                        # the padding row stays zero
    return losses


def test_fit_matches_the_float64_trajectory(seq_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(seq_dir)
    assert m.num_items == 96 and m.pad_idx == 96
    _fit_against_twin(m, 0.0)


def test_fit_with_dropout_replayed_from_recorded_flags(seq_dir, monkeypatch, tmp_path):
    """a first run records the flags its steps drew on the device; a second run of the same batches replays them and is
    compared with the twin under those flags"""
    import torch
    monkeypatch.chdir(tmp_path)
    m = _model(seq_dir, dropout_rate=0.5)
    _load_random(m, m.config.num_blocks)
    m.keep_out = []
    m.fit()
    keeps = [k.cpu().numpy() for k in m.keep_out]
    assert len(keeps) == 4 and 0.4 < np.mean([k.mean() for k in keeps]) < 0.6
    m2 = _model(seq_dir, dropout_rate=0.5)
    m2.keep_in = torch.cat(m.keep_out, 0).contiguous()
    _fit_against_twin(m2, 0.5, keeps=keeps)
    assert m2._keep_cursor == m2.keep_in.shape[0]                     # every recorded flag was consumed


def test_fit_with_l2_emb(seq_dir, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    m = _model(seq_dir, l2_emb=1e-3)
    losses = _fit_against_twin(m, 0.0, l2_emb=1e-3)
    assert (losses[:, 1] > 0).all()                                   # the l2 term's word


class _PredictOnly(object):
    """the reference's evaluator contract only: predict() -> ndarray (the generic path)"""

    def __init__(self, m):
        self.m = m

    def predict(self, users):
        return self.m.predict(users)


def test_evaluate_takes_the_fused_route(seq_dir, monkeypatch, tmp_path):
    from skrec.utils.py.evaluator import fused_route
    monkeypatch.chdir(tmp_path)
    m = _model(seq_dir, epochs=1, dropout_rate=0.5)
    m.fit()
    ev = m.evaluator
    Q, E, bias = m.predict_factors()
    assert bias is None and tuple(Q.shape) == (m.num_users, 64) and tuple(E.shape) == (96, 64)
    st = ev._device_state()
    assert fused_route(64, 64, 96, st["max_train"], ev.max_top, os.environ.get("SKR_FUSED_MODE"))
    users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    rows_dev, sums_dev, n_dev = ev.per_user_rows(m, users)
    rows_gen, sums_gen, n_gen = ev.per_user_rows(_PredictOnly(m), users)
    assert n_dev == n_gen == len(users)
    assert np.array_equal(rows_dev, rows_gen)
    pred = m.predict([0, 3])
    assert pred.shape == (2, 96)                                      # without the padding column
    # the query rows are kept between evaluations and dropped by a training step
    assert m._q_current
    q0 = Q.clone()
    m.train_epoch()
    assert not m._q_current
    assert not np.array_equal(m.predict_factors()[0].cpu().numpy(), q0.cpu().numpy())


def test_run_skrec_cli(seq_dir, tmp_path):
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "scikit-recommender_amd", "run_skrec.py")
    r = subprocess.run([sys.executable, script, "--recommender", "SASRec", "--data_dir", seq_dir, "--max_len", "10", "--hidden_units",
                        "32", "--num_heads", "2", "--epochs", "1", "--batch_size", "32", "--top_k", "[5,10]", "--metric",
                        "['Recall','NDCG']", "--seed", "7"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "epoch 0:" in r.stdout and "best:" in r.stdout and "Recall@5" in r.stdout
