"""CPU suite of SASRec: the three claims the kernel relies on, proven on the float64 twin (tests/sasrec_twin.py); the training
rows against a literal loop; the flat buffer's round trip; the config and every named limit; and the distance of the twin in
fp32 from its float64 self on the GPU suite's step cases (the figure that suite's tolerance refers to)."""
import numpy as np
import pytest
import torch

import sasrec_twin as T

I, TN, D, BLOCKS, HEADS = 29, 9, 12, 2, 2


def _case(seed=0, n=6):
    rng = np.random.default_rng(seed)
    raw = T.random_params(rng, I, TN, D, BLOCKS)
    seq, pos, neg = (np.full((n, TN), I, np.int64) for _ in range(3))
    for b in range(n):
        ln = TN if b == 0 else int(rng.integers(1, TN))
        seq[b, TN - ln:], pos[b, TN - ln:], neg[b, TN - ln:] = (rng.integers(0, I, ln) for _ in range(3))
    seq[1], pos[1], neg[1] = I, I, I                        # all padding
    seq[0, 4] = I                                           # an interior padding id under a real target
    keep = (rng.random((n, T.keep_bytes(D, TN, BLOCKS, HEADS))) >= 0.5).astype(np.uint8)
    return raw, tuple(torch.from_numpy(a) for a in (seq, pos, neg)), keep


def _loss_and_grads(raw, ids, keep, hooks=None, dtype=torch.float64):
    P = T.to_torch(raw, dtype)
    loss, _ = T.step_loss(P, *ids, BLOCKS, HEADS, keep, 0.5, hooks=hooks)
    loss.backward()
    return loss.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_padded_queries_and_the_query_mask_change_nothing(dtype):
    """a padded position's block output is multiplied by 0 and nothing else reads a padded query row: without the query mask,
    and with other values in the padded query rows, loss and gradients have the same bits"""
    raw, ids, keep = _case()
    l0, g0 = _loss_and_grads(raw, ids, keep, dtype=dtype)
    l1, g1 = _loss_and_grads(raw, ids, keep, hooks={"query_mask": False}, dtype=dtype)
    junk = torch.from_numpy(np.random.default_rng(1).standard_normal((ids[0].shape[0], TN, D))).to(dtype)
    l2, g2 = _loss_and_grads(raw, ids, keep, hooks={"padded_queries": junk}, dtype=dtype)
    assert np.isfinite(l0) and any(np.abs(v).max() > 0 for v in g0.values())
    for l, g in ((l1, g1), (l2, g2)):
        assert l.tobytes() == l0.tobytes()
        for k in g0:
            assert np.array_equal(g[k], g0[k]), k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_masked_keys_weigh_exactly_zero(dtype):
    """exp(-2^32 + 1 - max) is exactly 0 where the query has a real key of its own: the kernel may skip masked keys"""
    raw, ids, keep = _case()
    hooks = {"weights": []}
    P = T.to_torch(raw, dtype, requires_grad=False)
    T.forward(P, ids[0], BLOCKS, HEADS, hooks=hooks)
    real = (ids[0] != I).numpy()
    assert len(hooks["weights"]) == BLOCKS
    for w in hooks["weights"]:
        w = w.numpy()                                        # [n, heads, T_q, T_k]
        for b in range(w.shape[0]):
            for t in np.nonzero(real[b])[0]:
                masked = ~real[b] | (np.arange(TN) > t)
                assert (w[b, :, t][:, masked] == 0.0).all()
                np.testing.assert_allclose(w[b, :, t].sum(-1), 1.0, rtol=1e-6)


def test_sigmoid_of_minus_x_against_one_minus_sigmoid():
    """-log(1 - sigmoid(x) + 1e-24) and -log(sigmoid(-x) + 1e-24) agree in float64 for |x| <= 15 (beyond, 1 - sigmoid(x) loses
    its digits: 1e-16 in 3e-7 at 15)"""
    x = torch.linspace(-15, 15, 3001, dtype=torch.float64, requires_grad=True)
    tgt = torch.ones_like(x)
    a = -torch.log(1 - torch.sigmoid(x) + 1e-24)
    b = -torch.log(torch.sigmoid(-x) + 1e-24)
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-9)
    ga, = torch.autograd.grad(a.sum(), x)
    gb, = torch.autograd.grad(b.sum(), x)
    np.testing.assert_allclose(ga.numpy(), gb.numpy(), rtol=1e-9)
    la = T.loss_of_logits(x.detach(), x.detach(), tgt, stable=False)
    lb = T.loss_of_logits(x.detach(), x.detach(), tgt, stable=True)
    np.testing.assert_allclose(float(la), float(lb), rtol=1e-12)


def test_train_rows_against_a_literal_loop(golden):
    import os
    from conftest import REPO
    from skrec.recommender.SASRec import eval_windows, generate_train_data
    max_len = 10
    upt, users, seq, pos, n_items = T.tiny_train_rows(os.path.join(REPO, "tests", "golden", "tiny_seq_dataset.npz"), max_len)
    assert n_items == 96 and max(len(v) for v in upt.values()) - 1 > max_len      # a user longer than max_len
    got_seq, got_pos = generate_train_data(upt, users, n_items, max_len)
    assert got_seq.dtype == np.int32 and got_seq.shape == (len(users), max_len)
    assert np.array_equal(got_seq, seq) and np.array_equal(got_pos, pos)
    long_u = max(upt, key=lambda u: len(upt[u]))
    r = users.index(long_u)
    assert list(got_seq[r]) == upt[long_u][-max_len - 1:-1] and list(got_pos[r]) == upt[long_u][-max_len:]
    assert ((got_seq == n_items) == (got_pos == n_items)).all()
    # the evaluation windows: the last max_len items, all padding for a user without any
    del upt[users[0]]
    win = eval_windows(upt, 63, n_items, max_len)
    assert win.shape == (63, max_len) and (win[users[0]] == n_items).all()
    assert list(win[long_u]) == upt[long_u][-max_len:]
    short = min(upt, key=lambda u: len(upt[u]))
    k = len(upt[short])
    assert list(win[short][-k:]) == upt[short] and (win[short][:-k] == n_items).all()


@pytest.mark.parametrize("d", [64, 50])
def test_pack_and_views_round_trip(d):
    from skrec.recommender.SASRec import _Layout, pack_parameters, param_names, parameter_views
    blocks, Tn, ni = 2, 7, 11
    raw = T.random_params(np.random.default_rng(d), ni, Tn, d, blocks)
    lay = _Layout(ni, Tn, blocks)
    flat = pack_parameters(raw, lay, d)
    assert flat.numel() == (ni + 1) * 64 + Tn * 64 + T.shared_floats(blocks)
    v = parameter_views(flat, lay, d)
    assert list(v) == param_names(blocks) == T.param_names(blocks)
    for k in raw:
        assert tuple(v[k].shape) == raw[k].shape and np.array_equal(v[k].numpy(), raw[k]), k
        assert v[k].untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()          # views, not copies
    # the shared block is the kernel's layout; the padding row, the padded columns and rows are zero
    assert np.array_equal(flat[lay.shared:].numpy(), T.shared_block(raw, d, blocks))
    E = flat[:lay.P].view(ni + 1, 64).numpy()
    assert not E[ni].any() and not E[:, d:].any()
    back, rest = T.unpack_shared(flat[lay.shared:].numpy(), d, blocks)
    assert not rest.any() and all(np.array_equal(back[k], raw[k]) for k in back)
    assert int(np.count_nonzero(flat.numpy())) == sum(int(np.count_nonzero(a)) for a in raw.values())


def test_config_defaults_and_validation():
    from skrec.recommender.SASRec import SASRecConfig
    cfg = SASRecConfig()
    want = dict(lr=1e-3, l2_emb=0.0, hidden_units=64, dropout_rate=0.5, max_len=50, num_blocks=2, num_heads=1, batch_size=128,
                epochs=1000, early_stop=100)
    for k, v in want.items():
        got = getattr(cfg, k)
        assert got == v and type(got) is type(v), (k, got, v)
    cfg._validate()
    for bad in (dict(lr=1), dict(l2_emb=-1.0), dict(hidden_units=0), dict(hidden_units=2.0), dict(dropout_rate=1.0), dict(dropout_rate=1),
                dict(max_len=0), dict(num_blocks=0), dict(num_heads=0), dict(batch_size=0), dict(epochs=-1), dict(early_stop=1.5)):
        with pytest.raises(AssertionError):
            SASRecConfig(**bad)._validate()


@pytest.mark.parametrize("kw,exc,match", [
    (dict(hidden_units=65), NotImplementedError, "hidden_units <= 64"), (dict(max_len=65), ValueError, "max_len <= 64.*skr_sasrec_step"),
    (dict(num_blocks=5), ValueError, "num_blocks <= 4.*skr_sasrec_step"), (dict(num_heads=9, hidden_units=63), ValueError, "num_heads <= 8"),
    (dict(num_heads=3), ValueError, "num_heads must divide hidden_units.*skr_sasrec_step"),
    (dict(batch_size=2049), ValueError, "batch_size <= 2048.*skr_sasrec_step")])
def test_limits_are_refused_by_name(kw, exc, match):
    from skrec import _hip
    from skrec.recommender.SASRec import SASRec, SASRecConfig
    m = SASRec.__new__(SASRec)
    m.config = SASRecConfig(**kw)
    with pytest.raises(exc, match=match):
        m._check_limits(1)
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.config = SASRecConfig()
        m._check_limits(2)
    m._check_limits(1)
    assert (_hip.SKR_SASREC_MAX_HIDDEN, _hip.SKR_SASREC_MAX_LEN, _hip.SKR_SASREC_MAX_BLOCKS, _hip.SKR_SASREC_MAX_HEADS,
            _hip.SKR_SASREC_MAX_BATCH) == (64, 64, 4, 8, 2048)
    assert _hip.sasrec_shared_floats(2) == T.shared_floats(2) and _hip.sasrec_keep_bytes(50, 17, 2, 2) == T.keep_bytes(50, 17, 2, 2)
    L = _hip.lib()
    assert L.skr_sasrec_workspace(0, 50, 2, 1) == 0 and L.skr_sasrec_workspace(128, 65, 2, 1) == 0
    assert L.skr_sasrec_workspace(128, 50, 2, 1) > 0
    assert L.skr_sasrec_step(*([None] * 6), 1, 10, 64, 50, 2, 1, 0.5, None, None, 0, 0, None, None, None, None, 0, None, 1, None) == -1
    assert b"NULL" in L.skr_last_error()


def test_fp32_twin_distance_on_the_step_cases():
    """the figure tests/test_gpu_sasrec.py's gradient tolerance refers to: over its step cases, the largest distance of the
    twin's fp32 gradients from its float64 ones in units of max|grad| of the parameter (bk apart, whose gradient is zero in
    exact arithmetic).  That suite's bound may be as wide as the larger of the project's 2e-5 and 4 x this figure.  Measured:
    3.5e-3, at (n, T, d, heads, blocks, rate) = (1, 1, 64, 1, 2, 0.5), ln2_gamma_0: a single target whose logits lie near 14, where
    torch's fp32 sigmoid backward forms 1 - s from s = 0.999999 and loses its digits.  The kernel forms sigmoid(-x) instead, so
    the GPU suite keeps the project's 2e-5"""
    import test_gpu_sasrec as G
    worst, where = 0.0, None
    for key in G.STEP_CASES:
        c = G.cached_case(*key)
        n, Tn, d, heads, blocks, rate = key
        P = T.to_torch(c["raw"], torch.float32)
        ids = tuple(torch.from_numpy(a).long() for a in c["ids"])
        loss, _ = T.step_loss(P, *ids, blocks, heads, c["keep"], rate, stable=True)    # (fp32 rounds 1 - sigmoid(x) to 0 beyond 17)
        loss.backward()
        for k, w in c["grads"].items():
            if k.startswith("bk_"):                         # zero in exact arithmetic: rounding noise on both sides
                continue
            g = P[k].grad.numpy() if P[k].grad is not None else np.zeros(w.shape)
            m = np.abs(w).max()
            if m > 0:
                dist = float(np.abs(g - w).max() / m)
                if dist > worst:
                    worst, where = dist, (key, k)
    print("fp32 twin: largest distance", worst, "at", where)
    assert np.isfinite(worst) and G.GRAD_ATOL <= max(2e-5, 4 * worst)
