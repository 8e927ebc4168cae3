"""GPU suite: the load phase of the fused BPR step's kernel -- the ids and words in one round, then all five rows' loads from
addresses selected by the row's source (pre buffer, dense tables, workspace) -- through FusedBlocks against the dense
optimiser, bit for bit (int32 views of p, m and v).  What the other fused suites do not pin: every source in every one of the
five row positions, all three sources within one interaction, and a batch larger than one pass of the grid."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSITIONS = ("user", "positive item", "negative item", "positive bias block", "negative bias block")
PRE, DENSE, WORK = 0, 1, 2

# ---- every source in every position -------------------------------------------------------------------------------------
# nU = 300, nI = 130: three bias blocks, the last (items 128, 129) with two live lanes and lanes past the end of the buffer.
# Block 0 draws its items from 0 .. 127, blocks 1 and 2 from 0 .. 63, so that whole bias blocks stay cold for a block:
#   block 1, step 1, column 0:  USER_ALWAYS (workspace), item 128 as the positive (item row and bias block 2 from the pre
#                               buffer: block 0 named neither), ITEM_HOT as the negative (dense: block 0 named it, block 1
#                               not before this step) -- all three sources in one interaction
#   block 1, step 2, column 0:  item 129 as the negative (pre buffer; its bias block from the workspace)
#   block 2, step 1, column 0:  item 70 as the negative (item row and bias block 1 from the pre buffer: block 1 named neither)
NU, NI, B = 300, 130, 16
USER_ALWAYS, ITEM_HOT = 0, 5


def _schedule(k):
    rng = np.random.default_rng(4100 + k)
    u = np.empty((3 * k, B), np.int64)
    ij = np.empty((3 * k, 2 * B), np.int64)
    users = np.arange(1, NU)
    for s in range(3 * k):
        blk, st = divmod(s, k)
        pool = np.array([x for x in range(128 if blk == 0 else 64) if x != ITEM_HOT])
        u[s, 0] = USER_ALWAYS
        u[s, 1:] = rng.permutation(users)[:B - 1]
        ij[s] = rng.permutation(pool)[:2 * B]
        if (blk, st) == (0, 0):
            ij[s, 0] = ITEM_HOT
        elif (blk, st) == (1, 1):
            ij[s, 0], ij[s, B] = 128, ITEM_HOT
        elif (blk, st) == (1, 2):
            ij[s, B] = 129
        elif (blk, st) == (2, 1):
            ij[s, B] = 70
    return tuple(np.ascontiguousarray(x).astype(np.int32) for x in (u, ij[:, :B], ij[:, B:]))


def _sources(u, i, j, k, pre):
    """[3 blocks, k, 5, B] source of every reference, from build_fused_meta on CPU tensors: pre buffer when the n0 field is 7,
    dense when it is not and prev1 = 0, workspace otherwise.  prev_hot: what FusedBlocks hands the plan -- nothing is
    pre-advanced for the first block of a call, later blocks get the rows the block before named"""
    import torch
    from skrec.recommender.fused import build_fused_meta
    nfb = ((NU + NI) * 64 + NI + 63) // 64
    prev_hot = None
    if pre:
        prev_hot = torch.ones((3, nfb), dtype=torch.bool)
        for q in (1, 2):
            sl = slice((q - 1) * k, q * k)
            named = np.concatenate([u[sl].ravel(), NU + i[sl].ravel(), NU + j[sl].ravel(), NU + NI + (i[sl].ravel() >> 6),
                                    NU + NI + (j[sl].ravel() >> 6)])
            prev_hot[q] = False
            prev_hot[q, torch.from_numpy(np.unique(named).astype(np.int64))] = True
    t = [torch.from_numpy(x.reshape(-1)) for x in (u, i, j)]
    meta = build_fused_meta(t[0], t[1], t[2], 3, k, B, 0, NU, NU + NI, prev_hot=prev_hot)[0].numpy().astype(np.int64)
    n0f, prev1 = (meta >> 20) & 7, (meta >> 24) & 0x7f
    return np.where(n0f == 7, PRE, np.where(prev1 == 0, DENSE, WORK))


def _state(rng, n_rows, nI):
    """a model some way into training: lively rows and biases"""
    n_par = n_rows * 64 + nI
    p = (rng.standard_normal(n_par) * 0.05).astype(np.float32)
    g0 = (rng.standard_normal(n_par) * 0.01).astype(np.float32)
    v = (g0 * g0 * rng.uniform(0.5, 1.5, n_par) + 1e-7).astype(np.float32)
    return p, g0.copy(), v


def _opt(state, t0, **kw):
    import torch
    from skrec.recommender.base import DenseAdam
    o = DenseAdam(torch.from_numpy(state[0].copy()).cuda(), lr=1e-2, **kw)
    o.m.copy_(torch.from_numpy(state[1]).cuda())
    o.v.copy_(torch.from_numpy(state[2]).cuda())
    o.t = t0
    return o


_dense_cache = {}


def _dense(key, nU, nI, b, k, batches, seed):
    """the reference, computed once per case and shared by the settings: skr_bpr_step + one dense skr_adam_step per batch"""
    import torch
    from skrec import _hip
    if key not in _dense_cache:
        L = _hip.lib()
        state = _state(np.random.default_rng(seed), nU + nI, nI)
        u, i, j = (torch.from_numpy(x).cuda() for x in batches)
        a = _opt(state, 0, track_touch=True)
        loss = torch.zeros(2, device="cuda")
        sl = lambda t: (t[:nU * 64].view(nU, 64), t[nU * 64:(nU + nI) * 64].view(nI, 64), t[(nU + nI) * 64:])  # noqa: E731
        (U, V, bias), (gU, gV, gb) = sl(a.flat), sl(a.grad)
        for s in range(3 * k):
            _hip.check(L.skr_bpr_step(_hip.ptr(U), _hip.ptr(V), _hip.ptr(bias), _hip.ptr(U), _hip.ptr(V), _hip.ptr(u[s]),
                                      _hip.ptr(i[s]), _hip.ptr(j[s]), b, 1.0, 1e-3, 1.0, _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(gb),
                                      _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(loss), _hip.ptr(a.touch), _hip.ptr(a.grad), _hip.stream()))
            a.step()
        torch.cuda.synchronize()
        _dense_cache[key] = (state, (u, i, j), tuple(t.view(torch.int32).clone() for t in (a.flat, a.m, a.v)))
    return _dense_cache[key]


def _run_and_compare(state, cols, want, nU, nI, b, k, pre):
    import torch
    from skrec import _hip
    from skrec.recommender.fused import FusedBlocks
    u, i, j = cols
    c = _opt(state, 0)
    S = _hip.SKR_LOSS_SLOTS
    lc = torch.zeros((3 * k, S, 2), device="cuda")
    fb = FusedBlocks(c, 0, nU, nU + nI, 1e-3)
    assert fb.pre_advance == (pre == "1")
    fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), 3, k, b, lc.data_ptr(), 8 * S)
    c.end_blocks()
    torch.cuda.synchronize()
    assert c.t == 3 * k
    for name, got, w in zip("pmv", (c.flat, c.m, c.v), want):
        diff = int((got.view(torch.int32) != w).sum())
        assert diff == 0, f"{name}: {diff} elements differ"
    assert float(fb.work[:, 6 * fb.cap * 64:].abs().max()) == 0.0          # every gradient was consumed, the planes are zero


@pytest.mark.parametrize("pre", ["1", "0"])
@pytest.mark.parametrize("k", [4, 33])
def test_every_source_in_every_position(k, pre, monkeypatch):
    """three k-step blocks whose schedule puts each of the five row positions on each source at least once, and all three
    sources into one interaction (asserted on the host, from the plan's words, before any launch) == the dense reference,
    bits of p, m, v; every gradient plane zero afterwards.  pre = "0": the ten (position, source) pairs without the pre
    buffer"""
    monkeypatch.setenv("SKR_FUSED_PRE", pre)
    u, i, j = _schedule(k)
    for s in range(3 * k):                 # rows distinct within a step: deterministic gradients
        assert len(set(u[s])) == B and len(set(i[s]) | set(j[s])) == 2 * B
    src = _sources(u, i, j, k, pre == "1")
    for r, name in enumerate(POSITIONS):
        for source in ((PRE, DENSE, WORK) if pre == "1" else (DENSE, WORK)):
            assert (src[:, :, r, :] == source).any(), f"{name}: no reference takes source {source}"
    if pre == "1":
        per_interaction = [set(src[q, s, :, c]) for q in range(3) for s in range(k) for c in range(B)]
        assert any(len(x) == 3 for x in per_interaction)
        assert set(src[1, 1, :, 0]) == {PRE, DENSE, WORK}
    else:
        assert not (src == PRE).any()
    state, cols, want = _dense(("positions", k), NU, NI, B, k, (u, i, j), 4200 + k)
    _run_and_compare(state, cols, want, NU, NI, B, k, pre)


# ---- more interactions than one pass of the grid ------------------------------------------------------------------------
# the step launch has at most 4 096 workgroups of four wavefronts: with b = 16 388 the kernel's loop runs a second time for
# the first four interactions' wavefronts only
BIG_NU, BIG_NI, BIG_B, BIG_K = 20000, 40000, 16388, 2


@pytest.mark.parametrize("pre", ["1", "0"])
def test_batch_larger_than_one_pass_of_the_grid(pre, monkeypatch):
    """three 2-step blocks of 16 388 interactions, users and items distinct within a step == the dense reference, bits of p,
    m, v; every gradient plane zero afterwards"""
    monkeypatch.setenv("SKR_FUSED_PRE", pre)
    assert 4 * 4096 < BIG_B < 8 * 4096
    rng = np.random.default_rng(4300)
    u = np.stack([rng.permutation(BIG_NU)[:BIG_B] for _ in range(3 * BIG_K)]).astype(np.int32)
    ij = np.stack([rng.permutation(BIG_NI)[:2 * BIG_B] for _ in range(3 * BIG_K)]).astype(np.int32)
    i, j = np.ascontiguousarray(ij[:, :BIG_B]), np.ascontiguousarray(ij[:, BIG_B:])
    state, cols, want = _dense(("big",), BIG_NU, BIG_NI, BIG_B, BIG_K, (u, i, j), 4301)
    _run_and_compare(state, cols, want, BIG_NU, BIG_NI, BIG_B, BIG_K, pre)
