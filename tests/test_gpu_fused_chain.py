"""GPU suite: the catch-up of the fused BPR step's kernel with the block's per-step scalars held in lanes (read with
v_readlane_b32) and the refined reciprocal of the second bias correction shared by a step's updates -- against the forms it
replaced (skr_selftest_step_chain) and, through FusedBlocks, against the dense optimiser, bit for bit (int32 views of p, m
and v)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (t0, k, s_from, run_len): non-unit regime; unit regime; the two sets at t0 = 16 580; step index 63, the last lane of the tables.
# With beta2 = 0.999 the second bias correction turns 1.0f at step 16 628 (_first_unit below), so the block of t0 = 16 580 lies
# wholly in the non-unit regime; what those two sets are there for -- first_unit strictly inside the block and not on a multiple
# of four, and a run that starts non-unit and ends unit -- is covered by the same two shapes at t0 = 16 620 (first_unit = 7)
CHAIN_SETS = ([(0, 32, 0, r) for r in (1, 4, 5, 31)] + [(20000, 32, 0, r) for r in (1, 4, 5, 31)] +
              [(16580, 32, 0, 31), (16580, 32, 3, 9), (16620, 32, 0, 31), (16620, 32, 3, 9), (0, 64, 60, 4), (0, 64, 63, 1)])


def _first_unit(t0, k, beta2=0.999):
    """the smallest s of the block with float32(sqrt(1 - beta2^t)) == 1, as the host computes the scalars (doubles)"""
    for s in range(k):
        if np.float32(np.sqrt(1.0 - float(np.float32(beta2)) ** (t0 + 1 + s))) == np.float32(1.0):
            return s
    return k


def test_the_mixed_sets_straddle_first_unit():
    """the t0 = 16 620 sets and the blocks of the FusedBlocks cases are what their comments say (host arithmetic only; kept
    with the GPU cases it guards)"""
    fu = _first_unit(16620, 32)
    assert 0 < fu < 31 and fu % 4 != 0, fu            # strictly inside the block, not on a multiple of four
    assert 3 < fu < 3 + 9, fu                         # the run [3, 12) starts non-unit and ends unit
    assert _first_unit(0, 64) == 64 and _first_unit(20000, 32) == 0
    assert [_first_unit(16590 + 33 * q, 33) for q in range(3)] == [33, 4, 0]
    assert [_first_unit(16600 + 33 * q, 33) for q in range(3)] == [27, 0, 0]


@pytest.mark.parametrize("with_grad", [1, 0])
@pytest.mark.parametrize("t0,k,s_from,run_len", CHAIN_SETS)
def test_chain_matches_the_forms_it_replaced(t0, k, s_from, run_len, with_grad):
    """skr_selftest_step_chain on 2^22 hashed tuples: the advance the step kernel inlines == adam_grad_run (with the leading
    gradient update) / adam_zero_run (without), bits of p, m, v.  Every wavefront of ordinary magnitudes took the scaling-free
    form (the constructed number exactly), every control -- two of every 16 wavefronts hold lanes outside the ordinary ranges
    -- the general one"""
    from skrec import _hip
    n = 1 << 22
    out = (C.c_uint64 * 5)()
    _hip.check(_hip.lib().skr_selftest_step_chain(n, 1e-3, 0.9, 0.999, 1e-8, t0, k, s_from, run_len, with_grad, out, _hip.stream()))
    tested, bad, fast, ctl_general, ctl_fast = (int(x) for x in out)
    groups = n // 64
    controls = groups // 8
    print("selftest_step_chain", t0, k, s_from, run_len, with_grad, tested, bad, fast, ctl_general, ctl_fast)
    assert tested == n and bad == 0
    assert fast == groups - controls
    assert ctl_general == controls and ctl_fast == 0


# ---- through FusedBlocks ------------------------------------------------------------------------------------------------
# nU = 300, nI = 130: three bias blocks, the last with two live lanes and lanes past the end of the buffer.  Rows are distinct
# within a step (each float atomic then happens once: deterministic gradients), which needs 2 b <= nI - 3: b = 256 cannot
# have that among 130 items, so it runs with nI = 578 -- ten bias blocks, the last again with two live lanes.  b = 32 is the
# full-workgroup case at nI = 130.
NU = 300
ITEM_TWICE = 5                 # named at step 0 of a block and again only at step k - 1
ITEMS_NEVER = (7, 100)         # named by no batch
USER_ALWAYS = 0                # named in every step: empty runs
SHAPES = [(1, 130), (6, 130), (32, 130), (256, 578)]      # (b, nI)
# (k, t0); (33, 16 600) beside the (33, 16 590) asked for: its first block turns unit at index 27, no multiple of four
BLOCKS = [(1, 0), (1, 40000), (5, 0), (5, 40000), (33, 0), (33, 16590), (33, 16600), (33, 40000), (64, 0), (64, 40000)]


def _state(rng, nI):
    """a model some way into training: lively rows and biases, so that rows and bias blocks take the scaling-free forms;
    the second bias block holds lanes with untouched moments (m = v = +0), so that it takes the general one"""
    n_par = (NU + nI) * 64 + nI
    p = (rng.standard_normal(n_par) * 0.05).astype(np.float32)
    g0 = (rng.standard_normal(n_par) * 0.01).astype(np.float32)
    m = g0.copy()
    v = (g0 * g0 * rng.uniform(0.5, 1.5, n_par) + 1e-7).astype(np.float32)
    null = (NU + nI) * 64 + 64 + np.arange(0, 64, 5)
    m[null] = 0.0
    v[null] = 0.0
    return p, m, v


def _batches(rng, b, nI, k):
    """three blocks of k steps.  Column 0: USER_ALWAYS in every step, and ITEM_TWICE as the positive item at the first and
    the last step of every block; everything else distinct within a step and never ITEMS_NEVER"""
    import torch
    users = np.arange(1, NU)
    pool = np.array([x for x in range(nI) if x != ITEM_TWICE and x not in ITEMS_NEVER])
    n_steps = 3 * k
    u = np.empty((n_steps, b), np.int64)
    ij = np.empty((n_steps, 2 * b), np.int64)
    for s in range(n_steps):
        u[s, 0] = USER_ALWAYS
        u[s, 1:] = rng.permutation(users)[:b - 1]
        if s % k in (0, k - 1):
            ij[s, 0] = ITEM_TWICE
            ij[s, 1:] = rng.permutation(pool)[:2 * b - 1]
        else:
            ij[s] = rng.permutation(pool)[:2 * b]
    return tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in (u, ij[:, :b], ij[:, b:]))


def _opt(state, t0, **kw):
    import torch
    from skrec.recommender.base import DenseAdam
    o = DenseAdam(torch.from_numpy(state[0].copy()).cuda(), lr=1e-2, **kw)
    o.m.copy_(torch.from_numpy(state[1]).cuda())
    o.v.copy_(torch.from_numpy(state[2]).cuda())
    o.t = t0
    return o


_dense_cache = {}


def _dense(b, nI, k, t0):
    """the reference, computed once per case and shared by the two settings: skr_bpr_step + one dense skr_adam_step per batch"""
    import torch
    from skrec import _hip
    key = (b, nI, k, t0)
    if key not in _dense_cache:
        L = _hip.lib()
        rng = np.random.default_rng(9000 + 7 * b + k + t0)
        state = _state(rng, nI)
        u, i, j = _batches(rng, b, nI, k)
        a = _opt(state, t0, track_touch=True)
        loss = torch.zeros(2, device="cuda")
        sl = lambda t: (t[:NU * 64].view(NU, 64), t[NU * 64:(NU + nI) * 64].view(nI, 64), t[(NU + nI) * 64:])  # noqa: E731
        (U, V, bias), (gU, gV, gb) = sl(a.flat), sl(a.grad)
        for s in range(3 * k):
            _hip.check(L.skr_bpr_step(_hip.ptr(U), _hip.ptr(V), _hip.ptr(bias), _hip.ptr(U), _hip.ptr(V), _hip.ptr(u[s]),
                                      _hip.ptr(i[s]), _hip.ptr(j[s]), b, 1.0, 1e-3, 1.0, _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(gb),
                                      _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(loss), _hip.ptr(a.touch), _hip.ptr(a.grad), _hip.stream()))
            a.step()
        torch.cuda.synchronize()
        _dense_cache[key] = (state, (u, i, j), tuple(t.view(torch.int32).clone() for t in (a.flat, a.m, a.v)))
    return _dense_cache[key]


@pytest.mark.parametrize("pre", ["1", "0"])
@pytest.mark.parametrize("k,t0", BLOCKS)
@pytest.mark.parametrize("b,nI", SHAPES)
def test_fused_blocks_match_the_dense_optimiser(b, nI, k, t0, pre, monkeypatch):
    """three k-step blocks of the one-launch step == the dense reference, bits of p, m, v, and every gradient plane zero
    afterwards.  b = 1: one workgroup with three idle wavefronts; b = 6: a second workgroup with two; b = 32 / 256: full
    workgroups.  The schedule holds an item named at step 0 and again only at step k - 1 (a gradient update with k - 2
    zero-gradient updates behind it), a user named in every step (empty runs) and items never named.  pre = "0"
    (SKR_FUSED_PRE=0, set before FusedBlocks is constructed): first namings catch up from index 0 themselves -- long
    zero-gradient runs that start at 0.  t0 = 16 590 / 16 600 with k = 33: the blocks around step 16 628, where the
    second bias correction turns 1.0f"""
    import torch
    from skrec import _hip
    from skrec.recommender.fused import FusedBlocks
    monkeypatch.setenv("SKR_FUSED_PRE", pre)
    state, (u, i, j), want = _dense(b, nI, k, t0)
    c = _opt(state, t0)
    S = _hip.SKR_LOSS_SLOTS
    lc = torch.zeros((3 * k, S, 2), device="cuda")
    fb = FusedBlocks(c, 0, NU, NU + nI, 1e-3)
    assert fb.pre_advance == (pre == "1")
    fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), 3, k, b, lc.data_ptr(), 8 * S)
    c.end_blocks()
    torch.cuda.synchronize()
    assert c.t == t0 + 3 * k
    for name, got, w in zip("pmv", (c.flat, c.m, c.v), want):
        diff = int((got.view(torch.int32) != w).sum())
        assert diff == 0, f"{name}: {diff} elements differ"
    assert float(fb.work[:, 6 * fb.cap * 64:].abs().max()) == 0.0          # every gradient was consumed, the planes are zero
