"""GPU suite: the catch-up of the fused BPR step's kernel with two consecutive updates of a row in the halves of packed
fp32 instructions (chain_ordinary_group, adam_math.h: G pairs side by side, the end of a run as one narrower group, a pair
never across the step where the second bias correction turns 1.0f) -- every group shape against the forms it replaced
(skr_selftest_step_chain) and, through FusedBlocks, against the dense optimiser, bit for bit (int32 views of p, m and v)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 4                          # the widest layout the run may choose (pairs side by side); the shapes below cover G = 2 too
LENS = range(1, 2 * G + 4)     # run lengths 1 .. 2 G + 3: every narrower group, a full group, a full group and each remainder up to 3

# (t0, k, s_from, run_len).  Non-unit (t0 = 0) and unit (t0 = 20 000) regime, every length from an even and an odd s_from
SHAPE_SETS = [(t0, 32, s_from, r) for t0 in (0, 20000) for s_from in (2, 3) for r in LENS]
# k = 64, the last lanes of the tables: a pair at (62, 63), a lone update at 63, three updates whose second pair has an idle
# half behind index 63 (it must read a valid lane), and the longest run there is
LAST_LANE_SETS = [(0, 64, 62, 2), (0, 64, 63, 1), (0, 64, 61, 3), (0, 64, 0, 64), (20000, 64, 0, 64)]
# t0 = 16 620: first_unit = 7.  Counting pairs from s_from, index 7 is the second half of a pair from s_from 0 and 6, the first
# half from s_from 1, 3 and 7, the first update of the second group of four from s_from 3 and of the run from s_from 7; the
# runs end before it, on it, one past it and well past it
TURN_SETS = [(16620, 32, s_from, r) for s_from, rs in ((0, (7, 8, 9, 12, 25)), (1, (6, 7, 8, 12)), (3, (4, 5, 6, 12)), (6, (1, 2, 3, 12)),
                                                        (7, (1, 2, 12))) for r in rs]


def _first_unit(t0, k, beta2=0.999):
    """the smallest s of the block with float32(sqrt(1 - beta2^t)) == 1, as the host computes the scalars (doubles)"""
    for s in range(k):
        if np.float32(np.sqrt(1.0 - float(np.float32(beta2)) ** (t0 + 1 + s))) == np.float32(1.0):
            return s
    return k


def test_the_turn_sets_are_what_they_say():
    """host arithmetic only; kept with the GPU cases it guards"""
    assert _first_unit(16620, 32) == 7
    assert _first_unit(0, 64) == 64 and _first_unit(20000, 64) == 0
    assert [_first_unit(16600 + k * q, k) for k in (5, 33, 64) for q in range(3)] == [5, 5, 5, 27, 0, 0, 27, 0, 0]


@pytest.mark.parametrize("with_grad", [1, 0])
@pytest.mark.parametrize("t0,k,s_from,run_len", SHAPE_SETS + LAST_LANE_SETS + TURN_SETS)
def test_every_group_shape_matches_the_forms_it_replaced(t0, k, s_from, run_len, with_grad):
    """skr_selftest_step_chain on 2^20 hashed tuples: the advance the step kernel inlines == adam_grad_run (with the leading
    gradient update) / adam_zero_run (without), bits of p, m, v.  Every wavefront of ordinary magnitudes took the scaling-free
    form (the constructed number exactly), every control the general one"""
    from skrec import _hip
    n = 1 << 20
    out = (C.c_uint64 * 5)()
    _hip.check(_hip.lib().skr_selftest_step_chain(n, 1e-3, 0.9, 0.999, 1e-8, t0, k, s_from, run_len, with_grad, out, _hip.stream()))
    tested, bad, fast, ctl_general, ctl_fast = (int(x) for x in out)
    groups = n // 64
    controls = groups // 8                          # two wavefronts of every 16
    print("selftest_step_chain", t0, k, s_from, run_len, with_grad, tested, bad, fast, ctl_general, ctl_fast)
    assert tested == n and bad == 0
    assert fast == groups - controls
    assert ctl_general == controls and ctl_fast == 0


# ---- through FusedBlocks ------------------------------------------------------------------------------------------------
NU, NI, B = 300, 130, 6
ITEM_GAPS = 5          # named at steps 0, 1, 3, 6, 10, ...: naming distances 1, 2, 3, ... up to 2 G + 3, as far as a block holds them
ITEM_TWICE = 9         # named at the first and at the last step of every block: distance k - 1
ITEM_LATE = 11         # named once per block, at step min(2 G + 2, k - 1): from the second block on a zero-gradient run from 0
N_COUNTERS = 34
STEP_ROW = 0                                       # census: kernel
GRAD, RUN = 0, 1                                   # kind
REST, ORD, GENERAL = 0, 1, 3                       # class


def _gap_steps(k):
    """per block, the steps that name ITEM_GAPS: the distances 1 .. min(2 G + 3, k - 1) in order, a new block where the next one
    no longer fits.  Returns (three lists of steps, the distances placed)"""
    blocks, placed, pos = [[0]], [], 0
    for d in range(1, min(2 * G + 3, k - 1) + 1):
        if pos + d > k - 1:
            blocks.append([0])
            pos = 0
        pos += d
        blocks[-1].append(pos)
        placed.append(d)
    assert len(blocks) <= 3
    while len(blocks) < 3:
        blocks.append(list(blocks[0]))
    return blocks, placed


def test_the_schedule_holds_every_distance():
    """host arithmetic only"""
    for k in (5, 33, 64):
        blocks, placed = _gap_steps(k)
        assert placed == list(range(1, min(2 * G + 3, k - 1) + 1))
        got = sorted({b - a for steps in blocks for a, b in zip(steps, steps[1:])})
        assert got == placed and all(steps[-1] <= k - 1 for steps in blocks)
    assert _gap_steps(33)[1] == list(range(1, 2 * G + 4)) and _gap_steps(64)[1] == list(range(1, 2 * G + 4))


def _state(rng):
    """a model some way into training: lively rows and biases, so that every row takes the scaling-free forms"""
    n_par = (NU + NI) * 64 + NI
    p = (rng.standard_normal(n_par) * 0.05).astype(np.float32)
    g0 = (rng.standard_normal(n_par) * 0.01).astype(np.float32)
    g0 = np.where(np.abs(g0) < 1e-6, np.float32(1e-6), g0).astype(np.float32)
    v = (g0 * g0 * rng.uniform(0.5, 1.5, n_par) + 1e-7).astype(np.float32)
    return p, g0.copy(), v


def _batches(rng, k):
    """three blocks of k steps; rows distinct within a step (each float atomic then happens once: deterministic gradients).
    Returns the id columns and the number of item namings that have a run of two or more updates in front of them"""
    import torch
    special = (ITEM_GAPS, ITEM_TWICE, ITEM_LATE)
    pool = np.array([x for x in range(NI) if x not in special])
    gaps, _ = _gap_steps(k)
    late = min(2 * G + 2, k - 1)
    u = np.empty((3 * k, B), np.int64)
    ij = np.empty((3 * k, 2 * B), np.int64)
    long_runs = 0
    for q in range(3):
        for s in range(k):
            named = [ITEM_GAPS] * (s in gaps[q]) + [ITEM_TWICE] * (s in (0, k - 1)) + [ITEM_LATE] * (s == late)
            named = list(dict.fromkeys(named))
            u[q * k + s] = rng.permutation(NU)[:B]
            ij[q * k + s] = np.concatenate([named, rng.permutation(pool)[:2 * B - len(named)]]).astype(np.int64)
        long_runs += sum(b - a >= 2 for a, b in zip(gaps[q], gaps[q][1:])) + (k - 1 >= 2) + (q > 0 and late >= 2)
    return tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in (u, ij[:, :B], ij[:, B:])), long_runs


def _opt(state, t0, **kw):
    import torch
    from skrec.recommender.base import DenseAdam
    o = DenseAdam(torch.from_numpy(state[0].copy()).cuda(), lr=1e-2, **kw)
    o.m.copy_(torch.from_numpy(state[1]).cuda())
    o.v.copy_(torch.from_numpy(state[2]).cuda())
    o.t = t0
    return o


_dense_cache = {}


def _dense(k, t0):
    """the reference, computed once per case and shared by the two settings: skr_bpr_step + one dense skr_adam_step per batch"""
    import torch
    from skrec import _hip
    key = (k, t0)
    if key not in _dense_cache:
        L = _hip.lib()
        rng = np.random.default_rng(4100 + k + t0)
        state = _state(rng)
        (u, i, j), long_runs = _batches(rng, k)
        a = _opt(state, t0, track_touch=True)
        loss = torch.zeros(2, device="cuda")
        sl = lambda t: (t[:NU * 64].view(NU, 64), t[NU * 64:(NU + NI) * 64].view(NI, 64), t[(NU + NI) * 64:])  # noqa: E731
        (U, V, bias), (gU, gV, gb) = sl(a.flat), sl(a.grad)
        for s in range(3 * k):
            _hip.check(L.skr_bpr_step(_hip.ptr(U), _hip.ptr(V), _hip.ptr(bias), _hip.ptr(U), _hip.ptr(V), _hip.ptr(u[s]),
                                      _hip.ptr(i[s]), _hip.ptr(j[s]), B, 1.0, 1e-3, 1.0, _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(gb),
                                      _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(loss), _hip.ptr(a.touch), _hip.ptr(a.grad), _hip.stream()))
            a.step()
        torch.cuda.synchronize()
        _dense_cache[key] = (state, (u, i, j), long_runs, tuple(t.view(torch.int32).clone() for t in (a.flat, a.m, a.v)))
    return _dense_cache[key]


@pytest.fixture()
def census(monkeypatch):
    """switches the census on for the test (the library reads the variable again at every skr_fused_census call) and off after"""
    from skrec import _hip
    buf = (C.c_uint64 * N_COUNTERS)()

    def read(reset=1):
        _hip.check(_hip.lib().skr_fused_census(buf, N_COUNTERS, reset))
        return np.array(list(buf), dtype=np.int64)

    monkeypatch.setenv("SKR_FUSED_STATS", "1")
    read()
    yield read
    monkeypatch.setenv("SKR_FUSED_STATS", "0")
    read()


@pytest.mark.parametrize("pre", ["1", "0"])
@pytest.mark.parametrize("t0", [0, 16600, 40000])
@pytest.mark.parametrize("k", [5, 33, 64])
def test_fused_blocks_match_the_dense_optimiser(k, t0, pre, census, monkeypatch):
    """three k-step blocks of the one-launch step == the dense reference, bits of p, m, v.  One item is named at distances
    1, 2, ... 2 G + 3 (as far as a block of k steps holds them; k = 5 spreads 1 .. 4 over the three blocks), one at distance
    k - 1, one late in every block (a zero-gradient run from index 0 in the step kernel).  t0 = 16 600: the second bias
    correction turns 1.0f inside the first block (index 27 at k = 33 and 64).  pre = "0": the users' first namings catch up
    from index 0 themselves -- zero-gradient runs of every length.  The census must show every row evaluation of the step
    launches in the ordinary class, and at least the constructed runs"""
    import torch
    from skrec import _hip
    from skrec.recommender.fused import FusedBlocks
    monkeypatch.setenv("SKR_FUSED_PRE", pre)
    state, (u, i, j), long_runs, want = _dense(k, t0)
    c = _opt(state, t0)
    S = _hip.SKR_LOSS_SLOTS
    lc = torch.zeros((3 * k, S, 2), device="cuda")
    fb = FusedBlocks(c, 0, NU, NU + NI, 1e-3)
    census()
    fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), 3, k, B, lc.data_ptr(), 8 * S)
    c.end_blocks()
    torch.cuda.synchronize()
    cen = census()
    row = lambda kind, cls: int(cen[8 * STEP_ROW + 4 * kind + cls])  # noqa: E731
    print("pack census", k, t0, pre, long_runs, cen.tolist())
    assert c.t == t0 + 3 * k
    for name, got, w in zip("pmv", (c.flat, c.m, c.v), want):
        diff = int((got.view(torch.int32) != w).sum())
        assert diff == 0, f"{name}: {diff} elements differ"
    assert row(GRAD, GENERAL) == 0 and row(RUN, GENERAL) == 0 and row(RUN, REST) == 0
    assert row(GRAD, ORD) > 0 and row(RUN, ORD) >= long_runs
