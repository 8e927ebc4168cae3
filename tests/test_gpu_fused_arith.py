"""GPU suite: the gradient update of the fused BPR step's lazily advanced rows on the scaling-free forms against
the dense optimiser, bit for bit (int32 views of p, m and v), from a state with null, stale and special lanes, with the
census (SKR_FUSED_STATS=1, skr_fused_census) as the witness that the scaling-free form ran."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_COUNTERS = 34
STEP_ROW, STEP_BIAS, END, PRE = range(4)           # census: kernel
GRAD, RUN = 0, 1                                   # kind
REST, ORD, GENERAL = 0, 1, 3                       # class
END_PAIRED, END_SINGLE = 32, 33


def _counter(c, kernel, kind, cls):
    return int(c[8 * kernel + 4 * kind + cls])


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


@pytest.mark.parametrize("run_len", [1, 5])
@pytest.mark.parametrize("t0,tf", [(0, 0), (20000, 0), (16585, 0), (0, 1), (300, 1)])
def test_gradient_update_matches_the_dense_arithmetic(t0, tf, run_len):
    """skr_selftest_grad_math on 2^24 hashed tuples: the gradient update of the lazy rows == adam_elem / adam_elem_unit_bc2,
    bits of p, m, v; non-unit (t0 = 0), unit (t0 = 20 000, TF) and mixed (a block across step ~16 600) second bias
    corrections, torch's and TF's scalars; the gradient update alone (run_len = 1) and with four zero-gradient updates behind
    it in the same call (its quotient is then the first of the four side-by-side chains), against update by update.  Every
    wavefront of ordinary magnitudes took the scaling-free form (the constructed number exactly), every control -- two of
    every 16 wavefronts hold lanes outside the ordinary ranges -- the general one, with the same bits"""
    from skrec import _hip
    n = 1 << 24
    out = (C.c_uint64 * 5)()
    _hip.check(_hip.lib().skr_selftest_grad_math(n, 1e-3, 0.9, 0.999, 1e-8, t0, 32, tf, run_len, out, _hip.stream()))
    tested, bad, fast, ctl_general, ctl_fast = (int(x) for x in out)
    groups = n // 64
    controls = groups // 8                          # two wavefronts of every 16
    print("selftest_grad_math", t0, tf, run_len, tested, bad, fast, ctl_general, ctl_fast)
    assert tested == n and bad == 0
    assert fast == groups - controls
    assert ctl_general == controls and ctl_fast == 0


NU, NI, B = 192, 200, 32
N_PAR = (NU + NI) * 64 + NI
ITEM_NAN, ITEM_INF = 130, 131                       # bias lanes with a NaN p / v = +inf: no batch names these two items


def _preset(rng):
    """parameters and moments of a model some way into training, as float32 arrays [N_PAR]: lively user / item rows; the
    item biases one third NULL (m = v = +0, p = +0 or -0), one third STALE (moments decayed by 800 steps, p != 0), one third
    lively -- except the second bias block (items 64 .. 127), which is lively throughout, so that a bias block's gradient update
    can take the scaling-free form; and special lanes: m = -0, a NaN p beside null lanes, v = +inf, one item row with a denormal m"""
    p = (rng.standard_normal(N_PAR) * 0.05).astype(np.float32)
    g0 = (rng.standard_normal(N_PAR) * 0.01).astype(np.float32)
    m = g0.copy()
    v = (g0 * g0 * rng.uniform(0.5, 1.5, N_PAR) + 1e-7).astype(np.float32)
    bias0 = (NU + NI) * 64
    it = np.arange(NI)
    mixed = (it < 64) | (it >= 128)
    null, stale = bias0 + it[(it % 3 == 0) & mixed], bias0 + it[(it % 3 == 1) & mixed]
    m[null] = 0.0
    v[null] = 0.0
    p[null] = np.where((null // 3) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    d1, d2 = np.float32(1.0), np.float32(1.0)
    for _ in range(800):                            # the decays in float32, as the optimiser makes them
        d1 = np.float32(d1 + np.float32(0.1) * (np.float32(0.0) - d1))
        d2 = np.float32(d2 * np.float32(0.999))
    m[stale] = (m[stale] * d1).astype(np.float32)   # ~1e-39: below the ordinary range, some denormal
    v[stale] = (v[stale] * d2).astype(np.float32)
    p[stale] = np.where(np.abs(p[stale]) < 1e-3, np.float32(0.02), p[stale])
    for item in (6, 9, 42):                         # m = -0 (in no class until an update turns it into +0)
        m[bias0 + item] = np.float32(-0.0)
        v[bias0 + item] = 0.0
    p[bias0 + ITEM_NAN] = np.float32(np.nan)
    m[bias0 + ITEM_NAN] = 0.0
    v[bias0 + ITEM_NAN] = 0.0
    v[bias0 + ITEM_INF] = np.float32(np.inf)
    m[(NU + 7) * 64 + 3] = np.float32(1e-41)        # item row 7, lane 3: a denormal first moment
    return p, m, v


def _batches(rng, n_steps, name_null):
    """rows distinct inside a step (every float atomic happens once: deterministic gradients); the two special items unnamed.
    `name_null` False (the eps = 0 cases): the null items stay unnamed too.  With eps = 0 the DENSE optimiser turns their biases
    into NaN at the first step (-0 / 0); a batch that named one would carry the NaN through the scores into every row it
    touches, and from there on the test would compare the sign and payload bits that two different BPR kernels (skr_bpr_step
    here, the fused step there) give a NaN gradient -- nothing to do with the optimiser.  Unnamed, those lanes still take
    every update, in both optimisers, and are compared bit for bit like all others."""
    import torch
    items = np.array([x for x in range(NI) if x not in (ITEM_NAN, ITEM_INF) and (name_null or x % 3 != 0)])
    u = np.stack([rng.permutation(NU)[:B] for _ in range(n_steps)])
    ij = np.stack([rng.permutation(items)[:2 * B] for _ in range(n_steps)])
    return tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in (u, ij[:, :B], ij[:, B:]))


def _opt(state, t0, eps, **kw):
    import torch
    from skrec.recommender.base import DenseAdam
    o = DenseAdam(torch.from_numpy(state[0].copy()).cuda(), lr=1e-2, eps=eps, **kw)
    o.m.copy_(torch.from_numpy(state[1]).cuda())
    o.v.copy_(torch.from_numpy(state[2]).cuda())
    o.t = t0
    return o


def _bpr(opt, u, i, j, loss, touch):
    from skrec import _hip
    L = _hip.lib()
    sl = lambda t: (t[:NU * 64].view(NU, 64), t[NU * 64:(NU + NI) * 64].view(NI, 64), t[(NU + NI) * 64:])  # noqa: E731
    (U, V, bias), (gU, gV, gb) = sl(opt.flat), sl(opt.grad)
    _hip.check(L.skr_bpr_step(_hip.ptr(U), _hip.ptr(V), _hip.ptr(bias), _hip.ptr(U), _hip.ptr(V), _hip.ptr(u), _hip.ptr(i),
                              _hip.ptr(j), B, 1.0, 1e-3, 1.0, _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(gb), _hip.ptr(gU), _hip.ptr(gV),
                              _hip.ptr(loss), _hip.ptr(touch) if touch is not None else None,
                              _hip.ptr(opt.grad) if touch is not None else None, _hip.stream()))


_dense_cache = {}


def _dense(k, t0, eps):
    """the reference, computed once per case and shared: skr_bpr_step + one dense skr_adam_step per batch"""
    import torch
    key = (k, t0, eps)
    if key not in _dense_cache:
        rng = np.random.default_rng(7000 + k + t0)
        state = _preset(rng)
        u, i, j = _batches(rng, 3 * k, eps > 0)
        a = _opt(state, t0, eps, track_touch=True)
        loss = torch.zeros(2, device="cuda")
        for s in range(3 * k):
            _bpr(a, u[s], i[s], j[s], loss, a.touch)
            a.step()
        torch.cuda.synchronize()
        _dense_cache[key] = (state, (u, i, j), tuple(t.view(torch.int32).clone() for t in (a.flat, a.m, a.v)))
    return _dense_cache[key]


def _same_bits(opt, want):
    import torch
    for name, got, w in zip("pmv", (opt.flat, opt.m, opt.v), want):
        diff = int((got.view(torch.int32) != w).sum())
        assert diff == 0, f"{name}: {diff} elements differ"


CASES = [(k, t0, eps) for k in (3, 8) for t0 in (0, 2000, 16596) for eps in (1e-8, 0.0)]


@pytest.mark.parametrize("k,t0,eps", CASES)
def test_fused_step_with_null_stale_and_special_lanes(k, t0, eps, census):
    """three k-step blocks of the one-launch step from a preset state == the dense reference, bits of p, m, v.  nI = 200: four
    bias blocks, the last with 8 live lanes and lanes past the end of the buffer.  The census must show gradient updates of
    user / item rows on the scaling-free form, in the step launches and in the end launch"""
    import torch
    from skrec import _hip
    from skrec.recommender.fused import FusedBlocks
    state, (u, i, j), want = _dense(k, t0, eps)
    c = _opt(state, t0, eps)
    S = _hip.SKR_LOSS_SLOTS
    lc = torch.zeros((3 * k, S, 2), device="cuda")
    fb = FusedBlocks(c, 0, NU, NU + NI, 1e-3)
    census()
    fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), 3, k, B, lc.data_ptr(), 8 * S)
    c.end_blocks()
    torch.cuda.synchronize()
    cen = census()
    print("fused census", k, t0, eps, cen.tolist())
    assert c.t == t0 + 3 * k
    _same_bits(c, want)
    assert float(fb.work[:, 6 * fb.cap * 64:].abs().max()) == 0.0          # every gradient was consumed
    assert _counter(cen, STEP_ROW, GRAD, ORD) > 0 and _counter(cen, END, GRAD, ORD) > 0
    assert _counter(cen, STEP_BIAS, GRAD, ORD) > 0            # the all-lively bias block
    assert _counter(cen, STEP_BIAS, GRAD, GENERAL) > 0        # ... and the blocks with null / stale lanes
    assert _counter(cen, STEP_ROW, RUN, ORD) > 0              # runs behind a gradient update: its quotient as the first chain


@pytest.mark.parametrize("k,t0", [(8, 0), (8, 16596), (3, 2000)])
def test_end_launch_pairs_two_slots_per_wavefront(k, t0, census):
    """skr_bpr_fused_end alone on a hand-made workspace of nine slots (odd: a lone last slot) == the dense optimiser, bits of
    p, m, v of the slots' rows.  Pairs of neighbouring slots whose last namings lie 0, 1 and k - 1 steps apart (advanced
    together on the packed pair form), a pair with one row that fails the ordinary test (a stalled denormal m: both run one by
    one); (8, 16 596) straddles the step where the second bias correction turns 1.0f.  The census must show both forms"""
    import torch
    from skrec import _hip
    from skrec.recommender.base import DenseAdam
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(900 + k)
    rows, cap, lr = 16, 12, 1e-2
    n = rows * 64
    h = k // 2
    slot_row = [3, 5, 0, 9, 12, 1, 7, 14, 10]
    last = [h, h, h, min(h + 1, k - 1), 0, k - 1, 0, 1 % k, k - 1]
    nn = [1, 2, 3, 4, 5, 1, 2, 3, 4]
    p0 = (rng.standard_normal(n) * 0.05).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v0 = (m0 * m0 * rng.uniform(0.5, 1.5, n) + 1e-7).astype(np.float32)
    m0[7 * 64 + 11] = np.float32(1e-41)                     # slot 6 (row 7, last = 0): this lane gets g = 0 and stays denormal
    a = DenseAdam(torch.from_numpy(p0.copy()).cuda(), lr=lr)
    a.m.copy_(torch.from_numpy(m0).cuda())
    a.v.copy_(torch.from_numpy(v0).cuda())
    a.t = t0
    work = torch.zeros(9 * cap * 64, device="cuda")
    plane = cap * 64
    for s in range(k):
        for slot, (row, ls, c) in enumerate(zip(slot_row, last, nn)):
            if ls != s:
                continue
            g = torch.from_numpy((rng.standard_normal(64) * 0.01).astype(np.float32)).cuda()
            if slot == 6:
                g[11] = 0.0
            sl = slice(row * 64, row * 64 + 64)
            o = ((c & 1) * cap + slot) * 64
            work[o:o + 64] = a.flat[sl]
            work[2 * plane + o:2 * plane + o + 64] = a.m[sl]
            work[4 * plane + o:4 * plane + o + 64] = a.v[sl]
            og = 6 * plane + (((c + 2) % 3) * cap + slot) * 64
            work[og:og + 64] = g
            a.grad[sl] = g
        a.step()
    sb = torch.tensor(slot_row, dtype=torch.int32, device="cuda")
    sf = torch.tensor([c | (ls << 8) | (ls << 16) for c, ls in zip(nn, last)], dtype=torch.int32, device="cuda")
    ns = torch.tensor([len(slot_row)], dtype=torch.int32, device="cuda")
    P, M, V = (torch.full((n,), 7.0, device="cuda") for _ in range(3))
    census()
    _hip.check(L.skr_bpr_fused_end(P.data_ptr(), M.data_ptr(), V.data_ptr(), n, work.data_ptr(), cap, sb.data_ptr(), sf.data_ptr(),
                                   ns.data_ptr(), lr, 0.9, 0.999, 1e-8, t0, k, None, 0, 0, st))
    torch.cuda.synchronize()
    cen = census()
    print("end census", k, t0, cen.tolist())
    idx = torch.tensor(slot_row, device="cuda")
    for name, got, want in zip("pmv", (P, M, V), (a.flat, a.m, a.v)):
        gb, wb = got.view(rows, 64)[idx].view(torch.int32), want.view(rows, 64)[idx].view(torch.int32)
        assert int((gb != wb).sum()) == 0, f"{name}: {int((gb != wb).sum())} elements differ"
    untouched = torch.ones(rows, dtype=torch.bool, device="cuda")
    untouched[idx] = False
    assert bool((P.view(rows, 64)[untouched] == 7.0).all())                # rows without a slot are not written
    assert float(work[6 * plane:].abs().max()) == 0.0                       # the gradient buffers are left zero
    assert int(cen[END_PAIRED]) == 6 and int(cen[END_SINGLE]) == 3
