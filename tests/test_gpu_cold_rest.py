"""GPU suite: the cold Adam pass with a state word per row (skr_adam_block_cold_rest, DenseAdam.launch_cold).

A pass records per cold row what it found out -- QUIET (at rest by the eps form of the test, which stays true while nothing
but zero-gradient updates reach the row) or ZERO (all moments +0: nothing changes) -- and the next pass trusts the record
instead of reading the row again.  Reference throughout: skr_adam_block_cold (itself pinned to k dense skr_adam_step
launches by test_gpu_train.py) on a copy of the same buffers; every comparison is bit for bit on p, m and v, after every pass.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

B1, B2 = 0.9, 0.999
# the launch of skr_adam_block_cold (adam.hip, adam_block_cold_impl): 256 CUs x 5 workgroups (6 for k >= 32) of 4 wavefronts,
# 4 rows per wavefront and round.  Just over 4 x 6144 rows: the outer loop runs twice, the second round ragged, at both widths
BIG_ROWS = 4 * 256 * 6 * 4 + 37


def _bits(t):
    import torch
    return t.view(torch.int32)


def _same(got, want):
    import torch
    return all(torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _aged(rng, rows, age=None):
    """[rows, 64] p, m, v as `age[r]` steps without a gradient leave them (the recipe of test_gpu_train._aged_rows): lively,
    ordinary, at rest by the v form only (ages ~150-260), by the eps form (beyond), denormal, zero"""
    if age is None:
        age = rng.integers(0, 3000, rows)
        sweep = min(400, rows // 2)
        age[:sweep] = np.arange(sweep) * 5
    age = np.asarray(age)
    m = (rng.standard_normal((rows, 64)) * 1e-3 * np.exp(np.log(0.9) * age)[:, None]).astype(np.float32)
    v = (rng.random((rows, 64)) * 1e-6 * np.exp(np.log(0.999) * age)[:, None]).astype(np.float32)
    p = (rng.standard_normal((rows, 64)) * 0.05).astype(np.float32)
    return p, m, v


def _dev(x, n):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1)[:n].copy()).cuda()


def _cold_ref(st3, n, lr, b1, b2, eps, t0, k, tag, hot):
    from skrec import _hip
    p, m, v = st3
    _hip.check(_hip.lib().skr_adam_block_cold(_hip.ptr(p), _hip.ptr(m), _hip.ptr(v), n, lr, b1, b2, eps, t0, k, _hip.ptr(tag), hot,
                                              _hip.stream()))


def _cold_rest(st3, n, lr, b1, b2, eps, t0, k, tag, hot, words, pass_id):
    from skrec import _hip
    p, m, v = st3
    _hip.check(_hip.lib().skr_adam_block_cold_rest(_hip.ptr(p), _hip.ptr(m), _hip.ptr(v), n, lr, b1, b2, eps, t0, k, _hip.ptr(tag),
                                                   hot, _hip.ptr(words), pass_id, _hip.stream()))


def _trusted(reset=1):
    """(rows trusted as quiet, rows trusted as zero) since the last reset; re-reads SKR_COLD_STATS"""
    from skrec import _hip
    c = (C.c_uint64 * 2)()
    _hip.check(_hip.lib().skr_cold_rest_census(c, reset))
    return int(c[0]), int(c[1])


@pytest.fixture()
def census(monkeypatch):
    from skrec import _hip
    _hip.require_gpu()
    monkeypatch.setenv("SKR_COLD_STATS", "1")
    _trusted()                       # switches the census on and clears it
    yield _trusted
    monkeypatch.delenv("SKR_COLD_STATS")
    _trusted()                       # ... and off again for the tests behind this one


def _words(n):
    import torch
    return torch.zeros((n + 63) // 64, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("t0", [0, 16650])
@pytest.mark.parametrize("k", [1, 7, 32, 64])
@pytest.mark.parametrize("rows,tail", [(BIG_ROWS, 17), (1, 0), (2, 5), (3, 63), (5, 0), (0, 40)])
def test_chain_of_passes_is_bit_identical(rows, tail, k, t0, census):
    """six consecutive passes (pass_id counting up by one) with a fresh random tenth of the rows tagged hot each time; a hot
    row gets fresh lively values behind the pass, as a step would leave them.  p, m and v equal the reference's after every
    pass; in the large buffer rows ARE trusted, both ways"""
    import torch
    rng = np.random.default_rng(1000 * k + t0 + rows)
    n = rows * 64 + tail
    R = rows + (1 if tail else 0)
    p, m, v = _aged(rng, R)
    if rows > 100:
        m[100:140] = 0.0
        v[100:140] = 0.0             # never touched
    ref = [_dev(x, n) for x in (p, m, v)]
    got = [x.clone() for x in ref]
    tag, words = _words(n), _words(n)
    lr, eps = 1e-3, 1e-8
    gen = torch.Generator(device="cuda").manual_seed(k + t0)
    for c in range(6):
        hot = torch.from_numpy(rng.random(R) < 0.1).cuda()
        tag[hot] = c + 1
        _cold_ref(ref, n, lr, B1, B2, eps, t0 + c * k, k, tag, c + 1)
        _cold_rest(got, n, lr, B1, B2, eps, t0 + c * k, k, tag, c + 1, words, c + 1)
        assert _same(got, ref), f"pass {c}"
        sel = hot.repeat_interleave(64)[:n]
        fresh = (torch.randn(n, generator=gen, device="cuda") * 0.05, torch.randn(n, generator=gen, device="cuda") * 1e-3,
                 torch.rand(n, generator=gen, device="cuda") * 1e-6)
        for x_ref, x_got, f in zip(ref, got, fresh):
            x_ref[sel] = f[sel]
            x_got[sel] = f[sel]
    quiet, zero = census()
    if rows > 100:
        assert quiet > rows and zero > 40      # (~0.8 of the rows beyond age ~260 on each of 5 passes; the 40 zero rows)
    if tail:
        assert int(words[rows]) == 0           # the tail has no word


def test_edge_rows_in_one_buffer(census):
    """all-zero moments under p = +0, -0, +-inf, denormal, below 2^-60 (state ZERO) and NaN (never); m = -0 or v = -0 (not ZERO);
    one lively lane among 63 quiet ones; ordinary rows between them"""
    rng = np.random.default_rng(5)
    rows = 24
    p, m, v = _aged(rng, rows, age=rng.integers(0, 50, rows))
    for r, val in enumerate([0.0, -0.0, np.inf, -np.inf, 1e-42, 1e-20, np.nan]):
        p[r], m[r], v[r] = np.float32(val), 0.0, 0.0
    p[7, 13], m[7], v[7] = np.nan, 0.0, 0.0            # one NaN lane
    m[8], v[8] = -0.0, 0.0                             # quiet, then (m has become +0) zero
    m[9], v[9] = 0.0, -0.0                             # v = -0 fails the sign test: never flagged
    m[10], v[10] = 0.0, 0.0
    m[10, 41] = -0.0
    m[11] = np.float32(1e-30) * rng.standard_normal(64).astype(np.float32)
    m[11, 5] = 1e-3                                    # one lively lane
    m[12] = np.float32(1e-30) * rng.standard_normal(64).astype(np.float32)   # quiet
    n = rows * 64
    ref = [_dev(x, n) for x in (p, m, v)]
    got = [x.clone() for x in ref]
    tag, words = _words(n), _words(n)
    trusted = []
    for c in range(4):
        _cold_ref(ref, n, 1e-3, B1, B2, 1e-8, 100 + 8 * c, 8, tag, 1)
        _cold_rest(got, n, 1e-3, B1, B2, 1e-8, 100 + 8 * c, 8, tag, 1, words, c + 1)
        assert _same(got, ref), f"pass {c}"
        trusted.append(census())
    state = (words.cpu().numpy() & 3).tolist()
    assert trusted[0] == (0, 0)
    # the first pass flags rows 0-5 ZERO (not the NaN rows, not the rows with a -0 moment) and rows 8, 10, 12 QUIET; it also
    # turns the -0 moments into +0 (m: -0 + c1 * (0 - -0) = +0; v: -0 * b2 + (c2 * 0) * 0 = +0), so the second pass finds rows
    # 8 and 10 (trusted quiet) and row 9 (examined) all-zero and flags them ZERO for the third
    assert trusted[1] == (3, 6)
    assert trusted[2] == (1, 9)
    assert state[:6] == [2] * 6 and state[6] == 0 and state[7] == 0
    assert state[8] == 2 and state[9] == 2 and state[10] == 2
    assert state[11] == 0 and state[12] == 1 and state[13:] == [0] * (rows - 13)


@pytest.mark.parametrize("lr,b1,b2,eps", [(1e-3, B1, B2, 0.0), (0.0, B1, B2, 1e-8), (1e-3, 1.5, B2, 1e-8), (1e-3, 0.0, B2, 1e-8),
                                          (1e-3, B1, 0.0, 1e-8)])
def test_no_state_without_thresholds(lr, b1, b2, eps, census):
    """eps = 0, lr = 0, a beta outside (0, 1): the at-rest thresholds are off, no row is ever trusted, results are equal"""
    rng = np.random.default_rng(11)
    rows = 300
    p, m, v = _aged(rng, rows)
    m[200:260], v[200:260] = 0.0, 0.0
    n = rows * 64 + 9
    ref = [_dev(x, n) for x in (np.vstack([p, p[:1]]), np.vstack([m, m[:1]]), np.vstack([v, v[:1]]))]
    got = [x.clone() for x in ref]
    tag, words = _words(n), _words(n)
    for c in range(3):
        _cold_ref(ref, n, lr, b1, b2, eps, 40 + 7 * c, 7, tag, 1)
        _cold_rest(got, n, lr, b1, b2, eps, 40 + 7 * c, 7, tag, 1, words, c + 1)
        assert _same(got, ref), f"pass {c}"
    assert census() == (0, 0)
    assert int((words[:rows] & 3).abs().sum()) == 0


def test_broken_chain_reads_the_rows_again(census):
    """a flagged row is poked between two passes: with pass_id + 2 the pass trusts nothing and gives the reference's result;
    the rows' words carry on from there"""
    rng = np.random.default_rng(13)
    rows = 64
    p, m, v = _aged(rng, rows, age=np.full(rows, 1500))
    m[:16], v[:16] = 0.0, 0.0
    n = rows * 64
    ref = [_dev(x, n) for x in (p, m, v)]
    got = [x.clone() for x in ref]
    tag, words = _words(n), _words(n)
    for c in range(2):
        _cold_ref(ref, n, 1e-3, B1, B2, 1e-8, 8 * c, 8, tag, 1)
        _cold_rest(got, n, 1e-3, B1, B2, 1e-8, 8 * c, 8, tag, 1, words, c + 1)
    assert _same(got, ref)
    state = (words.cpu().numpy() & 3)
    assert (state[:16] == 2).all() and (state[16:] == 1).all()
    assert census() == (rows - 16, 16)
    for x in (ref, got):                               # a zero row and a quiet row become lively
        x[1][3 * 64:4 * 64] = 1e-3
        x[1][40 * 64:41 * 64] = -2e-3
        x[2][3 * 64:4 * 64] = 1e-6
    _cold_ref(ref, n, 1e-3, B1, B2, 1e-8, 16, 8, tag, 1)
    _cold_rest(got, n, 1e-3, B1, B2, 1e-8, 16, 8, tag, 1, words, 4)
    assert _same(got, ref)
    assert census() == (0, 0)
    assert not _same([got[0]], [_dev(p, n)])           # (the poked rows did move: the comparison above had something to see)
    _cold_ref(ref, n, 1e-3, B1, B2, 1e-8, 24, 8, tag, 1)
    _cold_rest(got, n, 1e-3, B1, B2, 1e-8, 24, 8, tag, 1, words, 5)
    assert _same(got, ref)
    assert census() == (rows - 16 - 1, 15)


def test_all_zero_moments_are_trusted_from_the_second_pass(census):
    """a fresh model: from the second pass on every cold row is trusted as zero (and nothing is read)"""
    import torch
    rng = np.random.default_rng(17)
    rows = 1000
    n = rows * 64 + 21
    p = (rng.standard_normal((rows + 1, 64)) * 0.05).astype(np.float32)
    p[500:600] = 0.0                                   # bias-like rows
    z = np.zeros_like(p)
    ref = [_dev(x, n) for x in (p, z, z)]
    got = [x.clone() for x in ref]
    tag, words = _words(n), _words(n)
    tag[torch.from_numpy(rng.random(rows + 1) < 0.2).cuda()] = 1
    n_cold = int((tag[:rows] != 1).sum())
    for c in range(3):
        _cold_ref(ref, n, 1e-3, B1, B2, 1e-8, 32 * c, 32, tag, 1)
        _cold_rest(got, n, 1e-3, B1, B2, 1e-8, 32 * c, 32, tag, 1, words, c + 1)
        assert _same(got, ref)
        assert census() == ((0, 0) if c == 0 else (0, n_cold))


def _opt_pass(opt, tag, serial, k):
    """one cold pass through DenseAdam, as FusedBlocks issues it"""
    import torch
    opt._ensure_side()
    torch.cuda.synchronize()
    opt.launch_cold(tag, serial, k)
    opt.end_blocks()
    opt.t += k
    torch.cuda.synchronize()


def _fresh_like(opt):
    from skrec.recommender.base import DenseAdam
    f = DenseAdam(opt.flat.clone(), lr=opt.lr, betas=opt.betas, eps=opt.eps)
    f.m.copy_(opt.m), f.v.copy_(opt.v)
    f.t = opt.t
    return f


@pytest.mark.parametrize("what", ["kept", "lr", "step", "t", "eps", "invalidate"])
def test_dense_adam_keeps_and_breaks_the_chain(what, census):
    """DenseAdam counts its passes up by one while nothing but blocked steps happen between them and by two after a changed
    lr or eps, a dense step() or a jump of t (or invalidate_rest()); after each, the next pass equals a fresh optimiser's"""
    import torch
    from skrec.recommender.base import DenseAdam
    rng = np.random.default_rng(19)
    rows = 700
    p, m, v = _aged(rng, rows)
    m[600:650], v[600:650] = 0.0, 0.0
    n = rows * 64 + 3
    opt = DenseAdam(_dev(np.vstack([p, p[:1]]), n), lr=1e-3)
    opt.m.copy_(_dev(np.vstack([m, m[:1]]), n)), opt.v.copy_(_dev(np.vstack([v, v[:1]]), n))
    opt.t = 5000
    tag = _words(n)
    tag[::9] = 1
    _opt_pass(opt, tag, 1, 8)
    _opt_pass(opt, tag, 1, 8)
    first = opt._rest_pass
    assert census()[0] > 100 and opt._rest_pass == first
    if what == "lr":
        opt.lr = 1.0                                   # no row is at rest any more
    elif what == "eps":
        opt.eps = 1e-30
    elif what == "step":
        opt.grad.copy_(_dev(np.vstack([p, p[:1]]), n))
        opt.step()
    elif what == "t":
        opt.t = 0
    elif what == "invalidate":
        opt.m[601 * 64:602 * 64] = 1e-2
        opt.invalidate_rest()
    want = _fresh_like(opt)
    _opt_pass(opt, tag, 1, 8)
    _opt_pass(want, tag, 1, 8)
    assert _same([opt.flat, opt.m, opt.v], [want.flat, want.m, want.v])
    quiet, zero = census()
    if what == "kept":
        assert opt._rest_pass == first + 1 and quiet > 100 and zero > 30
    else:
        assert opt._rest_pass == first + 2 and (quiet, zero) == (0, 0)
    # the chain picks up again behind the break
    want = _fresh_like(opt)
    _opt_pass(opt, tag, 1, 32)
    _opt_pass(want, tag, 1, 32)
    assert _same([opt.flat, opt.m, opt.v], [want.flat, want.m, want.v])
    assert opt._rest_pass == first + (2 if what == "kept" else 3)


@pytest.mark.parametrize("aged", [False, True])
@pytest.mark.parametrize("k", [8, 32])
def test_fused_blocks_with_and_without_state_words(k, aged, monkeypatch):
    """three fused BPR blocks (FusedBlocks -> DenseAdam.launch_cold) with SKR_COLD_REST on and off: flat, m and v bit-equal"""
    import torch
    from skrec import _hip
    from skrec.recommender.base import DenseAdam
    from skrec.recommender.fused import FusedBlocks
    rng = np.random.default_rng(23 + k)
    # (the library reads SKR_COLD_REST once, at its first pass without words: make that pass here, before the variable is set,
    #  so that this test leaves the process as it found it whichever test runs first)
    one = [_dev(np.zeros(64, np.float32), 64) for _ in range(3)]
    _cold_ref(one, 64, 1e-3, B1, B2, 1e-8, 0, 1, _words(64), 1)
    nU, nI, b, n_blocks = 400, 300, 64, 3
    n_par = (nU + nI) * 64 + nI
    init = _dev((rng.standard_normal(n_par) * 0.05).astype(np.float32), n_par)
    # rows distinct within a step (each float atomic of a gradient then happens once: a run is deterministic); three quarters
    # of the users are never named
    u = np.stack([rng.permutation(nU // 4)[:b] for _ in range(n_blocks * k)])
    ij = np.stack([rng.permutation(nI)[:2 * b] for _ in range(n_blocks * k)])
    i, j = ij[:, :b], ij[:, b:]
    u, i, j = (torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in (u, i, j))
    _, m0, v0 = _aged(rng, nU + nI + (nI + 63) // 64)
    S = _hip.SKR_LOSS_SLOTS
    out = []
    for rest in ("1", "0"):
        monkeypatch.setenv("SKR_COLD_REST", rest)
        c = DenseAdam(init.clone(), lr=1e-2)
        if aged:
            c.m.copy_(_dev(m0, n_par)), c.v.copy_(_dev(v0, n_par))
            c.t = 700
        lc = torch.zeros((n_blocks * k, S, 2), device="cuda")
        fb = FusedBlocks(c, 0, nU, nU + nI, 1e-3)
        fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), n_blocks, k, b, lc.data_ptr(), 8 * S)
        c.end_blocks()
        torch.cuda.synchronize()
        assert (c._rest_pass > 0) == (rest == "1")
        out.append((c.flat, c.m, c.v))
    differ = [int((_bits(a) != _bits(b_)).sum()) for a, b_ in zip(out[0], out[1])]
    assert differ == [0, 0, 0]
