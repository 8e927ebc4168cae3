"""GPU parity of csrc/train.hip where tests/test_gpu_train.py does not reach: the BPR batch behind all four entry points (wide rows,
spread loss slots, grad_scale, the capped grid, saturated and tied scores, every table mode, user sharding, the touch bytes block by
block), the gradient exchange (pack, both unpacks, the fallback beyond 16 ranks), the row helpers at the lengths where their loops
loop, LayerGCN's refinements at 128 / 192 / 256 columns with clamped norms, and both sparse products on 64-column slices of wide
tables.

Every numeric comparison is with a plain numpy float64 restatement written out here, computed from the same float32 inputs -- not
oracle.bpr_batch, not another kernel.  Every output buffer starts dirty: SENT where the kernel must overwrite, known values where it
must add; what the kernel must not touch (guard words behind every buffer, the other 64-column slices of wide tables, rows outside
an id list) is compared bit for bit.

The bound of a sum of k fp32 addends, used for the BPR gradients and words: tol = (k + 16) 2^-24 mass, mass = the sum of the
addends' magnitudes plus, per triple, 1/4 loss_scale grad_scale X_b |factor| -- what an error of the score x (relative to
X_b = sum|p q_i| + sum|p q_j| + |b_i| + |b_j|, the magnitudes its dot products add) does to an addend, the slope of the sigmoid
being at most 1/4.  It holds for any order of the additions, so the float atomics are covered; 16 covers the roundings inside one
addend (the wave reduction's 6 levels, the products, expf / log1pf).  Checked on the CPU: the fp32 oracle (oracle.bpr_batch, which
shares no code with the reference here) stays inside it with room -- its worst element is at 0.24 of the bound (n = 16389 on
37 x 23 rows), 0.13 at k ~ 450, its words below 0.002 of theirs."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gpu_utils import dev, to_dev
from skrec import _hip

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

U24 = 2.0 ** -24
SENT = np.float32(-1.2345678e9)
f32, f64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _at(t, off_floats):
    """address of float `off_floats` of a float32 device tensor"""
    return t.data_ptr() + 4 * int(off_floats)


# ------------------------------------------------------------------------------------------------
# 1. the BPR batch
# ------------------------------------------------------------------------------------------------
def _tables(rng, nU, nI, dim, mode, scale=0.3):
    """mode: same | split | alias_in (RP is P, RQ is Q, the regulariser's gradient buffers apart) | no_gb | no_bias"""
    r = lambda *s: (scale * rng.standard_normal(s)).astype(f32)  # noqa: E731
    c = dict(P=r(nU, dim), Q=r(nI, dim), bias=None if mode == "no_bias" else r(nI), g_split=mode in ("split", "alias_in"),
             gb=mode not in ("no_bias", "no_gb"))
    c["RP"], c["RQ"] = (r(nU, dim), r(nI, dim)) if mode == "split" else (c["P"], c["Q"])
    return c


def _bpr_ref(c, u, i, j, ls, reg, rscale, gs):
    """float64 restatement of one BPR batch: per triple x = p q_i - p q_j + b_i - b_j, l = logaddexp(0, -x),
    s = exp(-logaddexp(0, x)), c = -s loss_scale grad_scale; -> {buffer: [sum of addends, mass, addends per element]} and
    (value, mass) of the loss word (loss_scale sum l: no grad_scale) and of the L2 word (1/2 sum of squares of the regulariser
    rows and bias words).  The loss word's mass takes the slope of l in x, s <= 1, where the gradients' takes 1/4."""
    ls, reg, rscale, gs = (f64(f32(v)) for v in (ls, reg, rscale, gs))
    P, Q, RP, RQ = (c[k].astype(f64) for k in ("P", "Q", "RP", "RQ"))
    pu, qi, qj = P[u], Q[i], Q[j]
    x = (pu * qi).sum(1) - (pu * qj).sum(1)
    X = np.abs(pu * qi).sum(1) + np.abs(pu * qj).sum(1)
    if c["bias"] is not None:
        b = c["bias"].astype(f64)
        bi, bj = b[i], b[j]
        x = x + bi - bj
        X = X + np.abs(bi) + np.abs(bj)
    l = np.logaddexp(0.0, -x)
    cf = -np.exp(-np.logaddexp(0.0, x)) * ls * gs
    slack = np.abs(cf) + 0.25 * ls * gs * X                  # |c_b| + what an error of x does to c_b
    rs = reg * rscale
    acc = {}
    for name, like in (("gP", P), ("gQ", Q), ("gRP", P), ("gRQ", Q)):
        if name in ("gP", "gQ") or c["g_split"]:
            acc[name] = [np.zeros(like.shape), np.zeros(like.shape), np.zeros(like.shape, np.int64)]
    if c["gb"]:
        acc["gb"] = [np.zeros(len(c["bias"])), np.zeros(len(c["bias"])), np.zeros(len(c["bias"]), np.int64)]

    def add(name, rows, val, mag):
        d, m, k = acc[name]
        np.add.at(d, rows, val)
        np.add.at(m, rows, mag)
        np.add.at(k, rows, 1)
    cc, sk = cf[:, None], slack[:, None]
    same = c["RP"] is c["P"] and c["RQ"] is c["Q"] and not c["g_split"]
    if same:        # one addend per row: both parts of the gradient
        add("gP", u, cc * (qi - qj) + rs * pu, sk * np.abs(qi - qj) + rs * np.abs(pu))
        add("gQ", i, cc * pu + rs * qi, sk * np.abs(pu) + rs * np.abs(qi))
        add("gQ", j, -cc * pu + rs * qj, sk * np.abs(pu) + rs * np.abs(qj))
        ru, ri, rj = pu, qi, qj
    else:
        add("gP", u, cc * (qi - qj), sk * np.abs(qi - qj))
        add("gQ", i, cc * pu, sk * np.abs(pu))
        add("gQ", j, -cc * pu, sk * np.abs(pu))
        ru, ri, rj = RP[u], RQ[i], RQ[j]
        if rs != 0.0:
            tP, tQ = ("gRP", "gRQ") if c["g_split"] else ("gP", "gQ")
            add(tP, u, rs * ru, rs * np.abs(ru))
            add(tQ, i, rs * ri, rs * np.abs(ri))
            add(tQ, j, rs * rj, rs * np.abs(rj))
    sq = (ru ** 2).sum(1) + (ri ** 2).sum(1) + (rj ** 2).sum(1)
    if c["bias"] is not None:
        sq = sq + bi ** 2 + bj ** 2
        if c["gb"]:
            add("gb", i, cf + rs * bi, slack + rs * np.abs(bi))
            add("gb", j, -cf + rs * bj, slack + rs * np.abs(bj))
    return acc, (ls * l.sum(), ls * (l + X).sum()), (0.5 * sq.sum(), 0.5 * sq.sum()), x


def _bpr(entry, c, u, i, j, ls, reg, rscale, gs=1.0, dim=64, slots=1, world=1, rank=0, seed=0, zero_loss=False, n=None):
    """One launch of skr_bpr_<entry> on dirty buffers, compared with _bpr_ref.  All gradient buffers lie in one flat buffer
    [gP | gQ | gb | gRP | gRQ | guard] (gb padded to a whole block) with touch bytes over it, a tenth of them preset to the sticky 2:
      - an element that receives k > 0 addends is within (k + 16) 2^-24 (mass + |its start value|) of start + the float64 sum;
      - every other float of the buffer, guards and padding included, keeps its bits;
      - the touch bytes are 1 in exactly the blocks that hold an element with k > 0, 2 where they were 2, 0 elsewhere;
      - the loss and L2 words (their slots added up in float64) are within the same bound with k = the triples the launch owns --
        a bound that only exposes a lost triple while k is about 1000 or less: the small cases carry that; the guard words
        behind them keep their bits.
    world > 1: c holds the rank's LOCAL user tables (row u // world for the users u % world == rank), the batch is global."""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(1000 + seed)
    n = len(u) if n is None else n
    own = (u[:n] % world == rank) if world > 1 else np.ones(n, bool)
    acc, (loss, m_loss), (l2, m_l2), x = _bpr_ref(c, (u[:n][own] // world), i[:n][own], j[:n][own], ls, reg, rscale, gs)
    k_own = int(own.sum())
    layout, off = {}, 0
    for name in ("gP", "gQ", "gb", "gRP", "gRQ"):
        if name in acc:
            layout[name] = (off, acc[name][0].size)
            off += -(-acc[name][0].size // 64) * 64
    total = off + 128
    G0 = (0.05 * rng.standard_normal(total)).astype(f32)
    D, M, K = np.zeros(total), np.zeros(total), np.zeros(total, np.int64)
    for name, (o, sz) in layout.items():
        D[o:o + sz], M[o:o + sz], K[o:o + sz] = (a.reshape(-1) for a in acc[name])
    nb = (total + 63) // 64
    T0 = np.where(rng.random(nb + 2) < 0.1, 2, 0).astype(np.uint8)
    L0 = np.zeros(2 * slots + 2, f32) if zero_loss else (0.5 * rng.standard_normal(2 * slots + 2)).astype(f32)
    G, T, dl = to_dev(G0), to_dev(T0), to_dev(L0)
    up = {}

    def d(a):
        if a is None:
            return None
        if id(a) not in up:
            up[id(a)] = to_dev(a)
        return up[id(a)]
    ins = [d(c[k]) for k in ("P", "Q", "bias", "RP", "RQ")] + [d(np.ascontiguousarray(a, np.int32)) for a in (u, i, j)]
    before = [t.clone() for t in ins if t is not None]
    g = {name: _at(G, o) for name, (o, _) in layout.items()}
    grads = [g["gP"], g["gQ"], g.get("gb"), g.get("gRP", g["gP"]), g.get("gRQ", g["gQ"]), _hip.ptr(dl)]
    head = [_hip.ptr(t) for t in ins] + [n]
    tb = [_hip.ptr(T), _hip.ptr(G)]
    if entry == "step":
        assert (dim, slots, world, gs) == (64, 1, 1, 1.0)
        rc = L.skr_bpr_step(*head, ls, reg, rscale, *grads, *tb, st)
    elif entry == "spread":
        assert (dim, slots, world, gs) == (64, _hip.SKR_LOSS_SLOTS, 1, 1.0)
        rc = L.skr_bpr_step_spread(*head, ls, reg, rscale, *grads, *tb, st)
    elif entry == "dim":
        assert world == 1
        rc = L.skr_bpr_step_dim(*head, dim, ls, reg, rscale, *grads, slots, *tb, gs, st)
    else:
        assert entry == "sharded" and (dim, slots) == (64, 1)
        rc = L.skr_bpr_step_sharded(*head, ls, reg, rscale, *grads, *tb, world, rank, gs, st)
    _hip.check(rc)
    got, touch, words = _host(G), _host(T), _host(dl)
    for t, t0 in zip([t for t in ins if t is not None], before):
        assert torch.equal(t, t0)                                          # the inputs are only read
    hit = K > 0
    assert np.array_equal(_bits(got)[~hit], _bits(G0)[~hit]), "a float outside the batch's rows changed"
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(f64) - (G0.astype(f64) + D))[hit]
    tol = ((K + 16) * U24 * (M + np.abs(G0)))[hit]
    assert np.all(err <= tol), float((err / tol).max())
    blocks = np.pad(hit, (0, nb * 64 - total)).reshape(nb, 64).any(1)
    want_t = T0.copy()
    want_t[:nb][(T0[:nb] == 0) & blocks] = 1
    assert np.array_equal(touch, want_t), "touch bytes"
    assert _same(words[2 * slots:], L0[2 * slots:])
    changed = int(((_bits(words[:2 * slots:2]) != _bits(L0[:2 * slots:2]))).sum())
    if k_own == 0:
        assert _same(words, L0) or (zero_loss and not _bits(words).any())
    for w, ref, mass in ((0, loss, m_loss), (1, l2, m_l2)):
        start = L0[w:2 * slots:2].astype(f64)
        e = abs(words[w:2 * slots:2].astype(f64).sum() - (start.sum() + ref))
        assert np.isfinite(e) and e <= (k_own + 16) * U24 * (mass + np.abs(start).sum()), (w, e, mass)
    return dict(got=got, G0=G0, D=D, M=M, K=K, layout=layout, touch=touch, T0=T0, words=words, L0=L0, changed=changed, x=x, acc=acc,
                loss=(loss, m_loss), l2=(l2, m_l2), k=k_own)


def _triples(rng, nU, nI, n):
    return tuple(rng.integers(0, m, n).astype(np.int32) for m in (nU, nI, nI))


@pytest.mark.parametrize("slots", [1, 32])
@pytest.mark.parametrize("dim", [64, 128, 192, 256])
def test_bpr_step_dim_widths_slots_and_grad_scale(dim, slots):
    """skr_bpr_step_dim at every width, one and 32 loss slots, split tables: with grad_scale 0.25 a scale that leaked into the
    regulariser's part or into the loss word shows (the reference scales c only).  37 triples are 10 workgroups: with 32 slots more
    than one pair of words must have changed."""
    rng = np.random.default_rng(dim + slots)
    nU, nI, n = 41, 29, 37
    for gs in (1.0, 0.25):
        c = _tables(rng, nU, nI, dim, "split")
        u, i, j = _triples(rng, nU, nI, n)
        r = _bpr("dim", c, u, i, j, 1.0 / n, 1e-2, 0.5, gs=gs, dim=dim, slots=slots, seed=dim)
        assert r["changed"] > 1 if slots > 1 else r["changed"] == 1
    c = _tables(rng, nU, nI, dim, "same")
    _bpr("dim", c, *_triples(rng, nU, nI, n), 1.0, 1e-3, 1.0, gs=0.25, dim=dim, slots=slots, seed=dim + 1)


@pytest.mark.parametrize("entry", ["step", "spread"])
@pytest.mark.parametrize("n,nU,nI", [(16389, 3000, 2000), (16389, 37, 23), (1, 37, 23), (3, 37, 23), (4, 37, 23), (5, 37, 23),
                                     (515, 37, 23)])
def test_bpr_step_grid_cap_and_small_batches(entry, n, nU, nI):
    """n = 16389: 4096 workgroups of 4 wavefronts, one wavefront takes a second triple (the grid-stride loop's second trip); once with
    few addends per row (a tight bound) and once with hundreds of atomics per row; n = 1 .. 5 around one workgroup; skr_bpr_step
    and skr_bpr_step_spread (what BPRMF launches every step)."""
    rng = np.random.default_rng(n + nU)
    c = _tables(rng, nU, nI, 64, "same")
    slots = _hip.SKR_LOSS_SLOTS if entry == "spread" else 1
    r = _bpr(entry, c, *_triples(rng, nU, nI, n), 1.0, 1e-3, 1.0, slots=slots, seed=n)
    if entry == "spread":
        assert r["changed"] == min(32, -(-n // 4))


def test_bpr_step_empty_batch_changes_nothing():
    rng = np.random.default_rng(5)
    c = _tables(rng, 9, 7, 64, "same")
    for entry, kw in (("step", {}), ("spread", dict(slots=32)), ("dim", dict(dim=64)), ("sharded", dict(world=2, rank=1))):
        r = _bpr(entry, c, *_triples(rng, 9, 7, 4), 1.0, 1e-3, 1.0, n=0, **kw)
        assert _same(r["got"], r["G0"]) and _same(r["words"], r["L0"]) and np.array_equal(r["touch"], r["T0"])


@pytest.mark.parametrize("entry,dim", [("step", 64), ("dim", 128)])
def test_bpr_step_saturated_and_tied_scores(entry, dim):
    """x = 0 exactly (i == j), +-20, +-90 and +-200 (past +-90 expf(-|x|) underflows), near-ties |x| ~ 1e-6 that come out of a
    cancellation of two inner products of size 3: everything finite, within the bound; the gradients of an i == j triple cancel to
    the regulariser's part."""
    rng = np.random.default_rng(dim)
    targets = [0.0, 20.0, -20.0, 90.0, -90.0, 200.0, -200.0, 1e-6, -1e-6, 3e-7] * 3
    n = len(targets)
    P = (0.3 * rng.standard_normal((n, dim))).astype(f32)
    Q = np.zeros((2 * n, dim), f32)
    for b, t in enumerate(targets):
        p = P[b].astype(f64)
        if abs(t) >= 1.0:
            Q[2 * b], Q[2 * b + 1] = p * (0.5 * t / (p @ p)), -p * (0.5 * t / (p @ p))
        else:
            base = rng.standard_normal(dim) * 0.3 + p * (3.0 / (p @ p))
            Q[2 * b], Q[2 * b + 1] = base + p * (t / (p @ p)), base
    bias = (0.2 * rng.standard_normal(2 * n)).astype(f32)
    bias[1::2] = bias[0::2]                                   # b_i == b_j: the bias is read but leaves x alone
    u = np.arange(n, dtype=np.int32)
    i, j = 2 * u, 2 * u + 1
    tie = np.array(targets) == 0.0
    j[tie] = i[tie]
    c = dict(P=P, Q=Q, bias=bias, RP=P, RQ=Q, g_split=False, gb=True)
    reg = 1e-2
    r = _bpr(entry, c, u, i, j, 1.0, reg, 1.0, dim=dim, seed=dim)
    x = r["x"]
    assert np.all(x[tie] == 0.0) and x.max() > 199 and x.min() < -199 and np.abs(x[np.abs(np.array(targets)) < 1e-3]).max() < 1e-4
    assert np.all(np.isfinite(r["words"]))
    o = r["layout"]["gP"][0]
    rows = np.flatnonzero(tie)
    sl = (rows[:, None] * dim + np.arange(dim)).reshape(-1) + o
    part = f64(f32(reg)) * P[rows].astype(f64).reshape(-1)     # the regulariser's part alone
    assert np.allclose(r["D"][sl], part, rtol=1e-12, atol=0)
    assert np.all(np.abs(r["got"][sl] - (r["G0"][sl] + part)) <= 17 * U24 * (np.abs(part) + np.abs(r["G0"][sl])))


@pytest.mark.parametrize("entry,dim", [("step", 64), ("dim", 128)])
@pytest.mark.parametrize("mode", ["same", "split", "alias_in", "split_reg0", "no_gb", "no_bias"])
def test_bpr_step_table_modes(mode, entry, dim):
    """same tables; split tables; RP is P and RQ is Q with separate gradient buffers of the regulariser (must take the split path:
    the score part into gP, the regulariser's into gRP); split with reg = 0 (gRP / gRQ keep their bits and their touch bytes stay
    0); a bias without a gradient buffer (no bias gradient and no mark, the bias still in x and in the L2 word); no bias."""
    rng = np.random.default_rng(len(mode) * 7 + dim)
    nU, nI, n = 33, 21, 50
    c = _tables(rng, nU, nI, dim, "split" if mode == "split_reg0" else mode)
    reg = 0.0 if mode == "split_reg0" else 1e-2
    u, i, j = _triples(rng, nU, nI, n)
    r = _bpr(entry, c, u, i, j, 0.5, reg, 0.5, dim=dim, seed=dim)
    if mode == "split_reg0":
        for name in ("gRP", "gRQ"):
            o, sz = r["layout"][name]
            assert _same(r["got"][o:o + sz], r["G0"][o:o + sz]) and not (r["touch"][o // 64:(o + sz) // 64] == 1).any()
            assert not r["K"][o:o + sz].any()
    if mode == "alias_in":
        assert r["K"][r["layout"]["gRP"][0]:].any()           # the reference did send the regulariser's part to gRP
    if mode in ("no_gb", "no_bias"):
        assert "gb" not in r["layout"]
    if mode == "no_gb":                                        # a launch that ignored the bias would miss both words by far more than the bound
        _, (loss2, m2), (l22, _), _ = _bpr_ref(dict(c, bias=None), u, i, j, 0.5, reg, 0.5, 1.0)
        assert abs(loss2 - r["loss"][0]) > 100 * (n + 16) * U24 * m2 and abs(l22 - r["l2"][0]) > 100 * (n + 16) * U24 * l22


def _shard(c_glob, world, rank, rng):
    """rank's local user tables: row k is global user k * world + rank; ceil(nU / world) rows count, the rows behind them (up to nU,
    so that a global user id used as a local row stays inside the allocation) hold other numbers and must never be touched"""
    nU = c_glob["P"].shape[0]
    out = dict(c_glob)
    for k in ("P", "RP"):
        if k == "RP" and c_glob["RP"] is c_glob["P"]:
            out["RP"] = out["P"]
            continue
        loc = (0.3 * rng.standard_normal(c_glob[k].shape)).astype(f32)
        mine = c_glob[k][rank::world]
        loc[:len(mine)] = mine
        out[k] = loc
    return out


@pytest.mark.parametrize("world,mode,gs", [(2, "same", 1.0), (3, "split", 0.5)])
def test_bpr_step_sharded_rows_and_sums(world, mode, gs):
    """skr_bpr_step_sharded, every rank on one global batch: rank r's gP is the float64 gradient of the users u % world == r at local
    row u // world, the rows behind the local table's ceil(nU / world) keep their bits; the ranks' gQ, gb and words add up to the
    unsharded reference."""
    rng = np.random.default_rng(world)
    nU, nI, n = 101, 45, 300
    cg = _tables(rng, nU, nI, 64, mode)
    u, i, j = _triples(rng, nU, nI, n)
    acc, (loss, m_loss), (l2, m_l2), _ = _bpr_ref(cg, u, i, j, 1.0 / n, 1e-2, 0.5, gs)
    sums = {k: 0.0 for k in ("gQ", "gb", "gRQ", "loss", "l2") if k in acc or k in ("loss", "l2")}
    tols = dict(sums)
    for rank in range(world):
        r = _bpr("sharded", _shard(cg, world, rank, rng), u, i, j, 1.0 / n, 1e-2, 0.5, gs=gs, world=world, rank=rank, seed=rank)
        rows = -(-nU // world)
        assert not r["K"][rows * 64:nU * 64].any() and r["K"][:64 * len(range(rank, nU, world))].any()
        for k in sums:
            if k in ("loss", "l2"):
                w = 0 if k == "loss" else 1
                sums[k] += f64(r["words"][w]) - f64(r["L0"][w])
                tols[k] += (r["k"] + 16) * U24 * (r[k][1] + abs(f64(r["L0"][w])))
            else:
                o, sz = r["layout"][k]
                sums[k] = sums[k] + (r["got"][o:o + sz].astype(f64) - r["G0"][o:o + sz])
                tols[k] = tols[k] + np.where(r["K"] > 0, (r["K"] + 16) * U24 * (r["M"] + np.abs(r["G0"])), 0.0)[o:o + sz]
    assert abs(sums["loss"] - loss) <= tols["loss"] and abs(sums["l2"] - l2) <= tols["l2"]
    for k in sums:
        if k not in ("loss", "l2"):
            assert np.all(np.abs(sums[k] - acc[k][0].reshape(-1)) <= tols[k] + 1e-12), k


def test_bpr_step_sharded_rank_without_a_triple():
    """a rank that owns no user of the batch: every gradient float and touch byte as it was, +0 added to the loss words"""
    rng = np.random.default_rng(11)
    nU, nI, n, world = 60, 20, 70, 3
    cg = _tables(rng, nU, nI, 64, "same")
    u, i, j = _triples(rng, nU, nI, n)
    u = (u // world * world).astype(np.int32)                 # every user belongs to rank 0
    for rank in (1, 2):
        r = _bpr("sharded", _shard(cg, world, rank, rng), u, i, j, 1.0, 1e-2, 1.0, world=world, rank=rank, zero_loss=True)
        assert r["k"] == 0 and _same(r["got"], r["G0"]) and np.array_equal(r["touch"], r["T0"]) and not _bits(r["words"]).any()
    assert _bpr("sharded", _shard(cg, world, 0, rng), u, i, j, 1.0, 1e-2, 1.0, world=world, rank=0)["k"] == n


@pytest.mark.parametrize("entry,dim", [("step", 64), ("dim", 192)])
def test_bpr_step_touch_bytes_exact(entry, dim):
    """the flat [P | Q | bias] layout of the optimiser: the bytes equal to 1 are EXACTLY the 64-float blocks a row or a bias word of
    the batch lies in -- dim / 64 blocks per row, lane c marking the c-th -- bytes preset to 2 stay 2, every other byte stays 0"""
    rng = np.random.default_rng(9 + dim)
    nU, nI, n, cw = 50, 40, 30, dim // 64
    c = _tables(rng, nU, nI, dim, "same")
    u, i, j = _triples(rng, nU, nI, n)
    r = _bpr(entry, c, u, i, j, 1.0, 1e-3, 1.0, dim=dim, seed=dim)
    assert r["layout"] == dict(gP=(0, nU * dim), gQ=(nU * dim, nI * dim), gb=((nU + nI) * dim, nI))
    items = np.concatenate([i, j]).astype(np.int64)
    want = set((u.astype(np.int64)[:, None] * cw + np.arange(cw)).reshape(-1))
    want |= set((nU * cw + items[:, None] * cw + np.arange(cw)).reshape(-1))
    want |= set(((nU + nI) * dim + items) // 64)
    t, t0 = r["touch"], r["T0"]
    assert set(np.flatnonzero(t == 1)) == {b for b in want if t0[b] == 0}
    assert np.array_equal(t == 2, t0 == 2) and len(want) > 3 * cw and (t0[sorted(want)] == 2).any()
    assert not t[[b for b in range(len(t)) if b not in want and t0[b] == 0]].any()


# ------------------------------------------------------------------------------------------------
# 2. the gradient exchange
# ------------------------------------------------------------------------------------------------
def _pack(ids, gV, gb, guard=1):
    """skr_pack_grad_rows on copies -> (packed [n + guard, 66], gV after, gb after)"""
    n = len(ids)
    d_ids, dV = to_dev(np.ascontiguousarray(ids, np.int32)), to_dev(gV)
    db = to_dev(gb) if gb is not None else None
    out = torch.full((n + guard, 66), float(SENT), device=dev())
    _hip.check(_hip.lib().skr_pack_grad_rows(_hip.ptr(d_ids), n, _hip.ptr(dV), _hip.ptr(db), 64, _hip.ptr(out), _hip.stream()))
    return _host(out), _host(dV), None if gb is None else _host(db)


def _pack_ref(ids, gV, gb, guard=1):
    n = len(ids)
    out = np.full((n + guard, 66), SENT, f32)
    v = ids >= 0
    out[:n, 0] = ids.astype(np.int32).view(f32)
    out[:n][v, 1:65] = gV[ids[v]]
    out[:n][v, 65] = gb[ids[v]] if gb is not None else 0.0
    gV2, gb2 = gV.copy(), None if gb is None else gb.copy()
    gV2[ids[v]] = 0.0
    if gb is not None:
        gb2[ids[v]] = 0.0
    return out, gV2, gb2


@pytest.mark.parametrize("with_gb", [True, False])
@pytest.mark.parametrize("n", [1, 4, 5, 300])
def test_pack_grad_rows_vs_numpy(n, with_gb):
    """packed row = [id bits | the dense row | its bias word, 0 without gb] bit for bit; an empty slot gets the id word -1 and
    nothing else; the packed dense rows and bias words are +0 afterwards; every other row, and the row behind the pack, untouched"""
    rng = np.random.default_rng(n)
    nI = 700
    ids = rng.permutation(nI - 1)[:n].astype(np.int32)
    if n > 1:
        ids[rng.random(n) < 0.3] = -1
        ids[1], ids[n - 1] = -1, nI - 1
    gV, gb = rng.standard_normal((nI, 64)).astype(f32), rng.standard_normal(nI).astype(f32)
    got = _pack(ids, gV, gb if with_gb else None)
    want = _pack_ref(ids, gV, gb if with_gb else None)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    if with_gb:
        assert _same(got[2], want[2])
    if n > 1:
        assert _bits(got[0])[1, 0] == -1 and _same(got[0][1, 1:], np.full(65, SENT, f32))


def _round_trip(R, cap, nI, rng, empty_rank):
    """R simulated ranks pack `cap` slots each (ids through unique_padded_rows: ascending, then -1), the packs are concatenated and
    unpacked by both functions; -> per function (flat [V | b] after, touch after), the flat start values, the start touch bytes,
    the packs"""
    from skrec.parallel import unique_padded_rows
    L, st = _hip.lib(), _hip.stream()
    raw = rng.integers(0, nI - 1, (R, cap)).astype(np.int32)               # nI - 1 is kept for the highest rank alone
    raw[rng.random((R, cap)) < 0.3] = -1
    raw[:, 0] = 7 % (nI - 1)                                               # an id every rank holds
    if cap >= 2:
        raw[R - 1, 1] = nI - 1                                             # an id only the highest rank holds
    if empty_rank and R >= 3:
        raw[1] = -1                                                        # a rank whose slots are all empty
    ids = unique_padded_rows(torch.from_numpy(raw)).numpy()
    assert np.all((ids[:, 1:] > ids[:, :-1]) | (ids[:, 1:] < 0))
    packs = np.empty((R, cap, 66), f32)
    for r in range(R):
        gV, gb = rng.standard_normal((nI, 64)).astype(f32), rng.standard_normal(nI).astype(f32)
        got, want = _pack(ids[r], gV, gb, guard=0), _pack_ref(ids[r], gV, gb, guard=0)
        assert all(_same(a, b) for a, b in zip(got, want))
        packs[r] = np.where(np.broadcast_to((ids[r] >= 0)[:, None], (cap, 66)), got[0], f32(3.5))   # junk behind empty slots' ids
        packs[r, :, 0] = got[0][:, 0]
    flat0 = rng.standard_normal(nI * 64 + nI).astype(f32)
    nb = (len(flat0) + 63) // 64
    T0 = np.where(rng.random(nb + 1) < 0.1, 2, 0).astype(np.uint8)
    d_packs = to_dev(packs)
    outs = []
    for fn in (L.skr_unpack_grad_rows, L.skr_unpack_grad_rows_sorted):
        buf, touch = to_dev(flat0), to_dev(T0)
        _hip.check(fn(_hip.ptr(d_packs), cap, R, _hip.ptr(buf), _at(buf, nI * 64), 64, _hip.ptr(touch), _hip.ptr(buf), st))
        outs.append((_host(buf), _host(touch)))
    return outs, flat0, T0, packs, ids


def _unpack_ref(packs, flat0, T0, nI):
    """((g0 + r0) + r1) + ... in float32, the order both kernels document; the touch bytes of the ids present"""
    want = flat0.copy()
    V, b = want[:nI * 64].reshape(nI, 64), want[nI * 64:]
    t = T0.copy()
    for r in range(packs.shape[0]):
        ids = _bits(packs[r, :, 0])
        v = ids >= 0
        V[ids[v]] = V[ids[v]] + packs[r][v, 1:65]
        b[ids[v]] = b[ids[v]] + packs[r][v, 65]
        for blk in (ids[v], nI + ids[v] // 64):
            t[blk] = np.where(t[blk] == 0, 1, t[blk])
    return want, t


@pytest.mark.parametrize("R,cap,nI,empty_rank", [(3, 1, 10, False), (3, 63, 200, True), (2, 64, 130, False), (3, 65, 200, False),
                                                 (3, 4097, 9000, True), (17, 65, 300, False), (16, 5, 40, True), (17, 4, 64, True)])
def test_exchange_round_trip_vs_numpy(R, cap, nI, empty_rank):
    """pack on R ranks, concatenate, unpack with each function == the float32 rank-order sum done in numpy, bit for bit, dense rows and
    bias words; the touch bytes are exactly the blocks of the ids present (row block id, bias block n_items + id / 64).  17 ranks:
    the sorted form's fallback; cap 1 / 63..65 / 4097: pack_find's stride 1, 1 -> 2, and beyond 64 (its inner loop's second trip)."""
    rng = np.random.default_rng(R * 10000 + cap)
    outs, flat0, T0, packs, ids = _round_trip(R, cap, nI, rng, empty_rank)
    want, want_t = _unpack_ref(packs, flat0, T0, nI)
    assert not _same(want, flat0)
    if cap >= 2:
        assert (ids[:R - 1] != nI - 1).all() and (ids[R - 1] == nI - 1).any()
    assert all((ids[r] == 7 % (nI - 1)).any() for r in range(R) if not (empty_rank and R >= 3 and r == 1))
    for buf, touch in outs:
        assert _same(buf, want)
        assert np.array_equal(touch, want_t)


# ------------------------------------------------------------------------------------------------
# 3. row helpers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 32, 64, 100, 128])
def test_gather_and_scatter_rows_vs_numpy(dim):
    """skr_gather_rows / skr_scatter_rows (the 64-lane kernels at dim 64, the per-element ones elsewhere) == numpy indexing, bit for
    bit; scatter skips negative ids, duplicate ids carry identical rows; rows not named, and the row behind the output, untouched"""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(dim)
    rows, n = 37, 130
    T = rng.standard_normal((rows, dim)).astype(f32)
    idx = rng.integers(0, rows, n).astype(np.int32)
    idx[[0, n - 1]] = [rows - 1, 0]
    out = torch.full((n + 1, dim), float(SENT), device=dev())
    dT, d_idx = to_dev(T), to_dev(idx)
    _hip.check(L.skr_gather_rows(_hip.ptr(dT), _hip.ptr(d_idx), n, dim, _hip.ptr(out), st))
    want = np.full((n + 1, dim), SENT, f32)
    want[:n] = T[idx]
    assert _same(_host(out), want) and _same(_host(dT), T)
    new = rng.standard_normal((rows, dim)).astype(f32)
    sidx = rng.integers(0, rows - 6, n).astype(np.int32)             # duplicates; the last rows are never named
    sidx[rng.random(n) < 0.2] = -1
    sidx[3] = -1
    src = np.full((n + 1, dim), 99.0, f32)
    src[:n] = new[np.maximum(sidx, 0)]                               # identical rows behind identical ids
    table = np.full((rows + 1, dim), SENT, f32)
    table[:rows] = T
    d_tab, d_src, d_sidx = to_dev(table), to_dev(src), to_dev(sidx)
    _hip.check(L.skr_scatter_rows(_hip.ptr(d_src), _hip.ptr(d_sidx), n, dim, _hip.ptr(d_tab), st))
    v = sidx >= 0
    table[sidx[v]] = src[:n][v]
    assert _same(_host(d_tab), table) and len(set(sidx[v])) < v.sum() and _same(table[rows - 6:rows], T[rows - 6:])


LENGTHS = [1, 255, 257, 2048 * 256 + 3]          # the last: the grid-stride loops (2048 workgroups of 256) take a second trip


def _fma_once(a, x, y):
    """fl32(a x + y) with ONE rounding: the product of two float32 is exact in float64; s = fl64(p + y) and its exact error e
    (two-sum); where s lies exactly half-way between two float32 the error decides the direction instead of the tie rule"""
    p = f64(a) * x.astype(f64)
    yy = y.astype(f64)
    s = p + yy
    bb = s - p
    e = (p - (s - bb)) + (yy - bb)
    r = s.astype(f32)
    half = ((s.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)) & (e != 0)
    lo = np.where(r.astype(f64) > s, np.nextafter(r, f32(-np.inf)), r)
    hi = np.where(r.astype(f64) < s, np.nextafter(r, f32(np.inf)), r)
    return np.where(half, np.where(e > 0, hi, lo), r).astype(f32)


@pytest.mark.parametrize("n", LENGTHS)
def test_axpy_scale_scale_copy_sum_blocks_lengths(n):
    """skr_axpy == fma evaluated in float64 and rounded once; skr_scale, skr_scale_copy == the float32 product; skr_sum_blocks == the
    left-to-right float32 sum of 3 blocks; all bit for bit, the element behind every output keeps its sentinel"""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(n % 1000)
    a = f32(0.3)
    x = rng.standard_normal(n).astype(f32)
    y0 = np.append(rng.standard_normal(n).astype(f32), SENT)
    dx, dy = to_dev(x), to_dev(y0)
    _hip.check(L.skr_axpy(float(a), _hip.ptr(dx), _hip.ptr(dy), n, st))
    assert _same(_host(dy), np.append(_fma_once(a, x, y0[:n]), SENT))
    ds = to_dev(y0)
    _hip.check(L.skr_scale(float(a), _hip.ptr(ds), n, st))
    assert _same(_host(ds), np.append(a * y0[:n], SENT))
    dc = torch.full((n + 1,), float(SENT), device=dev())
    _hip.check(L.skr_scale_copy(float(a), _hip.ptr(dx), _hip.ptr(dc), n, st))
    assert _same(_host(dc), np.append(a * x, SENT)) and _same(_host(dx), x)
    blocks = rng.standard_normal((3, n)).astype(f32)
    db, do = to_dev(blocks), torch.full((n + 1,), float(SENT), device=dev())
    _hip.check(L.skr_sum_blocks(_hip.ptr(db), 3, n, _hip.ptr(do), st))
    assert _same(_host(do), np.append((blocks[0] + blocks[1]) + blocks[2], SENT))


@pytest.mark.parametrize("n_blocks", [1, 2, 3, 16])
def test_sum_blocks_counts(n_blocks):
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(n_blocks)
    n = 257
    blocks = (rng.standard_normal((n_blocks, n)) * 10.0 ** rng.integers(-3, 4, (n_blocks, 1))).astype(f32)
    want = blocks[0].copy()
    for b in range(1, n_blocks):
        want = want + blocks[b]
    db, do = to_dev(blocks), torch.full((n + 1,), float(SENT), device=dev())
    _hip.check(L.skr_sum_blocks(_hip.ptr(db), n_blocks, n, _hip.ptr(do), st))
    assert _same(_host(do), np.append(want, SENT))


@pytest.mark.parametrize("dim", [1, 64, 65, 192])
def test_clear_marked_rows_shapes(dim):
    """rows whose mask byte is non-zero become +0, the others keep their bits; the mask is cleared or kept as asked; the row and the
    (set) mask byte behind the table are not touched"""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(dim)
    for n_rows in (1, 63, 64, 65, 130):
        for clear in (0, 1):
            mask = np.where(rng.random(n_rows + 1) < 0.4, rng.integers(1, 256, n_rows + 1), 0).astype(np.uint8)
            mask[n_rows] = 1
            mask[0] = 1 if n_rows > 1 else clear                      # n_rows = 1: once marked, once not
            if n_rows > 2:
                mask[n_rows - 1], mask[n_rows - 2] = 255, 0
            T = rng.standard_normal((n_rows + 1, dim)).astype(f32)
            dm, dT = to_dev(mask), to_dev(T)
            _hip.check(L.skr_clear_marked_rows(_hip.ptr(dm), n_rows, clear, _hip.ptr(dT), dim, st))
            want = T.copy()
            want[:n_rows][mask[:n_rows] != 0] = 0.0
            wm = mask.copy()
            if clear:
                wm[:n_rows] = 0
            assert _same(_host(dT), want) and np.array_equal(_host(dm), wm), (n_rows, clear)


# ------------------------------------------------------------------------------------------------
# 4. refinements and wide products
# ------------------------------------------------------------------------------------------------
EPS = f64(f32(1e-8))      # the kernel's clamp, F.cosine_similarity's default eps (LayerGCN.py:214), as the float32 the kernel holds


def _refine_ref(Y, E, dZ, w_in=None):
    """float64: w = (y / max(|y|, eps)) . (e / max(|e|, eps)), Z = w y; backward of sum(Z dZ): clamp_min has slope 0 below the clamp,
    so d(y / n)/dy = (I - yh yh^T) / n for an unclamped norm and I / eps for a clamped one"""
    Y, E, dZ = (a.astype(f64) for a in (Y, E, dZ))
    nyr, ner = np.sqrt((Y * Y).sum(1)), np.sqrt((E * E).sum(1))
    ny, ne = np.maximum(nyr, EPS)[:, None], np.maximum(ner, EPS)[:, None]
    yh, eh = Y / ny, E / ne
    w = (yh * eh).sum(1)
    wb = (w if w_in is None else w_in.astype(f64))[:, None]
    dw = (dZ * Y).sum(1)[:, None]
    gy = np.where((nyr > EPS)[:, None], (eh - wb * yh) / ny, eh / ny)
    ge = np.where((ner > EPS)[:, None], (yh - wb * eh) / ne, yh / ne)
    return w, w[:, None] * Y, wb * dZ + dw * gy, dw * ge


def _refine_inputs(rng, n, dim):
    """rows 0..: a zero Y row, a zero E row, both zero, |Y| = 5e-9 and 5e-8 (the two sides of the clamp), the same for E, Y parallel
    and anti-parallel to E -- as many of them as n holds -- among ordinary rows"""
    Y, E, dZ = (rng.standard_normal((n, dim)).astype(f32) for _ in range(3))
    unit = lambda a: a.astype(f64) / np.linalg.norm(a.astype(f64))  # noqa: E731
    special = [lambda r: Y.__setitem__(r, 0), lambda r: E.__setitem__(r, 0),
               lambda r: (Y.__setitem__(r, 0), E.__setitem__(r, 0)),
               lambda r: Y.__setitem__(r, (unit(Y[r]) * 5e-9).astype(f32)), lambda r: Y.__setitem__(r, (unit(Y[r]) * 5e-8).astype(f32)),
               lambda r: E.__setitem__(r, (unit(E[r]) * 5e-9).astype(f32)), lambda r: E.__setitem__(r, (unit(E[r]) * 5e-8).astype(f32)),
               lambda r: Y.__setitem__(r, f32(1.5) * E[r]), lambda r: Y.__setitem__(r, f32(-0.75) * E[r])]
    if n >= 5:
        for r, fn in enumerate(special if n > len(special) else [special[k] for k in (0, 1, 2, 7, 8)]):
            fn(r)
    return Y, E, dZ


def _close(got, want, rtol, atol):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


@pytest.mark.parametrize("n", [1, 5, 777])
@pytest.mark.parametrize("dim", [128, 192, 256])
def test_layer_refine_wide_rows_vs_float64(dim, n):
    """skr_layer_refine_fwd, _bwd and _bwd_masked at 128 / 192 / 256 columns against _refine_ref, at the tolerances of
    test_layer_refine_fwd_bwd_vs_torch_autograd (rtol 1e-5 / atol 1e-6 forward, 2e-5 / 2e-6 backward).  Measured on the CPU on these
    inputs: torch's own fp32 autograd differs from the reference by at most 0.05 of the forward and 0.33 of the backward tolerance
    (the worst element over the nine cases, on the rows where torch and the formula agree), inside half of each.  The reference is
    cross-checked here against float64 F.cosine_similarity autograd: w on every row, dY on the rows whose Y norm is not clamped, dE
    on those whose E norm is not.  For the gradient of a clamped vector the installed torch (2.10) returns something else than the
    clamp_min form (y = (5e-9, 0, 0, 0), e = 1: dY_0 = 2.5e7 where I / eps gives 5e7), so there the formula of the kernel's comment
    and of the 64-column test stands alone.  (torch clamps at 1e-8, the kernel at the float32 next to it: 6e-10 apart.)"""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(dim + n)
    Y, E, dZ = _refine_inputs(rng, n, dim)
    w, Z, gY, gE = _refine_ref(Y, E, dZ)
    ty, te = torch.tensor(Y.astype(f64), requires_grad=True), torch.tensor(E.astype(f64), requires_grad=True)
    tw = torch.nn.functional.cosine_similarity(ty, te, dim=-1)
    (tw[:, None] * ty * torch.tensor(dZ.astype(f64))).sum().backward()
    free, free_e = np.linalg.norm(Y.astype(f64), axis=1) > EPS, np.linalg.norm(E.astype(f64), axis=1) > EPS
    _close(w, tw.detach().numpy(), 1e-8, 1e-14)
    _close(gE[free_e], te.grad.numpy()[free_e], 1e-8, 1e-13)
    _close(gY[free], ty.grad.numpy()[free], 1e-8, 1e-13)
    if n == 777:
        assert (~free).sum() == 3 and (~free_e).sum() == 3
    dY_, dE_, dZ_ = to_dev(Y), to_dev(E), to_dev(dZ)
    acc0, gE0 = rng.standard_normal((n + 1, dim)).astype(f32), rng.standard_normal((n + 1, dim)).astype(f32)
    acc0[n], gE0[n] = SENT, SENT
    Zd, Wd, accd = torch.full((n + 1, dim), float(SENT), device=dev()), torch.full((n + 1,), float(SENT), device=dev()), to_dev(acc0)
    _hip.check(L.skr_layer_refine_fwd(_hip.ptr(dY_), _hip.ptr(dE_), n, dim, _hip.ptr(Zd), _hip.ptr(Wd), _hip.ptr(accd), st))
    Zg, Wg, accg = _host(Zd), _host(Wd), _host(accd)
    _close(Wg[:n], w, 1e-5, 1e-6)
    _close(Zg[:n], Z, 1e-5, 1e-6)
    _close(accg[:n], acc0[:n] + Z, 1e-5, 1e-6)
    assert _same(Zg[n], np.full(dim, SENT, f32)) and Wg[n] == SENT and _same(accg[n], acc0[n])
    Z2 = torch.full((n + 1, dim), float(SENT), device=dev())
    _hip.check(L.skr_layer_refine_fwd(_hip.ptr(dY_), _hip.ptr(dE_), n, dim, _hip.ptr(Z2), _hip.ptr(Wd), None, st))   # no accum
    assert _same(_host(Z2), Zg)
    # backward, from the reference's own w (rounded to float32): independent of the forward kernel
    w32 = w.astype(f32)
    _, _, gY, gE = _refine_ref(Y, E, dZ, w32)
    dW = to_dev(w32)
    gYd, gEd = torch.full((n + 1, dim), float(SENT), device=dev()), to_dev(gE0)
    _hip.check(L.skr_layer_refine_bwd(_hip.ptr(dY_), _hip.ptr(dE_), _hip.ptr(dW), _hip.ptr(dZ_), n, dim, _hip.ptr(gYd), _hip.ptr(gEd), st))
    gYg, gEg = _host(gYd), _host(gEd)
    _close(gYg[:n], gY, 2e-5, 2e-6)
    _close(gEg[:n], gE0[:n] + gE, 2e-5, 2e-6)
    assert _same(gYg[n], np.full(dim, SENT, f32)) and _same(gEg[n], gE0[n])
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    if n >= 5:
        mask[:5] = [1, 0, 1, 0, 1]
    sel = mask.astype(bool)
    dm = to_dev(mask)
    for zs in (0, 1):
        gYm, gEm = torch.full((n + 1, dim), float(SENT), device=dev()), to_dev(gE0)
        _hip.check(L.skr_layer_refine_bwd_masked(_hip.ptr(dY_), _hip.ptr(dE_), _hip.ptr(dW), _hip.ptr(dZ_), n, dim, _hip.ptr(gYm),
                                                 _hip.ptr(gEm), _hip.ptr(dm), zs, st))
        a, b = _host(gYm), _host(gEm)
        want_skipped = np.zeros((int((~sel).sum()), dim), f32) if zs else np.full((int((~sel).sum()), dim), SENT, f32)
        assert _same(a[:n][sel], gYg[:n][sel]) and _same(b[:n][sel], gEg[:n][sel])          # the same arithmetic on the marked rows
        assert _same(a[:n][~sel], want_skipped) and _same(b[:n][~sel], gE0[:n][~sel]) and _same(a[n], gYg[n]) and _same(b[n], gE0[n])


def _wide(rng, rows, ld):
    return rng.standard_normal((rows, ld)).astype(f32)


def _slice_check(got, start, c, want, tol, rows=None):
    """slice c of the [n, ld] table `got` is within tol of `want` on `rows` (all by default); every other float keeps start's bits"""
    sl = slice(64 * c, 64 * c + 64)
    rows = np.ones(len(got), bool) if rows is None else rows
    keep = np.ones(got.shape, bool)
    keep[rows, sl] = False
    assert np.array_equal(_bits(got)[keep], _bits(start)[keep]), "a float outside the slice changed"
    err = np.abs(got[rows, sl] - want[rows])
    assert np.all(err <= tol[rows]), float((err / tol[rows]).max())


@pytest.mark.parametrize("ld", [128, 192, 256])
def test_csr_spmm_strided_slices_vs_scipy(ld):
    """skr_csr_spmm_strided on slice c of [n, ld] tables (X, addend, Y, accum advanced by 64 c floats) against scipy in float64 at the
    project's 2e-6 mass + 1e-6; rows that cross a 512-entry chunk boundary (zeroed by the first kernel, added to with atomics,
    finished by the last one), empty rows inside and at the end; the other slices of Y and accum keep their bits.  A stride below
    64 is refused."""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(ld)
    n_cols = 900
    lens = np.array([3, 0, 500, 20, 700, 1, 0, 64, 65, 200, 130, 511, 5, 0, 0, 0])        # rows 3, 4 and 9 cross 512, 1024, 1536
    n_rows = len(lens)
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    assert [int(rowptr[r] // 512 != (rowptr[r + 1] - 1) // 512) for r in (3, 4, 9, 2)] == [1, 1, 1, 0]
    col = np.concatenate([np.sort(rng.choice(n_cols, l, replace=False)) for l in lens]).astype(np.int32)
    val = rng.standard_normal(len(col)).astype(f32)
    A = sp.csr_matrix((val, col, rowptr), shape=(n_rows, n_cols))
    X, add, Y0, acc0 = _wide(rng, n_cols, ld), _wide(rng, n_rows, ld), np.full((n_rows, ld), SENT, f32), _wide(rng, n_rows, ld)
    d_rp, d_col, d_val, dX, dadd = to_dev(rowptr), to_dev(col), to_dev(val), to_dev(X), to_dev(add)
    for c in range(ld // 64):
        sl = slice(64 * c, 64 * c + 64)
        prod = A.astype(f64) @ X[:, sl].astype(f64)
        mass = abs(A).astype(f64) @ np.abs(X[:, sl]).astype(f64)
        for use_add in (False, True):
            want = prod + (add[:, sl] if use_add else 0.0)
            m = mass + (np.abs(add[:, sl]) if use_add else 0.0)
            dY, dacc = to_dev(Y0), to_dev(acc0)
            _hip.check(L.skr_csr_spmm_strided(n_rows, _hip.ptr(d_rp), _hip.ptr(d_col), _hip.ptr(d_val), _at(dX, 64 * c), 64, ld, len(col),
                                              _at(dadd, 64 * c) if use_add else None, _at(dY, 64 * c), _at(dacc, 64 * c), 0.25, st))
            _slice_check(_host(dY), Y0, c, want, 2e-6 * m + 1e-6)
            _slice_check(_host(dacc), acc0, c, acc0[:, sl] + 0.25 * want, 2e-6 * (m + np.abs(acc0[:, sl])) + 1e-6)
    # skr_csr_spmm, the same kernels at stride 64, on contiguous copies of slice 0; the row behind Y and accum keeps its bits
    x64, a64 = np.ascontiguousarray(X[:, :64]), np.ascontiguousarray(add[:, :64])
    y64, c64 = np.full((n_rows + 1, 64), SENT, f32), np.ascontiguousarray(np.vstack([acc0[:, :64], np.full((1, 64), SENT, f32)]))
    dx64, da64, dy64, dc64 = to_dev(x64), to_dev(a64), to_dev(y64), to_dev(c64)
    _hip.check(L.skr_csr_spmm(n_rows, _hip.ptr(d_rp), _hip.ptr(d_col), _hip.ptr(d_val), _hip.ptr(dx64), 64, len(col), _hip.ptr(da64),
                              _hip.ptr(dy64), _hip.ptr(dc64), 0.25, st))
    want = A.astype(f64) @ x64.astype(f64) + a64
    m = abs(A).astype(f64) @ np.abs(x64).astype(f64) + np.abs(a64)
    gy, gc = _host(dy64), _host(dc64)
    assert np.all(np.abs(gy[:n_rows] - want) <= 2e-6 * m + 1e-6) and _same(gy[n_rows], y64[n_rows]) and _same(gc[n_rows], c64[n_rows])
    assert np.all(np.abs(gc[:n_rows] - (c64[:n_rows] + 0.25 * want)) <= 2e-6 * (m + np.abs(c64[:n_rows])) + 1e-6)
    dY = to_dev(Y0)
    args = (n_rows, _hip.ptr(d_rp), _hip.ptr(d_col), _hip.ptr(d_val), _hip.ptr(dX), 64)
    assert L.skr_csr_spmm_strided(*args, 32, len(col), None, _hip.ptr(dY), None, 1.0, st) == -1
    assert _same(_host(dY), Y0)


@pytest.mark.parametrize("ld", [128, 192, 256])
def test_spmm_plan_strided_slices_vs_scipy(ld):
    """skr_spmm_plan_run_ex with skr_spmm_epilogue.ld on slice c of [n, ld] tables against scipy in float64 (2e-6 mass + 1e-6): a
    300 x 4100 matrix (n_cols no multiple of 128), long rows from 64 entries, rows of every kind and five with 600 to 1500 entries,
    dense enough for the plan's LDS-streamed path (asserted); without masks (the streamed path), with a column mask (the task
    kernels), with a row mask (skipped rows keep their bits), with both; the other slices of Y and accum keep their bits; three runs
    give the same bits.  Strides 66 and 32, and a refinement with a stride other than 64, are refused."""
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(ld + 1)
    n_rows, n_cols, long_from = 300, 4100, 64
    lens = np.minimum(rng.integers(0, 40, n_rows) ** 2 // 3, n_cols)
    lens[[7, 50, 120, 200, 299]] = [600, 900, 1500, 777, 640]
    lens[[0, 150]] = 0
    lens[1], lens[2] = long_from, long_from - 1
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(n_cols, l, replace=False)) for l in lens]).astype(np.int32)
    b, e = rowptr[5], rowptr[6]
    col[b:e] = np.arange(n_cols - (e - b), n_cols)                                     # only the last columns
    val = rng.standard_normal(len(col)).astype(f32)
    nnz = len(col)
    A = sp.csr_matrix((val, col, rowptr), shape=(n_rows, n_cols))
    cmask, rmask = (rng.random(n_cols) < 0.3).astype(np.uint8), (rng.random(n_rows) < 0.4).astype(np.uint8)
    rmask[[7, 50, 120]] = [1, 0, 1]
    X = _wide(rng, n_cols, ld)
    Xm = X * cmask[:, None].astype(f32)                # a column mask promises that the X rows outside it are zero
    add, Y0, acc0 = _wide(rng, n_rows, ld), np.full((n_rows, ld), SENT, f32), _wide(rng, n_rows, ld)
    d_rp, d_col, d_val = to_dev(rowptr), to_dev(col), to_dev(val)
    dX, dXm, dadd, d_cm, d_rm = to_dev(X), to_dev(Xm), to_dev(add), to_dev(cmask), to_dev(rmask)
    h = C.c_void_p()
    _hip.check(L.skr_spmm_plan_create(n_rows, n_cols, _hip.ptr(d_rp), _hip.ptr(d_col), _hip.ptr(d_val), nnz, long_from, C.byref(h), st))
    info = (C.c_int64 * 4)()
    _hip.check(L.skr_spmm_plan_info(h, info))
    assert (info[0] & 0xffffffff) == int((lens >= long_from).sum()) and (info[0] >> 32) > 0 and info[1] > 0

    def run(c, x, use_r, use_c, Yd, accd, mode=_hip.EPI_PLAIN, stride=ld):
        ep = _hip.SpmmEpilogue(mode=mode, addend=_at(dadd, 64 * c), Y=_at(Yd, 64 * c), accum=_at(accd, 64 * c), accum_scale=0.5, ld=stride)
        return L.skr_spmm_plan_run_ex(h, _at(x, 64 * c), 64, C.byref(ep), _hip.ptr(d_rm) if use_r else None, _hip.ptr(d_cm) if use_c else None, st)
    for c in range(ld // 64):
        sl = slice(64 * c, 64 * c + 64)
        for use_r, use_c in ((False, False), (False, True), (True, False), (True, True)):
            xs, x_np = (dXm, Xm) if use_c else (dX, X)
            want = A.astype(f64) @ x_np[:, sl].astype(f64) + add[:, sl]
            mass = abs(A).astype(f64) @ np.abs(x_np[:, sl]).astype(f64) + np.abs(add[:, sl])
            rows = rmask.astype(bool) if use_r else None
            outs = []
            for rep in range(3 if (use_r, use_c) in ((False, False), (True, True)) else 1):
                dY, dacc = to_dev(Y0), to_dev(acc0)
                _hip.check(run(c, xs, use_r, use_c, dY, dacc))
                outs.append((_host(dY), _host(dacc)))
            _slice_check(outs[0][0], Y0, c, want, 2e-6 * mass + 1e-6, rows)
            _slice_check(outs[0][1], acc0, c, acc0[:, sl] + 0.5 * want, 2e-6 * (mass + np.abs(acc0[:, sl])) + 1e-6, rows)
            assert all(_same(y, outs[0][0]) and _same(a, outs[0][1]) for y, a in outs[1:])
    dY, dacc = to_dev(Y0), to_dev(acc0)
    assert run(0, dX, False, False, dY, dacc, stride=66) == -1 and run(0, dX, False, False, dY, dacc, stride=32) == -1
    for mode in (_hip.EPI_REFINE_FWD, _hip.EPI_REFINE_BWD):
        ep = _hip.SpmmEpilogue(mode=mode, Y=_hip.ptr(dY), accum=None, ld=ld, E=_hip.ptr(dadd), w=_hip.ptr(dacc), Z=_hip.ptr(dacc),
                               rawY=_hip.ptr(dadd), dE=_hip.ptr(dacc))
        assert L.skr_spmm_plan_run_ex(h, _hip.ptr(dX), 64, C.byref(ep), None, None, st) == -1
    assert _same(_host(dY), Y0) and _same(_host(dacc), acc0)
    _hip.check(L.skr_spmm_plan_destroy(h))
