"""GPU parity of csrc/seq.hip where tests/test_gpu_seq.py does not reach: every width (C = dim / 64 = 1 .. 4) of fpmc_step_kernel,
transrec_step_kernel, transrec_t_kernel and of both modes of seq_scores_kernel, the batch lengths at which their loops change shape,
triples with an id outside its table, spread loss slots pair by pair, gradients and loss words that must be ADDED to, margins at
saturation and at exactly 0, TransRec at distance exactly 0, the score rows at the edges of their query blocks and item tiles, and
FPMC / TransRec trained at row widths 128, 192 and 256.

Every numeric comparison is with a plain numpy float64 restatement written out here, computed from the same float32 inputs -- not
torch autograd, not oracle/, not another kernel.  Every output buffer starts dirty: gradients and loss words at known non-zero values
(the kernels must add), TransRec's d_work and the score rows at SENT; what a kernel must not touch (guard words behind every buffer,
rows no surviving triple names, padded columns, pairs of loss words without a workgroup, rows of d_work beyond the grid, score rows
beyond B and columns beyond n_items) is compared bit for bit.

Which test reaches what:

  test_fpmc_step_widths_and_batch_lengths      fpmc_step_kernel<1..4>; n = 1, 3 (idle wavefronts), 5, 61, 253, 268, 4099 (capped grid:
                                               the grid-stride loop's second trip); ADD semantics; padded columns; one and 32 slots
  test_transrec_step_widths_and_batch_lengths  transrec_step_kernel<1..4> and transrec_t_kernel<1..4>; idle wavefronts' s_dt rows;
                                               n_parts = 1, 2, 16 (= T_WAVES), 64 (one 4-deep trip, no remainder), 67 (trip plus a
                                               remainder for three wavefronts), 1024; gT +=; d_work from SENT
  test_step_skips_out_of_range_triples         the `continue` of each of u, l, p, n, below and above its table
  test_step_with_every_triple_out_of_range     nothing but T's own reg * T and 1/2 |T|^2, once per batch
  test_step_loss_slots_pair_by_pair            add_loss: workgroup g -> pair g % 32; T's l2 in word 1 of pair 0; 1 slot == 32 slots
  test_fpmc_margins_at_the_edges               bpr_terms: x = 0 (p == n), +-2^-20, +-30, +-90 (denormal expf), +-120 (expf = 0)
  test_transrec_distances_at_the_edges         dp == 0, dn == 0, both 0, p == n, margins +-90 through the biases
  test_seq_scores_blocks_tiles_and_bad_rows    seq_scores_kernel<0 / 1, 1..4>; B = 1, QB, QB + 1; n_items = 1, 255, 256, 257;
                                               ld == n_items and ld > n_items; NaN rows; distance exactly 0
  test_models_train_wide_rows                  FPMC / TransRec at dp = 128, 192, 256 through _seq.py's dense Adam per batch
  (tests/test_seq_host.py                      embed_size = 257 is refused before any launch)

The bounds.  u = 2^-24.

(a) A sum of k fp32 addends -- FPMC's gradients, both models' loss words -- as tests/test_gpu_train_edges.py derives it:
    tol = (k + 16) u (mass + |start|), mass = the sum of the addends' magnitudes plus, per triple, what an error of the margin x does
    to the addend.  FPMC: x = y_p - y_n is accurate relative to X = sum|UI[u] IU[p]| + sum|UI[u] IU[n]| + sum|LI[l] IL[p]| +
    sum|LI[l] IL[n]|, the magnitudes its four inner products add; the coefficient c = -sigmoid(-x) has slope <= 1/4, so the
    addend c f + reg r of a row (f: the factor c multiplies) has mass (|c| + X / 4) |f| + reg |r|.  The loss l = log(1 + exp(-x))
    has slope <= 1: its mass is l + X; the l2 word's mass is its value.  The bound holds for any order of the additions, so the
    float atomics are covered; 16 covers the roundings inside one addend (at most 4 in-lane additions, 6 levels of the wave
    reduction, the products, the two final additions of x, expf / log1pf / the division).

(b) TransRec.  e = t - V[i] is computed with three roundings: |delta e_k| <= 3 u A_k, A_k = |U[u]_k| + |T_k| + |V[l]_k| + |V[i]_k|.
    d = |e|: |delta d| <= 3 u |A|_2 (triangle inequality over those roundings) + 8 u d (the sum of squares, relative (C + 7) u <= 11 u,
    halved by the square root, plus the root's own rounding).  So x = (-dp + bp) - (-dn + bn) is accurate to 16 u X with
    X = |A_p|_2 + |A_n|_2 + dp + dn + |bp| + |bn|, and c to 16 u X / 4.  The addend (c / d) e_k = c n_k, n = e / d, has the error
      delta c n_k  +  c delta e_k / d  -  c n_k delta d / d   <=   16 u [ (|c| + X / 4) |n_k| + |c| (A_k + |n_k| |A|_2) / d ],
    the bracket being its mass (15 of the 16: 4 for c's own roundings, 8 for d's, 3 for the product and the quotient; the A terms
    need 3).  It grows as 1 / d: the direction of a short difference of long rows is ill-conditioned, and the bound says so.  At
    d = 0 exactly the subgradient is 0 and the addend is reg r alone.  U[u], V[l] and T receive -c n_p + c n_n: both masses.  The
    biases receive +-c + reg b: mass |c| + X / 4 + reg |b|.  T's gradient has k = the surviving triples + 1 (reg T); its partial sums
    over idle wavefronts and skipped triples add exact zeros.

(c) Score rows, per element.  FPMC: each inner product within (dim + 16) u sum|a_k b_k|; the output within the two bounds plus one
    rounding of their sum.  TransRec: d within sqrt(sum_k (3 u A_k)^2) + (dim / 2 + 2) u d, A as in (b) with V[last] for V[l]; the
    output adds one rounding for + b[i].  A pair at distance exactly 0 scores b[i] bit for bit.

Checked on the CPU.  Every step and score case of this file is also run through an fp32 numpy restatement (_fp32_*: row sums
pairwise instead of lane-strided, addends accumulated row by row in reverse triple order instead of by atomics, T's gradient down the
batch) and held to the same bounds in the same run.  Its worst ratios to the bounds over all cases of the file:
  (a) FPMC gradients 0.095, loss words 0.141 (a triple alone, k = 1), totals over the slots 0.032;
  (b) TransRec gradients 0.075, loss words 0.114, totals 0.022;
  (c) FPMC scores 0.014, TransRec scores 0.067 (a sweep of 200 seeds x 4 widths, scales 1e-3 .. 10, zero distances: 0.106).
The kernels themselves, on the MI355X: (a) 0.095, 0.129, 0.045; (b) 0.075, 0.152, 0.027; (c) 0.028, 0.120.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gpu_utils import to_dev
from skrec import _hip

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

U24 = 2.0 ** -24
SENT = np.float32(-1.2345678e9)
GUARD = 64
f32, f64 = np.float32, np.float64
SEQ_WAVES, MAX_BLOCKS, SLOTS = 4, _hip.SKR_TRANSREC_MAX_BLOCKS, _hip.SKR_LOSS_SLOTS
TABLES = {"fpmc": ("UI", "IU", "IL", "LI"), "transrec": ("U", "V", "b", "T")}
WORST = {}               # (who, what) -> the worst error / bound of this process


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _at(t, off_floats):
    return t.data_ptr() + 4 * int(off_floats)


def _within(who, what, err, tol):
    err, tol = np.atleast_1d(err).astype(f64), np.atleast_1d(tol).astype(f64)
    assert np.all(np.isfinite(err)) and np.all(np.isfinite(tol)), (who, what, "not finite")
    if err.size:
        r = float(np.max(np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)))
        WORST[(who, what)] = max(WORST.get((who, what), 0.0), r)
        assert np.all(err <= tol), (who, what, r)


# ------------------------------------------------------------------------------------------------
# float64 restatements of the two steps
# ------------------------------------------------------------------------------------------------
class _Acc(object):
    """per gradient table: the float64 sum of its addends, their mass, the addends per element"""

    def __init__(self, **shapes):
        self.a = {k: [np.zeros(s), np.zeros(s), np.zeros(s, np.int64)] for k, s in shapes.items()}

    def add(self, name, rows, val, mag):
        d, m, k = self.a[name]
        if len(rows) == 0:
            return
        S = sp.csr_matrix((np.ones(len(rows)), (rows, np.arange(len(rows)))), shape=(d.shape[0], len(rows)))
        d += S @ val
        m += S @ mag
        k += np.bincount(rows, minlength=d.shape[0]).reshape((-1,) + (1,) * (d.ndim - 1))


def _survivors(u, l, p, q, nU, nI):
    ok = (u >= 0) & (u < nU) & (l >= 0) & (l < nI) & (p >= 0) & (p < nI) & (q >= 0) & (q < nI)
    idx = np.flatnonzero(ok)
    return (idx,) + tuple(a[idx].astype(np.int64) for a in (u, l, p, q))


def _fpmc_ref(c, u, l, p, q, reg):
    """x = (<UI[u], IU[p]> + <LI[l], IL[p]>) - (the same with n), l = logaddexp(0, -x), c = -exp(-logaddexp(0, x)); bound (a)"""
    idx, u, l, p, q = _survivors(u, l, p, q, c["nU"], c["nI"])
    reg = f64(f32(reg))
    UI, IU, IL, LI = (c[k].astype(f64) for k in TABLES["fpmc"])
    ui, li, iup, iun, ilp, iln = UI[u], LI[l], IU[p], IU[q], IL[p], IL[q]
    x = ((ui * iup).sum(1) + (li * ilp).sum(1)) - ((ui * iun).sum(1) + (li * iln).sum(1))
    X = (np.abs(ui) * (np.abs(iup) + np.abs(iun))).sum(1) + (np.abs(li) * (np.abs(ilp) + np.abs(iln))).sum(1)
    lo = np.logaddexp(0.0, -x)
    cf = -np.exp(-np.logaddexp(0.0, x))
    cc, sk, ab = cf[:, None], (np.abs(cf) + 0.25 * X)[:, None], np.abs
    acc = _Acc(gUI=UI.shape, gIU=IU.shape, gIL=IL.shape, gLI=LI.shape)
    acc.add("gUI", u, cc * (iup - iun) + reg * ui, sk * ab(iup - iun) + reg * ab(ui))
    acc.add("gLI", l, cc * (ilp - iln) + reg * li, sk * ab(ilp - iln) + reg * ab(li))
    acc.add("gIU", p, cc * ui + reg * iup, sk * ab(ui) + reg * ab(iup))
    acc.add("gIU", q, -cc * ui + reg * iun, sk * ab(ui) + reg * ab(iun))
    acc.add("gIL", p, cc * li + reg * ilp, sk * ab(li) + reg * ab(ilp))
    acc.add("gIL", q, -cc * li + reg * iln, sk * ab(li) + reg * ab(iln))
    l2 = 0.5 * sum((r ** 2).sum(1) for r in (ui, li, iup, iun, ilp, iln))
    return dict(acc=acc.a, idx=idx, lo=lo, lm=lo + X, l2=l2, once=0.0, x=x, cf=cf)


def _transrec_ref(c, u, l, p, q, reg):
    """t = (U[u] + T) + V[l], d_i = |t - V[i]|, x = (-d_p + b_p) - (-d_n + b_n); the subgradient of d at 0 is 0; bound (b)"""
    idx, u, l, p, q = _survivors(u, l, p, q, c["nU"], c["nI"])
    reg = f64(f32(reg))
    U, V, b, T = (c[k].astype(f64) for k in TABLES["transrec"])
    uu, vl, vp, vn, bp, bn, ab = U[u], V[l], V[p], V[q], b[p], b[q], np.abs
    t = (uu + T) + vl
    ep, en = t - vp, t - vn
    dp, dn = np.sqrt((ep ** 2).sum(1)), np.sqrt((en ** 2).sum(1))
    Ap, An = ab(uu) + ab(T) + ab(vl) + ab(vp), ab(uu) + ab(T) + ab(vl) + ab(vn)
    nAp, nAn = np.sqrt((Ap ** 2).sum(1)), np.sqrt((An ** 2).sum(1))
    x = (-dp + bp) - (-dn + bn)
    X = nAp + nAn + dp + dn + ab(bp) + ab(bn)
    lo = np.logaddexp(0.0, -x)
    cf = -np.exp(-np.logaddexp(0.0, x))
    sk = np.abs(cf) + 0.25 * X

    def unit(e, d, A, nA):
        """c e / d and its mass; both 0 at d == 0"""
        pos = (d > 0)[:, None]
        ds = np.where(d > 0, d, 1.0)[:, None]
        n = np.where(pos, e / ds, 0.0)
        mass = sk[:, None] * ab(n) + np.where(pos, ab(cf)[:, None] * (A + ab(n) * nA[:, None]) / ds, 0.0)
        return cf[:, None] * n, mass
    a_p, m_p = unit(ep, dp, Ap, nAp)
    a_n, m_n = unit(en, dn, An, nAn)
    g_t, m_t = -a_p + a_n, m_p + m_n
    acc = _Acc(gU=U.shape, gV=V.shape, gb=b.shape, gT=T.shape)
    acc.add("gU", u, g_t + reg * uu, m_t + reg * ab(uu))
    acc.add("gV", l, g_t + reg * vl, m_t + reg * ab(vl))
    acc.add("gV", p, a_p + reg * vp, m_p + reg * ab(vp))
    acc.add("gV", q, -a_n + reg * vn, m_n + reg * ab(vn))
    acc.add("gb", p, cf + reg * bp, sk + reg * ab(bp))
    acc.add("gb", q, -cf + reg * bn, sk + reg * ab(bn))
    acc.a["gT"] = [g_t.sum(0) + reg * T, m_t.sum(0) + reg * ab(T), np.full(T.shape, len(idx) + 1, np.int64)]      # reg T: once per batch
    l2 = 0.5 * (sum((r ** 2).sum(1) for r in (uu, vl, vp, vn)) + bp ** 2 + bn ** 2)
    return dict(acc=acc.a, idx=idx, lo=lo, lm=lo + X, l2=l2, once=0.5 * (T ** 2).sum(), x=x, cf=cf, dp=dp, dn=dn)


_REF = {"fpmc": _fpmc_ref, "transrec": _transrec_ref}


def _n_blocks(n):
    return min(-(-n // SEQ_WAVES), MAX_BLOCKS)


def _word_ref(ref, n, slots):
    """the loss words pair by pair: triple b is workgroup (b // 4) % blocks, which adds to pair g % slots; T's l2 to pair 0"""
    pair = ((ref["idx"] // SEQ_WAVES) % _n_blocks(n)) % slots
    D, M, K = np.zeros(2 * slots), np.zeros(2 * slots), np.zeros(2 * slots, np.int64)
    for w, val, mass in ((0, ref["lo"], ref["lm"]), (1, ref["l2"], ref["l2"])):
        np.add.at(D, 2 * pair + w, val)
        np.add.at(M, 2 * pair + w, mass)
        np.add.at(K, 2 * pair + w, 1)
    if ref["once"]:
        D[1] += ref["once"]
        M[1] += ref["once"]
        K[1] += 1
    return D, M, K


# ------------------------------------------------------------------------------------------------
# the fp32 restatements (another order of additions than the kernels') and the launches
# ------------------------------------------------------------------------------------------------
def _bpr_terms32(x):
    z = np.exp(-np.abs(x))
    lo = -(np.minimum(f32(0), x) - np.log1p(z))
    return lo, -np.where(x >= 0, z / (f32(1) + z), f32(1) / (f32(1) + z))


def _scatter32(g, rows, val):
    """g[rows] += val in fp32, row by row in reverse triple order"""
    n = len(rows)
    if n == 0:
        return
    S = sp.csr_matrix((np.ones(n, f32), (rows[::-1], np.arange(n))), shape=(g.shape[0], n))
    g += (S @ np.ascontiguousarray(val[::-1])).astype(f32)


def _fp32_step(kind, c, ids, n, reg, G0, layout, L0, slots, W0):
    idx, u, l, p, q = _survivors(*(a[:n] for a in ids), c["nU"], c["nI"])
    G, words, reg = G0.copy(), L0.copy(), f32(reg)
    g = {k: G[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in layout.items()}
    s32 = lambda a: a.sum(1, dtype=f32)  # noqa: E731
    once = f32(0)
    if kind == "fpmc":
        UI, IU, IL, LI = (c[k] for k in TABLES[kind])
        ui, li, iup, iun, ilp, iln = UI[u], LI[l], IU[p], IU[q], IL[p], IL[q]
        lo, cf = _bpr_terms32((s32(ui * iup) + s32(li * ilp)) - (s32(ui * iun) + s32(li * iln)))
        cc = cf[:, None]
        for name, rows, val in (("gUI", u, cc * (iup - iun) + reg * ui), ("gLI", l, cc * (ilp - iln) + reg * li),
                                ("gIU", p, cc * ui + reg * iup), ("gIU", q, -cc * ui + reg * iun),
                                ("gIL", p, cc * li + reg * ilp), ("gIL", q, -cc * li + reg * iln)):
            _scatter32(g[name], rows, val)
        l2 = f32(0.5) * sum(s32(r * r) for r in (ui, li, iup, iun, ilp, iln)) if len(idx) else np.zeros(0, f32)
    else:
        U, V, b, T = (c[k] for k in TABLES[kind])
        uu, vl, vp, vn, bp, bn = U[u], V[l], V[p], V[q], b[p], b[q]
        t = (uu + T) + vl
        ep, en = t - vp, t - vn
        dp, dn = np.sqrt(s32(ep * ep)), np.sqrt(s32(en * en))
        lo, cf = _bpr_terms32((-dp + bp) - (-dn + bn))
        with np.errstate(divide="ignore", invalid="ignore"):
            wp, wn = (np.where(d > 0, cf / d, f32(0))[:, None] for d in (dp, dn))
        g_t = -wp * ep + wn * en
        for name, rows, val in (("gU", u, g_t + reg * uu), ("gV", l, g_t + reg * vl), ("gV", p, wp * ep + reg * vp),
                                ("gV", q, -wn * en + reg * vn), ("gb", p, cf + reg * bp), ("gb", q, -cf + reg * bn)):
            _scatter32(g[name], rows, val)
        g["gT"] += g_t.sum(0, dtype=f32) + reg * T
        l2 = f32(0.5) * (sum(s32(r * r) for r in (uu, vl, vp, vn)) + bp * bp + bn * bn) if len(idx) else np.zeros(0, f32)
        once = f32(0.5) * (T * T).sum(dtype=f32)
    pair = ((idx // SEQ_WAVES) % _n_blocks(n)) % slots
    np.add.at(words, 2 * pair[::-1], lo.astype(f32)[::-1])
    np.add.at(words, 2 * pair[::-1] + 1, l2.astype(f32)[::-1])
    words[1] += once
    return G, words, None


def _launch_step(kind, c, ids, n, reg, G0, layout, L0, slots, W0):
    L, st = _hip.lib(), _hip.stream()
    G, dl = to_dev(G0), to_dev(L0)
    tabs = [to_dev(c[k]) for k in TABLES[kind]]
    dids = [to_dev(a) for a in ids]
    before = [t.clone() for t in tabs + dids]
    head = [_hip.ptr(t) for t in tabs + dids] + [n, c["nU"], c["nI"], c["dp"], reg]
    grads = [_at(G, o) for o, _ in layout.values()]
    if kind == "fpmc":
        W = None
        rc = L.skr_fpmc_step(*head, *grads, _hip.ptr(dl), slots, st)
    else:
        W = to_dev(W0)
        rc = L.skr_transrec_step(*head, *grads, _hip.ptr(W), _hip.ptr(dl), slots, st)
    _hip.check(rc)
    out = _host(G), _host(dl), None if W is None else _host(W)
    for t, t0 in zip(tabs + dids, before):
        assert torch.equal(t, t0)                                          # the inputs are only read
    return out


def _step(kind, c, ids, reg, slots=1, n=None, seed=0):
    """One launch on dirty buffers -- all gradients in one flat buffer, GUARD floats behind each -- compared with the float64
    restatement, after the fp32 restatement has been held to the same bounds:
      - an element with k > 0 addends is within (k + 16) u (mass + |start|) of start + the float64 sum; every other float of the
        buffer keeps its bits, and so does every padded column (its addends are zeros);
      - every loss word, pair by pair, likewise; the words behind them keep their bits;
      - TransRec: d_work started at SENT; afterwards one finite row per workgroup, SENT behind them."""
    ids = [np.ascontiguousarray(a, np.int32) for a in ids]
    n = len(ids[0]) if n is None else n
    rng = np.random.default_rng(7000 + seed)
    ref = _REF[kind](c, *(a[:n] for a in ids), reg)
    layout, off = {}, 0
    for name, (D, _, _) in ref["acc"].items():
        layout[name] = (off, D.shape)
        off += -(-D.size // 64) * 64 + GUARD
    G0 = (0.05 * rng.standard_normal(off)).astype(f32)
    G0[G0 == 0] = f32(0.05)
    L0 = (0.5 * rng.standard_normal(2 * slots + 2)).astype(f32)
    W0 = np.full(MAX_BLOCKS * c["dp"] + GUARD, SENT, f32)
    Dg, Mg, Kg = np.zeros(off), np.zeros(off), np.zeros(off, np.int64)
    pad = np.zeros(off, bool)
    for name, (o, s) in layout.items():
        for dst, src in zip((Dg, Mg, Kg), ref["acc"][name]):
            dst[o:o + src.size] = src.reshape(-1)
        if len(s) == 2 or name == "gT":
            cols = np.zeros(s, bool)
            cols[..., c["width"]:] = True
            pad[o:o + cols.size] = cols.reshape(-1)
    assert not Dg[pad].any() and not Mg[pad].any()
    Dw, Mw, Kw = _word_ref(ref, n, slots)
    runs = {}
    for who, fn in (("fp32", _fp32_step), ("kernel", _launch_step)):
        G, words, W = fn(kind, c, ids, n, reg, G0, layout, L0, slots, W0)
        hit = Kg > 0
        assert np.array_equal(_bits(G)[~hit], _bits(G0)[~hit]), (who, "a float outside the batch's rows changed")
        assert np.array_equal(_bits(G)[pad], _bits(G0)[pad]), (who, "a padded column changed")
        _within(who, kind + " gradients", np.abs(G.astype(f64) - (G0.astype(f64) + Dg))[hit], ((Kg + 16) * U24 * (Mg + np.abs(G0)))[hit])
        hw = Kw > 0
        assert _same(words[2 * slots:], L0[2 * slots:]), (who, "guard words behind the loss words")
        assert np.array_equal(_bits(words[:2 * slots])[~hw], _bits(L0[:2 * slots])[~hw]), (who, "a pair without a workgroup changed")
        w0 = L0[:2 * slots].astype(f64)
        _within(who, kind + " loss words", np.abs(words[:2 * slots].astype(f64) - (w0 + Dw))[hw], ((Kw + 16) * U24 * (Mw + np.abs(w0)))[hw])
        if W is not None:
            used = _n_blocks(n) * c["dp"]
            assert np.all(np.isfinite(W[:used])) and not np.any(W[:used] == SENT), (who, "d_work: a workgroup's partial is missing")
            assert _same(W[used:], W0[used:]), (who, "d_work beyond the grid")
        runs[who] = dict(g={k: G[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in layout.items()}, words=words)
    return dict(ref=ref, runs=runs, G0={k: G0[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in layout.items()}, L0=L0,
                words=(Dw, Mw, Kw))


def _make_tables(kind, rng, nU, nI, dim, width, scale=0.2):
    """rows of `width` floats, zero-padded to dim; T in multiples of 1 / 256, so that tests can place rows at exact distances"""
    def r(rows):
        out = np.zeros((rows, dim), f32)
        out[:, :width] = scale * rng.standard_normal((rows, width))
        return out
    c = dict(nU=nU, nI=nI, dp=dim, width=width)
    if kind == "fpmc":
        c.update(UI=r(nU), IU=r(nI), IL=r(nI), LI=r(nI))
    else:
        c.update(U=r(nU), V=r(nI), b=(scale * rng.standard_normal(nI)).astype(f32), T=(np.round(r(1)[0] * 256) / 256).astype(f32))
    return c


def _triples(rng, n, users, items):
    """users / items: (lo, hi) ranges; repeated rows everywhere, some triples with n == l and with p == n"""
    u = rng.integers(*users, n).astype(np.int32)
    l, p, q = (rng.integers(*items, n).astype(np.int32) for _ in range(3))
    q[::7] = l[::7]
    q[3::11] = p[3::11]
    return [u, l, p, q]


# ------------------------------------------------------------------------------------------------
# 1. every width, the batch lengths where the loops change shape
# ------------------------------------------------------------------------------------------------
NARROW = {64: 50, 128: 100, 192: 130, 256: 250}
STEP_CASES = ([(d, NARROW[d], n) for d in (64, 192) for n in (1, 3, 5, 61, 253, 268, 4099)] +
              [(d, NARROW[d], n) for d in (128, 256) for n in (1, 5, 4099)] + [(d, d, 5) for d in (64, 128, 192, 256)])


def _step_case(kind, dim, width, n):
    rng = np.random.default_rng(dim * 10000 + width * 7 + n)
    nU, nI = (37, 23) if n < 1000 else (40, 80)
    c = _make_tables(kind, rng, nU, nI, dim, width)
    return _step(kind, c, _triples(rng, n, (0, nU), (0, nI)), 1e-2, slots=SLOTS if n in (61, 4099) else 1, seed=n)


@pytest.mark.parametrize("dim,width,n", STEP_CASES)
def test_fpmc_step_widths_and_batch_lengths(dim, width, n):
    """n = 1 and 3: one workgroup with idle wavefronts; 5: two workgroups; 4099: 1024 workgroups, three wavefronts of the first take
    a second triple; every dim at a width that is no multiple of 64 and, at n = 5, at its full width"""
    r = _step_case("fpmc", dim, width, n)
    assert len(r["ref"]["idx"]) == n


@pytest.mark.parametrize("dim,width,n", STEP_CASES)
def test_transrec_step_widths_and_batch_lengths(dim, width, n):
    """as above; transrec_t_kernel adds 1, 1, 2, 16 (exactly T_WAVES), 64 (exactly one 4-deep trip), 67 (a trip and a remainder for
    three wavefronts) and 1024 partials; the idle wavefronts of n = 1 and 3 must write zero rows into their workgroup's partial (d_work
    starts at SENT: a wavefront that skipped its s_dt row, or a partial that was not written, shows in gT)"""
    r = _step_case("transrec", dim, width, n)
    assert len(r["ref"]["idx"]) == n and (r["ref"]["acc"]["gT"][2] == n + 1).all()


# ------------------------------------------------------------------------------------------------
# 2. out-of-range triples
# ------------------------------------------------------------------------------------------------
def _bad_value(col, k, nU, nI):
    return -1 if k % 2 == 0 else (nU if col == 0 else nI)


@pytest.mark.parametrize("dim,width", [(64, 50), (192, 130)])
@pytest.mark.parametrize("kind", ["fpmc", "transrec"])
def test_step_skips_out_of_range_triples(kind, dim, width):
    """one triple in five has exactly one bad id: each of u, l, p, n in turn, -1 and the table's length.  The restatement drops those
    triples; their good ids name rows (users 0 - 1, items 0 - 5) that no other triple names, which must keep their bits."""
    rng = np.random.default_rng(dim + len(kind))
    nU, nI, n = 30, 50, 80
    c = _make_tables(kind, rng, nU, nI, dim, width)
    ids = _triples(rng, n, (2, nU), (6, nI))
    for k, b in enumerate(range(2, n, 5)):                     # 16 triples: every (id, side) twice
        col = (k // 2) % 4
        ids[0][b] = rng.integers(0, 2)
        for a in ids[1:]:
            a[b] = rng.integers(0, 6)
        ids[col][b] = _bad_value(col, k, nU, nI)
    r = _step(kind, c, ids, 1e-2, seed=dim)
    assert len(r["ref"]["idx"]) == n - 16
    acc = r["ref"]["acc"]
    for name, rows in (("gUI", 2), ("gIU", 6), ("gIL", 6), ("gLI", 6)) if kind == "fpmc" else (("gU", 2), ("gV", 6), ("gb", 6)):
        assert not acc[name][2][:rows].any() and acc[name][2][rows:].any()


@pytest.mark.parametrize("dim,width", [(64, 50), (192, 130)])
@pytest.mark.parametrize("kind", ["fpmc", "transrec"])
def test_step_with_every_triple_out_of_range(kind, dim, width):
    """n = 9 > 0 and no triple survives: no row gradient and no word of the loss changes; TransRec's T still gets reg * T and the
    l2 word its 1/2 |T|^2 -- "T once per batch" is per launch, not per surviving batch: the documented behaviour"""
    rng = np.random.default_rng(dim + 3 * len(kind))
    nU, nI, n = 9, 7, 9
    c = _make_tables(kind, rng, nU, nI, dim, width)
    ids = _triples(rng, n, (0, nU), (0, nI))
    for b in range(n):
        ids[b % 4][b] = _bad_value(b % 4, b // 4, nU, nI)
    r = _step(kind, c, ids, 1e-2, seed=dim)
    assert len(r["ref"]["idx"]) == 0
    for who, run in r["runs"].items():
        for name, g in run["g"].items():
            assert name == "gT" or _same(g, r["G0"][name]), (who, name)
        assert _bits(run["words"][0]) == _bits(r["L0"][0]), who
        if kind == "fpmc":
            assert _same(run["words"], r["L0"]), who
        else:
            T = c["T"].astype(f64)
            assert np.allclose(r["ref"]["acc"]["gT"][0], f64(f32(1e-2)) * T, rtol=1e-12, atol=0)
            assert np.isclose(r["words"][0][1], 0.5 * (T ** 2).sum(), rtol=1e-12) and r["words"][0][1] > 0.1
            assert not _same(run["g"]["gT"][:width], r["G0"]["gT"][:width]) and run["words"][1] != r["L0"][1], who


# ------------------------------------------------------------------------------------------------
# 3. loss slots
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 700])
@pytest.mark.parametrize("kind", ["fpmc", "transrec"])
def test_step_loss_slots_pair_by_pair(kind, n):
    """SKR_LOSS_SLOTS pairs with 2 workgroups (30 pairs keep their bits) and with 175: _step holds every pair to the restatement of
    the workgroups g % 32 == its index -- T's l2 term counted in word 1 of pair 0 and nowhere else -- and the pairs without a
    workgroup to their bits.  The totals, and the totals of the same batch with one slot, agree within the bound."""
    rng = np.random.default_rng(n + len(kind))
    nU, nI = 40, 60
    c = _make_tables(kind, rng, nU, nI, 64, 50)
    ids = _triples(rng, n, (0, nU), (0, nI))
    r32 = _step(kind, c, ids, 1e-2, slots=SLOTS, seed=n)
    r1 = _step(kind, c, ids, 1e-2, slots=1, seed=n + 1)
    (D32, M32, K32), (D1, M1, K1) = r32["words"], r1["words"]
    assert (K32[0::2] > 0).sum() == min(SLOTS, -(-n // SEQ_WAVES)) and K32[0::2].sum() == n == K1[0]
    if kind == "transrec":
        once = r32["ref"]["once"]
        assert K32[1] == K32[0] + 1 and (K32[3::2] == K32[2::2]).all() and K1[1] == n + 1
        assert once > 1000 * (K32[1] + 16) * U24 * (M32[1] + 1.0)          # T's term in another word would break that word's bound
    for w in (0, 1):
        assert np.isclose(D32[w::2].sum(), D1[w], rtol=1e-12)
        for who in r32["runs"]:
            got32, start32 = r32["runs"][who]["words"][w:2 * SLOTS:2], r32["L0"][w:2 * SLOTS:2]
            used = K32[w::2] > 0
            assert np.all(_bits(got32)[used] != _bits(start32)[used]), (who, "a pair with a workgroup did not change")
            add32 = (got32.astype(f64) - start32.astype(f64)).sum()
            add1 = f64(r1["runs"][who]["words"][w]) - f64(r1["L0"][w])
            t32 = (n + 17) * U24 * (M1[w] + np.abs(start32).sum())
            t1 = (n + 17) * U24 * (M1[w] + abs(f64(r1["L0"][w])))
            _within(who, kind + " loss totals", abs(add32 - D1[w]), t32)
            _within(who, kind + " loss totals", abs(add32 - add1), t32 + t1)


# ------------------------------------------------------------------------------------------------
# 4. margins and distances at the edges
# ------------------------------------------------------------------------------------------------
def _reg_row_exactly(r, name, row, table_row, reg):
    """the gradient row received one addend and that addend was reg * row: one fp32 product, one fp32 addition to the start"""
    want = r["G0"][name][row] + f32(reg) * table_row
    for who, run in r["runs"].items():
        assert _same(run["g"][name][row], want.astype(f32)), (who, name, row)


MARGINS = [0.0, 2.0 ** -20, -2.0 ** -20, 30.0, -30.0, 90.0, -90.0, 120.0, -120.0]


@pytest.mark.parametrize("dim,width", [(64, 64), (128, 100), (192, 130), (256, 256)])
def test_fpmc_margins_at_the_edges(dim, width):
    """Triple b < 9 has user b and items 3b, 3b + 1, 3b + 2 to itself (p == n for b = 0) inside a random batch on the other rows.
    Its margin is exact: UI[u] = e_k1, LI[l] = e_k2, IU[p]_k1 = IL[p]_k2 = x / 4 and -x / 4 for n, random multiples of 1 / 256
    elsewhere (they meet zeros).  In fp32 as in float64: c = -1/2 at x = 0, -z / (1 + z) for x > 0, -1 / (1 + z) for x < 0;
    at +120 z = expf(-120) = 0, so l = 0 and c = 0: the six rows get reg * row exactly; at -120 l = 120, c = -1.
    The batch as a whole and every edge triple alone (n = 1: its loss word to 17 u (l + X)) are within the bound."""
    rng = np.random.default_rng(dim)
    nU, nI, E, reg = 40, 80, len(MARGINS), 1e-2
    c = _make_tables("fpmc", rng, nU, nI, dim, width)
    k1, k2 = width - 1, width // 2
    ids = _triples(rng, E + 40, (E, nU), (3 * E, nI))
    for b, x in enumerate(MARGINS):
        u, l, p, q = b, 3 * b, 3 * b + 1, 3 * b + (2 if b else 1)
        for a, v in zip(ids, (u, l, p, q)):
            a[b] = v
        if b == 0:
            continue
        for t in ("IU", "IL"):
            c[t][[p, q], :width] = np.round(c[t][[p, q], :width] * 256) / 256
        c["UI"][u], c["LI"][l] = 0.0, 0.0
        c["UI"][u, k1], c["LI"][l, k2] = 1.0, 1.0
        c["IU"][p, k1], c["IL"][p, k2], c["IU"][q, k1], c["IL"][q, k2] = x / 4, x / 4, -x / 4, -x / 4
    r = _step("fpmc", c, ids, reg, seed=dim)
    ref = r["ref"]
    assert np.array_equal(ref["x"][:E], np.array(MARGINS))
    assert ref["cf"][0] == -0.5 and ref["cf"][8] == -1.0 and abs(ref["cf"][7]) < 1e-50 and abs(ref["lo"][8] - 120) < 1e-12
    assert np.allclose(ref["cf"][[3, 4]], [-np.exp(-30.0), -1.0], rtol=1e-12)           # z / (1 + z) against 1 / (1 + z)
    b = 7                                                       # x = +120
    for name, row, tab in (("gUI", b, "UI"), ("gLI", 3 * b, "LI"), ("gIU", 3 * b + 1, "IU"), ("gIU", 3 * b + 2, "IU"),
                           ("gIL", 3 * b + 1, "IL"), ("gIL", 3 * b + 2, "IL")):
        _reg_row_exactly(r, name, row, c[tab][row], reg)
    _reg_row_exactly(r, "gUI", 0, c["UI"][0], reg)              # p == n: IU[p] - IU[n] = 0
    for name, tab in (("gIU", "IU"), ("gIL", "IL")):            # ... and the mirrored addends of the item row cancel
        assert np.allclose(ref["acc"][name][0][1], 2 * f64(f32(reg)) * c[tab][1].astype(f64), rtol=1e-9, atol=1e-18)
    for b in range(E):
        one = _step("fpmc", c, [a[b:b + 1] for a in ids], reg, seed=dim + b)
        assert one["ref"]["x"][0] == MARGINS[b]


@pytest.mark.parametrize("dim,width", [(64, 64), (128, 100), (192, 130), (256, 256)])
def test_transrec_distances_at_the_edges(dim, width):
    """Triple b < 6 has user b and items 3b .. 3b + 2 to itself inside a random batch on the other rows.  U[u], V[l] and T are
    multiples of 1 / 256, so t = (U[u] + T) + V[l] is exact and a row set to t lies at distance exactly 0, in fp32 as in float64:
      0: dp == 0, dn > 0      V[p] gets reg * V[p] exactly
      1: dn == 0, dp > 0      V[n] gets reg * V[n] exactly
      2: dp == dn == 0, p != n: x = b_p - b_n, U[u], V[l], V[p], V[n] get reg * row exactly, the biases +-c + reg b
      3: p == n               x == 0 exactly, c = -1/2, the mirrored addends of V[p] cancel to 2 reg V[p], U[u] gets reg U[u]
      4, 5: x ~ +-90 through the biases (expf's denormal range)
    An unconditional c / d is NaN at 0, 1 and 2."""
    rng = np.random.default_rng(dim + 1)
    nU, nI, E, reg = 40, 80, 6, 1e-2
    c = _make_tables("transrec", rng, nU, nI, dim, width)
    ids = _triples(rng, E + 40, (E, nU), (3 * E, nI))
    for b in range(E):
        u, l, p, q = b, 3 * b, 3 * b + 1, 3 * b + (1 if b == 3 else 2)
        for a, v in zip(ids, (u, l, p, q)):
            a[b] = v
        if b < 3:
            c["U"][u], c["V"][l] = np.round(c["U"][u] * 256) / 256, np.round(c["V"][l] * 256) / 256
            t = (c["U"][u] + c["T"]) + c["V"][l]
            for row in ((p,), (q,), (p, q))[b]:
                c["V"][row] = t
    c["b"][[13, 14, 16, 17]] = [45.25, -45.25, -45.25, 45.25]
    r = _step("transrec", c, ids, reg, seed=dim)
    ref = r["ref"]
    dp, dn, x = ref["dp"][:E], ref["dn"][:E], ref["x"][:E]
    assert dp[0] == 0 < dn[0] and dn[1] == 0 < dp[1] and dp[2] == 0 == dn[2] and dp[3] == dn[3] > 0 and x[3] == 0 and ref["cf"][3] == -0.5
    assert x[2] == f64(c["b"][7]) - f64(c["b"][8]) and 80 < x[4] < 100 and -100 < x[5] < -80
    _reg_row_exactly(r, "gV", 1, c["V"][1], reg)
    _reg_row_exactly(r, "gV", 5, c["V"][5], reg)
    for name, row, tab in (("gU", 2, "U"), ("gV", 6, "V"), ("gV", 7, "V"), ("gV", 8, "V")):
        _reg_row_exactly(r, name, row, c[tab][row], reg)
    assert np.allclose(ref["acc"]["gV"][0][10], 2 * f64(f32(reg)) * c["V"][10].astype(f64), rtol=1e-9, atol=1e-18)
    assert np.allclose(ref["acc"]["gU"][0][3], f64(f32(reg)) * c["U"][3].astype(f64), rtol=1e-9, atol=1e-18)
    want = (ref["cf"][2] + f64(f32(reg)) * c["b"][7], -ref["cf"][2] + f64(f32(reg)) * c["b"][8])
    assert np.allclose(ref["acc"]["gb"][0][[7, 8]], want, rtol=1e-12)
    for b in range(E):
        _step("transrec", c, [a[b:b + 1] for a in ids], reg, seed=dim + b)


# ------------------------------------------------------------------------------------------------
# 5. score rows
# ------------------------------------------------------------------------------------------------
def _scores_ref(mode, c, users, last):
    """float64 scores of valid users and bound (c), per element"""
    dim, ab = c["dp"], np.abs
    if mode == "fpmc":
        UI, IU, IL, LI = (c[k].astype(f64) for k in TABLES[mode])
        a, b = UI[users] @ IU.T, LI[last] @ IL.T
        ta, tb = ((dim + 16) * U24 * m for m in (ab(UI[users]) @ ab(IU).T, ab(LI[last]) @ ab(IL).T))
        return a + b, ta + tb + U24 * (ab(a + b) + ta + tb)
    U, V, bias, T = (c[k].astype(f64) for k in TABLES[mode])
    t = (U[users] + T) + V[last]
    d = np.sqrt(((t[:, None, :] - V[None]) ** 2).sum(-1))
    A = (ab(U[users]) + ab(T) + ab(V[last]))[:, None, :] + ab(V)[None]
    td = 3 * U24 * np.sqrt((A ** 2).sum(-1)) + (dim / 2 + 2) * U24 * d
    return -d + bias, td + U24 * (ab(-d + bias) + td)


def _fp32_scores(mode, c, users, B, last, ld, out0):
    out, nI = out0.copy(), c["nI"]
    for r in range(B):
        u = users[r]
        l = last[u] if 0 <= u < c["nU"] else -1
        if not 0 <= l < nI:
            out[r, :nI] = np.nan
        elif mode == "fpmc":
            out[r, :nI] = c["IU"] @ c["UI"][u] + c["IL"] @ c["LI"][l]
        else:
            e = ((c["U"][u] + c["T"]) + c["V"][l])[None] - c["V"]
            out[r, :nI] = -np.sqrt((e * e).sum(1, dtype=f32)) + c["b"]
    return out


def _launch_scores(mode, c, users, B, last, ld, out0):
    tabs = {k: to_dev(c[k]) for k in TABLES[mode]}
    du, dl, out = to_dev(users), to_dev(last), to_dev(out0)
    p = lambda k: _hip.ptr(tabs[k])  # noqa: E731
    if mode == "fpmc":
        head = (_hip.SKR_SEQ_FPMC, p("UI"), p("LI"), p("IU"), p("IL"), None, None)
    else:
        head = (_hip.SKR_SEQ_TRANSREC, p("U"), p("V"), p("V"), None, p("T"), p("b"))
    _hip.check(_hip.lib().skr_seq_scores(*head, _hip.ptr(du), B, _hip.ptr(dl), c["nU"], c["nI"], c["dp"], _hip.ptr(out), ld,
                                         _hip.stream()))
    return _host(out)


def _scores(mode, c, users, last, ld, exact=()):
    """rows of bad users are NaN in every column, every other element is within bound (c), the rows beyond B and the columns beyond
    n_items keep their bits; `exact`: (row, item) pairs at distance exactly 0, which score b[item] bit for bit"""
    users, last = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(last, np.int32)
    B, nI = len(users), c["nI"]
    out0 = np.full((B + 2, ld), SENT, f32)
    lu = np.where((users >= 0) & (users < c["nU"]), last[np.clip(users, 0, c["nU"] - 1)], -1)
    ok = (lu >= 0) & (lu < nI)
    want, tol = _scores_ref(mode, c, users[ok], lu[ok])
    for who, fn in (("fp32", _fp32_scores), ("kernel", _launch_scores)):
        got = fn(mode, c, users, B, last, ld, out0)
        assert _same(got[B:], out0[B:]) and _same(got[:, nI:], out0[:, nI:]), (who, "a float outside the score rows changed")
        assert np.isnan(got[:B, :nI][~ok]).all(), who
        _within(who, mode + " scores", np.abs(got[:B, :nI][ok].astype(f64) - want), tol)
        for row, item in exact:
            assert _bits(got[row, item]) == _bits(c["b"][item]), (who, row, item)
    return int(ok.sum())


QB = {"fpmc": 16, "transrec": 32}


@pytest.mark.parametrize("dim,width", [(64, 50), (128, 128), (192, 130), (256, 250)])
@pytest.mark.parametrize("mode", ["fpmc", "transrec"])
def test_seq_scores_blocks_tiles_and_bad_rows(mode, dim, width):
    """B = 1, QB and QB + 1 (QB = 16 users per workgroup for FPMC, 32 for TransRec) x n_items = 1, 255, 256, 257 (256 items per
    workgroup), ld == n_items and ld == n_items + 3 alternating, table scales 1e-3 .. 10.  User 0 has no last item (-1), user 1 the
    last item n_items; the list holds them, the ids -1 and n_users, and duplicates.  With B = 1 each kind of user is asked alone.
    TransRec: V[iz] = (U[2] + T) + V[last[2]] in multiples of 1 / 256: user 2 scores b[iz] on item iz."""
    nU, k = 12, 0
    for B in (1, QB[mode], QB[mode] + 1):
        for nI in (1, 255, 256, 257):
            rng = np.random.default_rng(dim * 1000 + B * 10 + nI + (mode == "fpmc"))
            c = _make_tables(mode, rng, nU, nI, dim, width, scale=(1e-3, 0.1, 1.0, 10.0)[k % 4])
            ld = nI + 3 * (k % 2)
            k += 1
            last = rng.integers(0, nI, nU).astype(np.int32)
            last[0], last[1] = -1, nI
            exact = []
            if mode == "transrec":
                iz = nI // 2
                last[2] = (iz + 1) % nI
                q = lambda a: (np.round(a * 256) / 256).astype(f32)  # noqa: E731
                if nI == 1:
                    c["V"][0] = q(c["V"][0])
                    c["U"][2] = -c["T"]                              # (U + T) + V[0] == V[0]
                else:
                    c["U"][2], c["V"][last[2]] = q(c["U"][2]), q(c["V"][last[2]])
                    c["V"][iz] = (c["U"][2] + c["T"]) + c["V"][last[2]]
            if B == 1:
                for u, n_ok in ((2, 1), (0, 0), (1, 0), (-1, 0), (nU, 0)):
                    assert _scores(mode, c, [u], last, ld, exact=[(0, iz)] if mode == "transrec" and u == 2 else ()) == n_ok
                continue
            users = rng.integers(2, nU, B).astype(np.int32)
            users[[0, 1, 2, 3, 4, 5, 6]] = [2, 5, 5, 0, 1, -1, nU]
            users[B - 1] = 2                                         # the last row: in a query block of its own when B = QB + 1
            if mode == "transrec":
                exact = [(0, iz), (B - 1, iz)]
            assert _scores(mode, c, users, last, ld, exact=exact) == B - 4


# ------------------------------------------------------------------------------------------------
# 6. wide rows through the models
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("embed_size", [100, 130, 256])
@pytest.mark.parametrize("name", ["FPMC", "TransRec"])
def test_models_train_wide_rows(seq_dir, monkeypatch, tmp_path, name, embed_size):
    """rows of 128, 192 and 256 floats: _seq.py steps them with one dense Adam launch per batch.  After one epoch at batch_size 64
    every padded column of the parameters, of Adam's m and v and of the gradient is exactly zero, the gradient buffer is all zero
    (every step consumed it), predict() equals the float64 scores of the model's own tables within bound (c), and step_losses has
    one finite row per batch."""
    from test_gpu_seq import _model
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SKR_ADAM_BLOCK", raising=False)
    m = _model(name, seq_dir, embed_size=embed_size, batch_size=64, epochs=1)
    e, d, nu, ni = embed_size, 64 * ((embed_size + 63) // 64), m.num_users, m.num_items
    assert m.dp == d and m.adam_block == 1
    before = m.optimizer.flat.clone()
    m.fit()
    torch.cuda.synchronize()
    o = m.optimizer
    assert not torch.equal(before, o.flat) and o.t > 1
    rows = (nu, ni, ni, ni) if name == "FPMC" else (nu, ni)
    pad = torch.zeros(o.flat.numel(), dtype=torch.bool)
    for off, n in zip(m._off, rows):
        pad[off:off + n * d].view(n, d)[:, e:] = True
    if name == "TransRec":
        pad[m._off[2] + ni:m._off[3]] = True                     # the bias block's padding
        pad[m._off[3] + e:m._off[3] + d] = True                  # T's
        assert m._off[3] + d == o.flat.numel()
    assert int(pad.sum()) == sum(rows) * (d - e) + (0 if name == "FPMC" else m._off[3] - m._off[2] - ni + d - e)
    for what, t in (("flat", o.flat), ("m", o.m), ("v", o.v), ("grad", o.grad)):
        assert not t.cpu()[pad].any(), what
        assert bool(torch.isfinite(t).all()), what
    assert not o.grad.any()
    assert o.m.cpu()[~pad].any() and o.v.cpu()[~pad].any()
    losses = m.step_losses.cpu().numpy()
    assert losses.shape == (len(m._make_iterator().epoch_columns()[1]), 2) and losses.shape[0] > 1
    assert np.all(np.isfinite(losses)) and np.all(losses > 0)
    users = np.flatnonzero(m._last_host >= 0)[[0, 1, -1]].astype(np.int32)
    mode = name.lower()
    names = ("UI", "IU", "IL", "LI") if name == "FPMC" else ("U", "V")
    c = dict(nU=nu, nI=ni, dp=d, width=e)
    for k, off, n in zip(names, m._off, rows):
        c[k] = o.flat[off:off + n * d].view(n, d).cpu().numpy()
    if name == "TransRec":
        c["b"], c["T"] = m._bias.cpu().numpy(), m._T.cpu().numpy()
    want, tol = _scores_ref(mode, c, users, m._last_host[users])
    got = m.predict(list(users))
    assert got.shape == (3, ni)
    _within("kernel", mode + " scores", np.abs(got.astype(f64) - want), tol)


@pytest.fixture()
def seq_dir(tmp_path, golden):
    from test_gpu_seq import _write_set
    return _write_set(golden("tiny_seq_dataset"), tmp_path / "tiny_seq")
