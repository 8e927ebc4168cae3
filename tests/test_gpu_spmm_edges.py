"""The SpMM plan (csrc/spmm.hip) at its edges: every path of the plan at the smallest shape that reaches it, with the path
NAMED -- a plain-Python restatement of the plan's hot-row selection says how many long rows, hot rows and tasks a matrix
must give, and every case asserts those numbers through skr_spmm_plan_info before it compares a product.

Exact inputs: val, X, addend and the initial accum hold integers in [-3, 3] (val: never 0), accum_scale is a power of two and
no row has more than 4096 entries, so every partial sum is an integer below 2^24 and exact in fp32 in ANY order: the
expected value is the float64 product, compared with np.array_equal.  One lost, doubled or misplaced entry changes a row by
at least 1.  Only the refinement epilogues use float inputs, with the bounds of test_gpu_train.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
HERE = os.path.dirname(os.path.abspath(__file__))
HOT_UB, HOT_V, TASK = 128, 128, 256
SWITCHES = ("SKR_SPMM_HOT", "SKR_SPMM_HOT_PF", "SKR_SPMM_TASK_SPAN", "SKR_SPMM_ROWS_WGS", "SKR_SPMM_TASK_WGS", "SKR_SPMM_HOT_WGS",
            "SKR_SPMM_HOT_DENSITY", "SKR_SPMM_CBLK", "SKR_SPMM_WINDOWS")


# ---------------------------------------------------------------------------------------------------------------------
# the plan, restated (include/skrec_hip.h on skr_spmm_plan_info, the comments of skr_spmm_plan_create)
# ---------------------------------------------------------------------------------------------------------------------
def default_cblk(n_cols):
    if n_cols < 8 * 256:
        return 16384
    nb = 8 * max(1, (n_cols + 4 * 28672) // (8 * 28672))
    return max((-(-n_cols // nb) + 63) // 64 * 64, 2048)


def restate(rows, n_cols, long_from, cblk=None, dens=4.0):
    """what the plan must hold: long rows (>= long_from entries); hot rows = the long rows with >= dens entries per 128 columns on
    average, densest first (ties: lower row first), at most 96 candidates, each cut into clamp(ceil(deg / (total / 64)), 1, 8)
    pieces, the selection stopping at the first candidate that would pass 128 virtual rows; tasks = one per 256 entries of
    every (long row, column block) segment, the hot rows' included; chunks = the virtual rows four at a time by load"""
    thr = long_from or 512
    cblk = cblk or default_cblk(n_cols)
    deg = [len(r) for r in rows]
    long_rows = [r for r in range(len(rows)) if deg[r] >= thr]
    hot, virt = [], []
    if dens > 0 and n_cols >= HOT_UB:
        cand = sorted((r for r in long_rows if deg[r] >= dens * n_cols / HOT_UB), key=lambda r: (-deg[r], r))[:96]
        total = float(sum(deg[r] for r in cand))
        for r in cand:
            pieces = min(8, max(1, math.ceil(deg[r] / (total / 64.0))))
            if len(virt) + pieces > HOT_V:
                break
            virt += [(r, q, pieces) for q in range(pieces)]
            hot.append(r)
    order = sorted(range(len(virt)), key=lambda q: -deg[virt[q][0]] / virt[q][2])      # (sorted() is stable, like the plan's sort)
    chunks = [[virt[q] for q in order[c:c + 4]] for c in range(0, len(order), 4)]
    begs = []                                                                          # first entry of every task, per row
    for r in long_rows:
        seg = np.bincount(np.asarray(rows[r]) // cblk, minlength=1)
        starts = np.concatenate([[0], np.cumsum(seg)])[:-1]
        begs.append((r, [int(s + t) for s, n in zip(starts, seg) for t in range(0, int(n), TASK)]))
    return dict(long=len(long_rows), hot=hot, virt=virt, chunks=chunks, tasks=sum(len(b) for _, b in begs), begs=begs,
                blocks=-(-n_cols // cblk), thr=thr)


def ints(rng, shape, zero=True):
    a = rng.integers(-3, 4, shape)
    if not zero:
        a = np.where(a == 0, 3, a)
    return a.astype(np.float32)


def pick(rng, n_cols, k, lo=0, hi=None):
    hi = n_cols if hi is None else hi
    return np.sort(rng.choice(np.arange(lo, hi), k, replace=False))


def extras(rng, n_cols, long_from, under):
    """beside every case's own rows: short rows of every length below the threshold, an empty row, and a long row that stays
    under the hot threshold (`under` entries)"""
    return [pick(rng, n_cols, k) for k in range(1, long_from)] + [np.zeros(0, np.int64), pick(rng, n_cols, under), pick(rng, n_cols, 1)]


class Plan:
    """a CSR on the device, its plan, the float64 matrix; the plan's numbers are compared with the restatement's at once"""

    def __init__(self, name, rows, n_cols, long_from, rng, cblk=None, expect_hot=None, val=None):
        import torch  # noqa: F401
        from gpu_utils import to_dev
        from skrec import _hip
        self.L, self.rows, self.n_rows, self.n_cols = _hip.lib(), rows, len(rows), n_cols
        assert max(len(r) for r in rows) <= 4096
        self.rowptr = np.zeros(self.n_rows + 1, np.int64)
        self.rowptr[1:] = np.cumsum([len(r) for r in rows])
        self.col = np.concatenate(list(rows) + [np.zeros(0, np.int64)]).astype(np.int32)
        self.nnz = len(self.col)
        self.val = ints(rng, self.nnz, zero=False) if val is None else val
        self.A = sp.csr_matrix((self.val.astype(np.float64), self.col, self.rowptr), shape=(self.n_rows, n_cols))
        self.dev = [to_dev(self.rowptr), to_dev(self.col), to_dev(self.val)]
        self.h = C.c_void_p()
        _hip.check(self.L.skr_spmm_plan_create(self.n_rows, n_cols, *(_hip.ptr(t) for t in self.dev), self.nnz, long_from, C.byref(self.h),
                                               _hip.stream()))
        info = (C.c_int64 * 4)()
        _hip.check(self.L.skr_spmm_plan_info(self.h, info))
        self.want = w = restate(rows, n_cols, long_from, cblk)
        got = dict(long=int(info[0] & 0xffffffff), hot=int(info[0] >> 32), tasks=int(info[1]), blocks=int(info[2]), thr=int(info[3] & 0xffffffff))
        print(f"{name}: plan {got}; restatement long={w['long']} hot={len(w['hot'])} virtual={len(w['virt'])} tasks={w['tasks']} "
              f"blocks={w['blocks']} pieces={sorted({p for _, _, p in w['virt']})}")
        assert got == dict(long=w["long"], hot=len(w["hot"]), tasks=w["tasks"], blocks=w["blocks"], thr=w["thr"]), (got, w)
        if expect_hot is not None:
            assert len(w["hot"]) == expect_hot, (len(w["hot"]), expect_hot)

    def close(self):
        from skrec import _hip
        _hip.check(self.L.skr_spmm_plan_destroy(self.h))

    def lists(self, ub):
        """restated: the length of every virtual row's list in X block ub"""
        out = {}
        for r, q, p in self.want["virt"]:
            n = int(np.sum(np.asarray(self.rows[r]) // HOT_UB == ub))
            out[(r, q)] = (n - q + p - 1) // p if n > q else 0
        return out

    def run(self, X, add=None, acc0=None, scale=0.5, row_mask=None, col_mask=None, keep=None, keep_scale=1.0):
        """one plain-epilogue run (masked, or dropped when `keep` is given): (Y, accum) as numpy; Y starts as 7, accum as acc0"""
        import torch
        from gpu_utils import dev, to_dev
        from skrec import _hip
        dX, dadd = to_dev(X), (to_dev(add) if add is not None else None)
        Y = torch.full((self.n_rows, 64), 7.0, device=dev())
        acc = to_dev(acc0.copy()) if acc0 is not None else None
        drm, dcm = (to_dev(m) if m is not None else None for m in (row_mask, col_mask))
        if keep is None:
            _hip.check(self.L.skr_spmm_plan_run_masked(self.h, _hip.ptr(dX), 64, _hip.ptr(dadd), _hip.ptr(Y), _hip.ptr(acc), scale, _hip.ptr(drm),
                                                       _hip.ptr(dcm), _hip.stream()))
        else:
            ep = _hip.SpmmEpilogue()
            ep.mode, ep.addend, ep.Y, ep.accum, ep.accum_scale = 0, _hip.ptr(dadd), _hip.ptr(Y), _hip.ptr(acc), scale
            dk = to_dev(keep if len(keep) else np.zeros(1, np.uint8))
            _hip.check(self.L.skr_spmm_plan_run_dropped(self.h, _hip.ptr(dX), 64, C.byref(ep), _hip.ptr(dk), keep_scale, _hip.stream()))
        torch.cuda.synchronize()
        return Y.cpu().numpy(), (acc.cpu().numpy() if acc is not None else None)

    def check_products(self, rng):
        """the plain run with addend and accum (hot rows through LDS), the same under an all-ones column mask and as an all-kept
        dropped run (hot rows through tasks): all equal the float64 product exactly"""
        X, add, acc0 = ints(rng, (self.n_cols, 64)), ints(rng, (self.n_rows, 64)), ints(rng, (self.n_rows, 64))
        want = self.A @ X.astype(np.float64) + add
        for kw in (dict(), dict(col_mask=np.ones(self.n_cols, np.uint8)), dict(keep=np.ones(self.nnz, np.uint8))):
            Y, acc = self.run(X, add, acc0, 0.5, **kw)
            bad = np.flatnonzero((Y != want).any(1))
            assert np.array_equal(Y, want), (list(kw), bad[:10], [len(self.rows[r]) for r in bad[:10]])
            assert np.array_equal(acc, acc0 + 0.5 * want), list(kw)


# ---------------------------------------------------------------------------------------------------------------------
# (a) - (h): the paths of the plan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [127, 128, 129, 300])
def test_a_x_block_edges(n_cols):
    """three rows name every column: no hot rows below 128 columns, exactly one X block at 128, a second block of one column at
    129, a last block of 44 columns at 300; 8 pieces each, so every list of a full block holds exactly 16 entries -- the prefetch
    boundary"""
    rng = np.random.default_rng(n_cols)
    rows = extras(rng, n_cols, 2, 3) + [np.arange(n_cols)] * 3
    p = Plan(f"a[{n_cols}]", rows, n_cols, 2, rng, expect_hot=0 if n_cols < 128 else 3)
    if n_cols >= 128:
        assert {pc for _, _, pc in p.want["virt"]} == {8} and set(p.lists(0).values()) == {16}
        if n_cols == 129:
            assert sorted(p.lists(1).values()) == [0] * 21 + [1] * 3
        if n_cols == 300:
            assert set(p.lists(2).values()) == {5, 6}
    p.check_products(rng)
    p.close()


def test_b_long_lists():
    """70 rows name every one of 300 columns: one piece each, 128 entries per list -- eight rounds of sixteen, seven of them
    fetched as needed"""
    rng = np.random.default_rng(2)
    rows = extras(rng, 300, 2, 5) + [np.arange(300)] * 70
    p = Plan("b", rows, 300, 2, rng, expect_hot=70)
    assert len(p.want["virt"]) == 70 and set(p.lists(0).values()) == {128} and set(p.lists(2).values()) == {44}
    p.check_products(rng)
    p.close()


def test_c_uneven_groups():
    """the four groups of one slot with lists of very different lengths: behind 64 filler rows (16 chunks) the rows A (128
    entries, all in X block 0), D (128, all in block 2), C (17, block 2) and B (15 in block 1, 1 in block 2) form one chunk;
    in block 2 its lists hold 0, 128, 17 and 1 entries, in block 0 128, 0, 0, 0"""
    rng = np.random.default_rng(3)
    n_cols = 384
    ex = extras(rng, n_cols, 2, 5)
    four = [np.arange(0, 128), np.arange(256, 384), pick(rng, n_cols, 17, 256, 384),
            np.concatenate([pick(rng, n_cols, 15, 128, 256), pick(rng, n_cols, 1, 256, 384)])]
    rows = ex + four + [pick(rng, n_cols, 130) for _ in range(64)]
    p = Plan("c", rows, n_cols, 2, rng, expect_hot=68)
    a = len(ex)
    assert [[r for r, _, _ in ch] for ch in p.want["chunks"]][16] == [a, a + 1, a + 2, a + 3] and len(p.want["virt"]) == 68
    l0, l2 = p.lists(0), p.lists(2)
    assert [l2[(a + k, 0)] for k in range(4)] == [0, 128, 17, 1] and [l0[(a + k, 0)] for k in range(4)] == [128, 0, 0, 0]
    p.check_products(rng)
    p.close()


def _matrix_d(rng):
    """one row of all 300 columns beside twenty hot rows of ten entries: 5 in X block 0, 4 in block 1, ONE in block 2"""
    ex = extras(rng, 300, 2, 5)
    light = [np.concatenate([pick(rng, 300, 5, 0, 128), pick(rng, 300, 4, 128, 256), pick(rng, 300, 1, 256, 300)]) for _ in range(20)]
    return ex, ex + [np.arange(300)] + light


def test_d_pieces_that_take_nothing():
    """degrees [300] + [10] * 20: 8 pieces for the heavy row, 2 for each light one; a light row's single entry in the last block
    goes to piece 0 and piece 1 takes nothing there; in block 0 its five entries are dealt 3 + 2, every second one each"""
    rng = np.random.default_rng(4)
    ex, rows = _matrix_d(rng)
    p = Plan("d", rows, 300, 2, rng, expect_hot=21)
    a = len(ex)
    assert [pc for r, q, pc in p.want["virt"] if q == 0] == [8] + [2] * 20
    l0, l2 = p.lists(0), p.lists(2)
    assert all(l2[(a + 1 + k, 0)] == 1 and l2[(a + 1 + k, 1)] == 0 and l0[(a + 1 + k, 0)] == 3 and l0[(a + 1 + k, 1)] == 2 for k in range(20))
    p.check_products(rng)
    p.close()


def test_e_threshold():
    """degrees 10, 9, 10 at 300 columns (threshold 9.375): the first and the third row are hot, the second goes by tasks; a row
    of exactly long_rows_from entries is long, one entry fewer is short"""
    rng = np.random.default_rng(5)
    rows = [pick(rng, 300, 10), pick(rng, 300, 9), pick(rng, 300, 10), pick(rng, 300, 2), pick(rng, 300, 1), np.zeros(0, np.int64)]
    p = Plan("e", rows, 300, 2, rng, expect_hot=2)
    assert p.want["hot"] == [0, 2] and p.want["long"] == 4
    p.check_products(rng)
    p.close()
    rows = [pick(rng, 300, k) for k in (10, 9, 10, 6, 5, 0, 3)]
    p = Plan("e[long_rows_from=6]", rows, 300, 6, rng, expect_hot=2)
    assert p.want["hot"] == [0, 2] and p.want["long"] == 4
    p.check_products(rng)
    p.close()


def test_f_cap_and_overflow():
    """100 candidates of distinct degree: the 96 densest are hot, the four lightest go by tasks.  33 rows of 36 and 63 of 12
    entries at 256 columns: 2 pieces and 1 piece, 95 rows fill exactly 128 virtual rows and the 96th goes by tasks"""
    rng = np.random.default_rng(6)
    ex = extras(rng, 256, 2, 5)
    degs = rng.permutation(np.arange(20, 120))
    p = Plan("f[cap]", ex + [pick(rng, 256, int(k)) for k in degs], 256, 2, rng, expect_hot=96)
    assert sorted(len(p.rows[r]) for r in p.want["hot"]) == list(range(24, 120)) and len(p.want["virt"]) == 108
    p.check_products(rng)
    p.close()
    degs = [36] * 33 + [12] * 63
    p = Plan("f[overflow]", ex + [pick(rng, 256, k) for k in degs], 256, 2, rng, expect_hot=95)
    assert len(p.want["virt"]) == 128 and len(ex) + 95 not in p.want["hot"]
    p.check_products(rng)
    p.close()


@pytest.mark.parametrize("n_cols", [500, 870, 1200, 1400])
def test_g_more_blocks_than_workgroups(n_cols, monkeypatch):
    """SKR_SPMM_HOT_WGS=3 (read per plan) with 4, 7, 10 and 11 X blocks: 2, 3 and 4 blocks per workgroup through the double
    buffer, an odd and an even count, a workgroup with a single block (7), with two of four (10) and one with none at all (4)"""
    monkeypatch.setenv("SKR_SPMM_HOT_WGS", "3")
    rng = np.random.default_rng(n_cols)
    n_ub = -(-n_cols // 128)
    assert n_ub in (4, 7, 10, 11)
    under = int(4 * n_cols / 128) - 1
    rows = extras(rng, n_cols, 2, under) + [np.arange(n_cols)] * 2 + [pick(rng, n_cols, n_cols // 3) for _ in range(10)] \
        + [pick(rng, n_cols, under + 2 + k) for k in range(12)] + [np.arange(n_cols - 60, n_cols), np.arange(0, 130)]
    p = Plan(f"g[{n_ub} blocks]", rows, n_cols, 2, rng)
    assert len(p.want["hot"]) >= 24 and len({pc for _, _, pc in p.want["virt"]}) >= 2
    p.check_products(rng)
    # that the three workgroups were in fact used: a second plan of the same matrix with the default (a workgroup per X block)
    # adds a hot row's terms in another order -- on float inputs the two agree to rounding and differ in some bit of the hot
    # rows, while every other row is bit-identical
    monkeypatch.delenv("SKR_SPMM_HOT_WGS")
    p1 = Plan(f"g[{n_ub} blocks, a workgroup each]", rows, n_cols, 2, rng, val=p.val)
    Xf = rng.standard_normal((n_cols, 64)).astype(np.float32)
    (Y3, _), (Y1, _) = p.run(Xf), p1.run(Xf)
    bound = 2e-6 * (abs(p.A) @ np.abs(Xf).astype(np.float64)) + 1e-6
    assert np.all(np.abs(Y3 - p.A @ Xf.astype(np.float64)) <= bound) and np.all(np.abs(Y1 - p.A @ Xf.astype(np.float64)) <= bound)
    hot = np.zeros(p.n_rows, bool)
    hot[p.want["hot"]] = True
    assert np.array_equal(Y3[~hot].view(np.int32), Y1[~hot].view(np.int32)) and not np.array_equal(Y3[hot].view(np.int32), Y1[hot].view(np.int32))
    p.close()
    p1.close()


@pytest.mark.parametrize("n_cols,cblk", [(256, 256), (2048, 256), (2304, 256), (2304, 512)])
def test_h_column_blocks(n_cols, cblk, monkeypatch):
    """SKR_SPMM_CBLK=256: 1, 8 and 9 column blocks (the last task launch has one live block); a segment of exactly 256 entries
    (one full task), a long row inside the last block, a hot row beside them.  A segment of 257 entries (a full task and one of
    a single entry) needs a wider block: 512 columns"""
    monkeypatch.setenv("SKR_SPMM_CBLK", str(cblk))
    rng = np.random.default_rng(n_cols + cblk)
    under = int(4 * n_cols / 128) - 1
    last = -(-n_cols // cblk) - 1
    rows = extras(rng, n_cols, 8, under) + [np.arange(0, 256), np.arange(n_cols - 256, n_cols), pick(rng, n_cols, 20, last * cblk, n_cols),
                                            pick(rng, n_cols, min(n_cols, 900)), pick(rng, n_cols, under + 1), pick(rng, n_cols, 8)]
    if cblk == 512:
        rows += [np.arange(512, 512 + 257), np.concatenate([pick(rng, n_cols, 3, 0, 1024), pick(rng, n_cols, 257, 1024, 1536)])]
    p = Plan(f"h[{n_cols} / {cblk}]", rows, n_cols, 8, rng, cblk=cblk)
    assert p.want["blocks"] == {(256, 256): 1, (2048, 256): 8, (2304, 256): 9, (2304, 512): 5}[(n_cols, cblk)] and len(p.want["hot"]) >= 2
    lens = sorted(e - b for r, begs in p.want["begs"] for b, e in zip(begs, begs[1:] + [len(rows[r])]))      # the tasks' lengths
    assert TASK in lens and (cblk == 256 or 1 in lens)
    p.check_products(rng)
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# (i) epilogues, masks and strides on hot rows
# ---------------------------------------------------------------------------------------------------------------------
def test_i_epilogues_masks_and_strides_on_hot_rows():
    """on the matrix of (d): the plain epilogue's forms (exact), the two refinement epilogues against the stand-alone kernels
    (float inputs, the bounds of test_spmm_row_epilogues_equal_the_separate_passes), a row mask that skips one hot row and
    keeps another -- what belongs to the skipped row stays bit-identical --, and the second 64-column slice of 128-float rows"""
    import torch
    from gpu_utils import dev, to_dev
    from skrec import _hip
    rng = np.random.default_rng(9)
    ex, rows = _matrix_d(rng)
    p = Plan("i", rows, 300, 2, rng, expect_hot=21)
    L, st, n = p.L, _hip.stream(), p.n_rows
    heavy, lightA, lightB = len(ex), len(ex) + 1, len(ex) + 2
    X, add, acc0, base = ints(rng, (300, 64)), ints(rng, (n, 64)), ints(rng, (n, 64)), ints(rng, (n, 64))
    raw = p.A @ X.astype(np.float64)
    rmask = (rng.random(n) < 0.5).astype(np.uint8)
    rmask[[heavy, lightA, lightB]] = [1, 0, 1]
    sel = rmask.astype(bool)
    dX = to_dev(X)

    def run_ex(Xd, rm=None, **kw):
        ep = _hip.SpmmEpilogue()
        for k, v in kw.items():
            setattr(ep, k, _hip.ptr(v) if isinstance(v, torch.Tensor) else v)
        _hip.check(L.skr_spmm_plan_run_ex(p.h, _hip.ptr(Xd) if isinstance(Xd, torch.Tensor) else Xd, 64, C.byref(ep), _hip.ptr(rm), None, st))
        torch.cuda.synchronize()
    full = lambda v: torch.full((n, 64), float(v), device=dev())  # noqa: E731
    # accum = scale * base + scale * y; accum = scale * y without reading accum (it holds NaN)
    Y, acc = full(7), full(9)
    run_ex(dX, mode=0, Y=Y, accum=acc, accum_base=to_dev(base), accum_scale=0.25)
    assert np.array_equal(Y.cpu().numpy(), raw) and np.array_equal(acc.cpu().numpy(), 0.25 * base + 0.25 * raw)
    acc = full(float("nan"))
    run_ex(dX, mode=0, addend=to_dev(add), accum=acc, accum_init=1, accum_scale=0.5)
    assert np.array_equal(acc.cpu().numpy(), 0.5 * (raw + add))
    # accum only at the marked rows; an addend that is not read outside them (NaN there)
    Y, acc = full(7), to_dev(acc0.copy())
    poisoned = np.where(sel[:, None], add, np.float32("nan"))
    run_ex(dX, mode=0, addend=to_dev(poisoned), addend_mask=to_dev(rmask), Y=Y, accum=acc, accum_mask=to_dev(rmask), accum_scale=2.0)
    want = raw + add * sel[:, None]
    assert np.array_equal(Y.cpu().numpy(), want) and np.array_equal(acc.cpu().numpy(), np.where(sel[:, None], acc0 + 2.0 * want, acc0))
    # a row mask: skipped rows keep Y and accum bit for bit
    Y, acc = full(7), to_dev(acc0.copy())
    run_ex(dX, to_dev(rmask), mode=0, addend=to_dev(add), Y=Y, accum=acc, accum_scale=0.5)
    assert np.array_equal(Y.cpu().numpy(), np.where(sel[:, None], raw + add, 7.0))
    assert np.array_equal(acc.cpu().numpy(), np.where(sel[:, None], acc0 + 0.5 * (raw + add), acc0))
    # the second 64-column slice of [*, 128] tables
    Xw, addw = ints(rng, (300, 128)), ints(rng, (n, 128))
    dXw, daddw, Yw, accw = to_dev(Xw), to_dev(addw), torch.full((n, 128), 7.0, device=dev()), torch.full((n, 128), 1.0, device=dev())
    run_ex(dXw.data_ptr() + 256, mode=0, ld=128, addend=daddw.data_ptr() + 256, Y=Yw.data_ptr() + 256, accum=accw.data_ptr() + 256, accum_scale=0.5)
    want = p.A @ Xw[:, 64:].astype(np.float64) + addw[:, 64:]
    assert np.array_equal(Yw.cpu().numpy(), np.hstack([np.full((n, 64), 7.0), want]))
    assert np.array_equal(accw.cpu().numpy(), np.hstack([np.ones((n, 64)), 1.0 + 0.5 * want]))
    # the refinements: float inputs
    Xf, E, addf, accf0, dE0, Yraw = (to_dev(rng.standard_normal(s).astype(np.float32)) for s in ((300, 64),) + ((n, 64),) * 5)
    Af = sp.csr_matrix((p.val.astype(np.float64), p.col, p.rowptr), shape=(n, 300))
    rawf = full(0)
    run_ex(Xf, mode=0, Y=rawf)
    wantf = Af @ Xf.cpu().numpy().astype(np.float64)
    mass = abs(Af) @ np.abs(Xf.cpu().numpy()).astype(np.float64)
    assert np.all(np.abs(rawf.cpu().numpy() - wantf) <= 2e-6 * mass + 1e-6)

    def close(a, b, tol=2e-6):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.all(np.abs(a - b) <= tol * (1.0 + np.abs(b))), np.abs(a - b).max()
    Zs, Ws, accs = full(0), torch.zeros(n, device=dev()), accf0.clone()
    _hip.check(L.skr_layer_refine_fwd(_hip.ptr(rawf), _hip.ptr(E), n, 64, _hip.ptr(Zs), _hip.ptr(Ws), _hip.ptr(accs), st))
    Yf, Zf, Wf, accf = full(0), full(0), torch.zeros(n, device=dev()), accf0.clone()
    run_ex(Xf, mode=1, Y=Yf, accum=accf, E=E, w=Wf, Z=Zf)
    close(Yf, rawf); close(Zf, Zs); close(Wf, Ws); close(accf, accs)
    Ym, Zm, Wm, accm = full(5), full(5), torch.full((n,), 5.0, device=dev()), accf0.clone()
    drm = to_dev(rmask)
    run_ex(Xf, drm, mode=1, Y=Ym, accum=accm, E=E, w=Wm, Z=Zm)
    dsel = torch.from_numpy(sel).to(dev())
    assert torch.equal(Zm[dsel], Zf[dsel]) and torch.equal(Wm[dsel], Wf[dsel]) and torch.equal(accm[dsel], accf[dsel])
    assert bool((Ym[~dsel] == 5).all()) and bool((Zm[~dsel] == 5).all()) and bool((Wm[~dsel] == 5).all()) and torch.equal(accm[~dsel], accf0[~dsel])
    dYs, dEs = full(0), dE0.clone()
    rawa = rawf + addf
    _hip.check(L.skr_layer_refine_bwd(_hip.ptr(Yraw), _hip.ptr(E), _hip.ptr(Ws), _hip.ptr(rawa), n, 64, _hip.ptr(dYs), _hip.ptr(dEs), st))
    dYf, dEf = full(0), dE0.clone()
    run_ex(Xf, mode=2, addend=addf, Y=dYf, E=E, w=Ws, rawY=Yraw, dE=dEf)
    close(dYf, dYs, 4e-6); close(dEf, dEs, 4e-6)
    dYm, dEm = full(3), dE0.clone()
    run_ex(Xf, drm, mode=2, addend=addf, Y=dYm, E=E, w=Ws, rawY=Yraw, dE=dEm)
    assert torch.equal(dYm[dsel], dYf[dsel]) and torch.equal(dEm[dsel], dEf[dsel])
    assert bool((dYm[~dsel] == 3).all()) and torch.equal(dEm[~dsel], dE0[~dsel])
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# (j) the launch-shape switches change no bit
# ---------------------------------------------------------------------------------------------------------------------
def _switch_outputs():
    """three fixed matrices -- 1500 rows with forty long rows inside one column block (twenty of them hot), the matrix of (b),
    and 2304 columns in 9 blocks of 256 (two task launches, or one that spans both) -- through the plain and the dropped run:
    {name: array}, with the float64 expectation beside every output"""
    out = {}
    for name, n_cols, long_from, cblk in (("wide", 1500, 32, None), ("b", 300, 2, None), ("blocks", 2304, 8, 256)):
        rng = np.random.default_rng(len(name))
        if name == "wide":
            lens = rng.integers(0, 32, 1500)
            lens[rng.choice(1500, 40, replace=False)] = [40] * 20 + [300] * 20
            rows = [pick(rng, n_cols, int(k)) for k in lens]
        elif name == "b":
            rows = extras(rng, 300, 2, 5) + [np.arange(300)] * 70
        else:
            rows = extras(rng, n_cols, 8, 60) + [pick(rng, n_cols, 900), pick(rng, n_cols, 600), np.arange(2048, 2304)] + [pick(rng, n_cols, 30) for _ in range(40)]
        old = os.environ.get("SKR_SPMM_CBLK")
        if cblk:
            os.environ["SKR_SPMM_CBLK"] = str(cblk)           # read per plan
        try:
            p = Plan("j[" + name + "]", rows, n_cols, long_from, rng, cblk=cblk)
        finally:
            if cblk:
                os.environ.pop("SKR_SPMM_CBLK") if old is None else os.environ.__setitem__("SKR_SPMM_CBLK", old)
        assert len(p.want["hot"]) > 0 and p.want["long"] > len(p.want["hot"])
        X, add, acc0 = ints(rng, (n_cols, 64)), ints(rng, (p.n_rows, 64)), ints(rng, (p.n_rows, 64))
        keep = (rng.random(p.nnz) < 0.5).astype(np.uint8)
        out[name + "/Y"], out[name + "/acc"] = p.run(X, add, acc0, 0.5)
        out[name + "/Yd"], out[name + "/accd"] = p.run(X, add, acc0, 0.5, keep=keep, keep_scale=2.0)
        want = p.A @ X.astype(np.float64) + add
        Ad = sp.csr_matrix((2.0 * p.val.astype(np.float64) * keep, p.col, p.rowptr), shape=(p.n_rows, n_cols))
        wantd = Ad @ X.astype(np.float64) + add
        out[name + "/want"] = np.stack([want, acc0 + 0.5 * want, wantd, acc0 + 0.5 * wantd])
        p.close()
    return out


def _equal_float64(o):
    for name in ("wide", "b", "blocks"):
        for k, key in enumerate(("/Y", "/acc", "/Yd", "/accd")):
            assert np.array_equal(o[name + key], o[name + "/want"][k]), name + key


def test_j_launch_shape_switches_change_no_bit(tmp_path):
    """SKR_SPMM_HOT_PF=2 (the other instance of the LDS-streamed kernel), SKR_SPMM_TASK_SPAN=2, SKR_SPMM_ROWS_WGS=256 and
    SKR_SPMM_TASK_WGS=8 (grid-stride loops): bit-identical outputs; SKR_SPMM_HOT=0: the same rows through tasks, equal to float64.
    The switches are read once per process: each setting runs in a fresh child, one at a time"""
    if any(v in os.environ for v in SWITCHES):
        pytest.skip("an SKR_SPMM_* switch is set in this process's environment")
    mine = _switch_outputs()
    _equal_float64(mine)
    for tag, env in (("A", dict(SKR_SPMM_HOT_PF="2", SKR_SPMM_TASK_SPAN="2", SKR_SPMM_ROWS_WGS="256", SKR_SPMM_TASK_WGS="8")),
                     ("B", dict(SKR_SPMM_HOT="0"))):
        path = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=240, cwd=os.path.join(HERE, ".."))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        theirs = np.load(path)
        _equal_float64(theirs)
        for k, v in mine.items():
            assert np.array_equal(v.view(np.int64 if v.dtype == np.float64 else np.int32), theirs[k].view(np.int64 if v.dtype == np.float64 else np.int32)), (tag, k)


# ---------------------------------------------------------------------------------------------------------------------
# (k) skr_csr_scatter_marked_rows and skr_mark_ids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_k_scatter_marked_rows_and_mark_ids(n_rows):
    """Y[c] += A[r, c] X[r] over the marked rows: no row, every row, and some rows marked (an empty one among them); rows of 300
    and of 65 entries; every row hits column 5.  Exact inputs: the order of the float atomics does not matter"""
    import torch
    from gpu_utils import dev, to_dev
    from skrec import _hip
    L, st = _hip.lib(), _hip.stream()
    rng = np.random.default_rng(n_rows)
    n_cols = 320
    lens = rng.integers(0, 12, n_rows)
    lens[0] = 300
    if n_rows > 2:
        lens[1], lens[2] = 65, 0
    rows = [np.union1d(pick(rng, n_cols, int(k)), [5]) if k else np.zeros(0, np.int64) for k in lens]
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32)
    val = ints(rng, len(col), zero=False)
    A = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n_rows, n_cols))
    X, Y0 = ints(rng, (n_rows, 64)), ints(rng, (n_cols, 64))
    d_rp, d_col, d_val, dX = to_dev(rowptr), to_dev(col), to_dev(val), to_dev(X)
    some = (rng.random(n_rows) < 0.4).astype(np.uint8)
    some[min(2, n_rows - 1)] = 1
    for mask in (np.zeros(n_rows, np.uint8), np.ones(n_rows, np.uint8), some):
        Y = to_dev(Y0.copy())
        _hip.check(L.skr_csr_scatter_marked_rows(n_rows, _hip.ptr(d_rp), _hip.ptr(d_col), _hip.ptr(d_val), _hip.ptr(to_dev(mask)), _hip.ptr(dX), 64,
                                                 _hip.ptr(Y), st))
        torch.cuda.synchronize()
        assert np.array_equal(Y.cpu().numpy(), Y0 + A.T @ (X.astype(np.float64) * mask[:, None]))
    # skr_mark_ids: nothing to mark, duplicates, negative ids, an offset; bytes outside stay as they were
    mk = torch.zeros(n_rows + 9, dtype=torch.uint8, device=dev())
    _hip.check(L.skr_mark_ids(None, 0, 0, _hip.ptr(mk), st))
    assert int(mk.sum()) == 0
    ids = np.array([0, n_rows - 1, -1, 0, n_rows - 1, -5, n_rows // 2, n_rows // 2], np.int32)
    _hip.check(L.skr_mark_ids(_hip.ptr(to_dev(ids)), len(ids), 4, _hip.ptr(mk), st))
    assert mk.nonzero().flatten().tolist() == sorted({4, 4 + n_rows - 1, 4 + n_rows // 2})
    _hip.check(L.skr_mark_ids(_hip.ptr(to_dev(ids)), len(ids), 0, _hip.ptr(mk), st))
    assert mk.nonzero().flatten().tolist() == sorted({4, 4 + n_rows - 1, 4 + n_rows // 2, 0, n_rows - 1, n_rows // 2})


# ---------------------------------------------------------------------------------------------------------------------
# (l) masked and dropped entries are not read
# ---------------------------------------------------------------------------------------------------------------------
def _matrix_l(rng, n_cols, avoid):
    """short rows of every length 1 .. 70, long rows of several tasks in two column blocks; the last short and the last long row
    name none of the columns in `avoid`"""
    free = np.flatnonzero(~avoid)
    rows = [pick(rng, n_cols, k) for k in range(1, 71)] + [np.zeros(0, np.int64)]
    rows += [np.union1d(pick(rng, n_cols, k), [0]) for k in (100, 333, 600, 777, 900)]
    rows += [np.sort(rng.choice(free, 9, replace=False)), np.sort(rng.choice(free, 400, replace=False))]
    return rows


def test_l_column_mask_unmarked_rows_of_x_are_not_read():
    """the X rows of every unmarked column are NaN: the masked run returns the float64 product of the marked entries exactly,
    with and without a row mask.  Column 0 is unmarked and is the first entry of the long rows' first task; two rows have no
    marked column at all"""
    rng = np.random.default_rng(12)
    n_cols = 3000
    cmask = (rng.random(n_cols) < 0.3).astype(np.uint8)
    cmask[0] = 0
    rows = _matrix_l(rng, n_cols, cmask == 0)       # (the last two rows: marked columns only -- see below)
    rows += [np.sort(rng.choice(np.flatnonzero(cmask == 0), 13, replace=False)), np.sort(rng.choice(np.flatnonzero(cmask == 0), 300, replace=False))]
    p = Plan("l[mask]", rows, n_cols, 100, rng)
    assert p.want["blocks"] == 2 and p.want["tasks"] > p.want["long"] >= 7
    firsts = [p.col[p.rowptr[r] + b] for r, begs in p.want["begs"] for b in begs]
    assert sum(1 for c in firsts if not cmask[c]) >= 5
    X, add, acc0 = ints(rng, (n_cols, 64)), ints(rng, (p.n_rows, 64)), ints(rng, (p.n_rows, 64))
    Xn = np.where(cmask[:, None] != 0, X, np.float32("nan"))
    want = p.A @ (X.astype(np.float64) * cmask[:, None]) + add
    Y, acc = p.run(Xn, add, acc0, 0.5, col_mask=cmask)
    bad = np.flatnonzero((Y != want).any(1))
    print("l[mask]: rows that differ", len(bad), "with NaN", int(np.isnan(Y).any(1).sum()),
          "marked entries of those rows mod 4", sorted({int(cmask[rows[r]].sum()) % 4 for r in bad}))
    assert np.array_equal(Y, want) and np.array_equal(acc, acc0 + 0.5 * want)
    rmask = (rng.random(p.n_rows) < 0.5).astype(np.uint8)
    sel = rmask.astype(bool)[:, None]
    Y, acc = p.run(Xn, add, acc0, 0.5, row_mask=rmask, col_mask=cmask)
    assert np.array_equal(Y, np.where(sel, want, 7.0)) and np.array_equal(acc, np.where(sel, acc0 + 0.5 * want, acc0))
    p.close()


def test_l_dropped_entries_rows_of_x_are_not_read():
    """`keep` drops every entry of a set P of columns -- the first column of several short rows and of several tasks among them --
    and half of the others; the X rows of P are NaN: the dropped run returns the float64 product of the kept entries exactly"""
    rng = np.random.default_rng(13)
    n_cols = 3000
    rows = _matrix_l(rng, n_cols, np.zeros(n_cols, bool))
    p = Plan("l[dropped]", rows, n_cols, 100, rng)
    firsts = [int(p.col[p.rowptr[r] + b]) for r, begs in p.want["begs"] for b in begs]
    P = np.zeros(n_cols, bool)
    P[firsts[::2]] = True
    P[[int(rows[r][0]) for r in range(0, 70, 3)]] = True
    P[rng.choice(n_cols, 300, replace=False)] = True
    keep = ((rng.random(p.nnz) < 0.5) & ~P[p.col]).astype(np.uint8)
    keep[p.rowptr[30]:p.rowptr[31]] = 0                      # a row with nothing kept
    X, add, acc0 = ints(rng, (n_cols, 64)), ints(rng, (p.n_rows, 64)), ints(rng, (p.n_rows, 64))
    Xn = np.where(P[:, None], np.float32("nan"), X)
    Ad = sp.csr_matrix((2.0 * p.val.astype(np.float64) * keep, p.col, p.rowptr), shape=(p.n_rows, n_cols))
    want = Ad @ np.where(P[:, None], 0.0, X.astype(np.float64)) + add
    Y, acc = p.run(Xn, add, acc0, 0.5, keep=keep, keep_scale=2.0)
    bad = np.flatnonzero((Y != want).any(1))
    kept = np.add.reduceat(np.append(keep, 0).astype(np.int64), p.rowptr[:-1]) * (np.diff(p.rowptr) > 0)
    print("l[dropped]: rows that differ", len(bad), "with NaN", int(np.isnan(Y).any(1).sum()), "kept entries of those rows mod 4",
          sorted({int(kept[r]) % 4 for r in bad}))
    assert np.array_equal(Y, want) and np.array_equal(acc, acc0 + 0.5 * want)
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# (m) LayerGCN end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_m_layergcn_step_does_not_read_the_skipped_rows(tiny_dir, monkeypatch, tmp_path):
    """LayerGCN's training step through the plan writes dY of the top refinement at the batch's rows only and relies on the
    column-masked product not reading the others: with those buffers full of NaN before the first step, three steps give the
    losses and parameters, bit for bit, that zero-filled buffers give"""
    import torch
    from gpu_utils import dev
    from skrec import RunConfig
    from skrec.recommender.LayerGCN import LayerGCN
    from skrec.utils.py.random import reset_global_sampler
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SKR_SPMM_PLAN", "1")
    monkeypatch.delenv("SKR_LIGHTGCN_DENSE", raising=False)
    outs = []
    for fill in (float("nan"), 0.0):
        import random
        reset_global_sampler(2020)
        np.random.seed(2021); random.seed(2021); torch.manual_seed(2021)
        m = LayerGCN(RunConfig(recommender="LayerGCN", data_dir=tiny_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                               metric=("Recall", "NDCG"), top_k=(5, 10), test_batch_size=16, test_thread=2, seed=2021),
                     dict(lr=1e-3, reg=1e-2, embed_dim=64, n_layers=4, dropout=0.0, batch_size=256, epochs=2))
        assert m.train_adj.uses_plan()
        for t in m._t:
            t.fill_(fill)
        rng = np.random.default_rng(77)
        losses = torch.zeros((3, 2), device=dev())
        for k in range(3):
            # four pairs of distinct users and items: ONE workgroup of the BPR kernel adds up the loss and every gradient row gets
            # one float atomic, so a step is reproducible bit for bit in itself (larger batches are not: float atomics)
            ids = rng.choice(m.num_items, 8, replace=False)
            u, i, j = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev())
                       for a in (rng.choice(m.num_users, 4, replace=False), ids[:4], ids[4:]))
            m.train_step(u, i, j, losses[k])
        torch.cuda.synchronize()
        outs.append((losses.cpu().numpy(), m.ego.cpu().numpy().copy()))
    (ln, en), (lz, ez) = outs
    assert not np.isnan(ln).any() and not np.isnan(en).any()
    assert np.array_equal(ln.view(np.int32), lz.view(np.int32)) and np.array_equal(en.view(np.int32), ez.view(np.int32))


if __name__ == "__main__":       # the child of test_j: the fixed products under this process's switches -> an .npz
    for _p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "scikit-recommender_amd")):
        sys.path.insert(0, os.path.abspath(_p))
    np.savez(sys.argv[1], **_switch_outputs())
