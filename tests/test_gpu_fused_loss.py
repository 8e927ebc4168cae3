"""The deferred loss words of the one-launch BPR step (csrc/bpr_fused.hip: skr_bpr_fused_step3 / _end3 / _block3): every
wavefront of a step launch stores its two sums into the block's partials, and the block's end launch folds them into the
SKR_LOSS_SLOTS pairs per step -- the sums the other form (skr_bpr_fused_step2 / _block2) adds with atomics per step, in a
fixed order.  Parameters and moments do not depend on the form.  Tiny tables, as tests/test_gpu_fused_launch.py."""
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":      # the child process of test_the_switch_takes_the_old_entries
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_REPO, os.path.join(_REPO, "scikit-recommender_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

N_USERS, N_ITEMS = 3000, 777      # 777 = 12 * 64 + 9: the last bias block ends past the flat buffer
N_PAR = (N_USERS + N_ITEMS) * 64 + N_ITEMS
N_BLOCKS = 3                      # both sets of words / slot tables (q = 0, 1, 0)
SENTINEL = 12345.0                # workspace state planes and pre buffers, as test_gpu_fused_launch.py
PART_SENTINEL = 1e30              # the partials: one stale word in a sum would swamp it
LR, REG = 1e-2, 1e-3


def _ids(rng, n_steps, b, distinct):
    if distinct:      # rows distinct within a step (each float atomic then happens once: deterministic gradients)
        u = np.stack([rng.permutation(N_USERS)[:b] for _ in range(n_steps)])
        ij = np.stack([rng.permutation(N_ITEMS)[:2 * b] for _ in range(n_steps)])
        return u, ij[:, :b], ij[:, b:]
    u = rng.integers(0, N_USERS // 50, (n_steps, b))       # popular items and repeated users inside a step
    i = np.minimum((rng.pareto(1.2, (n_steps, b)) * 5).astype(np.int64), N_ITEMS - 1)
    return u, i, (i + 1 + rng.integers(0, N_ITEMS - 1, (n_steps, b))) % N_ITEMS


def _state(rng):
    """parameters and non-zero moments"""
    import torch
    return tuple(torch.from_numpy(x.astype(np.float32)).cuda() for x in
                 (rng.standard_normal(N_PAR) * 0.05, rng.standard_normal(N_PAR) * 1e-3, rng.random(N_PAR) * 1e-6))


def _dev_ids(u, i, j):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in (u, i, j))


class _Run(object):
    pass


# ---- one block through the C entries: plan, then skr_bpr_fused_block2 (form 2) or _block3 (form 3) ------------------------
def _block(form, k, b, ids, state, loss=None, stride=None, t0=5):
    """returns the run: flat / m / v after the block, loss (float[k, S, 2] unless given), the partials"""
    import torch
    from skrec import _hip
    L, st = _hip.lib(), _hip.stream()
    S = _hip.SKR_LOSS_SLOTS
    u, i, j = ids
    r = _Run()
    r.flat, r.m, r.v = (x.clone() for x in state)
    nfb = (N_PAR + 63) // 64
    refs = k * 5 * b
    cap = min(refs, nfb)
    work = torch.zeros(9 * cap * 64, device="cuda")
    meta, sb, sf = (torch.empty(refs, dtype=torch.int32, device="cuda") for _ in range(3))
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(28 * nfb // 8 + 1, dtype=torch.int64, device="cuda")
    r.loss = torch.zeros((k, S, 2), device="cuda") if loss is None else loss
    stride = 2 * S if stride is None else stride
    r.part = torch.full((int(L.skr_bpr_fused_loss_part_floats(b, k)),), PART_SENTINEL, device="cuda")
    _hip.check(L.skr_bpr_fused_plan(u.data_ptr(), i.data_ptr(), j.data_ptr(), b, k, 0, N_USERS, N_USERS + N_ITEMS, nfb,
                                    scratch.data_ptr(), meta.data_ptr(), sb.data_ptr(), sf.data_ptr(), ns.data_ptr(), st))
    args = (r.flat.data_ptr(), r.m.data_ptr(), r.v.data_ptr(), N_PAR, work.data_ptr(), cap, u.data_ptr(), i.data_ptr(), j.data_ptr(),
            meta.data_ptr(), b, 0, N_USERS, N_USERS + N_ITEMS, LR, 0.9, 0.999, 1e-8, t0, k, REG, r.loss.data_ptr(), stride,
            sb.data_ptr(), sf.data_ptr(), ns.data_ptr(), None, 0, None)
    if form == 3:
        _hip.check(L.skr_bpr_fused_block3(*args, r.part.data_ptr(), st))
    else:
        _hip.check(L.skr_bpr_fused_block2(*args, st))
    torch.cuda.synchronize()
    assert float(work[6 * cap * 64:].abs().max()) == 0.0      # the gradient planes are left zero
    r.args, r.keep = args, (ids, work, meta, sb, sf, ns, scratch)      # (args holds addresses)
    return r


@functools.lru_cache(maxsize=None)
def _pair_case(k, b):
    """both forms (form 3 twice) from identical state, rows distinct inside a step"""
    rng = np.random.default_rng(7000 + 37 * k + b)
    ids = _dev_ids(*_ids(rng, k, b, True))
    state = _state(rng)
    return _block(2, k, b, ids, state), _block(3, k, b, ids, state), _block(3, k, b, ids, state)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _same_parameters(a, c):
    import torch
    return torch.equal(a.flat, c.flat) and torch.equal(a.m, c.m) and torch.equal(a.v, c.v)


# 1.  at most one workgroup per pair (b <= 4 * SKR_LOSS_SLOTS): the other form's single add per word has a fixed order too
@pytest.mark.gpu
@pytest.mark.parametrize("k,b", [(k, b) for b in (1, 3, 5, 128) for k in (1, 7, 32)])
def test_pairs_equal_the_adding_form_bit_for_bit(k, b):
    old, new, _ = _pair_case(k, b)
    assert np.array_equal(_words(old.loss), _words(new.loss))
    assert float(new.loss[:, 0, 0].min()) > 0.0      # (not vacuous: every step has a loss)
    assert _same_parameters(old, new)
    if b <= 4:
        assert float(new.loss[:, 1:, :].abs().max()) == 0.0
    n_pairs = (b + 3) // 4
    assert np.all(_words(new.loss[:, n_pairs:]) == 0)      # a pair no workgroup feeds: +0.0f, not -0.0f


# 2.  65 workgroups: pairs 0 and 1 are fed by three, the others by two, the last workgroup has one live wavefront
@pytest.mark.gpu
@pytest.mark.parametrize("k", [7, 32])
def test_pairs_of_several_workgroups(k):
    old, new, again = _pair_case(k, 259)
    got, want = new.loss.cpu().numpy(), old.loss.cpu().numpy()
    print(f"k={k}: largest relative difference of a loss word {np.abs(got / want - 1).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-5)
    assert np.array_equal(_words(new.loss), _words(again.loss))      # the fold's order is fixed
    assert _same_parameters(old, new) and _same_parameters(new, again)


# ---- FusedBlocks against the two-launch path (skr_bpr_step + DenseAdam.step) ------------------------------------------------
def _classic(state, u, i, j, b):
    """one skr_bpr_step plus a dense Adam step per batch; returns the optimiser and the loss sums [n_steps, 2]"""
    import torch
    from skrec import _hip
    from skrec.recommender.base import DenseAdam
    L, st = _hip.lib(), _hip.stream
    a = DenseAdam(state[0].clone(), lr=LR, track_touch=True)
    a.m.copy_(state[1]), a.v.copy_(state[2])
    loss = torch.zeros((len(u), 2), device="cuda")
    sl = lambda t: (t[:N_USERS * 64].view(N_USERS, 64), t[N_USERS * 64:(N_USERS + N_ITEMS) * 64].view(N_ITEMS, 64),  # noqa: E731
                    t[(N_USERS + N_ITEMS) * 64:])
    (U, V, bias), (gU, gV, gb) = sl(a.flat), sl(a.grad)
    for s in range(len(u)):
        _hip.check(L.skr_bpr_step(_hip.ptr(U), _hip.ptr(V), _hip.ptr(bias), _hip.ptr(U), _hip.ptr(V), _hip.ptr(u[s]), _hip.ptr(i[s]),
                                  _hip.ptr(j[s]), b, 1.0, REG, 1.0, _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(gb), _hip.ptr(gU),
                                  _hip.ptr(gV), _hip.ptr(loss[s]), _hip.ptr(a.touch), _hip.ptr(a.grad), st()))
        a.step()
    return a, loss


def _fused_blocks(state, defer=True):
    """defer None: as the environment chooses"""
    from skrec.recommender.base import DenseAdam
    from skrec.recommender.fused import FusedBlocks
    c = DenseAdam(state[0].clone(), lr=LR)
    c.m.copy_(state[1]), c.v.copy_(state[2])
    fb = FusedBlocks(c, 0, N_USERS, N_USERS + N_ITEMS, REG)
    if defer is not None:
        fb.loss_defer = defer
    return c, fb


def _run_blocks(fb, ids, n_blocks, k, b):
    """the loss words [n_blocks * k, S, 2] of n_blocks blocks"""
    import torch
    from skrec import _hip
    S = _hip.SKR_LOSS_SLOTS
    loss = torch.zeros((n_blocks * k, S, 2), device="cuda")
    u, i, j = ids
    fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), n_blocks, k, b, loss.data_ptr(), 8 * S)
    fb.opt.end_blocks()
    torch.cuda.synchronize()
    return loss


# 3.  the grid is capped at 4 096 workgroups and the wavefronts loop; the tables are small, so ids are shared
@pytest.mark.gpu
def test_grid_stride_launch():
    import torch
    k, b = 1, 16389
    rng = np.random.default_rng(31)
    u, i, j = _dev_ids(*_ids(rng, N_BLOCKS * k, b, False))
    state = _state(rng)
    a, want = _classic(state, u, i, j, b)
    c, fb = _fused_blocks(state)
    fb._size(k, b)
    assert fb.loss_part.numel() == k * 8 * 4096
    fb.loss_part.fill_(PART_SENTINEL)
    got = _run_blocks(fb, (u, i, j), N_BLOCKS, k, b)
    assert c.t == N_BLOCKS * k
    got, want = got.sum(1).cpu().numpy(), want.cpu().numpy()
    print(f"largest relative loss difference {np.abs(got / want - 1).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-4)
    # (float atomics on shared rows sum in an order that differs from launch to launch, in both paths: what holds of the
    #  parameters' side is what test_fused_launch_loss_words_with_rows_shared_inside_a_step holds)
    assert float(fb.work[:, 6 * fb.cap * 64:].abs().max()) == 0.0
    assert bool(torch.isfinite(c.flat).all())


# 4.  a stride of 0 (all steps collide on one set of words) and a buffer that is not zero
@pytest.mark.gpu
def test_stride_zero_adds_to_what_is_there():
    import torch
    k, b = 7, 259
    _, strided, _ = _pair_case(k, b)
    rng = np.random.default_rng(7000 + 37 * k + b)      # _pair_case's ids and state again
    ids = _dev_ids(*_ids(rng, k, b, True))
    state = _state(rng)
    pattern = torch.arange(1, 65, device="cuda", dtype=torch.float32) * 0.25
    loss = pattern.clone()
    r = _block(3, k, b, ids, state, loss=loss, stride=0)
    want = (pattern.double() + strided.loss.double().sum(0).view(-1)).cpu().numpy()
    np.testing.assert_allclose(r.loss.cpu().numpy(), want, rtol=1e-5)
    assert _same_parameters(r, strided)


# 5.  a shrinking batch leaves old pairs behind in the partials, which are never cleared
@pytest.mark.gpu
def test_stale_partials_are_never_read():
    k = 7
    rng = np.random.default_rng(77)
    state = _state(rng)
    cd, fd = _fused_blocks(state)
    co, fo = _fused_blocks(state, defer=False)
    fd._size(k, 259)
    fd.loss_part.fill_(PART_SENTINEL)
    part = fd.loss_part
    assert fo.loss_part is None
    for b in (3, 259, 3):
        ids = _dev_ids(*_ids(rng, N_BLOCKS * k, b, True))
        got, want = _run_blocks(fd, ids, N_BLOCKS, k, b), _run_blocks(fo, ids, N_BLOCKS, k, b)
        if b <= 4 * 32:
            assert np.array_equal(_words(got), _words(want))
            assert float(got[:, 1:, :].abs().max()) == 0.0
        else:
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-5)
        assert float(got[:, 0, 0].min()) > 0.0
        assert _same_parameters(cd, co)
    assert fd.loss_part is part      # one buffer all along


# 6.  both sets of words, then a shorter block on the same object
@pytest.mark.gpu
def test_run_blocks_then_a_shorter_block():
    k, k2, b = 7, 3, 259
    rng = np.random.default_rng(66)
    u, i, j = _dev_ids(*_ids(rng, N_BLOCKS * k + k2, b, True))
    state = _state(rng)
    a, want = _classic(state, u, i, j, b)
    c, fb = _fused_blocks(state)
    got = [_run_blocks(fb, (u, i, j), N_BLOCKS, k, b),
           _run_blocks(fb, tuple(x[N_BLOCKS * k:].contiguous() for x in (u, i, j)), 1, k2, b)]
    assert fb.loss_defer and c.t == N_BLOCKS * k + k2
    got = np.concatenate([g.sum(1).cpu().numpy() for g in got])
    want = want.cpu().numpy()
    print(f"largest relative loss difference {np.abs(got / want - 1).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-5)
    assert _same_parameters(a, c)


@pytest.mark.gpu
def test_bracketed_blocks_are_issued_through_step3_and_end3():
    """run_blocks' launch-by-launch timing path (`block_timing`): the same loss words and parameters as skr_bpr_fused_block3"""
    import torch
    k, b = 7, 128
    rng = np.random.default_rng(88)
    ids = _dev_ids(*_ids(rng, N_BLOCKS * k, b, True))
    state = _state(rng)
    c0, f0 = _fused_blocks(state)
    c1, f1 = _fused_blocks(state)
    f1.block_timing, f1.block_timing_skip = [], 1      # block 0 through _block3, blocks 1 and 2 launch by launch
    f1.block_event_pool = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(3)) for _ in range(N_BLOCKS)]
    want, got = _run_blocks(f0, ids, N_BLOCKS, k, b), _run_blocks(f1, ids, N_BLOCKS, k, b)
    assert len(f1.block_timing) == N_BLOCKS - 1
    assert np.array_equal(_words(got), _words(want)) and float(got[:, 0, 0].min()) > 0.0
    assert _same_parameters(c0, c1)


# 7.  SKR_FUSED_LOSS_DEFER=0 in a fresh process
def _child():
    k, b = 7, 259
    rng = np.random.default_rng(9000 + 37 * k + b)
    u, i, j = _dev_ids(*_ids(rng, N_BLOCKS * k, b, True))
    state = _state(rng)
    a, want = _classic(state, u, i, j, b)
    c, fb = _fused_blocks(state, defer=None)
    assert fb.loss_defer is False
    got = _run_blocks(fb, (u, i, j), N_BLOCKS, k, b)
    assert fb.loss_part is None
    np.testing.assert_allclose(got.sum(1).cpu().numpy(), want.cpu().numpy(), rtol=1e-5)
    assert _same_parameters(a, c)
    print("child OK")


@pytest.mark.gpu
def test_the_switch_takes_the_old_entries():
    import subprocess
    env = dict(os.environ, SKR_FUSED_LOSS_DEFER="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child OK" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


# 8.  refused with the library's error code, before any launch
@pytest.mark.gpu
def test_argument_checks():
    import torch
    from skrec import _hip
    L, st = _hip.lib(), _hip.stream()
    k, b = 1, 5
    _, new, _ = _pair_case(k, b)
    a = list(new.args)      # the 29 leading arguments of _block2 / _block3 (the tensors behind them are alive in the cached run)
    before = new.flat.clone()
    part = new.part.data_ptr()
    assert L.skr_bpr_fused_block3(*a, None, st) == -1
    neg = list(a)
    neg[22] = -64
    assert L.skr_bpr_fused_block3(*neg, part, st) == -1
    # _step3: _block's leading arguments up to k, then s, reg, d_loss64, d_pre, d_loss_part
    step = a[:20] + [0, REG, a[21], None]
    assert L.skr_bpr_fused_step3(*step, None, st) == -1
    # _end3: tables, slot tables, optimiser scalars, tags, which, then d_loss_part, d_loss64, stride, n_batch
    end = a[:6] + a[23:26] + a[14:20] + [None, 0, 0]
    assert L.skr_bpr_fused_end3(*end, None, a[21], 64, b, st) == -1
    assert L.skr_bpr_fused_end3(*end, part, None, 64, b, st) == -1
    assert L.skr_bpr_fused_end3(*end, part, a[21], -64, b, st) == -1
    assert b"NULL" in L.skr_last_error() or b"shape" in L.skr_last_error()
    assert int(L.skr_bpr_fused_loss_part_floats(1024, 32)) == 32 * 8 * 256
    assert int(L.skr_bpr_fused_loss_part_floats(259, 7)) == 7 * 8 * 65
    assert int(L.skr_bpr_fused_loss_part_floats(16389, 1)) == 8 * 4096
    assert int(L.skr_bpr_fused_loss_part_floats(0, 4)) == 0
    torch.cuda.synchronize()
    assert torch.equal(new.flat, before)      # nothing was launched


if __name__ == "__main__":
    _child()
