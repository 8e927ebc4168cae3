"""The launch shape of the one-launch BPR step (csrc/bpr_fused.hip): the first loads of the step, end and pre kernels take
their arguments from registers preloaded at wavefront launch (the parameter lists are ordered for it), and the owner's
stores are write-through.  None of it changes a parameter: FusedBlocks against one skr_bpr_step plus a dense skr_adam_step
per step, from moments that are not zero, at the edges the load phase and the row launches can get wrong."""
import functools

import numpy as np
import pytest

N_USERS, N_ITEMS = 3000, 777      # 777 = 12 * 64 + 9: the last bias block ends past the flat buffer
N_BLOCKS = 3                      # rows come from the dense tables, the workspace and (from the second block on) the pre buffer
SENTINEL = 12345.0


def _ids(rng, n_steps, b, distinct):
    if distinct:      # rows distinct within a step (each float atomic then happens once: deterministic gradients)
        u = np.stack([rng.permutation(N_USERS)[:b] for _ in range(n_steps)])
        ij = np.stack([rng.permutation(N_ITEMS)[:2 * b] for _ in range(n_steps)])
        return u, ij[:, :b], ij[:, b:]
    u = rng.integers(0, N_USERS // 50, (n_steps, b))       # popular items and repeated users inside a step
    i = np.minimum((rng.pareto(1.2, (n_steps, b)) * 5).astype(np.int64), N_ITEMS - 1)
    return u, i, (i + 1 + rng.integers(0, N_ITEMS - 1, (n_steps, b))) % N_ITEMS


def _slots_per_block(u, i, j, k):
    """distinct 64-float blocks of the flat buffer that each k-step block names: its number of workspace slots"""
    out = []
    for blk in range(len(u) // k):
        s = slice(blk * k, (blk + 1) * k)
        refs = np.concatenate([u[s].ravel(), N_USERS + i[s].ravel(), N_USERS + j[s].ravel(),
                               N_USERS + N_ITEMS + (i[s].ravel() >> 6), N_USERS + N_ITEMS + (j[s].ravel() >> 6)])
        out.append(len(np.unique(refs)))
    return out


class _Run(object):
    pass


def _launch_case(k, b, distinct, seed, classic=True, need_odd_slots=False):
    """the two-launch path (classic) and FusedBlocks after the same N_BLOCKS * k batches, both from the same parameters and
    the same non-zero moments; the workspace's state planes and the pre buffers are filled with SENTINEL beforehand (by
    contract nothing reads a state the block has not written)"""
    import torch
    from skrec import _hip
    from skrec.recommender.base import DenseAdam
    from skrec.recommender.fused import FusedBlocks
    L, st = _hip.lib(), _hip.stream
    n_steps = k * N_BLOCKS
    while True:
        rng = np.random.default_rng(seed)
        u, i, j = _ids(rng, n_steps, b, distinct)
        slots = _slots_per_block(u, i, j, k)
        if not need_odd_slots or any(n & 1 for n in slots):
            break
        seed += 1000
    n_par = (N_USERS + N_ITEMS) * 64 + N_ITEMS
    init = torch.from_numpy((rng.standard_normal(n_par) * 0.05).astype(np.float32)).cuda()
    m0 = torch.from_numpy((rng.standard_normal(n_par) * 1e-3).astype(np.float32)).cuda()
    v0 = torch.from_numpy((rng.random(n_par) * 1e-6).astype(np.float32)).cuda()
    u, i, j = (torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in (u, i, j))
    r = _Run()
    r.slots, r.k, r.b = slots, k, b
    if classic:
        a = DenseAdam(init.clone(), lr=1e-2, track_touch=True)
        a.m.copy_(m0), a.v.copy_(v0)
        r.loss_classic = torch.zeros((n_steps, 2), device="cuda")
        sl = lambda t: (t[:N_USERS * 64].view(N_USERS, 64), t[N_USERS * 64:(N_USERS + N_ITEMS) * 64].view(N_ITEMS, 64),  # noqa: E731
                        t[(N_USERS + N_ITEMS) * 64:])
        (U, V, bias), (gU, gV, gb) = sl(a.flat), sl(a.grad)
        for s in range(n_steps):
            _hip.check(L.skr_bpr_step(_hip.ptr(U), _hip.ptr(V), _hip.ptr(bias), _hip.ptr(U), _hip.ptr(V), _hip.ptr(u[s]), _hip.ptr(i[s]),
                                      _hip.ptr(j[s]), b, 1.0, 1e-3, 1.0, _hip.ptr(gU), _hip.ptr(gV), _hip.ptr(gb), _hip.ptr(gU),
                                      _hip.ptr(gV), _hip.ptr(r.loss_classic[s]), _hip.ptr(a.touch), _hip.ptr(a.grad), st()))
            a.step()
        r.classic = a
    c = DenseAdam(init.clone(), lr=1e-2)
    c.m.copy_(m0), c.v.copy_(v0)
    S = _hip.SKR_LOSS_SLOTS
    r.loss_slots = torch.zeros((n_steps, S, 2), device="cuda")
    fb = FusedBlocks(c, 0, N_USERS, N_USERS + N_ITEMS, 1e-3)
    fb._size(k, b)
    fb.work[:, :6 * fb.cap * 64] = SENTINEL
    fb.pre.fill_(SENTINEL)
    torch.cuda.synchronize()
    fb.run_blocks(u.data_ptr(), i.data_ptr(), j.data_ptr(), N_BLOCKS, k, b, r.loss_slots.data_ptr(), 8 * S)
    c.end_blocks()
    torch.cuda.synchronize()
    assert c.t == n_steps
    r.fused, r.fb = c, fb
    return r


@functools.lru_cache(maxsize=None)
def _distinct_case(k, b):
    return _launch_case(k, b, True, 9000 + 37 * k + b)


@functools.lru_cache(maxsize=None)
def _shared_case():
    return _launch_case(8, 259, False, 4242)


# 1, 3: fewer interactions than the workgroup has wavefronts; 5: a last workgroup whose id loads are clamped; 259: not a
# multiple of 4, more than one workgroup per loss slot
EDGES = [(k, b) for b in (1, 3, 5, 259) for k in (1, 7, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,b", EDGES)
def test_fused_launch_is_bit_identical_at_the_edges(k, b):
    import torch
    r = _distinct_case(k, b)
    a, c = r.classic, r.fused
    assert torch.equal(a.flat, c.flat)
    assert torch.equal(a.m, c.m) and torch.equal(a.v, c.v)
    assert float(r.fb.work[:, 6 * r.fb.cap * 64:].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("k,b", EDGES)
def test_fused_launch_loss_words(k, b):
    """per step, the sum over the slots of both loss words against the two-launch path; a wavefront without an interaction
    adds exactly nothing: with at most four interactions only the first workgroup's slot is ever written"""
    r = _distinct_case(k, b)
    got = r.loss_slots.sum(1).cpu().numpy()
    want = r.loss_classic.cpu().numpy()
    print(f"k={k} b={b}: largest relative loss difference {np.abs(got / want - 1).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-5)
    if b <= 4:
        assert float(r.loss_slots[:, 1:, :].abs().max()) == 0.0


@pytest.mark.gpu
def test_fused_launch_loss_words_with_rows_shared_inside_a_step():
    """float atomics on shared rows sum in an order that differs from launch to launch, in both paths: to rounding"""
    r = _shared_case()
    got = r.loss_slots.sum(1).cpu().numpy()
    want = r.loss_classic.cpu().numpy()
    print(f"largest relative loss difference {np.abs(got / want - 1).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-4)
    assert float(r.fb.work[:, 6 * r.fb.cap * 64:].abs().max()) == 0.0


def _pre_rows(r, q, n):
    """pre buffer q's planes, its first n slots ordered by the flat block they stand for (the numbering of the slots is the
    plan's atomics' and may differ from run to run)"""
    import torch
    fb = r.fb
    order = torch.argsort(fb.slot_block[q][:n])
    return fb.pre[q].view(3, fb.cap, 64)[:, :n][:, order]


@pytest.mark.gpu
def test_row_launches_keep_to_the_slots_in_use():
    """bpr_fused_end_kernel and bpr_fused_pre_kernel, two runs of a case with a lone last slot in an end launch: the same
    tables, moments and pre buffers bit for bit, equal to the two-launch path; the gradient planes are left zero; no slot
    past the block's count is touched in the planes the kernels do not own by contract (filled with SENTINEL beforehand)"""
    import torch
    k, b = 7, 259
    runs = [_launch_case(k, b, True, 555, classic=n == 1, need_odd_slots=True) for n in range(2)]
    ref = runs[1]
    assert any(n & 1 for n in ref.slots), ref.slots
    assert torch.equal(ref.classic.flat, ref.fused.flat)
    assert torch.equal(ref.classic.m, ref.fused.m) and torch.equal(ref.classic.v, ref.fused.v)
    for r in runs:
        fb, cap = r.fb, r.fb.cap
        # block 1 was planned into set 1, block 2 into set 0
        assert [int(fb.n_slots[0]), int(fb.n_slots[1])] == [r.slots[2], r.slots[1]]
        assert torch.equal(r.fused.flat, ref.fused.flat)
        assert torch.equal(r.fused.m, ref.fused.m) and torch.equal(r.fused.v, ref.fused.v)
        for q, n in ((0, r.slots[2]), (1, r.slots[1])):
            assert torch.equal(_pre_rows(r, q, n), _pre_rows(ref, q, n))
            assert bool((fb.pre[q].view(3, cap, 64)[:, n:] == SENTINEL).all())
        planes = fb.work[0].view(9, cap, 64)
        assert float(planes[6:].abs().max()) == 0.0
        assert bool((planes[:6, max(r.slots):] == SENTINEL).all())
