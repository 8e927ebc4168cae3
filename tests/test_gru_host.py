"""CPU suite of the GRU4RecPlus kernels' host side (csrc/gru.hip's argument checks, SessionGRU's block arithmetic): every check in
front of a launch answers -1 with a message in skr_last_error() before any pointer is used, so none of this needs a GPU."""
import numpy as np
import pytest
import torch

P = 16                                        # any non-NULL, aligned address: the checks fail before it is used
Q = 32                                        # a second one (the forward's new state must not be the old one)


def _lib():
    from skrec import _hip
    return _hip.lib()


def _fwd(L, B=4, in_dim=64, hid=64, act=0, h=P, h_new=Q):
    return L.skr_gru_cell_fwd(P, P, h, None, B, in_dim, hid, P, P, P, P, act, P, P, P, h_new, None)


def _bwd(L, B=4, in_dim=64, hid=64, act=0):
    return L.skr_gru_cell_bwd(P, P, P, B, in_dim, hid, P, P, act, P, P, P, P, P, P, P, P, P, P, None)


def _bwd_scatter(L, B=4, in_dim=64, hid=64, act=0, idx=P, g_table=P, touch=None, base=None):
    return L.skr_gru_cell_bwd_scatter(P, idx, P, B, in_dim, hid, P, P, act, P, P, P, P, P, P, P, P, P, P, 0.0, g_table, touch, base, None)


def _loss(L, B=4, hid=64, n_y=8, fact=0, loss=0):
    return L.skr_session_loss(P, B, hid, P, P, P, n_y, fact, loss, 1.0, P, P, P, None)


def _loss_sharded(L, B_local=4, hid=64, n_y=8, fact=0, loss=0, slot=0, B_global=4):
    return L.skr_session_loss_sharded(P, B_local, hid, P, P, P, n_y, fact, loss, 1.0, P, P, P, slot, B_global, None)


def _loss_grads(L, B_local=4, hid=64, n_y=8, fact=0, loss=0, slot=0, B_global=4, g_table=P, g_bias=P, touch=None, base=None):
    return L.skr_session_loss_grads(P, B_local, hid, P, P, P, n_y, fact, loss, 1.0, P, P, P, slot, B_global, 0.0, g_table, g_bias,
                                    touch, base, None)


def _out_grads(L, B=4, hid=64, n_y=8, touch=None, base=None):
    return L.skr_session_out_grads(P, P, B, hid, P, n_y, P, P, 0.0, P, P, touch, base, None)


def _scatter(L, n=4, dim=64, table=P, reg=0.0, touch=None, base=None):
    return L.skr_scatter_add_rows(P, P, n, dim, table, reg, P, touch, base, None)


def _refused(rc, L, *words):
    msg = L.skr_last_error()
    assert rc == -1 and msg, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_layer_sizes_are_checked():
    L = _lib()
    for call in (_fwd, _bwd, _bwd_scatter):
        _refused(call(L, hid=48), L, "32, 64 or 128", "48")
        _refused(call(L, in_dim=129), L, "in_dim <= 128", "129")
        _refused(call(L, in_dim=0), L, "in_dim")
    for call in (_loss, _loss_sharded, _loss_grads, _out_grads):
        _refused(call(L, hid=48), L, "32, 64 or 128", "48")
    _refused(_scatter(L, dim=0), L, "bad shape")


def test_unknown_kinds_are_named():
    L = _lib()
    for call in (_fwd, _bwd, _bwd_scatter):
        for act in (2, -1):
            _refused(call(L, act=act), L, "There is not hidden_act named '%d'." % act)
    for call in (_loss, _loss_sharded, _loss_grads):
        for fact in (3, -1):
            _refused(call(L, fact=fact), L, "There is not final_act named '%d'." % fact)
        for loss in (2, -1):
            _refused(call(L, loss=loss), L, "There is not loss named '%d'." % loss)


def test_batch_and_state_arguments_are_checked():
    L = _lib()
    _refused(_fwd(L, h=P, h_new=P), L, "in-place state")
    _refused(_fwd(L, B=-1), L, "bad batch")
    _refused(_bwd(L, B=-1), L, "negative batch")
    _refused(_bwd_scatter(L, B=-1), L, "negative batch")
    _refused(_scatter(L, n=-1), L, "bad shape")
    for call in (_loss, _out_grads):
        _refused(call(L, B=0), L)
        _refused(call(L, B=-3), L)
    _refused(_out_grads(L, n_y=0), L, "empty batch")
    _refused(L.skr_pop_sample(P, 0, None, 0, 4, P, None), L, "skr_pop_sample")
    _refused(L.skr_pop_sample(P, 5, None, 0, -1, P, None), L, "skr_pop_sample")
    # an empty batch is no error and launches nothing
    assert _fwd(L, B=0) == 0 and _bwd(L, B=0) == 0 and _bwd_scatter(L, B=0) == 0 and _scatter(L, n=0) == 0
    assert L.skr_pop_sample(P, 5, None, 0, 0, P, None) == 0


def test_loss_slots_and_target_counts_are_checked():
    L = _lib()
    _refused(_loss(L, B=9, n_y=8), L, "batch of 9 <= n_y = 8")                      # n_y < B_mean
    for call in (_loss_sharded, _loss_grads):
        _refused(call(L, B_local=4, slot=0, B_global=16, n_y=15), L, "batch of 16 <= n_y = 15")
        _refused(call(L, B_local=4, slot=13, B_global=16, n_y=40), L, "slots [13, 17) inside a batch of 16")
        _refused(call(L, B_local=4, slot=-1, B_global=16, n_y=40), L, "slots [-1, 3)")
        _refused(call(L, B_local=4, slot=0, B_global=4, n_y=8193), L, "n_y = 8193 <= 8192")
    _refused(_loss(L, n_y=8193), L, "n_y = 8193 <= 8192")
    _refused(_loss_grads(L, g_table=None), L, "skr_session_loss_grads: NULL")
    _refused(_loss_grads(L, g_bias=None), L, "skr_session_loss_grads: NULL")


def test_scatter_needs_its_table_and_touch_comes_in_pairs():
    L = _lib()
    _refused(_scatter(L, table=None, reg=0.5), L, "reg needs the table")
    _refused(_bwd_scatter(L, idx=None), L, "gathered input")
    _refused(_bwd_scatter(L, g_table=None), L, "gradient table")
    for call in (_scatter, _bwd_scatter, _out_grads, _loss_grads):
        _refused(call(L, touch=P, base=None), L, "touch: both pointers or neither")
        _refused(call(L, touch=None, base=P), L, "touch: both pointers or neither")


def blocks_of_rows(offset, rows, dim):
    """the 64-float blocks of a flat buffer that the rows [offset + r * dim, offset + r * dim + dim) overlap: mark_range's set"""
    out = set()
    for r in np.asarray(rows).reshape(-1):
        lo = offset + int(r) * dim
        out.update(range(lo >> 6, ((lo + dim - 1) >> 6) + 1))
    return out


@pytest.mark.parametrize("d", [1, 3, 32, 37, 48, 64, 100, 128])
def test_row_block_ids_name_every_block_a_row_overlaps(d):
    """SessionGRU.block_ids' arithmetic (row_block_ids) against the plain statement of the same set, row by row: a row that
    starts in the middle of a block overlaps more blocks than d // 64; the count per row is fixed and the padding names no
    block outside the row"""
    from skrec.recommender.GRU4RecPlus import row_block_ids
    rng = np.random.default_rng(d)
    idx = np.concatenate([np.arange(70), rng.integers(0, 100_000, 58), [2 ** 25 - 1]]).astype(np.int32).reshape(3, 43)
    o = 7
    got = row_block_ids(o, torch.from_numpy(idx), d).numpy()
    c = got.shape[1] // idx.shape[1]
    assert got.shape == (3, 43 * c) and got.dtype == np.int64
    per_row = got.reshape(3, 43, c)
    for s in range(3):
        for n in range(43):
            assert set(per_row[s, n].tolist()) == blocks_of_rows(64 * o, [idx[s, n]], d), (s, n, idx[s, n])
    # some row needs all c blocks (c is not an over-estimate)
    assert max(len(set(per_row[s, n].tolist())) for s in range(3) for n in range(43)) == c


@pytest.mark.parametrize("d,c", [(32, 1), (64, 1), (128, 2)])
def test_row_block_ids_of_the_shipped_widths_are_unchanged(d, c):
    """d = 32, 64, 128 (what GRU4RecPlus itself passes): first block + 0 .. c - 1, in this order"""
    from skrec.recommender.GRU4RecPlus import row_block_ids
    idx = torch.from_numpy(np.random.default_rng(1).integers(0, 50_000, (4, 9)).astype(np.int32))
    want = (5 + ((idx.long() * d) >> 6).unsqueeze(2) + torch.arange(c)).reshape(4, -1)
    assert torch.equal(row_block_ids(5, idx, d), want)
