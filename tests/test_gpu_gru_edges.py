"""GPU parity of csrc/gru.hip where tests/test_gpu_gru.py does not reach: the 16-row backward (more than 2048 sessions), input widths
that are no multiple of 4, buffers that already hold gradients, the 256-thread kernels behind SKR_GRU_SPLIT=0, saturated gates, logits
far from 1 (large, very negative, tied), one shard of a session-sharded loss against its rows of the whole batch, the touch bytes
block by block, and the popularity sampler's corners.

The reference is oracle/gru4rec.py called with torch.float64 tensors (autograd supplies the gradients); the tolerances are those of
tests/test_gpu_gru.py unless a test states another one and where it comes from."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gru4rec as G
from gpu_utils import to_dev
from skrec import _hip
from test_gpu_gru import _cell, _close
from test_gru_host import blocks_of_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

HERE = os.path.dirname(os.path.abspath(__file__))
HIDDEN = {"tanh": 0, "relu": 1}
FINAL = {"linear": 0, "relu": 1, "leaky_relu": 2}
LOSS = {"bpr_max": 0, "top1_max": 1}
GRADS = ("gWg", "gbg", "gWc", "gbc")


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _cell64(x, hprev, cell, act, dh):
    """oracle/gru4rec.py's cell on float64 tensors, autograd for dL/d. of L = sum(h' * dh).  Every session gets its own copy of the two
    bias rows: the gradient of a session's copy is that session's pre-activation gradient (their sum over the sessions the bias
    gradient), and |A|^T |D| -- the sum of the magnitudes of a weight gradient's B terms -- follows from it."""
    Wg, bg, Wc, bc = cell
    B = x.shape[0]
    tx, th, tWg, tWc = _t64(x, True), _t64(hprev), _t64(Wg, True), _t64(Wc, True)
    tbg, tbc = _t64(np.tile(bg, (B, 1)), True), _t64(np.tile(bc, (B, 1)), True)
    hn = G.gru_cell(tx, th, tWg, tbg, tWc, tbc, act)
    (hn * _t64(dh)).sum().backward()
    with torch.no_grad():
        H = th.shape[1]
        gates = torch.sigmoid(torch.cat([tx, th], 1) @ tWg + tbg)
        r, u = gates[:, :H], gates[:, H:]
        a_c = torch.cat([tx, r * th], 1)
        c = G.ACTS[act](a_c @ tWc + tbc)
        assert float((u * th + (1.0 - u) * c - hn).abs().max()) < 1e-13
        mass_g = torch.cat([tx, th], 1).abs().t() @ tbg.grad.abs()
        mass_c = a_c.abs().t() @ tbc.grad.abs()
    n = lambda t: t.detach().numpy()  # noqa: E731
    return dict(out=n(hn), r=n(r), u=n(u), c=n(c), dx=n(tx.grad), gWg=n(tWg.grad), gbg=n(tbg.grad.sum(0)), gWc=n(tWc.grad),
                gbc=n(tbc.grad.sum(0)), dg=n(tbg.grad), dc=n(tbc.grad), mass_g=n(mass_g), mass_c=n(mass_c))


def _case(seed, i_d, h, B, scale=1.0, n_rows=300):
    """the inputs of test_gru_cell_fwd_bwd: an embedding table with the sessions' row ids, the old state, the cell (its two kernels
    times `scale`), the incoming gradient"""
    rng = np.random.default_rng(seed)
    table = (0.5 * rng.standard_normal((n_rows, i_d))).astype(np.float32)
    idx = rng.integers(0, n_rows, B).astype(np.int32)
    hprev = (0.5 * rng.standard_normal((B, h))).astype(np.float32)
    Wg, bg, Wc, bc = _cell(rng, i_d, h)
    cell = ((scale * Wg).astype(np.float32), bg, (scale * Wc).astype(np.float32), bc)
    dh = rng.standard_normal((B, h)).astype(np.float32)
    return table, idx, hprev, cell, dh


def _upload(x, idx, hprev, cell, dh):
    d = {k: to_dev(v) for k, v in dict(x=x, h=hprev, Wg=cell[0], bg=cell[1], Wc=cell[2], bc=cell[3], dh=dh).items()}
    d["idx"] = None if idx is None else to_dev(idx)
    return d


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _forward(d, act):
    """-> r, u, c, h' (every output buffer starts as NaN: an element the kernel leaves out fails the comparison)"""
    B, h = d["h"].shape
    r, u, c, out = (_nan(B, h) for _ in range(4))
    _hip.check(_hip.lib().skr_gru_cell_fwd(_hip.ptr(d["x"]), _hip.ptr(d["idx"]), _hip.ptr(d["h"]), None, B, d["x"].shape[1], h,
                                           _hip.ptr(d["Wg"]), _hip.ptr(d["bg"]), _hip.ptr(d["Wc"]), _hip.ptr(d["bc"]), HIDDEN[act],
                                           _hip.ptr(r), _hip.ptr(u), _hip.ptr(c), _hip.ptr(out), _hip.stream()))
    return r, u, c, out


def _backward(d, act, gates, grads=None, scatter=None):
    """skr_gru_cell_bwd, or with scatter = (reg, g_table, touch, touch_base) skr_gru_cell_bwd_scatter
    -> dict(gWg, gbg, gWc, gbc, dx, work); `grads`: the four accumulators to add into (fresh zeros otherwise)"""
    B, h = d["h"].shape
    i_d = d["x"].shape[1]
    r, u, c = gates
    g = grads if grads is not None else [torch.zeros_like(d[k]) for k in ("Wg", "bg", "Wc", "bc")]
    dx, work = _nan(B, i_d), _nan(3 * B * h)
    L, st = _hip.lib(), _hip.stream()
    head = (_hip.ptr(d["x"]), _hip.ptr(d["idx"]), _hip.ptr(d["h"]), B, i_d, h, _hip.ptr(d["Wg"]), _hip.ptr(d["Wc"]), HIDDEN[act],
            _hip.ptr(r), _hip.ptr(u), _hip.ptr(c), _hip.ptr(d["dh"]), _hip.ptr(g[0]), _hip.ptr(g[1]), _hip.ptr(g[2]), _hip.ptr(g[3]),
            _hip.ptr(dx), _hip.ptr(work))
    if scatter is None:
        _hip.check(L.skr_gru_cell_bwd(*head, st))
    else:
        reg, g_table, touch, base = scatter
        _hip.check(L.skr_gru_cell_bwd_scatter(*head, reg, _hip.ptr(g_table), _hip.ptr(touch), _hip.ptr(base), st))
    torch.cuda.synchronize()
    res = dict(zip(GRADS, g))
    res.update(dx=dx, work=work)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_backward(got, o, weights_by_mass=0):
    """dx, the bias gradients and the pre-activation gradients of the work buffer at test_gru_cell_fwd_bwd's tolerance; the weight
    gradients too, or (weights_by_mass = B) element by element inside (B + 2) 2^-24 |A|^T |D| + 1e-6: a thread adds a weight's B
    products in session order in fp32, the a-priori bound of such a sum (B - 1 additions, the product, the rounded r*h)"""
    B, h = o["dc"].shape
    for k in ("dx", "gbg", "gbc"):
        print(k, np.abs(got[k] - o[k]).max() / np.abs(o[k]).max())
        _close(got[k], o[k], 2e-5)
    _close(got["work"][:B * h].reshape(B, h), o["dc"], 2e-5)
    _close(got["work"][B * h:].reshape(B, 2 * h), o["dg"], 2e-5)
    for k, m in (("gWg", "mass_g"), ("gWc", "mass_c")):
        err = np.abs(got[k] - o[k])
        print(k, err.max() / np.abs(o[k]).max(), "of the a-priori bound:", (err / ((B + 2) * 2.0 ** -24 * o[m] + 1e-6)).max())
        if weights_by_mass:
            assert weights_by_mass == B and np.all(err <= (B + 2) * 2.0 ** -24 * o[m] + 1e-6), k
        else:
            _close(got[k], o[k], 2e-5)


def _scattered(idx, rows, n_rows):
    want = np.zeros((n_rows, rows.shape[1]), np.float64)
    np.add.at(want, idx, rows)
    return want


# ---- 1. more than 2048 sessions: gru_bwd_rows_kernel<16, H> ---------------------------------------------------------------------
@pytest.mark.parametrize("i_d,h,B,act,dense", [(64, 64, 2049, "tanh", False), (37, 32, 2100, "relu", False), (128, 128, 2064, "tanh", True)])
def test_backward_for_many_sessions(i_d, h, B, act, dense):
    """SessionGRU.train_step with a batch_size above 2048: 16 sessions per workgroup, one weight row per reduction; a ragged last
    workgroup (2049 = 128 * 16 + 1), an input width that is no multiple of 4, gathered and dense (x_index = NULL) input rows"""
    table, idx, hprev, cell, dh = _case(i_d + h + B, i_d, h, B)
    x = table[idx]
    o = _cell64(x, hprev, cell, act, dh)
    d = _upload(x, None, hprev, cell, dh) if dense else _upload(table, idx, hprev, cell, dh)
    r, u, c, out = _forward(d, act)
    _close(out.cpu().numpy(), o["out"], 2e-5, 2e-6)
    _check_backward(_backward(d, act, (r, u, c)), o, weights_by_mass=B)


# ---- 2. input widths that are no multiple of 4: the clamped weight row of the 4-row kernel ----------------------------------------
@pytest.mark.parametrize("i_d,h,B,act", [(37, 64, 7, "tanh"), (1, 128, 5, "relu"), (3, 32, 130, "tanh"), (100, 32, 33, "relu")])
def test_backward_at_ragged_input_widths(i_d, h, B, act):
    """test_gru_cell_fwd_bwd's checks where the last group of four input columns is incomplete (a weight row past the end is
    computed from row in_dim - 1 and not stored), down to a single input column.  (hid = 32 from NaN-filled output buffers is
    also what showed lanes 32 .. 63 of the backward multiplying a zero weight with whatever LDS held.)"""
    n_rows = 300
    table, idx, hprev, cell, dh = _case(i_d + h + B, i_d, h, B, n_rows=n_rows)
    o = _cell64(table[idx], hprev, cell, act, dh)
    d = _upload(table, idx, hprev, cell, dh)
    r, u, c, out = _forward(d, act)
    _close(out.cpu().numpy(), o["out"])
    plain = _backward(d, act, (r, u, c))
    _check_backward(plain, o)
    L, st = _hip.lib(), _hip.stream()
    gtab, d_dx = torch.zeros((n_rows, i_d), device="cuda"), to_dev(plain["dx"])
    _hip.check(L.skr_scatter_add_rows(_hip.ptr(d_dx), _hip.ptr(d["idx"]), B, i_d, None, 0.0, _hip.ptr(gtab), None, None, st))
    want_tab = _scattered(idx, o["dx"], n_rows)
    _close(gtab.cpu().numpy(), want_tab, 2e-5)
    # the one-call form: weight gradients and dx bit for bit, the table gradient with the l2 term of the looked-up rows
    reg = 0.03
    gtab2 = torch.zeros((n_rows, i_d), device="cuda")
    one = _backward(d, act, (r, u, c), scatter=(reg, gtab2, None, None))
    for k in GRADS + ("dx", "work"):
        assert np.array_equal(one[k], plain[k]), k
    counts = np.bincount(idx, minlength=n_rows).astype(np.float64)
    _close(gtab2.cpu().numpy(), want_tab + reg * counts[:, None] * table, 2e-5)


# ---- 3. the accumulators are added into ----------------------------------------------------------------------------------------
def test_gradients_accumulate_onto_what_the_buffers_hold():
    """gru_bwd_weights_kernel's `+=` and the scatters' atomic adds: from buffers that already hold a pattern the result is the
    pattern plus the gradient, and a second identical call adds the gradient once more"""
    i_d, h, B, act, n_rows, reg = 48, 32, 5, "tanh", 300, 0.03
    table, idx, hprev, cell, dh = _case(i_d + h + B, i_d, h, B, n_rows=n_rows)
    o = _cell64(table[idx], hprev, cell, act, dh)
    o["gtab"] = _scattered(idx, o["dx"], n_rows) + reg * np.bincount(idx, minlength=n_rows)[:, None] * table.astype(np.float64)
    d = _upload(table, idx, hprev, cell, dh)
    gates = _forward(d, act)[:3]
    shapes = dict(gWg=(i_d + h, 2 * h), gbg=(2 * h,), gWc=(i_d + h, h), gbc=(h,), gtab=(n_rows, i_d))
    # a fixed pattern of the gradients' own magnitude (an overwrite instead of an add misses it by the pattern)
    pat = {k: (np.abs(o[k]).max() * np.sin(0.37 * np.arange(int(np.prod(s))) + 1.0)).astype(np.float32).reshape(s) for k, s in shapes.items()}
    acc = {k: to_dev(v) for k, v in pat.items()}
    gtab_plain = to_dev(pat["gtab"])
    L, st = _hip.lib(), _hip.stream()
    for n_calls in (1, 2):
        got = _backward(d, act, gates, grads=[acc[k] for k in GRADS], scatter=(reg, acc["gtab"], None, None))
        for k in GRADS:
            _close(got[k], pat[k].astype(np.float64) + n_calls * o[k], 2e-5)
        _close(acc["gtab"].cpu().numpy(), pat["gtab"].astype(np.float64) + n_calls * o["gtab"], 2e-5)
        # the scatter as a launch of its own
        d_dx = to_dev(got["dx"])
        _hip.check(L.skr_scatter_add_rows(_hip.ptr(d_dx), _hip.ptr(d["idx"]), B, i_d, _hip.ptr(d["x"]), reg, _hip.ptr(gtab_plain),
                                          None, None, st))
        _close(gtab_plain.cpu().numpy(), pat["gtab"].astype(np.float64) + n_calls * o["gtab"], 2e-5)


# ---- 4. SKR_GRU_SPLIT=0: gru_fwd_kernel<4, 128, true> at 128/128 and the 256-thread gru_bwd_rows_kernel<4, H> ---------------------
def _split_case(i_d, h, B, act, save_to=None, gates_from=None):
    """forward and backward at one shape against the fp64 oracle.  save_to: keep the saved gates and every backward output in an
    .npz; gates_from: such a file -- the backward then runs on ITS gates (the two forward kernels at 128/128 differ in the last
    bits by design, and a backward is comparable bit for bit only from the same r, u, c) and is returned"""
    table, idx, hprev, cell, dh = _case(i_d + h + B, i_d, h, B)
    o = _cell64(table[idx], hprev, cell, act, dh)
    d = _upload(table, idx, hprev, cell, dh)
    r, u, c, out = _forward(d, act)
    _close(out.cpu().numpy(), o["out"])
    for t, k in ((r, "r"), (u, "u"), (c, "c")):
        _close(t.cpu().numpy(), o[k])
    got = _backward(d, act, (r, u, c))
    _check_backward(got, o)
    if save_to:
        np.savez(save_to, r=r.cpu().numpy(), u=u.cpu().numpy(), c=c.cpu().numpy(), **got)
    if gates_from:
        f = np.load(gates_from)
        return _backward(d, act, tuple(to_dev(f[k]) for k in "ruc"))


@pytest.mark.parametrize("i_d,h,B,act", [(128, 128, 37, "tanh"), (64, 128, 16, "relu")])
def test_narrow_kernels_behind_the_split_switch(i_d, h, B, act, tmp_path):
    """SKR_GRU_SPLIT=0 (read once per process, so a fresh child process): the generic forward at the benchmarked shape and the
    256-thread backward against the fp64 oracle; and the backward's outputs -- dx, the four weight gradients, the work buffer --
    bit for bit equal to the default 1 024-thread form's from the same gates: a weight row is reduced by one wavefront through
    the same reduce16 tree whichever wavefront takes it, and the weights kernel is shared"""
    path = str(tmp_path / "narrow.npz")
    code = ("import os, sys; os.environ['SKR_GRU_SPLIT'] = '0'; sys.path[:0] = [%r, %r, %r]; import test_gpu_gru_edges as t; "
            "t._split_case(%d, %d, %d, %r, save_to=%r)" % (HERE, os.path.join(HERE, ".."), os.path.join(HERE, "..", "scikit-recommender_amd"),
                                                          i_d, h, B, act, path))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.join(HERE, ".."))
    narrow = np.load(path)
    wide = _split_case(i_d, h, B, act, gates_from=path)
    for k in GRADS + ("dx", "work"):
        assert np.array_equal(narrow[k], wide[k]), k


# ---- 5. saturated gates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i_d,h,B,act", [(64, 64, 16, "tanh"), (37, 64, 7, "relu"), (128, 128, 2049, "tanh")])
def test_saturated_gates(i_d, h, B, act):
    """both kernels of the cell times 8: r and u come within an ulp of 0 and 1 (at the largest shape 27 of them round to exactly
    1: their derivatives to 0), tanh's 1 - c*c cancels; the small-batch kernels and the many-session pair (matrix-core forward,
    16-row backward)"""
    table, idx, hprev, cell, dh = _case(i_d + h + B, i_d, h, B, scale=8.0)
    o = _cell64(table[idx], hprev, cell, act, dh)
    d = _upload(table, idx, hprev, cell, dh)
    r, u, c, out = _forward(d, act)
    tol = (2e-5, 2e-6) if B > 2048 else (1e-5, 1e-6)          # (test_gru_cell_forward_for_many_sessions' / test_gru_cell_fwd_bwd's)
    rr, uu = r.cpu().numpy(), u.cpu().numpy()
    assert (rr >= 0).all() and (rr <= 1).all() and (uu >= 0).all() and (uu <= 1).all()
    print("gates at exactly 0 or 1:", int(((rr == 0) | (rr == 1)).sum()), int(((uu == 0) | (uu == 1)).sum()), "of", rr.size)
    for t, k in ((r, "r"), (u, "u"), (c, "c"), (out, "out")):
        assert np.isfinite(t.cpu().numpy()).all()
        _close(t.cpu().numpy(), o[k], *tol)
    got = _backward(d, act, (r, u, c))
    assert all(np.isfinite(v).all() for v in got.values())
    _check_backward(got, o)


# ---- 6. the loss away from |logit| ~ 1 ---------------------------------------------------------------------------------------------
def _loss_oracle(E, bias, out, Y, fact, loss, reg, bpr_reg, dtype):
    """test_session_loss_and_grads' oracle in `dtype`, and the gradient of the pre-activation logits (the kernels' dlogits)"""
    tE, tb, to = (torch.tensor(np.asarray(a, dtype), requires_grad=True) for a in (E, bias, out))
    Yl = torch.as_tensor(Y, dtype=torch.long)
    items, bs = tE[Yl], tb[Yl]
    pre = to @ items.t() + bs
    pre.retain_grad()
    logits = G.final_act(pre, fact)
    main = G.bpr_max_loss(logits, bpr_reg) if loss == "bpr_max" else G.top1_max_loss(logits)
    (main + reg * 0.5 * (items.pow(2).sum() + bs.pow(2).sum())).backward()
    return dict(loss=np.float64(main.item()), dlog=pre.grad.numpy(), dout=to.grad.numpy(), gE=tE.grad.numpy(), gb=tb.grad.numpy())


def _loss_device(E, bias, out, Y, fact, loss, reg, bpr_reg, one_call, slot=0, B_global=None, sharded=False):
    """skr_session_loss (or _sharded) + skr_session_out_grads, or the one call skr_session_loss_grads; every output buffer dirty"""
    B, h = out.shape
    n_y = len(Y)
    L, st = _hip.lib(), _hip.stream()
    dE, db, do, dY = to_dev(E), to_dev(bias), to_dev(out), to_dev(Y)
    dlog, dout, lossbuf = _nan(B, n_y), _nan(B, h), _nan(1)
    gE, gb = torch.zeros_like(dE), torch.zeros_like(db)
    fk, lk = FINAL[fact], LOSS[loss]
    B_global = B if B_global is None else B_global
    head = (_hip.ptr(do), B, h, _hip.ptr(dE), _hip.ptr(db), _hip.ptr(dY), n_y, fk, lk, bpr_reg, _hip.ptr(dlog), _hip.ptr(dout), _hip.ptr(lossbuf))
    if one_call:
        _hip.check(L.skr_session_loss_grads(*head, slot, B_global, reg, _hip.ptr(gE), _hip.ptr(gb), None, None, st))
    else:
        if sharded:
            _hip.check(L.skr_session_loss_sharded(*head, slot, B_global, st))
        else:
            assert slot == 0 and B_global == B
            _hip.check(L.skr_session_loss(*head, st))
        _hip.check(L.skr_session_out_grads(_hip.ptr(dlog), _hip.ptr(do), B, h, _hip.ptr(dY), n_y, _hip.ptr(dE), _hip.ptr(db), reg,
                                           _hip.ptr(gE), _hip.ptr(gb), None, None, st))
    torch.cuda.synchronize()
    return dict(loss=np.float64(lossbuf.cpu().numpy()[0]), dlog=dlog.cpu().numpy(), dout=dout.cpu().numpy(), gE=gE.cpu().numpy(),
                gb=gb.cpu().numpy())


def _check_loss(got, want, floor=None, tag=""):
    """test_session_loss_and_grads' tolerances against the fp64 oracle: 2e-5 relative + 1e-7 for the loss, 5e-5 of a tensor's
    largest magnitude + 1e-7 for the gradients (dlogits, which that test does not compare, like the others); `floor`: per tensor
    the fp32-CPU restatement's own largest error, of which four times is allowed where that is more"""
    for k in ("loss", "dlog", "dout", "gE", "gb"):
        assert np.isfinite(got[k]).all(), k
        err = np.abs(np.asarray(got[k], np.float64) - want[k]).max()
        scale = np.abs(want[k]).max()
        tol = (2e-5 if k == "loss" else 5e-5) * scale + 1e-7
        if floor is not None:
            print(f"{tag} {k}: kernel error {err:.3e}, fp32-CPU error {floor[k]:.3e}, plain tolerance {tol:.3e}")
            tol = max(tol, 4.0 * floor[k])
        assert err <= tol, (k, err, tol)


def _loss_inputs(kind, B=5, S=59, h=32, n_items=200, seed=5):
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((n_items, h))
    bias = 0.1 * rng.standard_normal(n_items)
    out = rng.standard_normal((B, h))
    Y = rng.permutation(n_items)[:B + S].astype(np.int32)
    if kind == "hot":          # logits from -76 to +83
        out = (30.0 / np.sqrt(h)) * out
    elif kind == "hotter":     # logits from -101 to +111: past log(FLT_MAX) = 88.7, exp overflows without the shift by the row's max
        out = (40.0 / np.sqrt(h)) * out
    elif kind == "cold":       # every logit in [-47, -32]: the max is the masked column's 0 and z about 1e-14 (relu: all logits 0, a tie)
        out, E, bias = 0.5 * out, 0.3 * E, -40.0 + bias
    elif kind == "tied":       # every target row and bias word the same: a row's logits are all equal
        out, E, bias = 0.5 * out, np.tile(0.3 * E[:1], (n_items, 1)), np.full(n_items, 0.1)
    else:                      # test_session_loss_and_grads' law
        out, E = 0.5 * out, 0.3 * E
    return E.astype(np.float32), bias.astype(np.float32), out.astype(np.float32), Y


@pytest.mark.parametrize("one_call", [False, True])
@pytest.mark.parametrize("kind", ["hot", "hotter", "cold", "tied"])
@pytest.mark.parametrize("loss", ["bpr_max", "top1_max"])
@pytest.mark.parametrize("fact", ["linear", "relu", "leaky_relu"])
def test_loss_on_large_negative_and_tied_logits(loss, fact, kind, one_call):
    """a softmax without the `- mx` shift, a max taken without the masked column's 0, a 1e-24 guard in another place all pass at
    |logit| ~ 1 and none passes here.  `hot` reaches +83, which float32's exp still holds (log FLT_MAX = 88.7): a kernel without
    the shift passes it and fails `hotter` (+111).  Tolerances of test_session_loss_and_grads, but for the two hot inputs: there
    float32 itself cancels, so a tensor may differ by max(that tolerance, 4 x the fp32-CPU restatement's own largest error
    against fp64) -- 4 for the kernel's other summation order and its float atomics.

    Measured on an MI355X at `hot` (largest absolute error against fp64: kernel / fp32-CPU restatement / plain tolerance; the
    three final activations and the two forms of the call alike to the digits given):
      bpr_max   loss 3.5e-4 / 1.4e-4 / 6.9e-2   dlogits 6.2e-5 / 5.8e-5 / 1.2e-3   dout 2.0e-4 / 1.9e-4 / 2.6e-3
                gE 9.3e-4 / 8.7e-4 / 1.4e-2     gb 6.2e-5 / 5.8e-5 / 1.2e-3
      top1_max  loss 2.3e-8 / 9.6e-8 / 4.0e-5   dlogits 3.2e-10 / 9.4e-9 / 1.0e-7   dout 7.2e-10 / 2.2e-8 / 1.0e-7
                gE 3.6e-9 / 1.4e-7 / 1.8e-6     gb 3.1e-10 / 9.4e-9 / 2.3e-7
    (top1_max before the row kernel carried 2 - q_y instead of q_y: dlogits 4.7e-8, dout 1.3e-7 -- over both allowances.)"""
    E, bias, out, Y = _loss_inputs(kind)
    reg, bpr_reg = 0.01, 0.7
    want = _loss_oracle(E, bias, out, Y, fact, loss, reg, bpr_reg, np.float64)
    assert all(np.isfinite(v).all() for v in want.values())
    floor = None
    if kind in ("hot", "hotter"):
        cpu32 = _loss_oracle(E, bias, out, Y, fact, loss, reg, bpr_reg, np.float32)
        floor = {k: np.abs(np.asarray(cpu32[k], np.float64) - want[k]).max() for k in want}
    got = _loss_device(E, bias, out, Y, fact, loss, reg, bpr_reg, one_call)
    _check_loss(got, want, floor, tag=f"{loss}/{fact}/{'one call' if one_call else 'three launches'}")


@pytest.mark.parametrize("one_call", [False, True])
@pytest.mark.parametrize("loss", ["bpr_max", "top1_max"])
@pytest.mark.parametrize("B,S,h", [(1, 1, 32), (130, 70, 64), (16, 8176, 32)])
def test_loss_at_shapes_the_model_never_uses(B, S, h, loss, one_call):
    """one session with one other target; 130 sessions (skr_session_out_grads' 64-session loop twice and a tail of 2, nine tiles
    of 16 sessions in dL/dout, the last one ragged); n_y = 8192 exactly, the row buffer's size"""
    rng = np.random.default_rng(B + S + h)
    n_items = 500
    E = (0.3 * rng.standard_normal((n_items, h))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(n_items)).astype(np.float32)
    out = (0.5 * rng.standard_normal((B, h))).astype(np.float32)
    Y = rng.integers(0, n_items, B + S).astype(np.int32)          # repeated targets
    want = _loss_oracle(E, bias, out, Y, "leaky_relu", loss, 0.01, 0.7, np.float64)
    _check_loss(_loss_device(E, bias, out, Y, "leaky_relu", loss, 0.01, 0.7, one_call), want)


def test_loss_refuses_more_targets_than_its_row_buffer_holds():
    L = _hip.lib()
    B, h, n_y = 4, 32, 8193
    out, E, bias = torch.zeros((B, h), device="cuda"), torch.zeros((10, h), device="cuda"), torch.zeros(10, device="cuda")
    Y = torch.zeros(n_y, dtype=torch.int32, device="cuda")
    dlog, dout, loss = torch.zeros((B, n_y), device="cuda"), torch.full((B, h), 3.0, device="cuda"), torch.full((1,), 7.0, device="cuda")
    gE, gb = torch.zeros_like(E), torch.zeros_like(bias)
    head = (_hip.ptr(out), B, h, _hip.ptr(E), _hip.ptr(bias), _hip.ptr(Y), n_y, 0, 0, 1.0, _hip.ptr(dlog), _hip.ptr(dout), _hip.ptr(loss))
    assert L.skr_session_loss(*head, _hip.stream()) == -1 and b"8193 <= 8192" in L.skr_last_error()
    assert L.skr_session_loss_sharded(*head, 0, B, _hip.stream()) == -1
    assert L.skr_session_loss_grads(*head, 0, B, 0.0, _hip.ptr(gE), _hip.ptr(gb), None, None, _hip.stream()) == -1
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((dout == 3.0).all())            # nothing was launched


# ---- 7. a shard of the batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,fact", [("bpr_max", "linear"), ("top1_max", "leaky_relu")])
def test_a_shard_equals_its_rows_of_the_full_batch(loss, fact):
    """session rows [slot, slot + 8) of 24 through skr_session_loss_sharded and through skr_session_loss_grads: the row kernel is
    the same with the same mean, so dlogits equals the full call's rows bit for bit -- a positive taken from column `row` instead
    of `slot + row` does not; the loss words add up to the full loss, dL/dout rows and the summed output-side gradients agree
    within the one-call form's tolerance (float atomics); the full call itself against the fp64 oracle"""
    B, S, h, n_items = 24, 40, 64, 90
    rng = np.random.default_rng(B + S + h)
    E = (0.3 * rng.standard_normal((n_items, h))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(n_items)).astype(np.float32)
    out = (0.5 * rng.standard_normal((B, h))).astype(np.float32)
    Y = rng.integers(0, n_items, B + S).astype(np.int32)
    Y[3], Y[17] = Y[B + 1], Y[5]                       # a negative equal to a positive, two sessions with the same positive
    reg, bpr_reg = 0.01, 0.7
    full = _loss_device(E, bias, out, Y, fact, loss, reg, bpr_reg, one_call=True)
    _check_loss(full, _loss_oracle(E, bias, out, Y, fact, loss, reg, bpr_reg, np.float64))
    for one_call in (False, True):
        parts = []
        for slot in (0, 8, 16):
            # the l2 term of the shared target rows once, with the first shard (as ShardedSessionGRU's rank 0 adds it)
            p = _loss_device(E, bias, out[slot:slot + 8], Y, fact, loss, reg if slot == 0 else 0.0, bpr_reg, one_call, slot=slot,
                             B_global=B, sharded=True)
            assert np.array_equal(p["dlog"], full["dlog"][slot:slot + 8]), (one_call, slot)
            _close(p["dout"], full["dout"][slot:slot + 8], 2e-6, 1e-8)
            parts.append(p)
        total = sum(p["loss"] for p in parts)
        assert abs(total - full["loss"]) <= 1e-6 * abs(full["loss"]), (total, full["loss"])
        _close(sum(p["gE"].astype(np.float64) for p in parts), full["gE"], 2e-6, 1e-8)
        _close(sum(p["gb"].astype(np.float64) for p in parts), full["gb"], 2e-6, 1e-8)


# ---- 8. touch bytes ----------------------------------------------------------------------------------------------------------------
class _Flat(object):
    """a flat gradient buffer with DenseAdam's byte per 64-float block; some bytes hold the sticky 2 beforehand"""

    def __init__(self, n_floats, expected, rng):
        assert n_floats % 64 == 0
        self.grad = torch.zeros(n_floats, device="cuda")
        self.n_blocks = n_floats // 64
        self.expected = sorted(expected)
        assert self.expected and self.expected[-1] < self.n_blocks
        others = sorted(set(range(self.n_blocks)) - set(expected))
        self.sticky = list(rng.choice(self.expected, min(3, len(self.expected)), replace=False)) + list(rng.choice(others, 3, replace=False))
        before = np.zeros(self.n_blocks, np.uint8)
        before[self.sticky] = 2
        self.touch = to_dev(before)

    def view(self, start, shape):
        assert start % 64 == 0
        return self.grad[start:start + int(np.prod(shape))].view(*shape)

    def check(self):
        """a byte that held 2 still holds 2, every other block a row overlaps holds 1, everything else 0"""
        torch.cuda.synchronize()
        want = np.zeros(self.n_blocks, np.uint8)
        want[self.expected] = 1
        want[self.sticky] = 2
        got = self.touch.cpu().numpy()
        assert np.array_equal(got, want), (np.flatnonzero(got != want), got[got != want], want[got != want])


@pytest.mark.parametrize("dim", [48, 100])
def test_touch_bytes_of_scattered_rows(dim):
    """skr_scatter_add_rows: rows of 48 / 100 floats start in the middle of a block and overlap two / up to three"""
    rng = np.random.default_rng(dim)
    n_rows, n, start = 40, 13, 128
    idx = rng.integers(0, n_rows, n).astype(np.int32)
    idx[5] = idx[2]
    src = rng.standard_normal((n, dim)).astype(np.float32)
    f = _Flat(start + 4096 + 128, blocks_of_rows(start, idx, dim), rng)
    g_table = f.view(start, (n_rows, dim))
    d_src, d_idx = to_dev(src), to_dev(idx)          # (named: a temporary's memory may be handed to the next upload before the launch)
    _hip.check(_hip.lib().skr_scatter_add_rows(_hip.ptr(d_src), _hip.ptr(d_idx), n, dim, None, 0.0, _hip.ptr(g_table),
                                               _hip.ptr(f.touch), _hip.ptr(f.grad), _hip.stream()))
    f.check()
    _close(g_table.cpu().numpy(), _scattered(idx, src.astype(np.float64), n_rows), 2e-6)
    assert float(f.grad[:start].abs().max()) == 0.0 and float(f.grad[start + n_rows * dim:].abs().max()) == 0.0


def test_touch_bytes_of_the_first_layers_backward():
    """skr_gru_cell_bwd_scatter at in_dim = 48: the input rows' blocks and nothing else (the weight gradients carry no marks)"""
    i_d, h, B, act, n_rows, start = 48, 32, 5, "tanh", 300, 192
    table, idx, hprev, cell, dh = _case(i_d + h + B, i_d, h, B, n_rows=n_rows)
    d = _upload(table, idx, hprev, cell, dh)
    gates = _forward(d, act)[:3]
    f = _Flat(start + n_rows * i_d + 64, blocks_of_rows(start, idx, i_d), np.random.default_rng(1))
    g_table = f.view(start, (n_rows, i_d))
    got = _backward(d, act, gates, scatter=(0.0, g_table, f.touch, f.grad))
    f.check()
    _close(g_table.cpu().numpy(), _scattered(idx, got["dx"].astype(np.float64), n_rows), 2e-6)


@pytest.mark.parametrize("one_call", [False, True])
@pytest.mark.parametrize("h", [32, 128])
def test_touch_bytes_of_the_output_side_gradients(h, one_call):
    """skr_session_out_grads / skr_session_loss_grads: the target rows' blocks (h = 32: two rows share one, h = 128: a row fills
    two) and the block of every target's bias word"""
    rng = np.random.default_rng(h)
    B, S, n_items = 5, 12, 150
    Y = np.concatenate([rng.integers(0, 40, B + S - 6), rng.integers(130, n_items, 4), [6, 7]]).astype(np.int32)   # bias blocks 0 and 2
    rng.shuffle(Y)
    E = (0.3 * rng.standard_normal((n_items, h))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(n_items)).astype(np.float32)
    out = (0.5 * rng.standard_normal((B, h))).astype(np.float32)
    e_at, b_at = 64, 64 + n_items * h
    assert b_at % 64 == 0
    expected = blocks_of_rows(e_at, Y, h) | {(b_at + int(y)) >> 6 for y in Y}
    assert (b_at + 64) >> 6 not in expected
    f = _Flat(b_at + 192 + 64, expected, rng)
    gE, gb = f.view(e_at, (n_items, h)), f.view(b_at, (n_items,))
    L, st = _hip.lib(), _hip.stream()
    dE, db, do, dY = to_dev(E), to_dev(bias), to_dev(out), to_dev(Y)
    n_y = len(Y)
    dlog, dout, loss = _nan(B, n_y), _nan(B, h), _nan(1)
    if one_call:
        _hip.check(L.skr_session_loss_grads(_hip.ptr(do), B, h, _hip.ptr(dE), _hip.ptr(db), _hip.ptr(dY), n_y, 0, 0, 0.7, _hip.ptr(dlog),
                                            _hip.ptr(dout), _hip.ptr(loss), 0, B, 0.01, _hip.ptr(gE), _hip.ptr(gb), _hip.ptr(f.touch),
                                            _hip.ptr(f.grad), st))
    else:
        _hip.check(L.skr_session_loss(_hip.ptr(do), B, h, _hip.ptr(dE), _hip.ptr(db), _hip.ptr(dY), n_y, 0, 0, 0.7, _hip.ptr(dlog),
                                      _hip.ptr(dout), _hip.ptr(loss), st))
        _hip.check(L.skr_session_out_grads(_hip.ptr(dlog), _hip.ptr(do), B, h, _hip.ptr(dY), n_y, _hip.ptr(dE), _hip.ptr(db), 0.01,
                                           _hip.ptr(gE), _hip.ptr(gb), _hip.ptr(f.touch), _hip.ptr(f.grad), st))
    f.check()
    want = _loss_oracle(E, bias, out, Y, "linear", "bpr_max", 0.01, 0.7, np.float64)
    _close(gE.cpu().numpy(), want["gE"], 5e-5, 1e-7)
    _close(gb.cpu().numpy(), want["gb"], 5e-5, 1e-7)


def test_touch_and_its_base_come_together():
    """one of `touch` / `touch_base` without the other: -1 from all four entry points, before anything is launched"""
    L, st = _hip.lib(), _hip.stream()
    t = torch.zeros(256, device="cuda")
    i = torch.zeros(4, dtype=torch.int32, device="cuda")
    b = torch.zeros(8, dtype=torch.uint8, device="cuda")
    p, pi, pb = _hip.ptr(t), _hip.ptr(i), _hip.ptr(b)
    for touch, base in ((pb, None), (None, p)):
        assert L.skr_scatter_add_rows(p, pi, 4, 32, None, 0.0, p, touch, base, st) == -1 and b"touch" in L.skr_last_error()
        assert L.skr_gru_cell_bwd_scatter(p, pi, p, 4, 32, 32, p, p, 0, p, p, p, p, p, p, p, p, p, p, 0.0, p, touch, base, st) == -1
        assert b"touch" in L.skr_last_error()
        assert L.skr_session_out_grads(p, p, 4, 32, pi, 4, p, p, 0.0, p, p, touch, base, st) == -1 and b"touch" in L.skr_last_error()
        assert L.skr_session_loss_grads(p, 4, 32, p, p, pi, 4, 0, 0, 1.0, p, p, p, 0, 4, 0.0, p, p, touch, base, st) == -1
        assert b"touch" in L.skr_last_error()
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and int(b.max()) == 0


# ---- 10. the popularity sampler's corners ----------------------------------------------------------------------------------------
def _pop_sample(cs, u):
    d_cs, d_u = to_dev(np.asarray(cs, np.float64)), to_dev(np.asarray(u, np.float64))
    out = torch.full((len(u),), -7, dtype=torch.int32, device="cuda")
    _hip.check(_hip.lib().skr_pop_sample(_hip.ptr(d_cs), len(cs), _hip.ptr(d_u), 0, len(u), _hip.ptr(out), _hip.stream()))
    return out.cpu().numpy()


def test_pop_sampler_corners():
    """one item; a cumulative sum that ends below 1 with a uniform above it (the last item takes the draw, where np.searchsorted
    answers n_items); zero-weight items (repeated cumulative values: the first index wins, as in np.searchsorted)"""
    top = np.nextafter(1.0, 0.0)
    assert np.array_equal(_pop_sample([1.0], [0.0, 0.5, 1.0, top]), [0, 0, 0, 0])
    assert np.array_equal(_pop_sample([0.25], [0.0, 0.5]), [0, 0])
    cs = np.array([0.2, 0.5, 1.0 - 3e-16])
    assert cs[-1] < top and np.searchsorted(cs, top) == 3
    assert np.array_equal(_pop_sample(cs, [top, cs[-1], 0.5, np.nextafter(0.5, 1.0)]), [2, 2, 1, 2])
    cs = np.array([0.1, 0.3, 0.3, 0.3, 0.7, 0.7, 1.0])
    u = np.array([0.3, 0.2, np.nextafter(0.3, 1.0), 0.7, 0.05, 0.1, np.nextafter(0.7, 1.0), 1.0, 0.0])
    assert np.array_equal(_pop_sample(cs, u), np.searchsorted(cs, u))
    assert np.array_equal(np.searchsorted(cs, u), [1, 1, 4, 4, 0, 0, 6, 6, 0])
