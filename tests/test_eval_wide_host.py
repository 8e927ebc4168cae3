"""CPU suite of the wide fused evaluator (rows of 128 / 192 / 256 floats): the entry's argument checks answer before any device
call, the evaluator's routing decision is a pure function, and GRU4RecPlus hands out its factors at every width the entry takes."""
import types

import numpy as np
import pytest

P = 16                                        # any non-NULL, 16-byte aligned address: the checks fail before it is used


def _lib():
    from skrec import _hip
    return _hip.lib()


def _fused(L, dim, top_k=5, B=4, n_items=100, work=P, work_bytes=1 << 30):
    return L.skr_eval_fused_topk(P, P, B, P, None, n_items, dim, None, None, top_k, P, P, work, work_bytes, None)


@pytest.mark.parametrize("dim", [128, 192, 256])
def test_wide_rows_pass_the_width_check(dim, monkeypatch):
    """with top_k = 0 the first thing wrong with a 128 / 192 / 256-column call is top_k, not the width"""
    monkeypatch.delenv("SKR_FUSED_MODE", raising=False)
    L = _lib()
    rc = _fused(L, dim, top_k=0)
    msg = L.skr_last_error()
    assert rc == -1 and b"top_k" in msg and b"dim" not in msg, msg


@pytest.mark.parametrize("dim", [0, 32, 96, 320])
def test_other_widths_are_refused_by_name(dim, monkeypatch):
    monkeypatch.delenv("SKR_FUSED_MODE", raising=False)
    L = _lib()
    rc = _fused(L, dim, top_k=0)
    msg = L.skr_last_error()
    assert rc == -1 and b"dim" in msg, msg
    for w in (b"64", b"128", b"192", b"256"):
        assert w in msg, msg
    assert str(dim).encode() in msg, msg


def test_fp32_mode_is_refused_at_wide_rows_without_a_device(monkeypatch):
    """SKR_FUSED_MODE=fp32 exists at 64 columns only: a valid call shape at dim = 128 answers SKR_EINVAL naming the mode and the
    width -- on a host without a GPU, so before any device call"""
    monkeypatch.setenv("SKR_FUSED_MODE", "fp32")
    L = _lib()
    rc = _fused(L, 128)
    msg = L.skr_last_error()
    assert rc == -1 and b"fp32" in msg and b"128" in msg, msg


def test_routing_function():
    from skrec.utils.py.evaluator import fused_route
    for mode in (None, "", "f16x2", "bf16x3"):
        for w in (64, 128, 192, 256):
            assert fused_route(w, w, 1000, 100, 20, mode), (w, mode)
        assert not fused_route(96, 96, 1000, 100, 20, mode)
        assert not fused_route(64, 128, 1000, 100, 20, mode)       # unequal widths
        assert not fused_route(128, 64, 1000, 100, 20, mode)
        assert not fused_route(256, 192, 1000, 100, 20, mode)
    # fp32: the 64-column kernel only
    assert fused_route(64, 64, 1000, 100, 20, "fp32")
    for w in (128, 192, 256):
        assert not fused_route(w, w, 1000, 100, 20, "fp32")
    # K: the fused kernel's deepest list is 128
    for w in (64, 128, 256):
        assert fused_route(w, w, 1000, 100, 128, None)
        assert not fused_route(w, w, 1000, 100, 129, None)
        # every user must keep K unmasked items
        assert fused_route(w, w, 120, 100, 20, None)               # n_items - max_train == K
        assert not fused_route(w, w, 119, 100, 20, None)           # == K - 1


def test_routing_function_takes_cpu_tensors_shapes():
    import torch
    from skrec.utils.py.evaluator import fused_route
    ut, it = torch.zeros(7, 128), torch.zeros(50, 128)
    assert fused_route(int(ut.shape[1]), int(it.shape[1]), int(it.shape[0]), 10, 5, "bf16x3")
    assert not fused_route(int(ut.shape[1]), int(it.shape[1]), int(it.shape[0]), 10, 5, "fp32")


def _gru(last, final_act="linear"):
    from skrec.recommender.GRU4RecPlus import GRU4RecPlus
    m = GRU4RecPlus.__new__(GRU4RecPlus)      # predict_factors() reads three attributes: no device, no data set
    m.config = types.SimpleNamespace(final_act=final_act, layers=[last])
    m.cur_user_embeddings = np.zeros((3, last), np.float32)
    m.net = types.SimpleNamespace(E_out=np.zeros((5, last), np.float32), b_out=np.zeros(5, np.float32))
    return m


def test_gru_hands_out_its_factors_at_every_fused_width():
    for last in (64, 128, 192, 256):
        f = _gru(last).predict_factors()
        assert f is not None and f[0].shape[1] == last and f[1].shape[1] == last
    assert _gru(96).predict_factors() is None
    assert _gru(128, "relu").predict_factors() is None
