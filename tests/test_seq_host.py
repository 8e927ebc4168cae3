"""CPU suite: the sequential recommenders (FPMC, TransRec) are found by the registry with the reference's defaults, and
their C entry points reject bad arguments before any HIP call (no GPU needed)."""
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)

_REF_DEFAULTS = {
    "FPMC": dict(lr=0.001, reg=0.001, embed_size=64, batch_size=1024, epochs=500, early_stop=100),
    "TransRec": dict(lr=1e-3, reg=0.0, embed_size=64, batch_size=1024, epochs=500, early_stop=100),
}


@pytest.mark.parametrize("name", ["FPMC", "TransRec"])
def test_registry_finds_model_with_reference_defaults(name):
    from skrec import ModelRegistry
    reg = ModelRegistry()
    assert reg.load_skrec_model(name) is True
    model_class, config_class = reg.get_model(name)
    assert model_class.__name__ == name
    cfg = config_class()
    for k, v in _REF_DEFAULTS[name].items():
        got = getattr(cfg, k)
        assert got == v and type(got) is type(v), (k, got, v)
    cfg._validate()
    with pytest.raises(AssertionError):
        config_class(reg=-1.0)._validate()
    with pytest.raises(AssertionError):
        config_class(lr=1)._validate()      # the reference asserts a float


@pytest.mark.parametrize("name", ["FPMC", "TransRec"])
def test_embed_size_beyond_256_is_refused_before_any_launch(monkeypatch, name):
    """rows are padded to 64, 128, 192 or 256 floats: embed_size = 257 raises padded_width's NotImplementedError in
    ``_build``, before the tables are drawn and before anything of the kernel library is called"""
    import importlib
    import torch
    from skrec import _hip

    def no_lib():
        raise AssertionError("the kernel library is called before the width is checked")
    monkeypatch.setattr(_hip, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(_hip, "lib", no_lib)
    cls = getattr(importlib.import_module(f"skrec.recommender.{name}"), name)
    with pytest.raises(NotImplementedError, match="embedding widths up to 256"):
        cls.detached(8, 8, dict(embed_size=257))


def _err(L):
    return L.skr_last_error().decode()


def _buf(n=64 * 8):
    import ctypes
    return (ctypes.c_float * n)()


def test_fpmc_step_rejects_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    b = _buf()
    ok = [b] * 8
    g = [b] * 4

    def call(tabs=ok, n=4, nu=2, ni=2, dim=64, grads=g, loss=b, slots=1):
        return L.skr_fpmc_step(*tabs, n, nu, ni, dim, 1e-3, *grads, loss, slots, None)
    assert call(tabs=[None] + ok[1:]) == -1 and "NULL" in _err(L)
    assert call(loss=None) == -1 and "NULL" in _err(L)
    assert call(n=-1) == -1 and "n = -1" in _err(L)
    assert call(nu=0) == -1
    assert call(dim=100) == -1 and "dim" in _err(L)
    assert call(dim=320) == -1 and "dim" in _err(L)
    assert call(slots=5) == -1 and "loss_slots" in _err(L)
    with pytest.raises(ValueError):
        _hip.check(call(dim=0))


def test_transrec_step_rejects_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    b = _buf()
    ok = [b] * 8
    g = [b] * 4

    def call(tabs=ok, n=4, nu=2, ni=2, dim=64, grads=g, work=b, loss=b, slots=1):
        return L.skr_transrec_step(*tabs, n, nu, ni, dim, 0.0, *grads, work, loss, slots, None)
    assert call(work=None) == -1 and "NULL" in _err(L)
    assert call(grads=[b, b, b, None]) == -1 and "NULL" in _err(L)
    assert call(n=-2) == -1
    assert call(ni=-1) == -1
    assert call(dim=16) == -1 and "dim" in _err(L)
    assert call(slots=0) == -1 and "loss_slots" in _err(L)


def test_seq_scores_rejects_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    b = _buf()

    def call(mode=_hip.SKR_SEQ_FPMC, tabs=(b, b, b, b, None, None), users=b, B=2, last=b, nu=2, ni=4, dim=64, out=b, ld=4):
        return L.skr_seq_scores(mode, *tabs, users, B, last, nu, ni, dim, out, ld, None)
    assert call(mode=7) == -1 and "mode" in _err(L)
    assert call(users=None) == -1 and "NULL" in _err(L)
    assert call(tabs=(b, b, b, None, None, None)) == -1 and "NULL" in _err(L)       # FPMC needs the second item table
    assert call(mode=_hip.SKR_SEQ_TRANSREC) == -1 and "NULL" in _err(L)              # TransRec needs T and the biases
    assert call(ld=3) == -1 and "ld" in _err(L)
    assert call(B=-1) == -1
    assert call(dim=65) == -1 and "dim" in _err(L)
