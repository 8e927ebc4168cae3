"""CPU suite of HGN: the truncated-sequence view of the data set against the reference's (golden), the registry and the
config, the weight-decay Adam entry points in header, library and binding, and the argument checks of the HGN entry
points (no GPU needed)."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)


def _train_data(golden):
    import pandas as pd
    from skrec.io.dataset import ImplicitFeedback
    d = golden("tiny_seq_dataset")
    df = pd.DataFrame(d["train"], columns=["user", "item", "time"])
    df.insert(2, "rating", 1.0)
    return ImplicitFeedback(df, int(d["num_users"]), int(d["num_items"]))


def _restated(by_time, max_len, pad):
    """left-padded, cut from the left"""
    out = OrderedDict()
    for u, items in by_time.items():
        keep = list(items)[-max_len:]
        out[u] = np.array([pad] * (max_len - len(keep)) + keep, np.int32)
    return out


def test_truncated_seq_dict_equals_reference(golden):
    g = golden("golden_hgn")
    data = _train_data(golden)
    got = data.to_truncated_seq_dict(5, pad_value=96)
    assert list(got.keys()) == [int(u) for u in g["trunc_users"]]            # same users in the same order
    arr = np.stack(list(got.values()))
    assert arr.dtype == np.int32 and np.array_equal(arr, g["trunc_seqs"])
    assert 63 not in got                                                     # no training history, no entry


def test_truncated_seq_dict_shapes(golden):
    data = _train_data(golden)
    by_time = data.to_user_dict_by_time()
    longest = max(len(v) for v in by_time.values())
    shortest = min(len(v) for v in by_time.values())
    assert shortest < longest
    for max_len, pad in ((None, 0), (longest + 3, 96), (shortest + 1, 7), (1, 96)):
        got = data.to_truncated_seq_dict(max_len, pad_value=pad, padding="pre", truncating="pre")
        want = _restated(by_time, longest if max_len is None else max_len, pad)
        assert list(got.keys()) == list(want.keys())
        for u in want:
            assert np.array_equal(got[u], want[u]), (max_len, u)
    # a history shorter than the window: pads on the left, the items in time order on the right
    u = min(by_time, key=lambda k: len(by_time[k]))
    row = data.to_truncated_seq_dict(shortest + 2, pad_value=96)[u]
    assert list(row[:2]) == [96, 96] and list(row[2:]) == list(by_time[u])


def test_registry_finds_hgn_with_reference_defaults():
    from skrec import ModelRegistry
    reg = ModelRegistry()
    assert reg.load_skrec_model("HGN") is True
    model_class, config_class = reg.get_model("HGN")
    assert model_class.__name__ == "HGN" and config_class.__name__ == "HGNConfig"
    cfg = config_class()
    want = dict(lr=1e-3, reg=1e-3, seq_L=5, seq_T=3, embed_size=64, batch_size=1024, epochs=1000, early_stop=100)
    for k, v in want.items():
        got = getattr(cfg, k)
        assert got == v and type(got) is type(v), (k, got, v)
    cfg._validate()
    for bad in (dict(reg=-1.0), dict(lr=1), dict(seq_L=0), dict(seq_T=0), dict(seq_L=2.0), dict(embed_size=0),
                dict(batch_size=0), dict(epochs=-1), dict(early_stop=1.5)):
        with pytest.raises(AssertionError):
            config_class(**bad)._validate()


def test_weight_decay_adam_symbols_are_declared_exported_and_bound():
    from skrec import _hip
    from test_abi import _declared
    declared = _declared()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    L = _hip.lib()
    for name in ("skr_adam_step_wd", "skr_adam_block_cold_wd", "skr_adam_block_hot_wd", "skr_hgn_step", "skr_hgn_queries"):
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _hip.SIGNATURES and getattr(L, name).argtypes is not None, name
    # one float more than the plain entry points
    for name in ("skr_adam_step", "skr_adam_block_cold", "skr_adam_block_hot"):
        assert len(_hip.SIGNATURES[name + "_wd"][1]) == len(_hip.SIGNATURES[name][1]) + 1
    assert L.skr_abi_version() >= 11


def _err(L):
    return L.skr_last_error().decode()


def test_weight_decay_adam_rejects_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    b = (ctypes.c_float * 256)()
    i = (ctypes.c_int32 * 64)()
    assert L.skr_adam_step_wd(None, b, b, b, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 1, 0, None, None) == -1 and "NULL" in _err(L)
    assert L.skr_adam_step_wd(b, b, b, b, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 0, 0, None, None) == -1 and "step_t" in _err(L)
    assert L.skr_adam_block_cold_wd(b, b, b, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 0, 65, i, 1, None) == -1 and "k <= 64" in _err(L)
    assert L.skr_adam_block_cold_wd(b, b, b, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 0, 4, None, 1, None) == -1 and "NULL" in _err(L)
    assert L.skr_adam_block_hot_wd(b, b, b, b, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 5, 5, i, 1, 0, 64, i, None) == -1
    assert "step_t0 < step_t" in _err(L)
    assert L.skr_adam_block_hot_wd(b, b, b, b, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 0, 1, i, 1, 0, 64, None, None) == -1


def test_hgn_entry_points_reject_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    b = (ctypes.c_float * 64)()

    def step(tabs=(b,) * 9, n=4, nu=2, nr=3, pad=2, dim=64, sl=5, stt=3, outs=(b,) * 7, slots=1):
        return L.skr_hgn_step(*tabs, n, nu, nr, pad, dim, sl, stt, *outs, slots, None)
    assert step(tabs=(None,) + (b,) * 8) == -1 and "NULL" in _err(L)
    assert step(outs=(b,) * 5 + (None, b)) == -1 and "NULL" in _err(L)          # the scratch buffer
    assert step(n=-1) == -1 and "n = -1" in _err(L)
    assert step(pad=3) == -1 and "pad_idx" in _err(L)
    assert step(dim=128) == -1 and "dim" in _err(L)
    assert step(sl=0) == -1 and "seq_L" in _err(L)
    assert step(sl=_hip.SKR_HGN_MAX_L + 1) == -1 and "seq_L" in _err(L)
    assert step(stt=_hip.SKR_HGN_MAX_T + 1) == -1 and "seq_T" in _err(L)
    assert step(slots=3) == -1 and "loss_slots" in _err(L)
    assert step(n=0) == 0

    def queries(tabs=(b, b, b), users=None, n=2, win=b, nu=2, nr=3, pad=2, dim=64, sl=5, out=b):
        return L.skr_hgn_queries(*tabs, users, n, win, nu, nr, pad, dim, sl, out, None)
    assert queries(win=None) == -1 and "NULL" in _err(L)
    assert queries(n=3) == -1 and "user list" in _err(L)
    assert queries(dim=16) == -1 and "dim" in _err(L)
    assert queries(sl=33) == -1 and "seq_L" in _err(L)
    assert queries(n=0) == 0
    assert _hip.hgn_gate_floats(5) == 8704
