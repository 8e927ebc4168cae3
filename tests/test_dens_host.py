"""CPU suite of DENS (skrec/recommender/DENS.py, csrc/dens.hip's argument checks, tests/golden/golden_dens.npz): the config
against the reference's field for field, the limits, the registry, the C ABI's names and checks without a GPU, the
initialisation against the fixture, and the fixture itself against the float64 twin (tests/dens_twin.py) with computed choices."""
import ctypes
import os
import re

import numpy as np
import pytest

import dens_twin as T

SEED = 2021
CONFIG = dict(lr=1e-2, l2=1e-4, gamma=0.3, dim=64, batch_size=256, context_hops=2, K=1, n_negs=6, warmup=4, epochs=3)
MARGIN = 2.0 ** -12


def test_config_defaults_and_validation():
    from skrec.recommender.DENS import DENSConfig
    c = DENSConfig()
    assert dict(c.items()) == dict(lr=1e-3, l2=1e-4, gamma=0.3, dim=64, batch_size=2048, context_hops=3, K=1, n_negs=6, ns="dens",
                                   pool="mean", warmup=100, mess_dropout=False, mess_dropout_rate=0.1, edge_dropout=False,
                                   edge_dropout_rate=0.1, alpha=1.0, epochs=1000, early_stop=100)
    for bad in (dict(lr=1), dict(lr=-1e-3), dict(l2=-1.0), dict(l2=0), dict(gamma=-0.1), dict(gamma=1), dict(dim=0), dict(dim=64.0),
                dict(batch_size=0), dict(context_hops=-1), dict(K=0), dict(n_negs=0), dict(ns="mix"), dict(ns=1), dict(warmup=-1),
                dict(warmup=1.0), dict(mess_dropout=0), dict(mess_dropout_rate=-0.1), dict(edge_dropout=1), dict(edge_dropout_rate=-1.0),
                dict(epochs=-1), dict(early_stop=1.0)):
        with pytest.raises(AssertionError):
            DENSConfig(**bad)
    for ok in (dict(context_hops=0), dict(ns="rns"), dict(ns="dns"), dict(warmup=0), dict(gamma=0.0), dict(pool="sum")):
        DENSConfig(**ok)                      # the reference accepts these; check_limits names what the fused step does not run


def test_limits_are_named():
    from skrec.recommender.DENS import DENS, DENSConfig, check_limits
    check_limits(DENSConfig(dim=40, context_hops=0, n_negs=16, batch_size=2048, gamma=0.0))
    for kw, msg in ((dict(ns="rns"), "ns == 'dens'"), (dict(ns="dns"), "ns == 'dens'"), (dict(pool="sum"), "pool == 'mean'"),
                    (dict(pool="concat"), "pool == 'mean'"), (dict(K=2), "K == 1"), (dict(mess_dropout=True), "mess_dropout"),
                    (dict(edge_dropout=True), "edge_dropout"), (dict(dim=65), "dim <= 64"), (dict(context_hops=4), "context_hops <= 3"),
                    (dict(n_negs=17), "n_negs <= 16"), (dict(batch_size=2049), "batch_size <= 2048")):
        with pytest.raises(NotImplementedError, match=msg):
            check_limits(DENSConfig(**kw))
    with pytest.raises(NotImplementedError, match="one GPU"):
        check_limits(DENSConfig(), world=2)
    with pytest.raises(ValueError, match="warmup"):
        check_limits(DENSConfig(warmup=0))
    # the constructor raises before it touches the data set or the GPU
    with pytest.raises(NotImplementedError, match="dim <= 64"):
        DENS(None, dict(dim=128))
    with pytest.raises(ValueError, match="warmup"):
        DENS(None, dict(warmup=0))


def test_registry_finds_the_model():
    from skrec.utils.registry import ModelRegistry
    from skrec.recommender.DENS import DENS, DENSConfig
    reg = ModelRegistry()
    assert reg.load_skrec_model("DENS")
    assert reg.get_model("DENS") == (DENS, DENSConfig)


def test_abi_names_in_header_and_binding():
    """the new entry points and constants are declared in the header and bound in _hip.py with matching argument counts"""
    from conftest import REPO
    from skrec import _hip
    header = open(os.path.join(REPO, "include", "skrec_hip.h")).read()
    for name in ("skr_dens_workspace", "skr_dens_step", "skr_dens_step_timed"):
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]) == len(_hip.SIGNATURES[name][1]), name
    for name, value in (("SKR_DENS_MAX_BATCH", 2048), ("SKR_DENS_MAX_NEGS", 16), ("SKR_DENS_MAX_HOPS", 3)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", header)
        assert m and int(m.group(1)) == value == getattr(_hip, name), name
    assert int(re.search(r"#define\s+SKR_DENS_GROUPS\s+(\d+)", header).group(1)) == _hip.SKR_DENS_GROUPS
    # the struct: the header's members in order against the binding's fields
    body = re.search(r"typedef struct skr_dens_step_args \{(.*?)\} skr_dens_step_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            for part in decl.split(","):      # "const float* a, *b" / "float* hop[3]": the last identifier of each part
                members.append(re.findall(r"\w+", re.sub(r"\[.*\]", "", part))[-1])
    assert members == [f[0] for f in _hip.DensStepArgs._fields_]
    L = _hip.lib()
    assert L.skr_abi_version() >= 12


def test_abi_argument_checks_without_gpu():
    from skrec import _hip
    L = _hip.lib()
    p = 16                                    # any non-NULL, aligned address: the checks fail before it is used
    assert L.skr_dens_workspace(0, 2) == 0 and L.skr_dens_workspace(2049, 2) == 0 and L.skr_dens_workspace(16, 4) == 0
    assert L.skr_dens_workspace(16, -1) == 0
    assert 0 < L.skr_dens_workspace(16, 0) < L.skr_dens_workspace(16, 3) < L.skr_dens_workspace(2048, 3)

    def step(**kw):
        a = _hip.DensStepArgs()
        a.plan_a = a.plan_at = a.params = a.uids = a.pos = a.cand = a.grad = a.loss = a.work = a.ping = p
        for h in range(3):
            a.hop[h] = p
        for h in range(4):
            a.G[h] = p
        a.n_users, a.n_items, a.dim, a.n_hops, a.n_negs, a.n = 70, 45, 64, 2, 6, 16
        a.w, a.gamma, a.l2, a.work_bytes = 1.0, 0.3, 1e-4, 1 << 30
        for k, v in kw.items():
            if k == "hop1":
                a.hop[1] = v
            elif k == "G0":
                a.G[0] = v
            else:
                setattr(a, k, v)
        return L.skr_dens_step(ctypes.byref(a), None)
    assert L.skr_dens_step(None, None) == -1
    assert step(params=None) == -1 and b"NULL" in L.skr_last_error()
    assert step(n=2049) == -1 and b"at most 2048" in L.skr_last_error()
    assert step(dim=65) == -1 and b"dim" in L.skr_last_error()
    assert step(n_hops=4) == -1 and b"n_hops" in L.skr_last_error()
    assert step(n_negs=17) == -1 and b"n_negs" in L.skr_last_error()
    assert step(n_negs=0) == -1
    assert step(plan_a=None) == -1 and b"plans" in L.skr_last_error()
    assert step(hop1=None) == -1 and b"hop table" in L.skr_last_error()
    assert step(G0=None) == -1 and b"gradient table" in L.skr_last_error()
    assert step(ping=None) == -1 and b"ping" in L.skr_last_error()
    assert step(w=1.5) == -1 and step(gamma=-1.0) == -1
    assert step(work_bytes=64) == -1 and b"skr_dens_workspace" in L.skr_last_error()
    assert step(work=8) == -1 and b"aligned" in L.skr_last_error()
    assert step(n=0) == 0                     # an empty batch: nothing to launch
    assert L.skr_dens_step_timed(None, None, None) == -1


def test_initialisation_equals_the_reference(golden):
    """the four Linears are drawn before the two embeddings (DENS.py:163-178)"""
    import torch
    from skrec.recommender.DENS import GATES, init_parameters
    g = golden("golden_dens")
    torch.manual_seed(SEED)
    gates, eu, ei = init_parameters(64, 96, 64)
    for name in GATES:
        assert np.array_equal(gates[name][0].numpy(), g[f"init.{name}.weight"]), name
        assert np.array_equal(gates[name][1].numpy(), g[f"init.{name}.bias"]), name
    assert np.array_equal(eu.numpy(), g["init.user_embed"]) and np.array_equal(ei.numpy(), g["init.item_embed"])
    torch.manual_seed(SEED)                    # without the gates' draws the tables differ
    assert not np.array_equal(torch.nn.init.xavier_uniform_(torch.empty(64, 64)).numpy(), g["init.user_embed"])


def test_fixture_margin_share_is_within_its_cap(golden):
    g = golden("golden_dens")
    m = g["step_margin"]
    assert m.shape == (sum(g["step_sizes"]), 3) and m.size == 6867
    under = int((m < MARGIN).sum())
    print("groups under 2^-12:", under, "of", m.size, "smallest", m.min())
    assert under == int(g["groups_under_margin"]) and under <= 0.005 * m.size
    assert (m >= 0).all()
    assert (g["close_users"] <= 3).all()
    # the recorded choice holds the recorded item; the other admissible item differs from it
    b = np.concatenate([[0], np.cumsum(g["step_sizes"])])
    for s in range(9):
        cand, ch, it, sec = (g[k][b[s]:b[s + 1]] for k in ("step_cand", "step_choice", "step_item", "step_second"))
        assert np.array_equal(np.take_along_axis(cand, ch.astype(np.int64), 1), it)
        assert (sec != it).all()


def test_twin_with_computed_choices_reproduces_the_fixture(golden):
    """float64, from the recorded initial parameters: wherever the margin is at least 2^-12 the twin's own arg-max is the
    reference's item; elsewhere it is the reference's item or the other one of the near tie (and the reference's is then used,
    so that the run stays on the reference's path); the losses, the final parameters and the scores follow"""
    import torch
    g = golden("golden_dens")
    rowptr, items, ni = T.tiny_csr(golden("tiny_dataset"))
    rows = np.repeat(np.arange(64), np.diff(rowptr))
    A = T.dense_adjacency(rowptr, items, ni)
    # the recorded adjacency is both triangles of the train CSR with 1 / sqrt(deg deg)
    assert len(g["adj_val"]) == 2 * len(items)
    np.testing.assert_allclose(g["adj_val"], A[g["adj_rows"], g["adj_cols"]], rtol=2e-7)
    assert np.array_equal(g["adj_rows"][:len(items)], rows) and np.array_equal(g["adj_cols"][:len(items)], 64 + items)
    assert rowptr[64] == rowptr[63] and not (items == 95).any()          # a zero-degree user and a zero-degree item
    steps = T.fixture_steps(g)
    assert [len(s[0]) for s in steps] == [256, 256, 251] * 3
    P = {k: T.t64(g["init." + k], True) for k in T.NAMES}
    A64 = T.t64(A)
    opt = torch.optim.Adam(list(P.values()), lr=CONFIG["lr"])
    losses, left_out = [], 0
    for t, (users, pos, cand, choice, item, margin, second) in enumerate(steps):
        w = 1.0 - min(1.0, (t // 3) / CONFIG["warmup"])
        sure = margin >= MARGIN
        r = T.step_f64(P, A64, users, pos, cand, 2, w, CONFIG["gamma"], CONFIG["l2"], choices=np.where(sure, -1, choice))
        own_item = np.take_along_axis(cand, r["own"], 1)
        assert np.array_equal(own_item[sure], item[sure]), f"step {t}"
        assert ((own_item == item) | (own_item == second))[~sure].all(), f"step {t}"
        m, best, _ = T.margins(r["scores"], r["scale"], cand)
        np.testing.assert_allclose(m[sure], margin[sure], rtol=1e-2, atol=1e-6)     # the reference's fp32 tables against float64 ones
        left_out += int((~sure).sum())
        opt.zero_grad()
        r["total"].backward()
        opt.step()
        losses.append([r["mf"].item(), r["emb"].item(), r["total"].item()])
    assert left_out == int(g["groups_under_margin"])
    losses = np.array(losses)
    dev_p, dev_l = g["f64_dev_params"], float(g["f64_dev_loss"])
    print("loss dev", np.abs(losses / g["loss"].astype(np.float64) - 1).max(), "recorded", dev_l)
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-5)
    np.testing.assert_allclose(losses[:, 2], g["loss"][:, 2], rtol=2 * dev_l)
    for k, lim in zip(T.NAMES, dev_p):
        assert str(g["param_names"][list(T.NAMES).index(k)]) == k
        assert np.abs(P[k].detach().numpy() - g["final." + k]).max() <= 2 * lim, k
    assert g["pred"].shape == (3, 63, 96) and len(g["test_users"]) == 63
    assert g["f64_dev_scores"].max() < 1e-6 and dev_p.max() < 1e-6 and dev_l < 1e-6
    assert float(g["near_tie_gap"]) == 12.0 * g["f64_dev_scores"].max()
