"""GPU suite of LATTICE (csrc/lattice.hip, skrec/recommender/LATTICE.py): the sparse assembly of the mixed item graph, the
sampled product and the graph's hand-derived backward against the float64 twin (tests/lattice_twin.py) at the edges of their
row merges; ``gradient_step``, ordinary and build, against the twin's gradient; bit-reproducibility; the golden replay of the
reference's fit() from its recorded batches; fit() through the registry with the learning-rate schedule; the limits.

Tolerances of the kernel-level comparisons: the project's own (test_gpu_mgcn.py), rtol = 1e-4 and atol = 2e-5 * max|want| per
tensor; patterns and provenance slots are exact."""
import numpy as np
import pytest

import lattice_twin as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SEED = T.SEED
RTOL, ATOL = 1e-4, 2e-5


def _seed():
    import random
    import torch
    np.random.seed(SEED)
    random.seed(SEED)
    torch.manual_seed(SEED)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, want, what, rtol=RTOL, atol=ATOL):
    want = np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    err = np.abs(np.asarray(got, np.float64) - want)
    print(what, "max abs err", err.max() if err.size else 0.0, "max|want|", scale, "allowed atol", atol * scale)
    assert np.all(err <= atol * scale + rtol * np.abs(want)), (what, float(err.max()), float(scale))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the graphs of the kernel-level tests
# ---------------------------------------------------------------------------------------------------------------------
def _lists_case(I, k, mode, seed):
    """four lists (ids int32 [I, k], values float32 [I, k]) or None, and the projected rows F = [F_v, F_t] ([I, 64] float32
    or None) they come from"""
    rng = np.random.default_rng(seed)
    F = [rng.standard_normal((I, 64)).astype(np.float32), rng.standard_normal((I, 64)).astype(np.float32)]
    raw = [rng.standard_normal((I, 7)), rng.standard_normal((I, 5))]
    lists = []
    for m in range(2):
        ids, sims = T.knn_f64(F[m].astype(np.float64), k)
        lists.append((ids.astype(np.int32), sims.astype(np.float32)))
    for m in range(2):
        ids, vals = T.frozen_lists(raw[m], k)
        lists.append((ids.astype(np.int32), vals.astype(np.float32)))
    if mode == "coincide":            # every row: exactly k entries
        lists = [(lists[0][0].copy(), l[1]) for l in lists]
    elif mode == "disjoint":          # every row: 4 k entries
        assert 4 * k <= I
        perm = np.stack([rng.permutation(I)[:4 * k] for _ in range(I)]).astype(np.int32)
        lists = [(np.ascontiguousarray(perm[:, t * k:(t + 1) * k]), l[1]) for t, l in enumerate(lists)]
    elif mode == "image only":
        lists[1] = lists[3] = None
        F[1] = None
    elif mode == "text only":
        lists[0] = lists[2] = None
        F[0] = None
    elif mode == "zero row":          # r_0 = 0: q_0 = 0, the row keeps its frozen part only
        for m in range(2):
            lists[m][1][0] = 0.0
    elif mode == "hub":               # item 0 is listed by everybody, item I - 1 by nobody (but itself: taken out too)
        for t in range(4):
            ids = lists[t][0]
            ids[ids == I - 1] = 0     # a repeated id inside a list: the first counts
            ids[:, 0] = 0
    else:
        assert mode == "random"
    return lists, F


def _twin_lists(lists):
    return [None if l is None else (l[0].astype(np.int64), l[1].astype(np.float64)) for l in lists]


def _weights(lists, rng):
    if lists[0] is not None and lists[1] is not None:
        w = rng.random() * 0.6 + 0.2
        return np.array([w, 1.0 - w], np.float32)
    return np.array([1.0 if lists[0] is not None else 0.0, 1.0 if lists[1] is not None else 0.0], np.float32)


def _ptr_arrays(dev_lists):
    from skrec import _hip
    ids, vals = (_hip.vp * 4)(), (_hip.vp * 4)()
    for t, l in enumerate(dev_lists):
        if l is not None:
            ids[t], vals[t] = l[0].data_ptr(), l[1].data_ptr()
    return ids, vals


def _device_graph(lists, w, lam, I, k):
    """runs skr_lattice_graph -> dict of device tensors, every output pre-filled with a value it must overwrite"""
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    dl = [None if l is None else (_dev(l[0]), _dev(l[1])) for l in lists]
    ids, vals = _ptr_arrays(dl)
    cap = 4 * k * I
    out = dict(rowptr=torch.full((I + 1,), -7, dtype=torch.int64, device="cuda"), col=torch.full((cap,), -7, dtype=torch.int32, device="cuda"),
               val=torch.full((cap,), 7.0, device="cuda"), slots=torch.full((cap, 4), -7, dtype=torch.int32, device="cuda"),
               r=torch.full((I,), 7.0, device="cuda"), q=torch.full((I,), 7.0, device="cuda"), w=_dev(w), lists=dl, ids=ids, vals=vals)
    ws = int(L.skr_lattice_graph_workspace(I))
    work = torch.full((ws,), 255, dtype=torch.uint8, device="cuda")
    _hip.check(L.skr_lattice_graph(I, k, ids, vals, p(out["w"]), float(lam), p(out["rowptr"]), p(out["col"]), p(out["val"]), p(out["slots"]),
                                   p(out["r"]), p(out["q"]), p(work), ws, st))
    torch.cuda.synchronize()
    return out


GRAPH_CASES = [(I, k, "random") for I in (1, 2, 63, 64, 65, 130) for k in (1, 10, 32) if k <= I] + \
              [(65, 10, "coincide"), (130, 32, "coincide"), (130, 32, "disjoint"), (65, 10, "disjoint"), (65, 10, "image only"),
               (65, 10, "text only"), (65, 10, "zero row"), (130, 10, "hub")]


def _check_graph(I, k, mode, lam=0.3):
    lists, F = _lists_case(I, k, mode, 100 * I + k)
    w = _weights(lists, np.random.default_rng(I + k))
    G = T.union_graph(_twin_lists(lists), w.astype(np.float64), lam)
    D = _device_graph(lists, w, lam, I, k)
    nnz = len(G["col"])
    assert np.array_equal(D["rowptr"].cpu().numpy(), G["rowptr"])
    assert np.array_equal(D["col"].cpu().numpy()[:nnz], G["col"])
    assert np.array_equal(D["slots"].cpu().numpy()[:nnz], G["slots"])
    assert (D["col"][nnz:] == 0).all() and (D["val"][nnz:] == 0).all() and (D["slots"][nnz:] == -1).all()      # every element written
    _close(D["val"].cpu().numpy()[:nnz], G["val"], f"S I={I} k={k} {mode}")
    _close(D["r"].cpu().numpy(), G["r"], "r")
    _close(D["q"].cpu().numpy(), G["q"], "q")
    return lists, F, w, G, D


@pytest.mark.parametrize("I, k, mode", GRAPH_CASES)
def test_graph_equals_the_twin(I, k, mode):
    lists, F, w, G, D = _check_graph(I, k, mode)
    counts = np.diff(G["rowptr"])
    if mode == "coincide":
        assert (counts == k).all()
    if mode == "disjoint":
        assert (counts == 4 * k).all() and ((I, k) != (130, 32) or counts.max() == 128)
    if mode == "zero row":            # q_0 = 0: the row keeps lam times its frozen part, nothing else
        assert G["r"][0] == 0 and D["r"][0].item() == 0 and D["q"][0].item() == 0
        row0 = slice(0, int(G["rowptr"][1]))
        frozen = 0.3 * (w[0] * T._pick(G, 2) + w[1] * T._pick(G, 3))
        assert np.allclose(D["val"].cpu().numpy()[row0], frozen[row0], rtol=1e-6, atol=0)


def test_graph_is_bit_reproducible_and_checks_its_arguments():
    from skrec import _hip
    lists, F = _lists_case(130, 10, "random", 5)
    w = _weights(lists, np.random.default_rng(5))
    a, b = _device_graph(lists, w, 0.3, 130, 10), _device_graph(lists, w, 0.3, 130, 10)
    for key in ("rowptr", "col", "val", "slots", "r", "q"):
        assert (a[key] == b[key]).all(), key
    L = _hip.lib()
    assert L.skr_lattice_graph(10, 33, a["ids"], a["vals"], None, 0.5, None, None, None, None, None, None, None, 0, None) == -1
    assert L.skr_lattice_graph_workspace(0) == 0 and L.skr_lattice_workspace(2049, 10) == 0 and L.skr_lattice_workspace(0, 10) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sampled product
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 20])
@pytest.mark.parametrize("I, k, mode", [(1, 1, "random"), (65, 10, "random"), (130, 32, "disjoint"), (130, 10, "hub"), (64, 32, "random")])
def test_sddmm_equals_the_twin(I, k, mode, d):
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    lists, _ = _lists_case(I, k, mode, 7 * I + k)
    G = T.union_graph(_twin_lists(lists), [0.5, 0.5], 0.3)
    rows, col, nnz = G["rows"], G["col"], len(G["col"])
    rng = np.random.default_rng(I + d)
    rp, cl = _dev(G["rowptr"]), _dev(col.astype(np.int32))
    for nl in (1, 3):
        A = np.zeros((nl, I, 64), np.float32)
        B = np.zeros((nl, I, 64), np.float32)
        A[:, :, :d], B[:, :, :d] = rng.standard_normal((nl, I, d)), rng.standard_normal((nl, I, d))
        want = sum((A[l].astype(np.float64)[rows] * B[l].astype(np.float64)[col]).sum(1) for l in range(nl))
        dA, dB = _dev(A), _dev(B)
        g = torch.full((nnz,), 7.0, device="cuda")
        _hip.check(L.skr_lattice_sddmm(I, I, p(rp), p(cl), p(dA), I * 64, p(dB), I * 64, nl, None, 0, p(g), st))
        _close(g.cpu().numpy(), want, f"sddmm I={I} k={k} {mode} d={d} layers={nl}")
        # with a row mask: the unmarked rows' entries are zeros (or, accumulating, left alone)
        mask = (rng.random(I) < 0.5).astype(np.uint8)
        dm = _dev(mask)
        g2 = torch.full((nnz,), 7.0, device="cuda")
        _hip.check(L.skr_lattice_sddmm(I, I, p(rp), p(cl), p(dA), I * 64, p(dB), I * 64, nl, p(dm), 0, p(g2), st))
        _close(g2.cpu().numpy(), want * mask[rows], "masked")
        assert (g2.cpu().numpy()[mask[rows] == 0] == 0).all()
        _hip.check(L.skr_lattice_sddmm(I, I, p(rp), p(cl), p(dA), I * 64, p(dB), I * 64, nl, p(dm), 1, p(g2), st))
        _close(g2.cpu().numpy(), 2 * want * mask[rows], "masked, accumulated")
        g3 = g.clone()
        _hip.check(L.skr_lattice_sddmm(I, I, p(rp), p(cl), p(dA), I * 64, p(dB), I * 64, nl, None, 0, p(g3), st))
        assert torch.equal(g, g3)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the backward of the graph
# ---------------------------------------------------------------------------------------------------------------------
def _transpose(G):
    order = np.argsort(G["col"] * G["n"] + G["rows"], kind="stable")
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(G["col"], minlength=G["n"]))]).astype(np.int64)
    return rowptr_t, G["rows"][order].astype(np.int32), order.astype(np.int32)


@pytest.mark.parametrize("I, k, mode", [(1, 1, "random"), (2, 1, "random"), (65, 10, "random"), (130, 32, "random"), (130, 32, "disjoint"),
                                        (65, 10, "coincide"), (65, 10, "image only"), (65, 10, "text only"), (65, 10, "zero row"),
                                        (130, 10, "hub")])
def test_graph_backward_equals_the_twin(I, k, mode):
    import torch
    from skrec import _hip
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    lam = 0.3
    lists, F, w, G, D = _check_graph(I, k, mode, lam)
    nnz = len(G["col"])
    rng = np.random.default_rng(3 * I + k)
    g = rng.standard_normal(nnz).astype(np.float32)
    rowptr_t, col_t, perm_t = _transpose(G)
    if mode == "hub":
        counts = np.diff(rowptr_t)
        assert counts[0] == I and counts[I - 1] == 0        # a long row of S^T and an empty one
    want_dF, want_dw, want_dtheta = T.graph_backward(G, g.astype(np.float64), [None if f is None else f.astype(np.float64) for f in F])
    dF_dev = [None if f is None else _dev(f) for f in F]
    out = [None if f is None else torch.full((I, 64), 7.0, device="cuda") for f in F]
    Fp, dFp = (_hip.vp * 2)(), (_hip.vp * 2)()
    for m in range(2):
        if F[m] is not None:
            Fp[m], dFp[m] = dF_dev[m].data_ptr(), out[m].data_ptr()
    ws = int(L.skr_lattice_graph_bwd_workspace(I, nnz))
    tabs = [_dev(a) for a in (g, rowptr_t, col_t, perm_t)]
    dw = torch.full((4,), 7.0, device="cuda")

    def run():
        work = torch.full((ws,), 255, dtype=torch.uint8, device="cuda")
        _hip.check(L.skr_lattice_graph_bwd(I, k, nnz, p(tabs[0]), p(D["rowptr"]), p(D["col"]), p(D["slots"]), p(tabs[1]), p(tabs[2]), p(tabs[3]),
                                           D["ids"], D["vals"], p(D["w"]), lam, p(D["q"]), Fp, dFp, p(dw), p(work), ws, st))
        torch.cuda.synchronize()
    run()
    for m in range(2):
        if F[m] is not None:
            _close(out[m].cpu().numpy(), want_dF[m], f"dF[{m}] I={I} k={k} {mode}")
    got_dw = dw.cpu().numpy()
    scale = max(np.abs(want_dw).max(), 1e-30)
    # the dw sums run over all nnz entries: the project's tolerance on the tensor's largest element
    print("dw", got_dw, "want", want_dw, want_dtheta)
    assert np.all(np.abs(got_dw[:2] - want_dw) <= ATOL * scale + RTOL * np.abs(want_dw))
    if F[0] is not None and F[1] is not None:
        assert np.all(np.abs(got_dw[2:] - want_dtheta) <= ATOL * scale + RTOL * np.abs(want_dtheta))
    first = [None if o is None else o.clone() for o in out], dw.clone()
    for o in out:
        if o is not None:
            o.fill_(3.0)
    run()
    assert torch.equal(first[1], dw) and all(a is None or torch.equal(a, b) for a, b in zip(first[0], out))


# ---------------------------------------------------------------------------------------------------------------------
# 4. gradient_step against the twin
# ---------------------------------------------------------------------------------------------------------------------
def _detached(g, cfg, **kw):
    from skrec.recommender.LATTICE import LATTICE
    nu, ni = int(g["shape"][0]), int(g["shape"][1])
    feats = dict(img=g["image_embedding_weight_0"], txt=g["text_embedding_weight_0"])
    feats.update(kw)
    _seed()
    m = LATTICE.detached(nu, ni, dict(cfg), (g["adj_rowptr"], g["adj_cols"]), **feats)
    P = {k: v for k, v in T.fixture_params(g, 0).items() if k in m.parameters()}
    m.load_parameters(P)
    return m


def _twin_inputs(m):
    """(A dense, frozen lists) from the model's own arrays: the comparison is of the step, not of the adjacency"""
    N = m.num_users + m.num_items
    A = np.zeros((N, N))
    rp, col, val = m.adj.rowptr.cpu().numpy(), m.adj.col.cpu().numpy(), m.adj.val.cpu().numpy().astype(np.float64)
    A[np.repeat(np.arange(N), np.diff(rp)), col] = val
    frozen = [None, None]
    for idx, key in enumerate(("img", "txt")):
        if m.feat_dim[key]:
            frozen[idx] = (m.frozen[key][0].cpu().numpy().astype(np.int64), m.frozen[key][1].cpu().numpy().astype(np.float64))
    return A, frozen


def _compare_step(m, tcfg, users, pos, neg, what, build):
    A, frozen = _twin_inputs(m)
    P = {k: v.cpu().numpy().astype(np.float64) for k, v in m.parameters().items()}
    knn = None
    if tcfg["n_layers"] > 0:
        G = m._current_graph()
        knn = [G["learned"][key][0].cpu().numpy() if m.feat_dim[key] else None for key in ("img", "txt")]
    comps, want, _, _ = T.gradients_f64(P, A, frozen, users, pos, neg, tcfg, build=build, knn=knn)
    loss = m.gradient_step(users, pos, neg, build=build).cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in m.gradients().items()}
    print(what, "build" if build else "ordinary", "loss", loss, "twin", comps)
    np.testing.assert_allclose(loss[:2], np.array(comps), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(loss[2], sum(comps), rtol=1e-5)
    assert list(got) == [k for k in T.NAMES if k in P]
    for name in got:
        w_ = np.asarray(want[name], np.float64)
        err, scale = np.abs(got[name].astype(np.float64) - w_), float(np.abs(w_).max())
        print(f"{what}: {name}: max abs err {err.max():.3e}, max|want| {scale:.3e}")
        if name not in T.ROWS and (not build or tcfg["n_layers"] == 0):
            assert (got[name] == 0).all(), name          # an unreached modal tensor reads as zeros
            continue
        assert np.all(err <= ATOL * scale + RTOL * np.abs(w_)), (what, name, float(err.max()), scale)
    return loss, got


@pytest.fixture(scope="module")
def tiny_model(golden):
    g = golden("golden_lattice")
    cfg, tcfg = T.fixture_config(g)
    return g, cfg, tcfg, _detached(g, cfg)


@pytest.mark.parametrize("build", [True, False])
def test_gradient_step_on_the_first_batch(tiny_model, build):
    g, cfg, tcfg, m = tiny_model
    st = T.fixture_steps(g)[0]
    _compare_step(m, tcfg, st["users"], st["pos"], st["neg"], "first batch", build)
    for key in ("img", "txt"):          # the padding of every block of the modal gradient buffer is exactly zero
        F, ld = m.feat_dim[key], m.feat_ld[key]
        trs, tab = m._blocks(key, True)
        assert (tab.view(m.num_items, ld)[:, F:] == 0).all() and (trs[:64 * ld].view(64, ld)[:, F:] == 0).all()


@pytest.mark.parametrize("build", [True, False])
def test_gradient_step_on_one_row(tiny_model, build):
    g, cfg, tcfg, m = tiny_model
    _compare_step(m, tcfg, np.array([5]), np.array([7]), np.array([50]), "n = 1", build)


@pytest.mark.parametrize("build", [True, False])
def test_gradient_step_on_one_user_with_equal_items(tiny_model, build):
    g, cfg, tcfg, m = tiny_model
    rng = np.random.default_rng(3)
    n = 37
    pos, neg = rng.integers(0, 96, n), rng.integers(0, 96, n)
    neg[11] = pos[11]
    pos[20] = pos[4]
    _compare_step(m, tcfg, np.full(n, 3), pos, neg, "one user", build)


@pytest.mark.parametrize("build", [True, False])
def test_gradient_step_on_257_rows_with_duplicates_and_ids_out_of_range(tiny_model, build):
    g, cfg, tcfg, m = tiny_model
    rng = np.random.default_rng(257)
    users, pos, neg = rng.integers(0, 64, 257), rng.integers(0, 96, 257), rng.integers(0, 96, 257)
    users[3], pos[17], neg[40], users[256] = 64, -1, 96, -5
    _compare_step(m, tcfg, users, pos, neg, "257 rows", build)


@pytest.mark.parametrize("kw", [dict(cf_model="mf"), dict(n_layers=0), dict(n_layers=1), dict(n_layers=1, cf_model="mf"),
                                dict(weight_size=[64]), dict(embed_dim=20, feat_embed_dim=24, weight_size=[20, 20])],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_gradient_step_for_other_configs(golden, kw):
    g = golden("golden_lattice")
    cfg, _ = T.fixture_config(g)
    cfg.update(kw)
    tcfg = T.twin_config(**cfg)
    from skrec.recommender.LATTICE import LATTICE
    _seed()
    m = LATTICE.detached(64, 96, dict(cfg), (g["adj_rowptr"], g["adj_cols"]), img=g["image_embedding_weight_0"], txt=g["text_embedding_weight_0"])
    st = T.fixture_steps(g)[1]
    for build in (True, False):
        _compare_step(m, tcfg, st["users"], st["pos"], st["neg"], str(kw), build)


@pytest.mark.parametrize("which", ["img", "txt"])
def test_gradient_step_with_one_modality(golden, which):
    g = golden("golden_lattice")
    cfg, tcfg = T.fixture_config(g)
    m = _detached(g, cfg, **{"txt" if which == "img" else "img": None})
    assert "modal_weight" in m.parameters() and len(m.parameters()) == 6
    st = T.fixture_steps(g)[2]
    for build in (True, False):
        _, got = _compare_step(m, tcfg, st["users"], st["pos"], st["neg"], which + " only", build)
        assert (got["modal_weight"] == 0).all()          # reported, never moves


def test_gradient_step_on_a_full_batch():
    """n = 2048 on a seeded random 2100 x 2100 graph with F = 8"""
    from skrec.recommender.LATTICE import LATTICE
    rng = np.random.default_rng(2100)
    nu = ni = 2100
    deg = rng.integers(1, 20, nu)
    items = np.concatenate([np.sort(rng.choice(ni, k, replace=False)) for k in deg]).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    cfg = dict(lr=1e-2, reg=1e-2, lambda_coeff=0.5, n_layers=2, knn_k=10, batch_size=2048)
    _seed()
    m = LATTICE.detached(nu, ni, cfg, (rowptr, items), img=rng.standard_normal((ni, 8)).astype(np.float32),
                         txt=rng.standard_normal((ni, 8)).astype(np.float32))
    users, pos, neg = rng.integers(0, nu, 2048), rng.integers(0, ni, 2048), rng.integers(0, ni, 2048)
    _compare_step(m, T.twin_config(**cfg), users, pos, neg, "n = 2048", True)
    with pytest.raises(NotImplementedError, match="2048"):
        m.gradient_step(np.zeros(2049, np.int32), np.zeros(2049, np.int32), np.zeros(2049, np.int32))


def test_steps_and_the_graph_are_bit_reproducible(tiny_model):
    import torch
    g, cfg, tcfg, m = tiny_model
    st = T.fixture_steps(g)[2]
    for build in (True, False):
        l1 = m.gradient_step(st["users"], st["pos"], st["neg"], build=build).clone()
        g1, mg1, S1 = m._grad.clone(), m._mgrad.clone(), m.graph["S"].val.clone()
        m._grad.fill_(3.0)            # every element is written again
        m._work.fill_(255)
        m._version += 1               # the build step assembles the graph anew
        l2 = m.gradient_step(st["users"], st["pos"], st["neg"], build=build)
        assert torch.equal(l1, l2) and torch.equal(g1, m._grad) and torch.equal(mg1, m._mgrad)
        assert torch.equal(S1, m.graph["S"].val)
        assert build == bool(mg1.abs().max() > 0)


def test_handed_in_neighbour_lists_give_the_same_graph(tiny_model):
    """knn_out records the device's lists; the same lists handed back in, in another order, give the same pattern and values
    within the kernel tolerance (the similarities are then dot products over the lists, not skr_knn_topk's), and lists of
    other ids give another graph"""
    import torch
    g, cfg, tcfg, m = tiny_model
    out = {}
    G0 = m.rebuild_graph(knn_out=out)
    assert set(out) == {"img", "txt"} and out["img"].shape == (96, 10)
    for key in out:
        assert np.array_equal(out[key], G0["learned"][key][0].cpu().numpy())
    col0, val0 = G0["S"].col.clone(), G0["S"].val.clone()
    G1 = m.rebuild_graph(knn_in={k_: v[:, ::-1].copy() for k_, v in out.items()})
    assert torch.equal(G1["S"].col, col0)
    _close(G1["S"].val.cpu().numpy(), val0.cpu().numpy(), "S from handed-in lists")
    for key in out:
        want = T.cosine_at(m._F[key].cpu().numpy().astype(np.float64), out[key][:, ::-1])
        _close(G1["learned"][key][1].cpu().numpy(), want, "similarities of handed-in lists")
    other = {k_: (v + 1) % 96 for k_, v in out.items()}
    G2 = m.rebuild_graph(knn_in=other)
    assert not (G2["nnz"] == G0["nnz"] and torch.equal(G2["S"].col, col0))
    with pytest.raises(ValueError, match="neighbour id"):
        m.rebuild_graph(knn_in={k_: v + 96 for k_, v in out.items()})
    m.rebuild_graph()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the golden replay, fit()
# ---------------------------------------------------------------------------------------------------------------------
def _run_config(data_dir):
    from skrec import RunConfig
    return RunConfig(recommender="LATTICE", data_dir=data_dir, file_column="UIRT", sep="\t", hyperopt=False, gpu_id=0,
                     metric=("Precision", "Recall", "MAP", "NDCG", "MRR"), top_k=(5, 10, 20), test_batch_size=16,
                     test_thread=2, seed=SEED, sampler_mode="exact")


def _write_features(tiny_dir, g):
    import os
    np.savez(os.path.join(tiny_dir, "tiny.img.npz"), features=g["image_embedding_weight_0"])
    np.savez(os.path.join(tiny_dir, "tiny.txt.npz"), features=g["text_embedding_weight_0"])


class _Recorded(object):
    """the reference's evaluator contract on recorded scores: predict() -> ndarray (the generic path)"""

    def __init__(self, users, scores):
        self.row = {int(u): r for r, u in enumerate(users)}
        self.scores = scores

    def predict(self, users):
        return self.scores[[self.row[int(u)] for u in users]]


def test_replays_reference(golden, tiny_dir, monkeypatch, tmp_path):
    """The reference's recorded run, step by step: the same init bits, the reference's neighbour sets at every build, scores and
    final parameters within 6 x the fixture's own deviations, losses to rtol 1e-5, the two step counters."""
    from skrec.recommender.LATTICE import LATTICE
    monkeypatch.chdir(tmp_path)
    g = golden("golden_lattice")
    cfg, tcfg = T.fixture_config(g)
    k = cfg["knn_k"]
    _write_features(tiny_dir, g)
    _seed()
    m = LATTICE(_run_config(tiny_dir), dict(cfg))
    assert (m.num_users, m.num_items) == (64, 96) and m.feat_dim == {"img": 100, "txt": 37}
    P0 = m.parameters()
    want0 = T.fixture_params(g, 0)
    assert list(P0) == list(want0)
    for name, want in want0.items():
        assert np.array_equal(P0[name].cpu().numpy(), want), name        # same init, same seed
    assert np.array_equal(m.adj.rowptr.cpu().numpy(), g["norm_rowptr"]) and np.array_equal(m.adj.col.cpu().numpy(), g["norm_col"])
    assert np.abs(m.adj.val.cpu().numpy() - g["norm_val"]).max() <= float(np.spacing(np.float32(1.0)))
    for key, name in (("img", "image"), ("txt", "text")):
        assert np.array_equal(m.frozen[key][0].cpu().numpy(), np.sort(g[name + "_frozen_ids"], 1)), name
    ev = m.evaluator
    assert list(ev.metrics_list) == list(g["names"])
    test_users = np.fromiter(ev.user_pos_test.keys(), dtype=np.int32)
    assert np.array_equal(test_users, g["test_users"]) and len(test_users) == 63
    dev_p, dev_s = g["f64_dev_params"], g["f64_dev_scores"]
    steps = T.fixture_steps(g)
    assert len(steps) == 9
    losses, n_eval, n_build = [], 0, 0

    def same_sets():
        nonlocal n_build
        for idx, key in enumerate(("img", "txt")):
            got = m.graph["learned"][key][0].cpu().numpy()
            assert np.array_equal(np.sort(got, 1), np.sort(g["knn_ids"][n_build][idx][:, :k], 1)), (n_build, key)
        n_build += 1
    for s, st in enumerate(steps):
        if s % 3 == 0:
            assert m.set_epoch(s // 3) == T.schedule_lr(tcfg, s // 3)
        losses.append(m.train_step(st["users"], st["pos"], st["neg"], build=s % 3 == 0).cpu().numpy())
        if s % 3 == 0:
            same_sets()
        if (s + 1) % 3:
            continue
        report = np.array(list(m.evaluate().values()), np.float32)
        same_sets()
        pred = m.predict(test_users)
        ref = g["pred"][n_eval]
        print("evaluation", n_eval, "max score diff", np.abs(pred - ref).max(), "allowed", 6 * dev_s[n_eval])
        assert np.abs(pred - ref).max() <= 6 * dev_s[n_eval]
        rows, _, n = ev.per_user_rows(m, test_users)
        rows_ref, _, _ = ev.per_user_rows(_Recorded(test_users, ref), test_users)
        ok = ~np.isin(test_users, g["close_ids"][n_eval])
        print("near-tie users left out", int((~ok).sum()))
        assert n == 63 and (~ok).sum() == g["close_users"][n_eval]
        assert np.array_equal(rows[ok], rows_ref[ok])
        if ok.all():
            np.testing.assert_allclose(report, g["reports"][n_eval], rtol=1e-5, atol=0, err_msg=str(g["names"]))
        n_eval += 1
    assert n_eval == 3 and n_build == 6
    assert m.optimizer.t == 9 and m.modal_optimizer.t == 3
    losses = np.stack(losses)
    print("loss", losses[:, 2], "golden", g["loss"], "largest relative difference", np.abs(losses[:, 2] / g["loss"] - 1).max())
    np.testing.assert_allclose(losses[:, 2], g["loss"], rtol=1e-5)
    P1 = {k_: v.cpu().numpy() for k_, v in m.parameters().items()}
    final = T.fixture_params(g, 1)
    missed = []
    for idx, name in enumerate(T.NAMES):        # every tensor is measured before the assertion
        diff = np.abs(P1[name] - final[name]).max()
        print(name, "max abs diff", diff, "allowed", 6 * dev_p[idx])
        if not diff <= 6 * dev_p[idx]:
            missed.append((name, float(diff), float(6 * dev_p[idx])))
    assert not missed, missed


def test_fit_follows_the_schedule(golden, tiny_dir, monkeypatch, tmp_path):
    """fit() on the tiny set as run_skrec.py starts it -- the class from the registry, the run config, the model config"""
    import torch
    from skrec.utils.registry import ModelRegistry
    monkeypatch.chdir(tmp_path)
    g = golden("golden_lattice")
    cfg, tcfg = T.fixture_config(g)
    _write_features(tiny_dir, g)
    registry = ModelRegistry()
    assert registry.load_skrec_model("LATTICE")
    model_class, config_class = registry.get_model("LATTICE")
    _seed()
    m = model_class(_run_config(tiny_dir), dict(cfg))
    assert isinstance(m.config, config_class)
    lrs, mlrs, orig_step, orig_mstep = [], [], m.optimizer.step, m.modal_optimizer.step

    def step():
        lrs.append(m.optimizer.lr)
        orig_step()

    def mstep():
        mlrs.append(m.modal_optimizer.lr)
        orig_mstep()
    m.optimizer.step, m.modal_optimizer.step = step, mstep
    builds, orig_rebuild = [], m.rebuild_graph

    def rebuild(*a, **k_):
        builds.append(len(lrs))
        return orig_rebuild(*a, **k_)
    m.rebuild_graph = rebuild
    first = None
    orig_eval = m.evaluate

    def evaluate(tu=None):
        nonlocal first
        if first is None:
            first = torch.stack(m.step_losses).cpu().numpy()
        return orig_eval(tu)
    m.evaluate = evaluate
    best = m.fit()
    assert np.isfinite(np.array(list(best.values()))).all()
    assert lrs == [T.schedule_lr(tcfg, e) for e in range(3) for _ in range(3)] and lrs[-1] == 1e-2 * 0.25
    assert mlrs == [T.schedule_lr(tcfg, e) for e in range(3)]
    # one build before the first step, one per evaluation; an evaluation's graph serves the next epoch's build step
    assert builds == [0, 3, 6, 9]
    last = torch.stack(m.step_losses).cpu().numpy()
    assert np.isfinite(first).all() and np.isfinite(last).all() and last[:, 2].mean() < first[:, 2].mean()


def test_limits_raise_on_the_device_too():
    from skrec.recommender.LATTICE import LATTICE
    z = lambda F: np.zeros((8, F), np.float32)        # noqa: E731
    for kw, word in ((dict(embed_dim=65), "embed_dim"), (dict(feat_embed_dim=65), "feat_embed_dim"), (dict(weight_size=[64] * 5), "weight_size"),
                     (dict(n_layers=5), "n_layers"), (dict(batch_size=2049), "batch_size"), (dict(knn_k=33), "knn_k"),
                     (dict(cf_model="ngcf"), "cf_model")):
        with pytest.raises(NotImplementedError, match=word):
            LATTICE.detached(8, 8, dict(kw), img=z(4), txt=z(4))
    with pytest.raises(NotImplementedError, match="feature width"):
        LATTICE.detached(8, 8, {}, img=z(4097))
    with pytest.raises(ValueError, match="no modality"):
        LATTICE.detached(8, 8, {})
