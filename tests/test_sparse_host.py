"""CPU suite of skrec/recommender/_sparse.py.  The library calls of ``DeviceCSR.spmm`` and ``_graph.run_plan`` -- entry, order,
arguments, the epilogue field by field -- against sequences written out below: ``_hip.lib`` is a recorder, the tables are
CPU tensors, every address is noted as the name of the tensor it falls in and the byte offset.  Then the ways to build a
matrix (same arrays from each, one padding entry for an empty one) and the names the move left behind."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from skrec import _hip
from skrec.recommender._sparse import DeviceCSR

STREAM = 77
N = 5                   # a 5 x 5 matrix, row 3 empty, 6 entries
DENSE = np.array([[0, 1, 0, 0, 2], [3, 0, 0, 0, 0], [0, 0, 4, 5, 0], [0, 0, 0, 0, 0], [0, 6, 0, 0, 0]], np.float32)


class Recorder(object):
    """stands for the loaded library: every attribute is a function that notes (entry, arguments) and returns 0"""

    def __init__(self):
        self.calls, self.tensors, self.scratch = [], {}, None

    def name(self, **tensors):
        self.tensors.update(tensors)

    def _note(self, a):
        if isinstance(a, ctypes.c_void_p):
            return "plan"
        if hasattr(a, "_obj"):              # byref(...)
            if isinstance(a._obj, ctypes.Structure):
                fields = {f: self._note(getattr(a._obj, f)) for f, _ in a._obj._fields_}
                return {f: v for f, v in fields.items() if v not in (0, None) or f == "mode"}
            return "&plan"
        if isinstance(a, int) and a >= 1 << 20:      # an address
            for name, t in self.tensors.items():
                if t.data_ptr() <= a < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                    return f"{name}+{a - t.data_ptr()}"
            if self.scratch is None:        # a table the matrix allocated itself: named by its first address
                self.scratch = a
            return f"scratch+{a - self.scratch}"
        return a

    def __getattr__(self, entry):
        def fn(*args):
            self.calls.append((entry,) + tuple(self._note(a) for a in args))
            return 0
        return fn


@pytest.fixture()
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_hip, "lib", lambda: r)
    monkeypatch.setattr(_hip, "stream", lambda: STREAM)
    return r


def _matrix(rec):
    m = DeviceCSR(sp.csr_matrix(DENSE), "cpu")
    assert m.nnz == 6 and m.rowptr.tolist() == [0, 2, 3, 5, 5, 6]
    rec.name(rowptr=m.rowptr, col=m.col, val=m.val)
    return m


def _tables(rec, W):
    t = {k: torch.zeros(N, W) for k in ("X", "Y", "ADD", "ACC", "BASE", "E", "Z", "RAWY", "DE")}
    t["w"] = torch.zeros(N)
    t.update({k: torch.ones(N, dtype=torch.uint8) for k in ("RM", "CM", "AM", "DM")})
    rec.name(**t)
    return t


def _shape_args(shape, t):
    """(Y, keywords) of ``spmm`` for each of the argument shapes the models use"""
    return {
        "plain": (t["Y"], {}),
        "addend_accum": (t["Y"], dict(addend=t["ADD"], accum=t["ACC"], accum_scale=1.0)),
        "accum_base": (t["Y"], dict(accum=t["ACC"], accum_scale=0.25, accum_base=t["BASE"])),
        "accum_init": (t["Y"], dict(accum=t["ACC"], accum_scale=0.5, accum_init=True)),
        "no_Y_accum": (None, dict(accum=t["ACC"], accum_scale=1.0)),
        "refine_fwd": (t["Y"], dict(accum=t["ACC"], refine_fwd=(t["E"], t["w"], t["Z"]))),
        "refine_bwd": (t["Y"], dict(addend=t["ADD"], refine_bwd=(t["E"], t["w"], t["RAWY"], t["DE"]))),
        "masks": (t["Y"], dict(addend=t["ADD"], accum=t["ACC"], row_mask=t["RM"], col_mask=t["CM"], accum_mask=t["AM"],
                               addend_mask=t["DM"])),
    }[shape]


SHAPES = ["plain", "addend_accum", "accum_base", "accum_init", "no_Y_accum", "refine_fwd", "refine_bwd", "masks"]
CSR = ("rowptr+0", "col+0", "val+0")
CREATE = ("skr_spmm_plan_create", 5, 5) + CSR + (6, 0, "&plan", STREAM)

# (SKR_SPMM_PLAN, width, shape) -> the calls of a matrix's first product (which creates the plan where it runs one)
EXPECTED = {
    ("0", 64, "plain"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, None, "Y+0", None, 1.0, STREAM)],
    ("0", 64, "addend_accum"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, "ADD+0", "Y+0", "ACC+0", 1.0, STREAM)],
    ("0", 64, "accum_base"): [
        ("skr_scale_copy", 0.25, "BASE+0", "ACC+0", 320, STREAM),
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, None, "Y+0", "ACC+0", 0.25, STREAM)],
    ("0", 64, "accum_init"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, None, "Y+0", "ACC+0", 0.5, STREAM)],
    ("0", 64, "no_Y_accum"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, None, "scratch+0", "ACC+0", 1.0, STREAM)],
    ("0", 64, "refine_fwd"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, None, "Y+0", None, 1.0, STREAM),
        ("skr_layer_refine_fwd", "Y+0", "E+0", 5, 64, "Z+0", "w+0", "ACC+0", STREAM)],
    ("0", 64, "refine_bwd"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, "ADD+0", "scratch+0", None, 1.0, STREAM),
        ("skr_layer_refine_bwd", "RAWY+0", "E+0", "w+0", "scratch+0", 5, 64, "Y+0", "DE+0", STREAM)],
    ("0", 64, "masks"): [
        ("skr_csr_spmm", 5, *CSR, "X+0", 64, 6, "ADD+0", "Y+0", "ACC+0", 1.0, STREAM)],
    ("0", 128, "plain"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, None, "Y+0", None, 1.0, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, None, "Y+256", None, 1.0, STREAM)],
    ("0", 128, "addend_accum"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, "ADD+0", "Y+0", "ACC+0", 1.0, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, "ADD+256", "Y+256", "ACC+256", 1.0, STREAM)],
    ("0", 128, "accum_base"): [
        ("skr_scale_copy", 0.25, "BASE+0", "ACC+0", 640, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, None, "Y+0", "ACC+0", 0.25, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, None, "Y+256", "ACC+256", 0.25, STREAM)],
    ("0", 128, "accum_init"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, None, "Y+0", "ACC+0", 0.5, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, None, "Y+256", "ACC+256", 0.5, STREAM)],
    ("0", 128, "no_Y_accum"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, None, "scratch+0", "ACC+0", 1.0, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, None, "scratch+256", "ACC+256", 1.0, STREAM)],
    ("0", 128, "refine_fwd"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, None, "Y+0", None, 1.0, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, None, "Y+256", None, 1.0, STREAM),
        ("skr_layer_refine_fwd", "Y+0", "E+0", 5, 128, "Z+0", "w+0", "ACC+0", STREAM)],
    ("0", 128, "refine_bwd"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, "ADD+0", "scratch+0", None, 1.0, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, "ADD+256", "scratch+256", None, 1.0, STREAM),
        ("skr_layer_refine_bwd", "RAWY+0", "E+0", "w+0", "scratch+0", 5, 128, "Y+0", "DE+0", STREAM)],
    ("0", 128, "masks"): [
        ("skr_csr_spmm_strided", 5, *CSR, "X+0", 64, 128, 6, "ADD+0", "Y+0", "ACC+0", 1.0, STREAM),
        ("skr_csr_spmm_strided", 5, *CSR, "X+256", 64, 128, 6, "ADD+256", "Y+256", "ACC+256", 1.0, STREAM)],
    ("1", 64, "plain"): [
        CREATE,
        ("skr_spmm_plan_run_masked", "plan", "X+0", 64, None, "Y+0", None, 1.0, None, None, STREAM)],
    ("1", 64, "addend_accum"): [
        CREATE,
        ("skr_spmm_plan_run_masked", "plan", "X+0", 64, "ADD+0", "Y+0", "ACC+0", 1.0, None, None, STREAM)],
    ("1", 64, "accum_base"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="Y+0", accum="ACC+0", accum_base="BASE+0", accum_scale=0.25), None, None, STREAM)],
    ("1", 64, "accum_init"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, accum_init=1, Y="Y+0", accum="ACC+0", accum_scale=0.5), None, None, STREAM)],
    ("1", 64, "no_Y_accum"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, accum="ACC+0", accum_scale=1.0), None, None, STREAM)],
    ("1", 64, "refine_fwd"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=1, Y="Y+0", accum="ACC+0", accum_scale=1.0, E="E+0", w="w+0", Z="Z+0"), None, None, STREAM)],
    ("1", 64, "refine_bwd"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=2, addend="ADD+0", Y="Y+0", accum_scale=1.0, E="E+0", w="w+0", rawY="RAWY+0", dE="DE+0"), None, None, STREAM)],
    ("1", 64, "masks"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, addend="ADD+0", Y="Y+0", accum="ACC+0", accum_scale=1.0, accum_mask="AM+0", addend_mask="DM+0"), "RM+0", "CM+0", STREAM)],
    ("1", 128, "plain"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="Y+0", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, Y="Y+256", accum_scale=1.0, ld=128), None, None, STREAM)],
    ("1", 128, "addend_accum"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, addend="ADD+0", Y="Y+0", accum="ACC+0", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, addend="ADD+256", Y="Y+256", accum="ACC+256", accum_scale=1.0, ld=128), None, None, STREAM)],
    ("1", 128, "accum_base"): [
        ("skr_scale_copy", 0.25, "BASE+0", "ACC+0", 640, STREAM),
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="Y+0", accum="ACC+0", accum_scale=0.25, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, Y="Y+256", accum="ACC+256", accum_scale=0.25, ld=128), None, None, STREAM)],
    ("1", 128, "accum_init"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="Y+0", accum="ACC+0", accum_scale=0.5, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, Y="Y+256", accum="ACC+256", accum_scale=0.5, ld=128), None, None, STREAM)],
    ("1", 128, "no_Y_accum"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="scratch+0", accum="ACC+0", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, Y="scratch+256", accum="ACC+256", accum_scale=1.0, ld=128), None, None, STREAM)],
    ("1", 128, "refine_fwd"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="Y+0", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, Y="Y+256", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_layer_refine_fwd", "Y+0", "E+0", 5, 128, "Z+0", "w+0", "ACC+0", STREAM)],
    ("1", 128, "refine_bwd"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, addend="ADD+0", Y="scratch+0", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, addend="ADD+256", Y="scratch+256", accum_scale=1.0, ld=128), None, None, STREAM),
        ("skr_layer_refine_bwd", "RAWY+0", "E+0", "w+0", "scratch+0", 5, 128, "Y+0", "DE+0", STREAM)],
    ("1", 128, "masks"): [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, addend="ADD+0", Y="Y+0", accum="ACC+0", accum_scale=1.0, ld=128, accum_mask="AM+0", addend_mask="DM+0"), "RM+0", "CM+0", STREAM),
        ("skr_spmm_plan_run_ex", "plan", "X+256", 64, dict(mode=0, addend="ADD+256", Y="Y+256", accum="ACC+256", accum_scale=1.0, ld=128, accum_mask="AM+0", addend_mask="DM+0"), "RM+0", "CM+0", STREAM)],
}

# _graph.run_plan(mat, X, ...) without and with a base
EXPECTED_RUN_PLAN = {
    False: [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, addend="ADD+0", accum="ACC+0", accum_scale=0.5), None, None, STREAM)],
    True: [
        CREATE,
        ("skr_spmm_plan_run_ex", "plan", "X+0", 64, dict(mode=0, Y="Y+0", accum="ACC+0", accum_base="BASE+0", accum_scale=0.25), None, None, STREAM)],
}


def _spmm_calls(rec, monkeypatch, plan, W, shape):
    monkeypatch.setenv("SKR_SPMM_PLAN", plan)
    monkeypatch.delenv("SKR_SPMM_LONG_FROM", raising=False)
    m, t = _matrix(rec), _tables(rec, W)
    Y, kw = _shape_args(shape, t)
    assert m.spmm(t["X"], Y, **kw) is Y
    return list(rec.calls)          # (while the matrix is alive: its end destroys the plan)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("plan", ["0", "1"])
def test_spmm_call_sequence(rec, monkeypatch, plan, W, shape):
    assert _spmm_calls(rec, monkeypatch, plan, W, shape) == EXPECTED[plan, W, shape]


def test_the_plan_is_created_once(rec, monkeypatch):
    monkeypatch.setenv("SKR_SPMM_PLAN", "1")
    m, t = _matrix(rec), _tables(rec, 64)
    m.spmm(t["X"], t["Y"])
    m.spmm(t["X"], t["Y"])
    assert [c[0] for c in rec.calls] == ["skr_spmm_plan_create", "skr_spmm_plan_run_masked", "skr_spmm_plan_run_masked"]


def _run_plan_calls(rec, base):
    from skrec.recommender._graph import run_plan
    m, t = _matrix(rec), _tables(rec, 64)
    if base:
        run_plan(m, t["X"], Y=t["Y"], accum=t["ACC"], accum_base=t["BASE"], accum_scale=0.25)
    else:
        run_plan(m, t["X"], accum=t["ACC"], addend=t["ADD"], accum_scale=0.5)
    return list(rec.calls)


@pytest.mark.parametrize("base", [False, True])
def test_run_plan_call_sequence(rec, monkeypatch, base):
    monkeypatch.setenv("SKR_SPMM_PLAN", "0")        # run_plan goes through the plan whatever the setting
    assert _run_plan_calls(rec, base) == EXPECTED_RUN_PLAN[base]


# ---- the ways to build a matrix -----------------------------------------------------------------
def _builds(rows, cols, vals, n_rows, n_cols):
    """the same matrix from scipy, from CSR arrays (under both names) and from COO triples"""
    from skrec.recommender._graph import _device_csr
    ref = sp.csr_matrix((vals, (rows, cols)), shape=(n_rows, n_cols))
    arrays = (torch.from_numpy(ref.indptr.astype(np.int64)), torch.from_numpy(ref.indices.astype(np.int32)),
              torch.from_numpy(ref.data.astype(np.float32)))
    coo = (torch.from_numpy(rows.astype(np.int64)), torch.from_numpy(cols.astype(np.int64)), torch.from_numpy(vals))
    return ref, {"scipy": DeviceCSR(ref, "cpu"), "from_arrays": DeviceCSR.from_arrays((n_rows, n_cols), *arrays),
                 "_device_csr": _device_csr((n_rows, n_cols), *arrays), "from_coo": DeviceCSR.from_coo(*coo, n_rows, n_cols)}


def test_every_constructor_builds_the_same_matrix():
    rows, cols = np.array([4, 0, 2, 0, 1, 2]), np.array([1, 2, 0, 0, 1, 2])     # unsorted, no duplicate, row 3 empty
    vals = np.arange(1, 7, dtype=np.float32) / 8
    ref, built = _builds(rows, cols, vals, 5, 3)
    for how, m in built.items():
        assert m.shape == (5, 3) and type(m.shape[0]) is int and m.nnz == 6 and type(m.nnz) is int, how
        assert (m.rowptr.dtype, m.col.dtype, m.val.dtype) == (torch.int64, torch.int32, torch.float32), how
        assert m.rowptr.is_contiguous() and m.col.is_contiguous() and m.val.is_contiguous(), how
        assert m.rowptr.tolist() == ref.indptr.tolist() == [0, 2, 3, 5, 5, 6], how
        assert m.col.tolist() == ref.indices.tolist() and np.array_equal(m.val.numpy(), ref.data), how


def test_from_arrays_makes_views_contiguous():
    rp, col, val = torch.tensor([0, 9, 1, 9, 2])[::2], torch.tensor([1, 7, 0, 7], dtype=torch.int32)[::2], torch.ones(4)[::2]
    m = DeviceCSR.from_arrays((2, 2), rp, col, val)
    assert m.rowptr.is_contiguous() and m.col.is_contiguous() and m.val.is_contiguous()
    assert m.rowptr.tolist() == [0, 1, 2] and m.col.tolist() == [1, 0] and m.nnz == 2


def test_an_empty_matrix_keeps_one_padding_entry():
    none = np.zeros(0, np.int64)
    _, built = _builds(none, none, np.zeros(0, np.float32), 3, 2)
    built["from_device_coo"] = DeviceCSR.from_device_coo(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                                                         torch.zeros(0), 3)
    for how, m in built.items():
        assert m.nnz == 0 and m.rowptr.tolist() == [0, 0, 0, 0], how
        assert m.col.tolist() == [0] and m.val.tolist() == [0.0], how
        assert (m.col.dtype, m.val.dtype) == (torch.int32, torch.float32), how


def test_from_device_coo_is_the_square_from_coo():
    r, c, v = torch.tensor([2, 0, 1]), torch.tensor([0, 2, 1]), torch.tensor([1.0, 2.0, 3.0])
    a, b = DeviceCSR.from_device_coo(r, c, v, 3), DeviceCSR.from_coo(r, c, v, 3, 3)
    assert a.shape == b.shape == (3, 3) and a.col.tolist() == b.col.tolist() == [2, 1, 0] and a.val.tolist() == [2.0, 3.0, 1.0]


def test_the_old_names_are_the_moved_objects():
    from skrec import parallel
    from skrec.recommender import LayerGCN, LightGCL, LightGCN, _graph, _sparse
    assert LightGCN.DeviceCSR is _graph.DeviceCSR is LightGCL.DeviceCSR is parallel.DeviceCSR is _sparse.DeviceCSR
    assert LightGCN.padded_width is _sparse.padded_width and LightGCN.pad_columns is _sparse.pad_columns
    assert LightGCL._device_csr is _graph._device_csr
    assert callable(LightGCN.build_adjacency) and callable(LightGCN.build_adjacency_device)
    assert LayerGCN.DEVICE_ADJ_MIN_PAIRS == LightGCN.DEVICE_ADJ_MIN_PAIRS == 1 << 21
    assert "DEVICE_ADJ_MIN_PAIRS" in vars(LayerGCN) and not hasattr(parallel, "_csr_from_device_coo")
    assert callable(DeviceCSR.from_device_coo)
