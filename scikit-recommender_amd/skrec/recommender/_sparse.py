"""Sparse matrices in HBM and the row widths of the dense tables they multiply: ``DeviceCSR`` (the CSR arrays, the SpMM plan
built at the first product, ``spmm`` with its row epilogues), ``padded_width`` and ``pad_columns``.  Every model that
multiplies by an adjacency imports from here; ``DeviceCSR.from_arrays`` is the only code that sets a matrix's arrays and
``DeviceCSR._run_epilogue`` the only code that fills a ``skr_spmm_epilogue``.
"""
import ctypes
import os

import numpy as np
import scipy.sparse as sp
import torch

from .. import _hip

__all__ = ["DeviceCSR", "padded_width", "pad_columns"]

_NO_REFINE = (None,) * 5        # E, w, Z, rawY, dE of an epilogue without a refinement


class DeviceCSR(object):
    """A scipy matrix as (rowptr int64, col int32, val fp32) in HBM; duplicates summed, columns
    ascending per row -- the same canonical form as the reference's coalesced COO tensor
    (utils/torch.py:32-35)."""

    def __init__(self, mat, device):
        csr = sp.csr_matrix(mat).astype(np.float32)
        csr.sum_duplicates()
        csr.sort_indices()
        self._set_arrays(csr.shape, torch.from_numpy(csr.indptr.astype(np.int64)).to(device),
                         torch.from_numpy(csr.indices.astype(np.int32)).to(device),
                         torch.from_numpy(csr.data.astype(np.float32)).to(device))

    def _set_arrays(self, shape, rowptr, col, val):
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(col.numel())
        self.rowptr, self.col, self.val = rowptr.contiguous(), col.contiguous(), val.contiguous()
        if self.nnz == 0:       # the kernels are handed valid addresses: an empty matrix keeps one padding entry
            self.col = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
            self.val = torch.zeros(1, dtype=torch.float32, device=rowptr.device)
        self._plan = None
        self._scratch = {}      # row width -> [n_rows, width] scratch of the plan-free and the wide paths

    @classmethod
    def from_arrays(cls, shape, rowptr, col, val):
        """a matrix around CSR arrays that are already in HBM (rowptr int64, col int32, val fp32; canonical form)"""
        self = cls.__new__(cls)
        self._set_arrays(shape, rowptr, col, val)
        return self

    @classmethod
    def from_coo(cls, rows, cols, vals, n_rows, n_cols=None):
        """build from int64 row / col and fp32 value tensors already in HBM (entries must be unique); square unless
        ``n_cols`` is given"""
        n_cols = n_rows if n_cols is None else n_cols
        order = torch.argsort(rows * n_cols + cols)
        rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
        return cls.from_arrays((n_rows, n_cols), rowptr, cols[order].int(), vals[order].float())

    @classmethod
    def from_device_coo(cls, rows, cols, vals, n_rows):
        """the square ``from_coo``"""
        return cls.from_coo(rows, cols, vals, n_rows)

    # matrices with at least this many non-zeros are multiplied through a plan (skr_spmm_plan_*: 16-byte gathers, long rows
    # column-blocked); smaller ones through the plan-free kernel.  SKR_SPMM_PLAN=0 / 1 forces one or the other.
    PLAN_MIN_NNZ = 1 << 16

    def _plan_handle(self, long_rows_from=0):
        """the matrix's plan, built at the first product (one-time analysis on the device)"""
        h = self._plan
        if h is None:
            h = ctypes.c_void_p()
            if not long_rows_from:      # tuning switch: rows of at least this many entries are cut into column-blocked tasks (0 = 512)
                long_rows_from = int(os.environ.get("SKR_SPMM_LONG_FROM", "0"))
            _hip.check(_hip.lib().skr_spmm_plan_create(self.shape[0], self.shape[1], _hip.ptr(self.rowptr), _hip.ptr(self.col),
                                                       _hip.ptr(self.val), self.nnz, int(long_rows_from), ctypes.byref(h),
                                                       _hip.stream()))
            self._plan = h
        return h

    def plan_info(self):
        info = (ctypes.c_int64 * 4)()
        _hip.check(_hip.lib().skr_spmm_plan_info(self._plan_handle(), info))
        return dict(long_rows=info[0] & 0xffffffff, hot_rows=info[0] >> 32, tasks=info[1], column_blocks=info[2],
                    long_rows_from=info[3] & 0xffffffff, column_windows=info[3] >> 32)

    def __del__(self):
        h = getattr(self, "_plan", None)
        if h is not None:
            try:
                _hip.lib().skr_spmm_plan_destroy(h)
            except Exception:   # noqa: BLE001 -- interpreter shutdown
                pass
            self._plan = None

    def scatter_marked_rows(self, row_mask, X, Y):
        """Y[c] += A[r, c] * X[r] over the entries of the rows marked in ``row_mask`` (uint8 [n_rows]): the product with the
        TRANSPOSE where X is zero outside the marked rows (skr_csr_scatter_marked_rows); Y must be initialised"""
        _hip.check(_hip.lib().skr_csr_scatter_marked_rows(self.shape[0], _hip.ptr(self.rowptr), _hip.ptr(self.col), _hip.ptr(self.val),
                                                          _hip.ptr(row_mask), _hip.ptr(X), 64, _hip.ptr(Y), _hip.stream()))
        return Y

    def uses_plan(self):
        """whether products of this matrix go through the plan (which honours the row / column masks)"""
        mode = os.environ.get("SKR_SPMM_PLAN", "auto")
        return mode == "1" or (mode != "0" and self.nnz >= self.PLAN_MIN_NNZ)

    def _run_epilogue(self, x, row_mask, col_mask, *fields):
        """one run of the plan on the 64 columns at address ``x`` with a row epilogue.  ``fields``: those of skr_spmm_epilogue
        in the header's order (include/skrec_hip.h: mode, accum_init, addend, Y, accum, accum_base, accum_scale, ld, E, w, Z,
        rawY, dE, accum_mask, addend_mask), tables as addresses; the fields left out at the end are zero"""
        ep = _hip.SpmmEpilogue(*fields)
        _hip.check(_hip.lib().skr_spmm_plan_run_ex(self._plan_handle(), x, 64, ctypes.byref(ep), _hip.ptr(row_mask),
                                                   _hip.ptr(col_mask), _hip.stream()))

    def _before_product(self, X, Y, W, accum, accum_scale, accum_base, accum_init, refine_fwd, refine_bwd):
        """what a product without the full row epilogue needs first: the table that receives the raw rows (scratch where
        the caller keeps none, or where they are the dZ of a refinement) and the initial value of ``accum``.  Returns the
        table."""
        raw = Y
        if Y is None or refine_bwd is not None:
            raw = self._scratch.get(W)
            if raw is None:
                raw = self._scratch[W] = torch.empty((self.shape[0], W), dtype=torch.float32, device=X.device)
        if refine_fwd is None and refine_bwd is None and accum is not None and accum_base is not None:
            _hip.check(_hip.lib().skr_scale_copy(float(accum_scale), _hip.ptr(accum_base), _hip.ptr(accum), self.shape[0] * W,
                                                 _hip.stream()))
        elif accum is not None and accum_init:
            accum.zero_()
        return raw

    def _after_product(self, raw, Y, W, accum, refine_fwd, refine_bwd):
        """LayerGCN's refinements as launches of their own over the whole rows of ``raw``"""
        L, st, n = _hip.lib(), _hip.stream(), self.shape[0]
        if refine_fwd is not None:
            E, w, Z = refine_fwd
            _hip.check(L.skr_layer_refine_fwd(_hip.ptr(raw), _hip.ptr(E), n, W, _hip.ptr(Z), _hip.ptr(w), _hip.ptr(accum), st))
        elif refine_bwd is not None:
            E, w, rawY, dE = refine_bwd
            _hip.check(L.skr_layer_refine_bwd(_hip.ptr(rawY), _hip.ptr(E), _hip.ptr(w), _hip.ptr(raw), n, W, _hip.ptr(Y), _hip.ptr(dE),
                                              st))
        return Y

    def spmm(self, X, Y, addend=None, accum=None, accum_scale=1.0, row_mask=None, col_mask=None, accum_base=None, accum_init=False,
             refine_fwd=None, refine_bwd=None, accum_mask=None, addend_mask=None):
        """Y = A @ X (+ addend); accum += accum_scale * Y.
        ``row_mask`` (uint8 [n_rows]): only rows with a non-zero byte are needed (the others may be left untouched);
        ``col_mask`` (uint8 [n_cols]): rows of X with a zero byte ARE zero, their entries may be skipped.  Both are
        hints: the plan-free kernel computes the whole product.
        Row-local passes that ride in the product's row epilogue (skr_spmm_epilogue, include/skrec_hip.h):
        ``accum_base``: accum = accum_scale * accum_base + accum_scale * Y (accum is not read: the layer mean with its E0 term);
        ``accum_init``: accum = accum_scale * Y, resp. accum = Z (accum is not read);
        ``refine_fwd`` = (E, w, Z): LayerGCN's refinement of the finished rows, w = cos(Y, E), Z = w * Y, accum += Z
        (Y keeps the raw rows; may be None);
        ``refine_bwd`` = (E, w, rawY, dE): the finished rows are dZ of a refinement; Y receives dY, dE its E0 part.
        ``accum_mask`` (uint8 [n_rows]): accum is only needed on the rows with a non-zero byte; ``addend_mask`` (uint8
        [n_rows]): addend IS zero on the rows with a zero byte (hints again: the plan-free path reads / updates every row)."""
        W = int(X.shape[1])
        if W != 64:
            return self._spmm_wide(X, Y, W, addend, accum, accum_scale, row_mask, col_mask, accum_base, accum_init, refine_fwd,
                                   refine_bwd, accum_mask, addend_mask)
        if self.uses_plan():
            if Y is not None and accum_base is None and not accum_init and refine_fwd is None and refine_bwd is None \
                    and accum_mask is None and addend_mask is None:
                _hip.check(_hip.lib().skr_spmm_plan_run_masked(self._plan_handle(), _hip.ptr(X), 64, _hip.ptr(addend), _hip.ptr(Y),
                                                               _hip.ptr(accum), float(accum_scale), _hip.ptr(row_mask),
                                                               _hip.ptr(col_mask), _hip.stream()))
                return Y
            p, mode, refine = _hip.ptr, _hip.EPI_PLAIN, _NO_REFINE
            if refine_fwd is not None:
                E, w, Z = refine_fwd
                mode, refine = _hip.EPI_REFINE_FWD, (p(E), p(w), p(Z), None, None)
            elif refine_bwd is not None:
                E, w, rawY, dE = refine_bwd
                mode, refine = _hip.EPI_REFINE_BWD, (p(E), p(w), None, p(rawY), p(dE))
            self._run_epilogue(p(X), row_mask, col_mask, mode, bool(accum_init), p(addend), p(Y), p(accum), p(accum_base),
                               float(accum_scale), 0, *refine, p(accum_mask), p(addend_mask))
            return Y
        # small graphs: the plan-free kernel computes whole products; the row-local passes are launches of their own
        plain = refine_fwd is None and refine_bwd is None
        raw = self._before_product(X, Y, 64, accum, accum_scale, accum_base, accum_init, refine_fwd, refine_bwd)
        _hip.check(_hip.lib().skr_csr_spmm(self.shape[0], _hip.ptr(self.rowptr), _hip.ptr(self.col), _hip.ptr(self.val), _hip.ptr(X), 64,
                                           self.nnz, _hip.ptr(addend), _hip.ptr(raw), _hip.ptr(accum) if plain else None,
                                           float(accum_scale), _hip.stream()))
        return self._after_product(raw, Y, 64, accum, refine_fwd, refine_bwd)

    def _spmm_wide(self, X, Y, W, addend, accum, accum_scale, row_mask, col_mask, accum_base, accum_init, refine_fwd, refine_bwd,
                   accum_mask, addend_mask):
        """Embedding widths beyond 64 (tables [n, W], W = 64 C; narrower widths are zero-padded by the models): the product is
        separable in the columns, so it runs slice by slice through the 64-column kernels with the tables' row stride
        (skr_spmm_epilogue.ld / skr_csr_spmm_strided); LayerGCN's refinements reduce over whole rows and are launches of
        their own over the full width."""
        n, C = self.shape[0], W // 64
        assert W % 64 == 0 and 2 <= C <= 4, "pad the embedding width to a multiple of 64 (at most 256)"
        plain = refine_fwd is None and refine_bwd is None
        raw = self._before_product(X, Y, W, accum, accum_scale, accum_base, accum_init, refine_fwd, refine_bwd)
        sl = lambda t, c: None if t is None else t.data_ptr() + 256 * c      # noqa: E731  the c-th 64-column slice
        for t in (X, raw, addend, accum):
            assert t is None or (t.is_contiguous() and t.shape[1] == W)
        for c in range(C):
            if self.uses_plan():
                self._run_epilogue(sl(X, c), row_mask, col_mask, _hip.EPI_PLAIN, 0, sl(addend, c), sl(raw, c),
                                   sl(accum, c) if plain else None, None, float(accum_scale), W, *_NO_REFINE,
                                   _hip.ptr(accum_mask) if plain else None, _hip.ptr(addend_mask))
            else:
                _hip.check(_hip.lib().skr_csr_spmm_strided(n, _hip.ptr(self.rowptr), _hip.ptr(self.col), _hip.ptr(self.val), sl(X, c),
                                                           64, W, self.nnz, sl(addend, c), sl(raw, c),
                                                           sl(accum, c) if plain else None, float(accum_scale), _hip.stream()))
        return self._after_product(raw, Y, W, accum, refine_fwd, refine_bwd)


def padded_width(d):
    """the kernels' row widths are multiples of 64 floats (one 256-byte access per lane group): an embedding of another width
    -- n_dim / embed_size / embed_dim are free integers in the reference -- lives in zero-padded rows.  Padded columns have
    zero gradients, stay zero under Adam and add nothing to a dot product, a norm or a propagation."""
    dp = 64 * ((int(d) + 63) // 64)
    if dp > 256:
        raise NotImplementedError("embedding widths up to 256 are supported by the MI355X kernels")
    return dp


def pad_columns(t, dp):
    return t if t.shape[1] == dp else torch.nn.functional.pad(t, (0, dp - t.shape[1]))
