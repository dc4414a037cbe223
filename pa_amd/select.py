"""Selective reads: decode only the selected rows of a flat column or of a
List<primitive> column.

A `Selection` is an LSB-first Arrow bitmap in HBM over a column's rows (a
List column's top-level rows).  It
is resolved against the column's page metas on the device (k_sel_count, one
readback); pages without a selected row are then never uploaded, planned,
staged or decoded.  The decoders here return exactly the selected rows, in
row order, as dense Arrow buffers (values, validity, for Binary / Utf8
offsets that start at 0):

  Selection                      the bitmap: from a bool tensor, a packed bitmap or row ranges
  page_runs                      maximal runs of adjacent touched pages (what a file read uploads)
  ColumnDecoder.select           fixed width / Boolean  (sb_plan_selected_column + sb_decode_selected)
  BinaryColumnDecoder.select     Binary / Utf8          (... + sb_decode_binary_selected)
  read_selected                  one shot
  StrawboatFile.read_selected    from a file: uploads only the touched runs

List<T> / LargeList<T> over a fixed-width leaf: the result is the dense List
array of the selected rows (offsets from 0, list validity, the rows' leaves
back to back, leaf validity).  The footer's num_values of a nested page is
its level count, so the selection is resolved against the page ROWS, each
page's first u32, fetched first:

  list_page_rows                 from a chunk in HBM    (sb_list_page_rows)
  StrawboatFile.page_rows        from the file, 4 bytes a page (sb_file_page_rows)
  ListColumnDecoder.select       sb_plan_selected_list_column + sb_decode_list_selected
  read_selected_list             one shot
  StrawboatFile.read_selected_list

The selected leaf count is known only after the decode: the plan reports the
touched pages' leaves as a bound (leaf_bound), outputs are allocated for
that, written_leaves() is read back.  Deeper chains, Struct / Map and Utf8 /
Boolean leaves under a list are out of scope: StrawboatError(E_NYI)."""
from __future__ import annotations

import ctypes
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .binary import BINARY, LARGE_BINARY, LARGE_UTF8, UTF8, BinaryOutC, _ow
from .read import PageMeta, _as_device_bytes, physical_type, refuse_wide, resolve_context

_BINARY_TYPES = (BINARY, LARGE_BINARY, UTF8, LARGE_UTF8)


def _error(st: int, msg: str) -> N.StrawboatError:
    """StrawboatError with .page = the failing page's index in the column (or None)."""
    e = N.StrawboatError(st, msg)
    m = re.search(r"\bpage (\d+)", msg)
    e.page = int(m.group(1)) if m else None
    return e


def normalize_ranges(ranges: Sequence[Tuple[int, int]], n_rows: int) -> List[Tuple[int, int]]:
    """Half-open row ranges -> sorted, disjoint, non-adjacent, non-empty ones
    (host only).  A range that starts below 0, ends before it starts or
    reaches past n_rows is an argument error."""
    rs = []
    for a, b in ranges:
        a, b = int(a), int(b)
        if a < 0 or b < a or b > n_rows:
            raise N.StrawboatError(N.E_ARG, f"row range [{a}, {b}) does not lie in [0, {n_rows})")
        if b > a:
            rs.append((a, b))
    rs.sort()
    out: List[Tuple[int, int]] = []
    for a, b in rs:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def page_runs(page_metas: Sequence[PageMeta], touched: Sequence[int]) -> List[Tuple[int, int, int, int]]:
    """The maximal runs of adjacent touched pages as (byte offset in the
    column chunk, byte length, first page, pages) -- host only.  `touched`
    holds page indices in ascending order."""
    starts = [0]
    for m in page_metas:
        starts.append(starts[-1] + m.length)
    runs: List[Tuple[int, int, int, int]] = []
    for p in touched:
        p = int(p)
        if not 0 <= p < len(page_metas) or (runs and p < runs[-1][2] + runs[-1][3]):
            raise N.StrawboatError(N.E_ARG, f"touched page {p}: not an ascending index into the column's pages")
        if runs and runs[-1][2] + runs[-1][3] == p:
            off, ln, first, n = runs[-1]
            runs[-1] = (off, ln + page_metas[p].length, first, n + 1)
        else:
            runs.append((starts[p], page_metas[p].length, p, 1))
    return runs


class ResolvedSelection:
    """A selection resolved against one column's pages (sb_select)."""

    def __init__(self, selection: "Selection", page_metas: Sequence[PageMeta], ctx):
        L = N.lib()
        self.selection = selection  # keeps the bitmap alive
        self.ctx = ctx
        self.metas = list(page_metas)
        metas = (N.PageMetaC * max(1, len(self.metas)))(*[N.PageMetaC(m.length, m.num_values) for m in self.metas])
        h = ctypes.c_void_p()
        st = L.sb_select_create(ctx._h, ctypes.c_void_p(selection.bitmap.data_ptr()), selection.n_rows, metas,
                                len(self.metas), ctypes.byref(h))
        if st:
            raise _error(st, ctx.error())
        self._h = h
        self.num_rows = int(L.sb_select_num_rows(h))
        self.pages: List[int] = []
        self.counts: List[int] = []
        pi, cnt = ctypes.c_uint64(), ctypes.c_uint64()
        for i in range(int(L.sb_select_num_pages(h))):
            L.sb_select_page(h, i, ctypes.byref(pi), ctypes.byref(cnt))
            self.pages.append(pi.value)
            self.counts.append(cnt.value)

    def runs(self):
        return page_runs(self.metas, self.pages)

    def close(self):
        if getattr(self, "_h", None):
            N.lib().sb_select_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Selection:
    """Rows wanted from a flat column, as a device bitmap (bit i = row i).

    mask: a torch bool tensor of n_rows entries (host or device), or a packed
    LSB-first uint8 bitmap tensor on the device (n_rows must be given);
    ranges: half-open (start, end) row ranges, merged and sorted on the host
    and expanded to the bitmap on the device."""

    def __init__(self, mask=None, ranges=None, n_rows: Optional[int] = None, device=None):
        import torch

        from .write import pack_bits

        if (mask is None) == (ranges is None):
            raise N.StrawboatError(N.E_ARG, "a selection takes a mask or ranges")
        if device is None:
            device = mask.device if mask is not None and mask.is_cuda else torch.cuda.current_device()
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.ranges = None
        if mask is not None and mask.dtype == torch.uint8:  # already packed
            if n_rows is None or not mask.is_cuda or mask.numel() * 8 < n_rows:
                raise N.StrawboatError(N.E_ARG, "a packed selection is a device uint8 bitmap of at least n_rows bits")
            self.n_rows = int(n_rows)
            bits = mask.contiguous()
        else:
            if mask is not None:
                if mask.dtype != torch.bool or (n_rows is not None and mask.numel() != n_rows):
                    raise N.StrawboatError(N.E_ARG, "a selection mask is a bool tensor of n_rows entries")
                self.n_rows = mask.numel()
                flat = mask.reshape(-1)
            else:
                if n_rows is None:
                    raise N.StrawboatError(N.E_ARG, "ranges need n_rows")
                self.n_rows = int(n_rows)
                self.ranges = normalize_ranges(ranges, self.n_rows)
                # +1 at each start, -1 at each end: disjoint ranges, so the running sum is 0 or 1
                delta = torch.zeros(self.n_rows + 1, dtype=torch.int32, device=dev)
                if self.ranges:
                    r = torch.tensor(self.ranges, dtype=torch.int64, device=dev)
                    delta[r[:, 0]] += 1
                    delta[r[:, 1]] -= 1
                flat = torch.cumsum(delta, 0, dtype=torch.int32)[: self.n_rows] > 0
            bits = pack_bits(flat, self.n_rows, dev)
        nbytes = 4 * max((self.n_rows + 31) // 32, 1)  # whole 32-bit words, as the kernels read them
        if bits.numel() < nbytes or bits.data_ptr() % 4:
            padded = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            padded[: min(bits.numel(), nbytes)] = bits[:nbytes]
            bits = padded
        self.bitmap = bits
        self.device = dev

    def resolve(self, page_metas: Sequence[PageMeta], ctx=None) -> ResolvedSelection:
        """Against a column's pages: .num_rows selected rows, .pages the
        touched page indices, .counts their selected rows."""
        return ResolvedSelection(self, page_metas, resolve_context(ctx, self.bitmap))


class _SelectedBase:
    def _plan(self, chunk, page_metas, phys: int, nullable: bool, selection, ctx, packed: bool):
        import torch

        self._torch = torch
        self.ctx = resolve_context(ctx, chunk)
        self.nullable = bool(nullable)
        self.phys = phys
        self.chunk = _as_device_bytes(chunk, self.ctx.device)
        self.resolved = selection if isinstance(selection, ResolvedSelection) else selection.resolve(page_metas, self.ctx)
        self.selection = self.resolved.selection
        L = N.lib()
        desc = N.ColumnDescC(phys, int(self.nullable))
        h = ctypes.c_void_p()
        st = L.sb_plan_selected_column(self.ctx._h, ctypes.byref(desc), self.resolved._h,
                                       ctypes.c_void_p(self.chunk.data_ptr()), self.chunk.numel(), int(bool(packed)),
                                       ctypes.byref(h))
        if st:
            raise _error(st, self.ctx.error())
        self._h = h
        self.num_rows = int(L.sb_plan_num_rows(h))
        self.num_pages = int(L.sb_plan_num_pages(h))

    def stats(self):
        """(pages decoded in place, pages compacted through scratch, scratch bytes)."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        st = N.lib().sb_plan_selected_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        if st:
            raise _error(st, "not a selective plan")
        return a.value, b.value, c.value

    def check(self):
        bad = ctypes.c_int64(-1)
        st = N.lib().sb_plan_status(self.ctx._h, self._h, ctypes.byref(bad))
        if st:
            e = _error(st, self.ctx.error())
            if bad.value >= 0:
                e.page = bad.value
            raise e

    def close(self):
        if getattr(self, "_h", None):
            N.lib().sb_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SelectedColumnDecoder(_SelectedBase):
    """ColumnDecoder.select: the selected rows of a fixed-width or Boolean column."""

    def __init__(self, chunk, page_metas, dtype, nullable: bool, selection, ctx=None, packed: bool = False):
        self.dtype = np.dtype(dtype)
        refuse_wide(self.dtype, "selective read")
        self._plan(chunk, page_metas, physical_type(self.dtype), nullable, selection, ctx, packed)

    def alloc_outputs(self):
        torch = self._torch
        dev = f"cuda:{self.ctx.device}"
        nbytes = max((self.num_rows + 31) // 32, 1) * 4
        if self.dtype == np.bool_:
            values = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        else:
            tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.dtype.itemsize]
            values = torch.empty(max(self.num_rows, 1), dtype=tdt, device=dev)
        validity = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if self.nullable else None
        return values, validity

    def decode_async(self, values=None, validity=None):
        if values is None:
            values, validity = self.alloc_outputs()
        out = N.PrimitiveOutC(values.data_ptr(), validity.data_ptr() if validity is not None else None)
        st = N.lib().sb_decode_selected(self.ctx._h, self._h, ctypes.byref(out))
        if st:
            raise _error(st, self.ctx.error())
        return values, validity

    def decode(self, values=None, validity=None):
        """(values[:num_rows], validity bitmap | None)."""
        v, m = self.decode_async(values, validity)
        self.check()
        return (v if self.dtype == np.bool_ else v[: self.num_rows]), m


class SelectedBinaryDecoder(_SelectedBase):
    """BinaryColumnDecoder.select: the selected rows of a Binary / Utf8 column."""

    def __init__(self, chunk, page_metas, physical_type: int = UTF8, nullable: bool = False, selection=None, ctx=None,
                 packed: bool = False):
        if physical_type not in _BINARY_TYPES:
            raise N.StrawboatError(N.E_ARG, f"physical type {physical_type} is not Binary / Utf8")
        self._plan(chunk, page_metas, physical_type, nullable, selection, ctx, packed)
        self.values_bytes = int(N.lib().sb_plan_values_bytes(self._h))  # the touched pages': the capacity bound

    def alloc_outputs(self):
        torch = self._torch
        dev = f"cuda:{self.ctx.device}"
        odt = torch.int64 if _ow(self.phys) == 8 else torch.int32
        offsets = torch.zeros(self.num_rows + 1, dtype=odt, device=dev)
        values = torch.empty(max(self.values_bytes, 16), dtype=torch.uint8, device=dev)
        validity = None
        if self.nullable:
            validity = torch.zeros(max((self.num_rows + 31) // 32, 1) * 4, dtype=torch.uint8, device=dev)
        return offsets, values, validity

    def decode_async(self, offsets=None, values=None, validity=None):
        if offsets is None:
            offsets, values, validity = self.alloc_outputs()
        out = BinaryOutC(offsets.data_ptr(), values.data_ptr(), values.numel(),
                         validity.data_ptr() if validity is not None else None)
        st = N.lib().sb_decode_binary_selected(self.ctx._h, self._h, ctypes.byref(out))
        if st:
            raise _error(st, self.ctx.error())
        return offsets, values, validity

    def written_bytes(self) -> int:
        """Values bytes the last decode wrote (waits for it)."""
        n = ctypes.c_uint64()
        st = N.lib().sb_plan_selected_values_bytes(self.ctx._h, self._h, ctypes.byref(n))
        if st:
            raise _error(st, self.ctx.error())
        return n.value

    def decode(self, *outs):
        """(offsets, values narrowed to the bytes written, validity bitmap | None)."""
        o, v, m = self.decode_async(*outs)
        self.check()
        return o[: self.num_rows + 1], v[: self.written_bytes()], m


def list_page_rows(chunk, page_metas: Sequence[PageMeta], ctx=None) -> List[int]:
    """The top-level rows of every page of a nested column chunk in HBM (each
    page's first u32: sb_list_page_rows, one small kernel and one readback).
    The footer's num_values of such a page is its level count."""
    ctx = resolve_context(ctx, chunk)
    buf = _as_device_bytes(chunk, ctx.device)
    n = len(page_metas)
    metas = (N.PageMetaC * max(1, n))(*[N.PageMetaC(m.length, m.num_values) for m in page_metas])
    rows = (ctypes.c_uint64 * max(1, n))()
    st = N.lib().sb_list_page_rows(ctx._h, ctypes.c_void_p(buf.data_ptr()), buf.numel(), metas, n, rows)
    if st:
        raise _error(st, ctx.error())
    return [int(rows[i]) for i in range(n)]


class SelectedListDecoder(_SelectedBase):
    """ListColumnDecoder.select: the selected top-level rows of a List<T> /
    LargeList<T> column over a fixed-width leaf, as a dense List array.

    num_rows: the selected rows; num_pages: the touched pages; leaf_bound:
    the touched pages' leaves, which bounds the selected leaves (only the
    decode learns their count: written_leaves()).  Outputs are allocated for
    leaf_bound leaves."""

    def __init__(self, chunk, page_metas, dtype, list_nullable: bool, item_nullable: bool, selection, ctx=None,
                 large: bool = False, packed: bool = False):
        import torch

        from .nested import ListDescC, _lib as _list_lib

        self._torch = torch
        self.ctx = resolve_context(ctx, chunk)
        phys = int(dtype) if isinstance(dtype, (int, np.integer)) else physical_type(np.dtype(dtype))
        self.phys = phys
        self.dtype = None if isinstance(dtype, (int, np.integer)) else np.dtype(dtype)
        self.list_nullable, self.item_nullable = bool(list_nullable), bool(item_nullable)
        self.offset_width = 8 if large else 4
        self.chunk = _as_device_bytes(chunk, self.ctx.device)
        self.metas = list(page_metas)
        if isinstance(selection, ResolvedSelection):
            self.resolved, self._own_resolved = selection, False
        else:
            if packed:
                raise N.StrawboatError(N.E_ARG, "a packed chunk holds only the touched pages: resolve the selection "
                                                "against the page rows first (PageMeta(length, rows))")
            rows = list_page_rows(self.chunk, self.metas, self.ctx)
            self.resolved = selection.resolve([PageMeta(m.length, r) for m, r in zip(self.metas, rows)], self.ctx)
            self._own_resolved = True
        self.selection = self.resolved.selection
        L = _list_lib()
        metas = (N.PageMetaC * max(1, len(self.metas)))(*[N.PageMetaC(m.length, m.num_values) for m in self.metas])
        desc = ListDescC(phys, int(self.list_nullable), int(self.item_nullable), self.offset_width)
        h = ctypes.c_void_p()
        st = L.sb_plan_selected_list_column(self.ctx._h, ctypes.byref(desc), self.resolved._h, metas, len(self.metas),
                                            ctypes.c_void_p(self.chunk.data_ptr()), self.chunk.numel(),
                                            int(bool(packed)), ctypes.byref(h))
        if st:
            if self._own_resolved:
                self.resolved.close()
            raise _error(st, self.ctx.error())
        self._h = h
        self.num_rows = int(L.sb_plan_num_rows(h))
        self.num_pages = int(L.sb_plan_num_pages(h))
        self.leaf_bound = int(L.sb_plan_num_leaves(h))

    def alloc_outputs(self):
        torch = self._torch
        dev = f"cuda:{self.ctx.device}"
        odt = torch.int64 if self.offset_width == 8 else torch.int32
        offsets = torch.zeros(self.num_rows + 1, dtype=odt, device=dev)
        tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.dtype.itemsize]
        values = torch.empty(max(self.leaf_bound, 1), dtype=tdt, device=dev)
        bm = lambda n: torch.zeros(max((n + 31) // 32, 1) * 4, dtype=torch.uint8, device=dev)  # noqa: E731
        lv = bm(self.num_rows) if self.list_nullable else None
        fv = bm(self.leaf_bound) if self.item_nullable else None
        return offsets, lv, values, fv

    def decode_async(self, offsets=None, list_validity=None, values=None, leaf_validity=None):
        from .nested import ListOutC

        if offsets is None:
            offsets, list_validity, values, leaf_validity = self.alloc_outputs()
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        out = ListOutC(p(offsets), p(list_validity), p(values), p(leaf_validity))
        st = N.lib().sb_decode_list_selected(self.ctx._h, self._h, ctypes.byref(out))
        if st:
            raise _error(st, self.ctx.error())
        return offsets, list_validity, values, leaf_validity

    def written_leaves(self) -> int:
        """Leaves the last decode wrote (waits for it)."""
        n = ctypes.c_uint64()
        st = N.lib().sb_plan_selected_leaves(self.ctx._h, self._h, ctypes.byref(n))
        if st:
            raise _error(st, self.ctx.error())
        return n.value

    def decode(self, *outs):
        """(offsets[:num_rows + 1], list validity | None, values narrowed to
        the leaves written, leaf validity | None)."""
        o, lv, v, fv = self.decode_async(*outs)
        self.check()
        return o[: self.num_rows + 1], lv, v[: self.written_leaves()], fv

    def close(self):
        super().close()
        if getattr(self, "_own_resolved", False):
            self.resolved.close()
            self._own_resolved = False


def read_selected_list(chunk, page_metas: Sequence[PageMeta], dtype, list_nullable: bool, item_nullable: bool,
                       selection, ctx=None, large: bool = False, packed: bool = False):
    """One shot: the selected rows of a List<T> column chunk ->
    (offsets, list validity | None, values, leaf validity | None)."""
    dec = SelectedListDecoder(chunk, page_metas, dtype, list_nullable, item_nullable, selection, ctx, large, packed)
    try:
        return dec.decode()
    finally:
        dec.close()


def read_selected(chunk, page_metas: Sequence[PageMeta], dtype_or_physical_type, nullable: bool, selection,
                  ctx=None, packed: bool = False):
    """One shot: the selected rows of a flat column chunk.  A numpy dtype
    gives (values, validity); a Binary / Utf8 physical type (pa_amd.UTF8 ...)
    gives (offsets, values, validity)."""
    if isinstance(dtype_or_physical_type, int) and dtype_or_physical_type in _BINARY_TYPES:
        dec = SelectedBinaryDecoder(chunk, page_metas, dtype_or_physical_type, nullable, selection, ctx, packed)
    else:
        dec = SelectedColumnDecoder(chunk, page_metas, dtype_or_physical_type, nullable, selection, ctx, packed)
    try:
        return dec.decode()
    finally:
        dec.close()


def file_read_selected(f, col: int, selection: Selection, ctx=None):
    """StrawboatFile.read_selected: resolve against the footer's metas,
    upload only the runs of touched pages into one packed buffer
    (sb_file_upload, one call per run), decode with packed = 1."""
    import torch

    from .file import _DTYPE

    if not 0 <= col < f.num_columns or len(f.leaves) != f.num_columns:
        raise N.StrawboatError(N.E_ARG, f"column {col} out of range")
    leaf = f.leaves[col]
    if leaf.depth:
        raise N.StrawboatError(N.E_NYI, f"leaf {leaf.name}: row selection of a nested leaf is not implemented")
    if leaf.flags or not leaf.physical_type:
        raise N.StrawboatError(N.E_NYI, f"leaf {leaf.name}: {leaf.arrow_type} has no page path here")
    ctx = resolve_context(ctx, selection.bitmap)
    cm = f.columns[col]
    res = selection.resolve(cm.pages, ctx)
    try:
        runs = res.runs()
        total = sum(r[1] for r in runs)
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device=f"cuda:{ctx.device}")
        pos = 0
        for off, ln, _, _ in runs:
            f._check(N.lib().sb_file_upload(ctx._h, f._h, cm.offset + off, ln, ctypes.c_void_p(buf.data_ptr() + pos)))
            pos += ln
        f.last_uploaded_bytes = total
        pt = leaf.physical_type
        what = pt if pt in _BINARY_TYPES else _DTYPE[pt]
        return read_selected(buf[:max(total, 1)], cm.pages, what, leaf.nullable, res, ctx, packed=True)
    finally:
        res.close()


def file_read_selected_list(f, col: int, selection: Selection, ctx=None):
    """StrawboatFile.read_selected_list: the page rows come from the file
    (page_rows: one 4-byte read per page), the selection is resolved against
    them, only the runs of touched pages are uploaded and decoded with
    packed = 1."""
    import torch

    from .file import _DTYPE

    if not 0 <= col < f.num_columns or len(f.leaves) != f.num_columns:
        raise N.StrawboatError(N.E_ARG, f"column {col} out of range")
    leaf = f.leaves[col]
    if leaf.depth != 1 or leaf.flags or leaf.struct_mask or leaf.map_mask or leaf.physical_type not in _DTYPE \
            or _DTYPE[leaf.physical_type] == np.bool_:
        raise N.StrawboatError(N.E_NYI, f"leaf {leaf.name}: row selection takes one List / LargeList nest over a "
                                        f"fixed-width leaf")
    ctx = resolve_context(ctx, selection.bitmap)
    cm = f.columns[col]
    rows = f.page_rows(col)
    res = selection.resolve([PageMeta(m.length, r) for m, r in zip(cm.pages, rows)], ctx)
    try:
        runs = res.runs()
        total = sum(r[1] for r in runs)
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device=f"cuda:{ctx.device}")
        pos = 0
        for off, ln, _, _ in runs:
            f._check(N.lib().sb_file_upload(ctx._h, f._h, cm.offset + off, ln, ctypes.c_void_p(buf.data_ptr() + pos)))
            pos += ln
        f.last_uploaded_bytes = total
        return read_selected_list(buf[:max(total, 1)], cm.pages, _DTYPE[leaf.physical_type], leaf.list_nullable[0],
                                  leaf.nullable, res, ctx, large=leaf.large_list[0], packed=True)
    finally:
        res.close()
