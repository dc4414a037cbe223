"""Selective reads, host side: the page runs a file read uploads, the range
normalisation of a Selection, and the argument checks of every new ABI call.
Each ABI case returns before the context or any other pointer is followed,
so they are stand-in non-NULL addresses and no GPU is needed."""
import ctypes

import pytest

import pa_amd
from pa_amd import PageMeta
from pa_amd import _native as N
from pa_amd.binary import BinaryOutC

_buf = ctypes.create_string_buffer(256)
PTR = ctypes.addressof(_buf)  # a non-NULL pointer the entry points never follow in these cases

METAS = [PageMeta(10, 1), PageMeta(20, 2), PageMeta(30, 3), PageMeta(5, 1), PageMeta(7, 4)]


def test_page_runs():
    assert pa_amd.page_runs(METAS, []) == []
    assert pa_amd.page_runs([], []) == []
    assert pa_amd.page_runs(METAS, range(5)) == [(0, 72, 0, 5)]
    assert pa_amd.page_runs(METAS, [0, 2, 4]) == [(0, 10, 0, 1), (30, 30, 2, 1), (65, 7, 4, 1)]
    assert pa_amd.page_runs(METAS, [1, 3]) == [(10, 20, 1, 1), (60, 5, 3, 1)]
    assert pa_amd.page_runs(METAS, [0, 1]) == [(0, 30, 0, 2)]  # a run at the front
    assert pa_amd.page_runs(METAS, [3, 4]) == [(60, 12, 3, 2)]  # a run at the back
    assert pa_amd.page_runs(METAS, [0, 1, 3, 4]) == [(0, 30, 0, 2), (60, 12, 3, 2)]
    for bad in ([5], [-1], [2, 1], [1, 1]):
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.page_runs(METAS, bad)
        assert e.value.status == N.E_ARG


def test_range_normalisation():
    norm = pa_amd.normalize_ranges
    assert norm([], 10) == []
    assert norm([(0, 10)], 10) == [(0, 10)]
    assert norm([(2, 6), (4, 8)], 10) == [(2, 8)]  # overlapping
    assert norm([(2, 4), (4, 8)], 10) == [(2, 8)]  # adjacent
    assert norm([(2, 8), (3, 4)], 10) == [(2, 8)]  # nested
    assert norm([(3, 3), (0, 0), (10, 10)], 10) == []  # empty
    assert norm([(7, 9), (5, 5), (0, 2), (4, 5)], 10) == [(0, 2), (4, 5), (7, 9)]  # unordered
    assert norm([(7, 9), (0, 2), (1, 8)], 10) == [(0, 9)]
    for bad in ([(0, 11)], [(11, 12)], [(-1, 2)], [(5, 3)]):
        with pytest.raises(pa_amd.StrawboatError) as e:
            norm(bad, 10)
        assert e.value.status == N.E_ARG


def test_select_argument_checks():
    L = N.lib()
    metas = (N.PageMetaC * 1)(N.PageMetaC(10, 10))
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert L.sb_select_create(None, PTR, 10, metas, 1, out) == N.E_ARG
    assert L.sb_select_create(PTR, None, 10, metas, 1, out) == N.E_ARG
    assert L.sb_select_create(PTR, PTR, 10, None, 1, out) == N.E_ARG
    assert L.sb_select_create(PTR, PTR, 10, metas, 1, None) == N.E_ARG
    assert h.value is None
    assert L.sb_select_num_rows(None) == 0 and L.sb_select_num_pages(None) == 0
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.sb_select_page(None, 0, ctypes.byref(a), ctypes.byref(b)) == N.E_ARG
    L.sb_select_destroy(None)


def test_selected_plan_argument_checks():
    L = N.lib()
    desc = N.ColumnDescC(N.INT32, 1)
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert L.sb_plan_selected_column(None, ctypes.byref(desc), PTR, PTR, 64, 0, out) == N.E_ARG
    assert L.sb_plan_selected_column(PTR, None, PTR, PTR, 64, 0, out) == N.E_ARG
    assert L.sb_plan_selected_column(PTR, ctypes.byref(desc), None, PTR, 64, 0, out) == N.E_ARG
    assert L.sb_plan_selected_column(PTR, ctypes.byref(desc), PTR, PTR, 64, 1, None) == N.E_ARG
    assert h.value is None
    po = N.PrimitiveOutC(PTR, PTR)
    assert L.sb_decode_selected(None, PTR, ctypes.byref(po)) == N.E_ARG
    assert L.sb_decode_selected(PTR, None, ctypes.byref(po)) == N.E_ARG
    assert L.sb_decode_selected(PTR, PTR, None) == N.E_ARG
    bo = BinaryOutC(PTR, PTR, 64, PTR)
    assert L.sb_decode_binary_selected(None, PTR, ctypes.byref(bo)) == N.E_ARG
    assert L.sb_decode_binary_selected(PTR, None, ctypes.byref(bo)) == N.E_ARG
    assert L.sb_decode_binary_selected(PTR, PTR, None) == N.E_ARG
    n = ctypes.c_uint64(777)
    assert L.sb_plan_selected_values_bytes(None, PTR, ctypes.byref(n)) == N.E_ARG
    assert L.sb_plan_selected_values_bytes(PTR, None, ctypes.byref(n)) == N.E_ARG
    assert L.sb_plan_selected_values_bytes(PTR, PTR, None) == N.E_ARG
    assert L.sb_plan_selected_stats(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == N.E_ARG
    assert n.value == 777
