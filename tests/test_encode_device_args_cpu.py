"""The four device encode entry points' argument checks: the status for each
kind of bad argument, and which check wins when two apply.  Every case
returns before the context or any device pointer is read, so the context
and the buffers are stand-in non-NULL addresses and no GPU is needed."""
import ctypes

import pa_amd
from pa_amd import _native as N
from pa_amd import binary as B
from pa_amd import nested as NS

_buf = ctypes.create_string_buffer(64)
PTR = ctypes.addressof(_buf)  # a non-NULL pointer the entry points never follow in these cases
BIG = 40000  # rows of one page past the 16384 a List / nested page may hold


def _tail(metas_cap):
    olen, npg = ctypes.c_uint64(777), ctypes.c_uint64(777)
    metas = (N.PageMetaC * max(metas_cap, 1))()
    return olen, npg, (PTR, 1 << 20, ctypes.byref(olen), metas, metas_cap, ctypes.byref(npg))


def _flat(phys=N.INT32, valid=PTR, n=10, nullable=1, values=PTR, page=3, metas_cap=8):
    olen, npg, tail = _tail(metas_cap)
    opts = pa_amd.WriteOptions().c()
    st = N.lib().sb_encode_column_device(PTR, phys, values, valid, n, nullable, ctypes.byref(opts), page, *tail)
    return st, npg.value, olen.value


def _list(phys=N.INT32, offs=PTR, lvalid=PTR, cvalid=PTR, n=10, page=3, metas_cap=8):
    olen, npg, tail = _tail(metas_cap)
    opts = pa_amd.WriteOptions().c()
    st = N.lib().sb_encode_list_column_device(PTR, phys, offs, lvalid, 1, PTR, cvalid, 1, n, ctypes.byref(opts), page,
                                              *tail)
    return st, npg.value, olen.value


def _binary(offs=PTR, valid=PTR, n=10, page=3, metas_cap=8):
    olen, npg, tail = _tail(metas_cap)
    opts = pa_amd.WriteOptions().c()
    st = B._lib().sb_encode_binary_column_device(PTR, B.UTF8, PTR, 100, offs, valid, n, 1, ctypes.byref(opts), page,
                                                 *tail)
    return st, npg.value, olen.value


def _nested(phys=N.INT32, depth=1, offs=PTR, nvalid=PTR, lvalid=PTR, leaf_offs=None, n=10, page=3, metas_cap=8):
    olen, npg, tail = _tail(metas_cap)
    opts = pa_amd.WriteOptions().c()
    desc = NS.NestedDescC(phys, depth, (ctypes.c_int32 * NS.MAX_NEST)(1, 0, 0, 0), 1, 4, 0)
    nests = (NS.NestDevC * NS.MAX_NEST)()
    nests[0].d_offsets, nests[0].d_validity = offs, nvalid
    st = NS._encode_device_lib().sb_encode_nested_column_device(PTR, ctypes.byref(desc), nests, PTR, leaf_offs, 100,
                                                                lvalid, n, ctypes.byref(opts), page, *tail)
    return st, npg.value, olen.value


def test_flat_column_argument_checks():
    for phys in (99, B.UTF8):  # an unsupported type is an argument error here
        assert _flat(phys=phys)[0] == N.E_ARG
    assert _flat(valid=None)[0] == N.E_ARG
    assert _flat(values=None)[0] == N.E_ARG
    assert _flat(metas_cap=2) == (N.E_ARG, 4, 777)  # the pages are reported, the length is left alone
    assert _flat(n=0) == (0, 0, 0)
    assert _flat(phys=N.BOOLEAN, n=0) == (0, 0, 0)


def test_list_column_argument_checks():
    for phys in (99, B.UTF8, N.BOOLEAN):  # not yet implemented, reported before the bitmaps are looked at
        assert _list(phys=phys, lvalid=None)[0] == N.E_NYI
    assert _list(phys=99, offs=None)[0] == N.E_ARG  # (the offsets come first)
    assert _list(lvalid=None)[0] == N.E_ARG
    assert _list(cvalid=None)[0] == N.E_ARG
    assert _list(metas_cap=2) == (N.E_ARG, 4, 777)
    assert _list(n=BIG, page=0) == (N.E_NYI, 1, 0)
    assert _list(n=BIG, page=0, metas_cap=0) == (N.E_ARG, 1, 777)  # (the room for the metas comes first)
    assert _list(n=0) == (0, 0, 0)


def test_binary_column_argument_checks():
    assert _binary(offs=None)[0] == N.E_ARG
    assert _binary(valid=None)[0] == N.E_ARG
    assert _binary(metas_cap=2)[:2] == (N.E_ARG, 4)
    assert _binary(n=0, offs=None) == (0, 0, 0)


def test_nested_column_argument_checks():
    for depth in (0, NS.MAX_NEST + 1):
        assert _nested(depth=depth)[0] == N.E_NYI
    assert _nested(phys=99, offs=None)[0] == N.E_NYI  # (the type comes before the nests' pointers)
    assert _nested(offs=None)[0] == N.E_ARG
    assert _nested(nvalid=None)[0] == N.E_ARG
    assert _nested(lvalid=None)[0] == N.E_ARG
    assert _nested(phys=B.UTF8)[0] == N.E_ARG  # a Binary / Utf8 leaf without its offsets
    assert _nested(metas_cap=2) == (N.E_ARG, 4, 777)
    assert _nested(n=BIG, page=0) == (N.E_NYI, 1, 0)
    assert _nested(phys=N.BOOLEAN, n=0) == (0, 0, 0)
    assert _nested(phys=B.UTF8, leaf_offs=PTR, n=0) == (0, 0, 0)
