"""The host nested writers on legal Arrow arrays outside the normal form of
nestgen.gen (a null list slot empty, children of a null struct slot null,
every offsets buffer from 0):

  refused   a dead list / map slot -- null itself, or under a null slot of
            the run of structs directly above -- that is not empty: SB_E_ARG
            before a page is written (it would emit one level, while the leaf
            slice taken through the offsets keeps its children's values);
  accepted  valid children and valid empty lists under a null struct slot,
            offsets that start above 0 (lists, maps and Binary leaves),
            children longer than the offsets reach, nullable nests without a
            validity: each reads back as its logical value;
  lengths   encode_field checks every buffer against its slot count before C
            reads it.

The reference is the logical Arrow value (nestgen.logical, pinned against
pyarrow's to_pylist() here), not another writer of ours.  The device writer on
the same arrays: tests/test_gpu_nested_loose.py."""
import ctypes

import numpy as np
import pytest

import pa_amd
from oracle import nest as NE
from oracle.nest import A
from tests import nestgen
from tests import test_nested_write_cpu as W

STEPS = (0, 7, 33)
ROWS = nestgen.DEAD_ROWS
E_ARG = 6


def metas_of(pm):
    return [(m.length, m.num_values) for m in pm]


def read_back(f, cols):
    return NE.read_field(f, [(c, metas_of(pm)) for c, pm in cols])


def status_of(call):
    with pytest.raises(pa_amd.StrawboatError) as e:
        call()
    return e.value.status


# ---- the reference itself -------------------------------------------------------
def accepted_arrays():
    """(name, field, array) of every accepted generator: the loose slices and
    the twins of the refusal cases."""
    for name in nestgen.loose_shapes():
        yield (name,) + nestgen.loose_array(name)
    for name in nestgen.dead_fields():
        for row in ROWS:
            f, _, twin = nestgen.dead_case(name, row)
            yield f"{name}@{row}", f, twin


def test_logical_is_pyarrows_value():
    """logical() against pyarrow: the loose slices, and the refused arrays
    (whose dead children no reader may show) with their twins."""
    pytest.importorskip("pyarrow")
    for name, f, a in accepted_arrays():
        assert nestgen.to_pa(f, a).to_pylist() == nestgen.to_pa(f, nestgen.logical(f, a)).to_pylist(), name
    for name in nestgen.dead_fields():
        for row in ROWS:
            f, bad, twin = nestgen.dead_case(name, row)
            assert nestgen.to_pa(f, bad).to_pylist() == nestgen.to_pa(f, nestgen.logical(f, twin)).to_pylist(), (name, row)


def test_oracle_alone_reproduces_logical():
    for name, f, a in accepted_arrays():
        for step in (0, 16):
            NE.equal(f, NE.read_field(f, NE.write_field(f, a, step)), nestgen.logical(f, a), values_under_nulls=False,
                     path=name)


# ---- 1. refusals ------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("case", list(nestgen.dead_fields()))
def test_dead_slot_with_children_is_refused(case, row):
    f, bad, twin = nestgen.dead_case(case, row)
    pf = nestgen.pa_amd_field(f)
    opts = pa_amd.WriteOptions(max_page_size=16, seed=W.SEED)
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field(pf, nestgen.host_array(bad), opts)
    assert e.value.status == E_ARG and "not empty" in str(e.value)
    # the twin: the same array with that one range empty
    got, exp = W.write_both(f, twin, "none", 16)
    W.check_same(f, got, exp)
    NE.equal(f, read_back(f, got), nestgen.logical(f, twin), values_under_nulls=False)
    if case == "top_list":
        ch = bad.children[0]
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.encode_list_column(bad.offsets, ch.values, bad.validity, ch.validity, True, True, opts)
        assert e.value.status == E_ARG and "not empty" in str(e.value)
        ch = twin.children[0]
        assert pa_amd.encode_list_column(twin.offsets, ch.values, twin.validity, ch.validity, True, True, opts) == got[0]


def test_the_smallest_dead_slot():
    """List<Int32> [None (offsets 0..2), [3]]: three leaf values for one leaf slot."""
    f = nestgen.lst(nestgen.leaf("i32", True, "item"), True)
    a = A("list", 2, np.array([False, True]), offsets=np.array([0, 2, 3], np.int64),
          children=[A("leaf", 3, np.ones(3, bool), values=np.array([1, 2, 3], np.int32))])
    assert status_of(lambda: pa_amd.encode_field(nestgen.pa_amd_field(f), nestgen.host_array(a))) == E_ARG
    lg = nestgen.logical(f, a)
    assert lg.offsets.tolist() == [0, 0, 1] and lg.children[0].values.tolist() == [3]


# ---- 2. accepted loose arrays -------------------------------------------------------
@pytest.mark.parametrize("codec", ["none", "lz4"])
@pytest.mark.parametrize("shape", list(nestgen.loose_shapes()))
def test_loose_arrays_byte_identical_and_logical(shape, codec):
    f, a = nestgen.loose_array(shape)
    lg = nestgen.logical(f, a)
    if shape == "list_bool":  # page 0's Boolean leaf slice starts inside a byte
        assert a.offsets[0] % 8 != 0
    for step in STEPS:
        got, exp = W.write_both(f, a, codec, step)
        W.check_same(f, got, exp)
        NE.equal(f, read_back(f, got), lg, values_under_nulls=False, path=f"{shape}/{step}")


def test_nullable_nests_without_a_validity():
    """A nullable nest whose array carries no validity reads all valid."""
    f, a = nestgen.loose_array("list_null_struct_list", 120)

    def strip(x):
        return A(x.kind, x.length, None, x.offsets, [strip(c) for c in x.children], x.values)

    a = strip(a)
    got, exp = W.write_both(f, a, "none", 33)
    W.check_same(f, got, exp)
    NE.equal(f, read_back(f, got), nestgen.logical(f, a), values_under_nulls=False)


# ---- 3. length checks ---------------------------------------------------------------
def _ints(n, valid=True):
    return A("leaf", n, np.ones(n, bool) if valid else None, values=np.arange(n, dtype=np.int32))


def _strs(n):
    return A("leaf", n, np.ones(n, bool), values=(np.arange(n + 1, dtype=np.int64), b"x" * n))


def length_cases():
    i32, utf8 = nestgen.leaf("i32", True, "item"), nestgen.leaf("utf8", True, "item")
    lst_i, lst_s = nestgen.lst(i32, True), nestgen.lst(utf8, True)
    st = nestgen.struct([nestgen.leaf("i32", True, "x"), nestgen.leaf("i32", True, "y")], True)
    offs = np.arange(9, dtype=np.int64)  # 8 rows of one item
    ok = np.ones(8, bool)
    short_strs, past_strs = _strs(8), _strs(8)
    short_strs.values = (short_strs.values[0][:8], short_strs.values[1])
    past_strs.values = (past_strs.values[0], b"x" * 7)
    short_leaf_valid = _ints(8)
    short_leaf_valid.validity = np.ones(7, bool)
    short_values = _ints(8)
    short_values.values = short_values.values[:7]
    return {
        "offsets_short": (lst_i, A("list", 8, ok, offsets=offs[:8], children=[_ints(8)])),
        "offsets_past_child": (lst_i, A("list", 8, ok, offsets=offs, children=[_ints(7)])),
        "struct_child_length": (st, A("struct", 8, ok, children=[_ints(8), _ints(7)])),
        "leaf_values_short": (lst_i, A("list", 8, ok, offsets=offs, children=[short_values])),
        "nest_bitmap_short": (lst_i, A("list", 8, ok[:7], offsets=offs, children=[_ints(8)])),
        "leaf_bitmap_short": (lst_i, A("list", 8, ok, offsets=offs, children=[short_leaf_valid])),
        "binary_offsets_short": (lst_s, A("list", 8, ok, offsets=offs, children=[short_strs])),
        "binary_offsets_past_bytes": (lst_s, A("list", 8, ok, offsets=offs, children=[past_strs])),
    }


@pytest.mark.parametrize("case", list(length_cases()))
def test_short_buffers_are_refused(case):
    f, a = length_cases()[case]
    assert status_of(lambda: pa_amd.encode_field(nestgen.pa_amd_field(f), nestgen.host_array(a))) == E_ARG


def test_length_cases_are_one_edit_from_a_good_array():
    f = nestgen.lst(nestgen.leaf("i32", True, "item"), True)
    a = A("list", 8, np.ones(8, bool), offsets=np.arange(9, dtype=np.int64), children=[_ints(8)])
    NE.equal(f, read_back(f, pa_amd.encode_field(nestgen.pa_amd_field(f), nestgen.host_array(a))), a)


def test_negative_first_offset_of_an_empty_column_is_refused():
    """sb_encode_nested_column with n_rows = 0 reads offsets[0] as the
    child's entry count: a negative one is refused."""
    from pa_amd import _native as N
    from pa_amd import nested as NS

    L = NS._encode_lib()
    opts = pa_amd.WriteOptions().c()
    vals = np.zeros(4, np.int32)
    for first, want in ((-1, E_ARG), (0, 0)):
        offs = np.array([first], np.int64)
        nests = (NS.NestInC * NS.MAX_NEST)()
        nests[0].h_offsets = offs.ctypes.data
        desc = NS.NestedDescC(N.INT32, 1, (ctypes.c_int32 * NS.MAX_NEST)(0, 0, 0, 0), 0, 4, 0)
        out = ctypes.POINTER(ctypes.c_uint8)()
        metas = ctypes.POINTER(N.PageMetaC)()
        olen, npg = ctypes.c_uint64(), ctypes.c_uint64()
        st = L.sb_encode_nested_column(ctypes.byref(desc), nests, vals.ctypes.data_as(ctypes.c_void_p), None, 0, None, 0,
                                       ctypes.byref(opts), 0, 1, ctypes.byref(out), ctypes.byref(olen),
                                       ctypes.byref(metas), ctypes.byref(npg))
        assert st == want, first
        if st == 0:
            assert npg.value == 0 and olen.value == 0
            L.sb_free(metas)
            L.sb_free(out)
