"""The device writer for nested fields, the parts that need no GPU: the two
C symbols, the NULL-context refusal, sb_encode_nested_device_bound against
the host writer's chunk for every leaf of the reference's integration shapes
and of nestgen.shapes(), and the binding's buffer-length checks."""
import ctypes

import numpy as np
import pytest

import pa_amd
from pa_amd import _native as N
from pa_amd import nested as NS
from tests import nestgen

CODECS = {"none": 0, "lz4": 1, "zstd": 2, "snappy": 3}
STEPS = (1, 33, 0)


def test_symbols_exported():
    L = N.lib()
    for name in ("sb_encode_nested_device_bound", "sb_encode_nested_column_device"):
        assert name in N.EXPORTED
        assert getattr(L, name) is not None


def test_null_context_is_an_argument_error():
    L = NS._encode_device_lib()
    ln = (ctypes.c_int32 * NS.MAX_NEST)(1, 0, 0, 0)
    desc = NS.NestedDescC(N.INT32, 1, ln, 1, 4, 0)
    nests = (NS.NestDevC * NS.MAX_NEST)()
    opts = pa_amd.WriteOptions().c()
    olen, npg = ctypes.c_uint64(), ctypes.c_uint64()
    metas = (N.PageMetaC * 1)()
    st = L.sb_encode_nested_column_device(None, ctypes.byref(desc), nests, None, None, 0, None, 10, ctypes.byref(opts),
                                          0, None, 0, ctypes.byref(olen), metas, 1, ctypes.byref(npg))
    assert st == N.E_ARG


def _fields():
    out = []
    for name, (f, a) in nestgen.io_rs_cases(np.random.default_rng(77)).items():
        out.append((name, f, a))
    for k, (name, f) in enumerate(nestgen.shapes().items()):
        out.append((name, f, nestgen.gen(f, 600, np.random.default_rng(900 + k))))
    return out


FIELDS = _fields()


@pytest.mark.parametrize("name", [x[0] for x in FIELDS])
def test_bound_covers_the_host_chunk(name):
    f, a = next((f, a) for n, f, a in FIELDS if n == name)
    pf, ha = nestgen.pa_amd_field(f), nestgen.host_array(a)
    for codec in CODECS.values():
        for step in STEPS:
            opts = pa_amd.WriteOptions(default_compression=codec, default_compress_ratio=2.0,
                                       max_page_size=step or None, seed=5)
            cols = pa_amd.encode_field(pf, ha, opts)
            for path, (chunk, metas) in zip(pf.leaf_paths(), cols):
                nulls, mask, leaf_null, large = NS.init_chain(path)
                arrs = NS._arrays_on_path(ha, path)
                ln = (ctypes.c_int32 * NS.MAX_NEST)(*([int(x) for x in nulls] + [0] * (NS.MAX_NEST - len(nulls))))
                desc = NS.NestedDescC(path[-1].physical_type, len(nulls), ln, int(leaf_null), 8 if large else 4, mask)
                la = arrs[-1]
                vlen = len(la.values[1]) if isinstance(la.values, tuple) else 0
                P = min(step or a.length, a.length)
                bound = NS.nested_device_bound(desc, a.length, sum(x.length for x in arrs), la.length, vlen, P)
                assert bound >= len(chunk), (name, codec, step, bound, len(chunk))
                assert bound >= sum(m.length for m in metas)


def _list_i32(n=10):
    torch = pytest.importorskip("torch")
    fld = pa_amd.Field.list(pa_amd.Field.leaf(np.int32, True, "item"), True)
    offs = torch.arange(0, 2 * n + 1, 2, dtype=torch.int64)
    child = pa_amd.DeviceArray("leaf", 2 * n, torch.ones(2 * n, dtype=torch.bool),
                               values=torch.zeros(2 * n, dtype=torch.int32))
    return fld, pa_amd.DeviceArray("list", n, torch.ones(n, dtype=torch.bool), offs, [child])


def test_short_offsets_are_refused():
    fld, arr = _list_i32()
    arr.offsets = arr.offsets[:-1]
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(fld, arr)
    assert e.value.status == N.E_ARG


def test_struct_child_of_the_wrong_length_is_refused():
    torch = pytest.importorskip("torch")
    fld = pa_amd.Field.struct([pa_amd.Field.leaf(np.int32, False, "x"), pa_amd.Field.leaf(np.uint8, False, "y")], False)
    x = pa_amd.DeviceArray("leaf", 8, values=torch.zeros(8, dtype=torch.int32))
    y = pa_amd.DeviceArray("leaf", 7, values=torch.zeros(7, dtype=torch.uint8))
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(fld, pa_amd.DeviceArray("struct", 8, children=[x, y]))
    assert e.value.status == N.E_ARG


def test_short_bitmap_and_child_are_refused():
    torch = pytest.importorskip("torch")
    fld, arr = _list_i32()
    arr.validity = torch.zeros(1, dtype=torch.uint8)  # 8 bits for 10 slots
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(fld, arr)
    assert e.value.status == N.E_ARG
    fld, arr = _list_i32()
    arr.children[0].length = 19  # the offsets end at 20
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(fld, arr)
    assert e.value.status == N.E_ARG
